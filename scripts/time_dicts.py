"""Times zd_decode_async on dictionary-set plans: 65,536 records of 4 KiB of
gen.text, zstd -3, input and output resident in HBM, each step between device
events.  Three decodes of the same records:
  a  one 112 KiB trained dictionary through zd_plan_create_dict (the shape of
     scripts/time_dict.py);
  b  the same frames through a set of that one dictionary (zd_plan_create_dicts);
  c  the records spread round-robin over 8 dictionaries (the 112 KiB one and
     seven 16 KiB ones trained on other text), as ONE set plan, against EIGHT
     single-dictionary plans, one per dictionary, decoded one after another.
Per decode: the step time, the plan creation time (a second plan of the shape,
so the workspace comes from the cache as in steady use) and the bit-exact flag.
Writes one JSON line (appended to the file given).
usage: python scripts/time_dicts.py [out.jsonl] [records] [steps]"""
import concurrent.futures as cf
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zstd-decompressor_amd")]

import torch  # noqa: E402

from corpus import gen, zdict  # noqa: E402
from zstd_decompressor.batch import Dictionary, DictionarySet, Plan  # noqa: E402

NREC = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 20
WARMUP = 3
REC = 4096
NDICT = 8


def samples(seed, count):
    t = gen.text(count * REC, seed=seed)
    return [t[i:i + REC] for i in range(0, len(t), REC)]


dicts = [zdict.train(samples(0xD1C2, 2048), 112 << 10)]
dicts += [zdict.train(samples(0xD700 + k, 512), 16 << 10) for k in range(1, NDICT)]
assert len({zdict.dict_id(d) for d in dicts}) == NDICT
src = gen.text(NREC * REC, seed=0xD1C5)
recs = [src[i:i + REC] for i in range(0, NREC * REC, REC)]
with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:      # ctypes drops the GIL
    one = list(ex.map(lambda r: zdict.compress(r, dicts[0], 3), recs, chunksize=256))
    spread = list(ex.map(lambda ir: zdict.compress(ir[1], dicts[ir[0] % NDICT], 3), enumerate(recs), chunksize=256))

dev = torch.device("cuda", 0)
stream = torch.cuda.current_stream(dev)


def resident(data):
    t = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    t[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


def make(datas, dictionaries):
    """The plans of one decode (creation timed on a second set of them) and their buffers."""
    for data, d in zip(datas, dictionaries):
        Plan(data, dictionary=d).close()
    t0 = time.perf_counter()
    plans = [Plan(data, dictionary=d) for data, d in zip(datas, dictionaries)]
    create_ms = (time.perf_counter() - t0) * 1e3
    bufs = [(resident(data), torch.zeros(int(p.info.out_bytes) + 64, dtype=torch.uint8, device=dev))
            for data, p in zip(datas, plans)]
    return plans, bufs, create_ms


def run(datas, dictionaries, want):
    plans, bufs, create_ms = make(datas, dictionaries)
    ms = []
    for k in range(WARMUP + STEPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        for p, (s, d) in zip(plans, bufs):
            p.decode_async(s.data_ptr(), d.data_ptr(), int(p.info.out_bytes), stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        if k >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    exact = True
    for p, (s, d), w in zip(plans, bufs, want):
        st, total, _, _, _ = p.results(d.data_ptr(), stream.cuda_stream)
        exact = exact and st == 0 and bytes(d[:total].cpu().numpy().tobytes()) == w
    med = statistics.median(ms)
    res = {"plans": len(plans), "compressed_bytes": sum(map(len, datas)), "step_ms_median": round(med, 3),
           "step_ms_min": round(min(ms), 3), "step_ms_max": round(max(ms), 3),
           "gbps": round(sum(map(len, want)) / med / 1e6, 1), "create_ms": round(create_ms, 2), "bit_exact": exact,
           "executors": sorted({p.info.executors for p in plans}),
           "workspace_bytes": sum(p.info.workspace_bytes for p in plans)}
    for p in plans:
        p.close()
    return res


D = [Dictionary(d) for d in dicts]
set1 = DictionarySet(D[:1], fallback=0)
set8 = DictionarySet(D, fallback=0)
res = {"workload": "%d records of %d B of gen.text, zstd -3; dictionaries of %s B; %d steps of zd_decode_async "
                   "after %d warm-up, input and output in HBM" % (NREC, REC, [len(d) for d in dicts], STEPS, WARMUP),
       "decoded_bytes": len(src),
       "a_one_dictionary": run([b"".join(one)], [D[0]], [src]),
       "b_set_of_one": run([b"".join(one)], [set1], [src]),
       "c_set_of_8_one_plan": run([b"".join(spread)], [set8], [src]),
       "c_eight_plans": run([b"".join(spread[k::NDICT]) for k in range(NDICT)], D,
                            [b"".join(recs[k::NDICT]) for k in range(NDICT)])}
for h in [set1, set8] + D:
    h.close()
line = json.dumps(res)
print(line)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "a").write(line + "\n")
