"""Times zd_decode_async on a dictionary plan against the same records
compressed without a dictionary: 65,536 records of 4 KiB of gen.text, zstd -3,
a 112 KiB trained dictionary (corpus/zdict.py); both inputs resident in HBM,
each step between device events, mode-2 kernel times from one more step.
Writes one JSON line.
usage: python scripts/time_dict.py [out.json] [records] [steps]"""
import concurrent.futures as cf
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zstd-decompressor_amd")]

import torch  # noqa: E402

from corpus import gen, libzstd, zdict  # noqa: E402
from zstd_decompressor.batch import Dictionary, Plan  # noqa: E402

NREC = int(sys.argv[2]) if len(sys.argv) > 2 else 65536
STEPS = int(sys.argv[3]) if len(sys.argv) > 3 else 20
WARMUP = 3
REC = 4096

train = gen.text(2048 * REC, seed=0xD1C2)
dct = zdict.train([train[i:i + REC] for i in range(0, len(train), REC)], 112 << 10)
src = gen.text(NREC * REC, seed=0xD1C5)
recs = [src[i:i + REC] for i in range(0, NREC * REC, REC)]
with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:      # ctypes drops the GIL
    with_dict = b"".join(ex.map(lambda r: zdict.compress(r, dct, 3), recs, chunksize=256))
    without = b"".join(ex.map(lambda r: libzstd.compress(r, 3), recs, chunksize=256))

dev = torch.device("cuda", 0)


def run(data, dictionary):
    Plan(data, dictionary=dictionary).close()      # (the first plan of a shape allocates the workspace the next reuses)
    plan = Plan(data, dictionary=dictionary)
    n = int(plan.info.out_bytes)
    d_src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    d_src[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    d_dst = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev)
    ms = []
    for k in range(WARMUP + STEPS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, s.cuda_stream)
        e1.record(s)
        e1.synchronize()
        if k >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    st, total, _, _, _ = plan.results(d_dst.data_ptr(), s.cuda_stream)
    exact = st == 0 and bytes(d_dst[:total].cpu().numpy().tobytes()) == src
    plan.set_profiling(2)
    plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, s.cuda_stream)
    s.synchronize()
    kt = {k: round(v, 3) for k, v in plan.kernel_times().items()}
    info = plan.refresh_info()
    med = statistics.median(ms)
    res = {"compressed_bytes": len(data), "step_ms_median": round(med, 3), "step_ms_min": round(min(ms), 3),
           "step_ms_max": round(max(ms), 3), "gbps": round(len(src) / med / 1e6, 1), "bit_exact": exact,
           "kernel_ms": kt, "executors": info.executors, "plan_host_ms": round(info.host_ns / 1e6, 2),
           "plan_device_ms": round(info.device_ns / 1e6, 2)}
    plan.close()
    return res


d = Dictionary(dct)
res = {"workload": "%d records of %d B of gen.text, zstd -3, %d B trained dictionary; %d steps of zd_decode_async "
                   "after %d warm-up, input and output in HBM" % (NREC, REC, len(dct), STEPS, WARMUP),
       "decoded_bytes": len(src), "dictionary": run(with_dict, d), "no_dictionary": run(without, None)}
d.close()
line = json.dumps(res)
print(line)
if len(sys.argv) > 1:
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    open(sys.argv[1], "w").write(line + "\n")
