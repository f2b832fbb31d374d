"""Times a Batch (scattered chunks, per-chunk buffers; zd_batch_create /
zd_batch_decode_async) against a Plan over the same frames packed into one
buffer with one contiguous output, on two workloads:
  frames   8,192 frames of 128 KiB of gen.text, zstd -3 (Plan.from_device)
  records  65,536 records of 4 KiB with a 112 KiB trained dictionary (Plan
           with dictionary=: the device walk takes none)
Creation: the wall time of the call, and for the batch its split into gather /
walk / host / upload (zd_batch_info); decode: each step between device events
after warm-up.  Medians with min and max.  The unique source text is
replicated to the workload's size (--unique-mib).  Writes one JSON line.
The device-creation leg (device_ab): the same four arrays uploaded once, then
zd_batch_create (host arrays) and zd_batch_create_device (device arrays)
alternating in this process, --creates times each: the wall time of each call
and its zd_batch_info phase split, then the decode time of a batch of each
kind.  --ab-out appends one line per workload with that leg alone.
usage: python scripts/time_batch.py [out.jsonl] [--steps N] [--creates N] [--unique-mib N] [--scale F]
                                    [--ab-out ab.jsonl]"""
import argparse
import concurrent.futures as cf
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zstd-decompressor_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corpus import gen, libzstd, zdict  # noqa: E402
from zstd_decompressor.batch import Batch, Dictionary, Plan  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--steps", type=int, default=20)
ap.add_argument("--creates", type=int, default=5)
ap.add_argument("--unique-mib", type=int, default=64)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's chunk count")
ap.add_argument("--ab-out", help="append the device-creation leg of each workload here, one line each")
args = ap.parse_args()
WARMUP = 3
dev = torch.device("cuda", 0)


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def compress_all(pieces, fn):
    with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:      # ctypes drops the GIL
        return list(ex.map(fn, pieces, chunksize=64))


def timed_steps(launch, stream):
    ms = []
    for k in range(WARMUP + args.steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        launch()
        e1.record(stream)
        e1.synchronize()
        if k >= WARMUP:
            ms.append(e0.elapsed_time(e1))
    return ms


def workload(name, chunk, nchunks, unique, compress, dictionary, dict_bytes):
    """unique: distinct source chunks; the workload is their frames repeated to nchunks."""
    frames_u = compress_all(unique, compress)
    reps = (nchunks + len(unique) - 1) // len(unique)
    frames = (frames_u * reps)[:nchunks]
    sources = (unique * reps)[:nchunks]
    packed = b"".join(frames)
    sizes = [len(f) for f in frames]
    offs = np.concatenate(([0], np.cumsum(sizes)[:-1])).tolist()
    out_bytes = sum(len(s) for s in sources)
    d_src = torch.zeros(len(packed) + 64, dtype=torch.uint8, device=dev)
    d_src[: len(packed)].copy_(torch.frombuffer(bytearray(packed), dtype=torch.uint8))
    d_dst = torch.zeros(out_bytes + 64, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev)
    caps = [len(x) for x in sources]
    dst_offs = np.concatenate(([0], np.cumsum(caps)[:-1])).tolist()
    src_ptrs = [d_src.data_ptr() + o for o in offs]
    dst_ptrs = [d_dst.data_ptr() + o for o in dst_offs]
    expect = torch.frombuffer(bytearray(b"".join(sources)), dtype=torch.uint8)

    # ---- the batch ----
    def make_batch():
        return Batch(src_ptrs, sizes, dst_ptrs, caps, dictionary=dictionary, stream=s.cuda_stream)
    make_batch().close()            # (the first object of a shape allocates the workspace the next reuses)
    wall, split = [], {"gather": [], "walk": [], "host": [], "upload": []}
    b = None
    for _ in range(args.creates):
        if b is not None:
            b.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        b = make_batch()
        wall.append((time.perf_counter() - t0) * 1e3)
        for k in split:
            split[k].append(getattr(b.info, k + "_ns") / 1e6)
    d_dst.zero_()
    bms = timed_steps(lambda: b.decode_async(s.cuda_stream), s)
    st, ln = b.results(s.cuda_stream)
    b_exact = not any(st) and sum(ln) == out_bytes and bool(torch.equal(d_dst[:out_bytes].cpu(), expect))
    b_exec, b_gathered, b_ws = b.info.executors, b.info.gathered_bytes, b.info.workspace_bytes
    b.close()

    # ---- the plan over the packed frames ----
    def make_plan():
        if dictionary is None:
            return Plan.from_device(d_src.data_ptr(), len(packed), stream=s.cuda_stream)
        return Plan(packed, dictionary=dictionary)
    make_plan().close()
    pwall = []
    p = None
    for _ in range(args.creates):
        if p is not None:
            p.close()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = make_plan()
        pwall.append((time.perf_counter() - t0) * 1e3)
    d_dst.zero_()
    n = int(p.info.out_bytes)
    pms = timed_steps(lambda: p.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, s.cuda_stream), s)
    pst, total, _, _, _ = p.results(d_dst.data_ptr(), s.cuda_stream)
    p_exact = pst == 0 and total == out_bytes and bool(torch.equal(d_dst[:out_bytes].cpu(), expect))
    p_exec = p.info.executors
    p.close()

    # ---- creation from device arrays against creation from host arrays ----
    d_arrs = [torch.tensor(v, dtype=torch.int64, device=dev) for v in (src_ptrs, sizes, dst_ptrs, caps)]
    torch.cuda.synchronize()

    def make_device_batch():
        return Batch.from_device(*d_arrs, dictionary=dictionary, stream=s.cuda_stream)
    makers = {"host": make_batch, "device": make_device_batch}
    for m in makers.values():
        m().close()
    ab = {k: {"wall": [], "gather": [], "walk": [], "host": [], "upload": []} for k in makers}
    for _ in range(args.creates):
        for k, m in makers.items():                      # alternating
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = m()
            ab[k]["wall"].append((time.perf_counter() - t0) * 1e3)
            for ph in ("gather", "walk", "host", "upload"):
                ab[k][ph].append(getattr(x.info, ph + "_ns") / 1e6)
            x.close()
    device_ab = {}
    for k, m in makers.items():
        x = m()
        d_dst.zero_()
        ms = timed_steps(lambda: x.decode_async(s.cuda_stream), s)
        st, ln = x.results(s.cuda_stream)
        exact = not any(st) and sum(ln) == out_bytes and bool(torch.equal(d_dst[:out_bytes].cpu(), expect))
        device_ab[k] = {"create_wall_ms": stats(ab[k]["wall"]),
                        "create_ms": {ph: stats(ab[k][ph]) for ph in ("gather", "walk", "host", "upload")},
                        "decode_ms": stats(ms), "bit_exact": exact, "executors": x.info.executors,
                        "device_built": x.info.device_built, "nblocks": x.info.nblocks}
        x.close()
    device_ab["create_device_over_host"] = round(device_ab["device"]["create_wall_ms"]["median"] /
                                                 device_ab["host"]["create_wall_ms"]["median"], 4)
    device_ab["decode_device_over_host"] = round(device_ab["device"]["decode_ms"]["median"] /
                                                 device_ab["host"]["decode_ms"]["median"], 4)
    if args.ab_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.ab_out)), exist_ok=True)
        with open(args.ab_out, "a") as f:
            f.write(json.dumps({"workload": name, "chunks": nchunks, "chunk_bytes": chunk,
                                "dictionary_bytes": dict_bytes, "steps": args.steps, "warmup": WARMUP,
                                "creates": args.creates, **device_ab}) + "\n")

    bmed, pmed = statistics.median(bms), statistics.median(pms)
    csum = sum(statistics.median(v) for v in split.values())
    return {
        "workload": name, "chunks": nchunks, "chunk_bytes": chunk, "compressed_bytes": len(packed),
        "decoded_bytes": out_bytes, "dictionary_bytes": dict_bytes,
        "batch": {"create_wall_ms": stats(wall), "create_ms": {k: stats(v) for k, v in split.items()},
                  "create_sum_ms": round(csum, 3),
                  "gather_share_of_decode": round(statistics.median(split["gather"]) / bmed, 4),
                  "decode_ms": stats(bms), "gbps": round(out_bytes / bmed / 1e6, 1), "bit_exact": b_exact,
                  "executors": b_exec, "gathered_bytes": b_gathered, "workspace_bytes": b_ws},
        "plan": {"kind": "from_device" if dictionary is None else "host walk, dictionary",
                 "create_wall_ms": stats(pwall), "decode_ms": stats(pms), "gbps": round(out_bytes / pmed / 1e6, 1),
                 "bit_exact": p_exact, "executors": p_exec},
        "decode_batch_over_plan": round(bmed / pmed, 4),
        "device_ab": device_ab,
    }


def main():
    res = {"steps": args.steps, "warmup": WARMUP, "creates": args.creates, "unique_mib": args.unique_mib}
    # 8,192 x 128 KiB, zstd -3
    chunk, nchunks = 128 << 10, max(1, int(8192 * args.scale))
    nu = min(nchunks, max(1, (args.unique_mib << 20) // chunk))
    text = gen.text(nu * chunk, seed=0xBA7C0)
    unique = [text[i:i + chunk] for i in range(0, nu * chunk, chunk)]
    res["frames"] = workload("8192 x 128 KiB gen.text, zstd -3", chunk, nchunks, unique,
                             lambda r: libzstd.compress(r, 3), None, 0)
    # 65,536 x 4 KiB with a trained dictionary
    rec, nrec = 4096, max(1, int(65536 * args.scale))
    train = gen.text(2048 * rec, seed=0xD1C2)
    dct = zdict.train([train[i:i + rec] for i in range(0, len(train), rec)], 112 << 10)
    nu = min(nrec, max(1, (args.unique_mib << 20) // rec))
    text = gen.text(nu * rec, seed=0xD1C5)
    unique = [text[i:i + rec] for i in range(0, nu * rec, rec)]
    d = Dictionary(dct)
    res["records"] = workload("65536 x 4 KiB gen.text, zstd -3, trained dictionary", rec, nrec, unique,
                              lambda r: zdict.compress(r, dct, 3), d, len(dct))
    d.close()
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
