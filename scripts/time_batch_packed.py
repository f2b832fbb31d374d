"""Times the size query and the packed batches (zd_chunk_sizes_device,
zd_batch_create_device_packed) against zd_batch_create_device over the same
sources with destinations precomputed, on the two workloads of
scripts/time_batch.py:
  frames   8,192 frames of 128 KiB of gen.text, zstd -3
  records  65,536 records of 4 KiB with a 112 KiB trained dictionary
Both kinds of batch alternate in one process, --reps times each (default 9):
  (a) sizes    zd_k_chunk_sizes between device events, and beside it the layout
               + gather + walk-count phases (zd_batch_info gather_ns + walk_ns)
               of the device creation over the same table
  (b) create   the wall time of each creation call and its phase split
  (c) decode   one zd_batch_decode_async of each batch between device events
Medians with min and max; one JSON line per workload, appended to the output.
usage: python scripts/time_batch_packed.py [out.jsonl] [--reps N] [--unique-mib N] [--scale F]"""
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
from zstd_decompressor import _lib  # noqa: E402
from zstd_decompressor.batch import Batch, Dictionary  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out", nargs="?")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--unique-mib", type=int, default=64)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's chunk count")
args = ap.parse_args()
WARMUP = 3
ALIGN = 16
PHASES = ("gather", "walk", "host", "upload")
dev = torch.device("cuda", 0)


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def compress_all(pieces, fn):
    with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:      # ctypes drops the GIL
        return list(ex.map(fn, pieces, chunksize=64))


def timed(launch, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    launch()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def workload(name, chunk, nchunks, unique, compress, dictionary, dict_bytes):
    print("%s: compressing" % name, file=sys.stderr, flush=True)
    frames_u = compress_all(unique, compress)
    reps = (nchunks + len(unique) - 1) // len(unique)
    frames = (frames_u * reps)[:nchunks]
    sources = (unique * reps)[:nchunks]
    packed = b"".join(frames)
    sizes = [len(f) for f in frames]
    offs = np.concatenate(([0], np.cumsum(sizes)[:-1])).tolist()
    caps = [len(x) for x in sources]
    assert all(c % ALIGN == 0 for c in caps)           # (so the packed layout is the contiguous one)
    out_bytes = sum(caps)
    d_src = torch.zeros(len(packed) + 64, dtype=torch.uint8, device=dev)
    d_src[: len(packed)].copy_(torch.frombuffer(bytearray(packed), dtype=torch.uint8))
    d_dst = torch.zeros(out_bytes + 64, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev)
    dst_offs = np.concatenate(([0], np.cumsum(caps)[:-1])).tolist()
    expect = torch.frombuffer(bytearray(b"".join(sources)), dtype=torch.uint8)
    t_src, t_size, t_dst, t_cap = (torch.tensor(v, dtype=torch.int64, device=dev) for v in (
        [d_src.data_ptr() + o for o in offs], sizes, [d_dst.data_ptr() + o for o in dst_offs], caps))
    torch.cuda.synchronize()

    print("%s: timing" % name, file=sys.stderr, flush=True)
    # ---- (a) the size query ----
    q_size = torch.empty(nchunks, dtype=torch.int64, device=dev)
    q_status = torch.empty(nchunks, dtype=torch.int32, device=dev)
    q_exact = torch.empty(nchunks, dtype=torch.uint8, device=dev)
    L = _lib.lib()
    flags = _lib.SIZES_DICT if dictionary is not None else 0

    def query():
        _lib.check(L.zd_chunk_sizes_device(t_src.data_ptr(), t_size.data_ptr(), nchunks, flags, q_size.data_ptr(),
                                           q_status.data_ptr(), q_exact.data_ptr(), s.cuda_stream))
    for _ in range(WARMUP):
        timed(query, s)
    sizes_ms = [timed(query, s) for _ in range(args.reps)]
    sizes_right = bool(torch.equal(q_size, t_cap)) and not bool(q_status.any()) and bool(q_exact.all())

    # ---- (b) creation, alternating ----
    makers = {
        "device": lambda: Batch.from_device(t_src, t_size, t_dst, t_cap, dictionary=dictionary, stream=s.cuda_stream),
        "packed": lambda: Batch.packed(t_src, t_size, align=ALIGN, dictionary=dictionary, stream=s.cuda_stream),
    }
    for m in makers.values():
        m().close()            # (the first object of a shape allocates the workspace the next reuses)
    ab = {k: {"wall": [], **{ph: [] for ph in PHASES}} for k in makers}
    for _ in range(args.reps):
        for k, m in makers.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            x = m()
            ab[k]["wall"].append((time.perf_counter() - t0) * 1e3)
            for ph in PHASES:
                ab[k][ph].append(getattr(x.info, ph + "_ns") / 1e6)
            x.close()

    # ---- (c) decode, alternating ----
    batches = {k: m() for k, m in makers.items()}
    assert batches["packed"].out_bytes == out_bytes
    batches["packed"].bind_output(d_dst.data_ptr(), out_bytes)
    dec = {k: [] for k in batches}
    for k, x in batches.items():
        for _ in range(WARMUP):
            timed(lambda: x.decode_async(s.cuda_stream), s)
    for _ in range(args.reps):
        for k, x in batches.items():
            dec[k].append(timed(lambda: x.decode_async(s.cuda_stream), s))
    out = {}
    for k, x in batches.items():
        d_dst.zero_()
        x.decode_async(s.cuda_stream)
        st, ln = x.results(s.cuda_stream)
        exact = not any(st) and sum(ln) == out_bytes and bool(torch.equal(d_dst[:out_bytes].cpu(), expect))
        out[k] = {"create_wall_ms": stats(ab[k]["wall"]), "create_ms": {ph: stats(ab[k][ph]) for ph in PHASES},
                  "decode_ms": stats(dec[k]), "bit_exact": exact, "executors": x.info.executors,
                  "nblocks": x.info.nblocks}
        x.close()
    parent_phases = [g + w for g, w in zip(ab["device"]["gather"], ab["device"]["walk"])]
    return {
        "workload": name, "chunks": nchunks, "chunk_bytes": chunk, "compressed_bytes": len(packed),
        "decoded_bytes": out_bytes, "dictionary_bytes": dict_bytes, "reps": args.reps, "warmup": WARMUP, "align": ALIGN,
        "sizes_ms": stats(sizes_ms), "sizes_right": sizes_right,
        "device_layout_gather_walk_ms": stats(parent_phases),
        **out,
        "create_packed_over_device": round(out["packed"]["create_wall_ms"]["median"] /
                                           out["device"]["create_wall_ms"]["median"], 4),
        "decode_packed_over_device": round(out["packed"]["decode_ms"]["median"] /
                                           out["device"]["decode_ms"]["median"], 4),
    }


def main():
    lines = []
    chunk, nchunks = 128 << 10, max(1, int(8192 * args.scale))
    nu = min(nchunks, max(1, (args.unique_mib << 20) // chunk))
    text = gen.text(nu * chunk, seed=0xBA7C0)
    unique = [text[i:i + chunk] for i in range(0, nu * chunk, chunk)]
    lines.append(workload("8192 x 128 KiB gen.text, zstd -3", chunk, nchunks, unique,
                          lambda r: libzstd.compress(r, 3), None, 0))
    rec, nrec = 4096, max(1, int(65536 * args.scale))
    train = gen.text(2048 * rec, seed=0xD1C2)
    dct = zdict.train([train[i:i + rec] for i in range(0, len(train), rec)], 112 << 10)
    nu = min(nrec, max(1, (args.unique_mib << 20) // rec))
    text = gen.text(nu * rec, seed=0xD1C5)
    unique = [text[i:i + rec] for i in range(0, nu * rec, rec)]
    d = Dictionary(dct)
    lines.append(workload("65536 x 4 KiB gen.text, zstd -3, trained dictionary", rec, nrec, unique,
                          lambda r: zdict.compress(r, dct, 3), d, len(dct)))
    d.close()
    for line in lines:
        print(json.dumps(line))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            for line in lines:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
