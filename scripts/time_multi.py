"""Times multi-frame batches (zd_multi_create_device, zd_multi_decode_async, zd_k_multi_join, zd_k_multi_copy):
  (a) one frame   8,192 chunks of one 128 KiB frame each, against Batch.from_device (zd_batch_create_device) over
                  the same entries: decode ms of both, the join pass alone, creation ms of both
  (b) in place    2,048 chunks of four 32 KiB frames each, every frame with a Frame_Content_Size, against
                  zd_batch_create_device over the 8,192 frames as separate chunks with the destinations computed
                  on the host (the same inner batch): decode ms of both
  (c) staged      the same chunks written without Frame_Content_Size (three of four frames staged): decode ms,
                  the join + copy passes alone (zd_multi_finish_async between events), the copy's bytes per second
  (d) parent      the plain, dictionary, prefix and chain batch workloads and the sequential seekable read of
                  scripts/time_seekable.py on this build against --parent (the parent commit's library)
Every side is a library file loaded into this one process, the sides of a comparison alternate inside every
repetition, --reps repetitions after warm-up, min / median / max between device events around the decode call.
Every decode's statuses are checked and every side's bytes compared with the source; a step that fails ends the
script.  Appends one JSON line per comparison to the output file.
usage: python scripts/time_multi.py OUT.jsonl [--parent LIB] [--reps 9] [--scale F] [--only a|b|c|d]"""
import argparse
import concurrent.futures as cf
import ctypes as C
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zstd-decompressor_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corpus import gen, libzstd  # noqa: E402
from zstd_decompressor import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--parent", help="libzd.so of the parent commit (comparison d)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's size")
ap.add_argument("--only", choices=("a", "b", "c", "d"))
args = ap.parse_args()
WARMUP = 2
dev = torch.device("cuda", 0)


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def compress_all(items, fn):
    with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:      # ctypes drops the GIL
        return list(ex.map(fn, items, chunksize=8))


def upload(b):
    t = torch.empty(len(b) + 64, dtype=torch.uint8, device=dev)
    t[: len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return t


def stream():
    return torch.cuda.current_stream(dev)


def timed(fn):
    """ms between device events around fn()"""
    s = stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    fn()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1)


def emit(res):
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def race(sides):
    """The sides alternating, the order rotated every repetition."""
    keys = list(sides)
    for rep in range(WARMUP + args.reps):
        for k in keys[rep % len(keys):] + keys[:rep % len(keys)]:
            sides[k].decode(rep >= WARMUP)
    return {k: stats(s.ms) for k, s in sides.items()}


def same(t, want: bytes, what):
    if not np.array_equal(t.cpu().numpy(), np.frombuffer(want, dtype=np.uint8)):
        raise SystemExit(f"{what}: bytes differ from the source")


class Frames:
    """n frames of `size` bytes of seeded text each (the distinct ones compressed, then repeated), back to back on
    the device; chunk i is frames [i per, (i + 1) per)."""

    def __init__(self, n, size, seed, fcs=True):
        nu = min(n, max(1, (64 << 20) // size))
        self.text = gen.text(nu * size + size, seed=seed)[: nu * size]
        recs = [self.text[i:i + size] for i in range(0, nu * size, size)]
        frames = compress_all(recs, lambda r: libzstd.compress(r, 3, content_size=fcs))
        self.n, self.size, self.nu = n, size, nu
        self.frames = (frames * ((n + nu - 1) // nu))[:n]
        self.src = upload(b"".join(self.frames))
        self.c_off = np.cumsum([0] + [len(f) for f in self.frames])
        self.total = n * size

    def content(self, first, count):
        return b"".join(self.text[(i % self.nu) * self.size:(i % self.nu + 1) * self.size]
                        for i in range(first, first + count))


def tensor(v):
    return torch.tensor(v, dtype=torch.int64, device=dev)


class Side:
    def check(self):
        F, k = self.F, max(1, (1 << 20) // self.F.size)
        k = min(k, F.n)
        same(self.dst[: k * F.size], F.content(0, k), "the first bytes")
        same(self.dst[F.total - k * F.size:F.total], F.content(F.n - k, k), "the last bytes")


class MultiSide(Side):
    """zd_multi_create_device over chunks of `per` frames each"""

    def __init__(self, L, F, per):
        self.L, self.F, n = L, F, F.n // per
        self.dst = torch.zeros(F.total + 64, dtype=torch.uint8, device=dev)
        base = F.src.data_ptr()
        self.arrs = (tensor([base + int(F.c_off[i * per]) for i in range(n)]),
                     tensor([int(F.c_off[(i + 1) * per] - F.c_off[i * per]) for i in range(n)]),
                     tensor([self.dst.data_ptr() + i * per * F.size for i in range(n)]), tensor([per * F.size] * n))
        torch.cuda.synchronize()
        s = C.c_void_p(stream().cuda_stream)
        self.create_ms, self.h = [], None
        for _ in range(3):
            if self.h:
                L.zd_multi_destroy(self.h)
            self.h = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.zd_multi_create_device(*[C.c_void_p(a.data_ptr()) for a in self.arrs], n, 0, None, None, s,
                                                C.byref(self.h)), "zd_multi_create_device")
            self.create_ms.append((time.perf_counter() - t0) * 1e3)
        self.info = _lib.MultiInfo()
        _lib.check(L.zd_multi_info_get_sized(self.h, C.byref(self.info), C.sizeof(self.info)))
        self.ms, self.finish_ms = [], []

    def decode(self, keep):
        s = C.c_void_p(stream().cuda_stream)
        ms = timed(lambda: _lib.check(self.L.zd_multi_decode_async(self.h, s), "zd_multi_decode_async"))
        bad = C.c_uint64()
        _lib.check(self.L.zd_multi_results(self.h, s, None, None, 0, C.byref(bad)))
        if bad.value:
            raise SystemExit(f"{bad.value} chunks failed")
        fin = timed(lambda: _lib.check(self.L.zd_multi_finish_async(self.h, s), "zd_multi_finish_async"))
        if keep:
            self.ms.append(ms)
            self.finish_ms.append(fin)

    def close(self):
        self.L.zd_multi_destroy(self.h)


class DeviceBatchSide(Side):
    """zd_batch_create_device over every frame as a chunk of its own, the destinations computed on the host"""

    def __init__(self, L, F):
        self.L, self.F = L, F
        self.dst = torch.zeros(F.total + 64, dtype=torch.uint8, device=dev)
        base = F.src.data_ptr()
        self.arrs = (tensor([base + int(o) for o in F.c_off[:-1]]), tensor([len(f) for f in F.frames]),
                     tensor([self.dst.data_ptr() + i * F.size for i in range(F.n)]), tensor([F.size] * F.n))
        torch.cuda.synchronize()
        s = C.c_void_p(stream().cuda_stream)
        self.create_ms, self.h = [], None
        for _ in range(3):
            if self.h:
                L.zd_batch_destroy(self.h)
            self.h = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.zd_batch_create_device(*[C.c_void_p(a.data_ptr()) for a in self.arrs], F.n, 0, None, s,
                                                C.byref(self.h)), "zd_batch_create_device")
            self.create_ms.append((time.perf_counter() - t0) * 1e3)
        self.ms = []

    def decode(self, keep):
        s = C.c_void_p(stream().cuda_stream)
        ms = timed(lambda: _lib.check(self.L.zd_batch_decode_async(self.h, s), "zd_batch_decode_async"))
        bad = C.c_uint64()
        _lib.check(self.L.zd_batch_results(self.h, s, None, None, 0, C.byref(bad)))
        if bad.value:
            raise SystemExit(f"{bad.value} chunks failed")
        if keep:
            self.ms.append(ms)

    def close(self):
        self.L.zd_batch_destroy(self.h)


def compare(label, F, per, extra=None):
    L = _lib.lib()
    sides = {"multi_frame_batch": MultiSide(L, F, per), "device_batch": DeviceBatchSide(L, F)}
    ms = race(sides)
    for s in sides.values():
        s.check()
    m, I = sides["multi_frame_batch"], sides["multi_frame_batch"].info
    res = {"comparison": label, "chunks": F.n // per, "frames": F.n, "decoded_bytes": F.total, "reps": args.reps,
           "warmup": WARMUP, "ms": ms, "finish_passes_ms": stats(m.finish_ms),
           "multi_over_batch": round(ms["multi_frame_batch"]["median"] / ms["device_batch"]["median"], 4),
           "multi_gbps": round(F.total / ms["multi_frame_batch"]["median"] / 1e6, 1),
           "multi_create_ms": stats(m.create_ms), "batch_create_ms": stats(sides["device_batch"].create_ms),
           "info_frames": I.frames, "frames_in_place": I.frames_in_place, "staged_frames": I.staged_frames,
           "staged_bytes": I.staged_bytes, "copy_pieces": I.copy_pieces, "executors": I.batch.executors}
    if I.staged_frames:
        copied = I.staged_frames * F.size
        res["copied_bytes"] = copied
        res["finish_gbps"] = round(copied / statistics.median(m.finish_ms) / 1e6, 1)
    res.update(extra or {})
    emit(res)
    for s in sides.values():
        s.close()


def one_frame():
    n = max(1, int(8192 * args.scale))
    compare("a: 8192 chunks of one 128 KiB frame / zd_batch_create_device over the same entries",
            Frames(n, 128 << 10, 0x3A17A), 1)


def in_place():
    n = max(4, int(8192 * args.scale) // 4 * 4)
    compare("b: 2048 chunks of four 32 KiB frames with Frame_Content_Size / zd_batch_create_device over the 8192 frames",
            Frames(n, 32 << 10, 0x3A17B), 4)


def staged():
    n = max(4, int(8192 * args.scale) // 4 * 4)
    compare("c: 2048 chunks of four 32 KiB frames without Frame_Content_Size (three of four staged) / "
            "zd_batch_create_device over the 8192 frames", Frames(n, 32 << 10, 0x3A17B, fcs=False), 4)


def parent():
    """time_seekable.py's comparison against the parent commit's library, and its sequential read on both."""
    spec = importlib.util.spec_from_file_location("time_seekable", os.path.join(ROOT, "scripts", "time_seekable.py"))
    argv = sys.argv
    sys.argv = [argv[0], args.out, "--parent", args.parent, "--reps", str(args.reps), "--scale", str(args.scale)]
    try:
        ts = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ts)
    finally:
        sys.argv = argv
    ts.PARENT = ts.load(args.parent)
    ts.emit = lambda res: emit(dict(res, comparison="d" + res["comparison"][1:]))
    ts.parent()
    arc = ts.Arc(max(2 << 20, int((1 << 30) * args.scale)), 1 << 20, 0x5EE4A)
    sides = {"new": ts.ReadSide(_lib.lib(), arc, [(0, arc.total)]), "parent": ts.ReadSide(ts.PARENT, arc, [(0, arc.total)])}
    ms = race(sides)
    for s in sides.values():
        s.check()
        s.close()
    emit({"comparison": "d: seekable read, one range over 1 GiB of 1 MiB entries: this build against the parent commit's",
          "reps": args.reps, "warmup": WARMUP, "ms": ms, "entries": arc.n, "decoded_bytes": arc.total,
          "new_over_parent": round(ms["new"]["median"] / ms["parent"]["median"], 4)})


def main():
    if args.only in (None, "a"):
        one_frame()
    if args.only in (None, "b"):
        in_place()
    if args.only in (None, "c"):
        staged()
    if args.only in (None, "d"):
        if not args.parent:
            raise SystemExit("comparison d needs --parent LIB")
        parent()


if __name__ == "__main__":
    main()
