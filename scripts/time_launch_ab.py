"""Two builds of libzd.so decoding one chain batch, both loaded into this process: the host launch cost of
launch_pipeline, which a chain batch of many levels shows most (256 levels x 4 chunks: over a thousand
launches a decode with ZD_F_CHAIN_BLOCK_PARALLEL).  The batch: --depth levels x --width chains of 16 KiB text pages,
1 % of the bytes edited per version (--unique distinct chains, the rest repeat them), level 0 over external
bases; once on the streaming executor and once with ZD_F_CHAIN_BLOCK_PARALLEL.  The sides alternate inside
every repetition with the order rotated, --reps repetitions after 3 of warm-up; decode = device events around
zd_batch_decode_async, host call = wall clock of the call alone; median (min-max).  Every decode's statuses are
checked and every side's bytes compared with the records.  Appends one JSON line per executor to OUT.jsonl.
--swap creates the second library's batch first (allocation placement); the same library file given twice,
or a copy of it, is the control.
usage: python scripts/time_launch_ab.py OUT.jsonl PARENT_LIB THIS_LIB [--reps 15] [--depth 256] [--width 4]
           [--unique 512] [--swap]
(PARENT_LIB: lib/libzd.so built from the commit to compare against, THIS_LIB: this tree's)"""
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zstd-decompressor_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corpus import gen, zdict  # noqa: E402
from zstd_decompressor import _lib  # noqa: E402

out_path, parent_lib, this_lib = sys.argv[1:4]


def opt(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


REPS, WARMUP, PAGE, DEPTH, WIDTH = opt("--reps", 15), 3, 16 << 10, opt("--depth", 256), opt("--width", 4)
NU = min(WIDTH, opt("--unique", 512))
dev = torch.device("cuda", 0)
vpp = C.POINTER(C.c_void_p)


def load(path):
    L = C.CDLL(path)
    for name, (res, argt) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, argt
    return L


def u64(v):
    return (C.c_uint64 * len(v))(*v)


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def upload(b):
    t = torch.empty(len(b) + 64, dtype=torch.uint8, device=dev)
    t[: len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return t


rng = np.random.default_rng(0xDC01)
bases = [gen.text(PAGE, seed=0xDC10 + k)[:PAGE] for k in range(NU)]
recs, frames, prev = [], [], bases
for lv in range(DEPTH):
    cur = []
    for k in range(NU):
        b = bytearray(prev[k])
        for p in rng.choice(PAGE, PAGE // 100, replace=False):
            b[p] ^= int(rng.integers(1, 256))
        cur.append(bytes(b))
        frames.append(zdict.prefix_compress(cur[-1], prev[k], 3))
    recs += [cur[k % NU] for k in range(WIDTH)]
    frames[-NU:] = [frames[len(frames) - NU + k % NU] for k in range(WIDTH)]
    prev = cur
M = DEPTH * WIDTH
src = upload(b"".join(frames))
so = np.cumsum([0] + [len(f) for f in frames])
base = upload(b"".join(bases))
expect = np.frombuffer(b"".join(recs), dtype=np.uint8)


class Side:
    def __init__(self, L, flags):
        self.L, self.flags = L, flags
        self.dst = torch.zeros(M * PAGE + 64, dtype=torch.uint8, device=dev)
        self.sp = u64([src.data_ptr() + int(so[i]) for i in range(M)])
        self.ss = u64([len(f) for f in frames])
        self.dp = u64([self.dst.data_ptr() + i * PAGE for i in range(M)])
        self.dc = u64([PAGE] * M)
        self.pp = u64([base.data_ptr() + (i % NU) * PAGE if i < WIDTH else 0 for i in range(M)])
        self.ps = u64([PAGE if i < WIDTH else 0 for i in range(M)])
        self.par = (C.c_int64 * M)(*[i - WIDTH if i >= WIDTH else -1 for i in range(M)])
        s = torch.cuda.current_stream(dev)
        self.h = C.c_void_p()
        _lib.check(L.zd_batch_create_chain(C.cast(self.sp, vpp), self.ss, C.cast(self.dp, vpp), self.dc,
                                           C.cast(self.pp, vpp), self.ps, self.par, M, flags,
                                           C.c_void_p(s.cuda_stream), C.byref(self.h)), "zd_batch_create_chain")
        self.dev_ms, self.wall_ms = [], []

    def run(self, timed):
        self.dst.zero_()
        s = torch.cuda.current_stream(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(dev)
        e0.record(s)
        t0 = time.perf_counter()
        _lib.check(self.L.zd_batch_decode_async(self.h, C.c_void_p(s.cuda_stream)), "zd_batch_decode_async")
        t1 = time.perf_counter()
        e1.record(s)
        e1.synchronize()
        bad = C.c_uint64()
        _lib.check(self.L.zd_batch_results(self.h, C.c_void_p(s.cuda_stream), None, None, 0, C.byref(bad)))
        if bad.value:
            raise SystemExit(f"{bad.value} chunks failed")
        if timed:
            self.dev_ms.append(e0.elapsed_time(e1))
            self.wall_ms.append((t1 - t0) * 1e3)

    def check(self):
        if not np.array_equal(self.dst[: M * PAGE].cpu().numpy(), expect):
            raise SystemExit("an output differs from its record")


LP, LT = load(parent_lib), load(this_lib)
for label, flags in (("chain batch, streaming executor", 0),
                     ("chain batch, CHAIN_BLOCK_PARALLEL", _lib.F_CHAIN_BLOCK_PARALLEL)):
    if "--swap" in sys.argv:        # the other creation order (allocation placement)
        sides = {"this": Side(LT, flags), "parent": Side(LP, flags)}
    else:
        sides = {"parent": Side(LP, flags), "this": Side(LT, flags)}
    keys = list(sides)
    for rep in range(WARMUP + REPS):
        for k in keys[rep % 2:] + keys[:rep % 2]:
            sides[k].run(rep >= WARMUP)
    for s in sides.values():
        s.check()
    p, t = sides["parent"], sides["this"]
    inside = lambda a, b: min(b) <= statistics.median(a) <= max(b)
    line = {"comparison": f"{label}: {DEPTH} levels x {WIDTH} chunks of 16 KiB, one zd_batch_decode_async", "reps": REPS,
            "created_first": list(sides)[0], "libs": [os.path.basename(parent_lib), os.path.basename(this_lib)],
            "warmup": WARMUP, "decode_ms": {"parent": stats(p.dev_ms), "this": stats(t.dev_ms)},
            "host_call_ms": {"parent": stats(p.wall_ms), "this": stats(t.wall_ms)},
            "this_over_parent_decode": round(statistics.median(t.dev_ms) / statistics.median(p.dev_ms), 4),
            "this_median_inside_parent_range": inside(t.dev_ms, p.dev_ms),
            "parent_median_inside_this_range": inside(p.dev_ms, t.dev_ms), "bit_exact": True}
    print(json.dumps(line), flush=True)
    with open(out_path, "a") as f:
        f.write(json.dumps(line) + "\n")
    for s in sides.values():
        s.L.zd_batch_destroy(s.h)
