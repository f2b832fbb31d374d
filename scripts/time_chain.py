"""Times chain batches (zd_batch_create_chain, zd_k_execute_chain) on time_prefix.py's page workload: 16 KiB text
pages, 1 % of the bytes edited per version, 8,192 chains of depth 4 over an external base page each (32,768 chunks).
  (A) chain     ONE chain batch over all 32,768 chunks: its creation and one decode
  (B) links     FOUR prefix batches of 8,192 chunks, created and decoded one after another, level k's prefixes the
                outputs of level k - 1: the way without chain batches.  With --parent also on the parent commit's
                library, which shows prefix batches unchanged
  (C) no links  a chain batch whose every parent is -1 against the prefix batch over the same 8,192 chunks
Every side is a library file loaded into this one process; the sides alternate inside every repetition (order rotated),
--reps repetitions after warm-up; creation is host wall clock around the create call (it synchronises), decode is
device events around zd_batch_decode_async; median (min-max).  Every decode's statuses are checked and every side's
bytes compared with the records; a step that fails ends the script.  Appends one JSON line per comparison.
usage: python scripts/time_chain.py OUT.jsonl [--parent LIB] [--reps 9] [--scale F] [--unique N]"""
import argparse
import concurrent.futures as cf
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

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--parent", help="libzd.so of the parent commit (side B on it too)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of the 8,192 chains")
ap.add_argument("--unique", type=int, default=2048, help="distinct chains compressed; the rest repeat them")
args = ap.parse_args()
WARMUP, PAGE, DEPTH = 2, 16 << 10, 4
dev = torch.device("cuda", 0)
vpp = C.POINTER(C.c_void_p)


def load(path):
    L = C.CDLL(path)
    for name, (res, argt) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, argt
    return L


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def u64(v):
    return (C.c_uint64 * len(v))(*v)


def upload(b):
    t = torch.empty(len(b) + 64, dtype=torch.uint8, device=dev)
    t[: len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return t


def chains(nu):
    """nu seeded base pages (time_prefix.py's generator) and DEPTH versions of each, every version its predecessor
    with 1 % of the bytes edited: (bases, versions[level][chain], frames[level][chain])."""
    text = gen.text(nu * PAGE + PAGE, seed=0x9A6E0)
    rng = np.random.default_rng(0x9A6E1)
    bases = [text[i * PAGE:(i + 1) * PAGE] for i in range(nu)]
    vers, prev = [], bases
    for _ in range(DEPTH):
        cur = []
        for o in prev:
            b = bytearray(o)
            for p in rng.choice(PAGE, PAGE // 100, replace=False):
                b[p] ^= int(rng.integers(1, 256))
            cur.append(bytes(b))
        vers.append(cur)
        prev = cur
    with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:      # ctypes drops the GIL
        frames = [list(ex.map(lambda i, l=l: zdict.prefix_compress(vers[l][i], (bases if l == 0 else vers[l - 1])[i], 3),
                              range(nu), chunksize=32)) for l in range(DEPTH)]
    return bases, vers, frames


class Work:
    """The workload on the device: n chains, chunk (level l, chain c) is chunk l * n + c."""

    def __init__(self, n, nu):
        self.n, self.nu = n, nu
        self.bases, self.vers, frames = chains(nu)
        rep = (n + nu - 1) // nu
        flat = [f for l in range(DEPTH) for f in (frames[l] * rep)[:n]]
        self.src = upload(b"".join(flat))
        self.sizes = [len(f) for f in flat]
        self.so = np.cumsum([0] + self.sizes)
        self.base = upload(b"".join(self.bases))[: nu * PAGE].repeat(rep)[: n * PAGE].contiguous()   # every chain its own base
        self.compressed = sum(self.sizes)

    def record(self, i):
        return self.vers[i // self.n][(i % self.n) % self.nu]


class Side:
    """One way of decoding the workload with library L into its own output tensor."""

    def __init__(self, L, W, levels):
        self.L, self.W, self.levels = L, W, levels
        self.dst = torch.zeros(levels * W.n * PAGE + 64, dtype=torch.uint8, device=dev)
        self.create_ms, self.decode_ms, self.create_each = [], [], []
        self.kept = {}

    def arrays(self, l0, l1, prefix_of):
        """the six host arrays of levels [l0, l1) (built once, kept)"""
        if (l0, l1) not in self.kept:
            self.kept[(l0, l1)] = self.build(l0, l1, prefix_of)
        return self.kept[(l0, l1)]

    def build(self, l0, l1, prefix_of):
        W, n = self.W, self.W.n
        idx = range(l0 * n, l1 * n)
        sp = u64([W.src.data_ptr() + int(W.so[i]) for i in idx])
        ss = u64([W.sizes[i] for i in idx])
        dp = u64([self.dst.data_ptr() + i * PAGE for i in idx])
        dc = u64([PAGE] * len(idx))
        pp = u64([prefix_of(i) for i in idx])
        ps = u64([PAGE if prefix_of(i) else 0 for i in idx])
        return sp, ss, dp, dc, pp, ps, len(idx)

    def decode(self, h):
        s = torch.cuda.current_stream(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        _lib.check(self.L.zd_batch_decode_async(h, C.c_void_p(s.cuda_stream)), "zd_batch_decode_async")
        e1.record(s)
        e1.synchronize()
        bad = C.c_uint64()
        _lib.check(self.L.zd_batch_results(h, C.c_void_p(s.cuda_stream), None, None, 0, C.byref(bad)))
        if bad.value:
            raise SystemExit(f"{bad.value} chunks failed")
        return e0.elapsed_time(e1)

    def check(self):
        """the first and last 64 chunks' bytes and a digest of everything"""
        total = self.levels * self.W.n
        out = self.dst[: total * PAGE].cpu().numpy()
        for i in list(range(min(64, total))) + list(range(max(0, total - 64), total)):
            if bytes(out[i * PAGE:(i + 1) * PAGE]) != self.W.record(i):
                raise SystemExit(f"chunk {i} differs from its record")
        return int(out.sum(dtype=np.uint64))


class ChainSide(Side):
    """(A) one chain batch over levels x n chunks, or (C) with levels = 1 a chain batch without links."""

    def run(self, timed):
        W, n = self.W, self.W.n
        base_of = lambda i: W.base.data_ptr() + i * PAGE if i < n else 0
        sp, ss, dp, dc, pp, ps, m = self.arrays(0, self.levels, base_of)
        if "par" not in self.kept:
            self.kept["par"] = (C.c_int64 * m)(*[i - n if i >= n else -1 for i in range(m)])
        par = self.kept["par"]
        h = C.c_void_p()
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        _lib.check(self.L.zd_batch_create_chain(C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, C.cast(pp, vpp), ps, par, m, 0,
                                                s, C.byref(h)), "zd_batch_create_chain")
        t1 = time.perf_counter()
        ms = self.decode(h)
        self.L.zd_batch_destroy(h)
        if timed:
            self.create_ms.append((t1 - t0) * 1e3)
            self.decode_ms.append(ms)


class LinkSide(Side):
    """(B) one prefix batch per level, created and decoded one after another; (C) with levels = 1 one prefix batch."""

    def run(self, timed):
        W, n = self.W, self.W.n
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        create, decode = [], 0.0
        for l in range(self.levels):
            pre = (lambda i: W.base.data_ptr() + i * PAGE) if l == 0 else (lambda i: self.dst.data_ptr() + (i - n) * PAGE)
            sp, ss, dp, dc, pp, ps, m = self.arrays(l, l + 1, pre)
            h = C.c_void_p()
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            _lib.check(self.L.zd_batch_create_prefix(C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, C.cast(pp, vpp), ps, m, 0,
                                                     s, C.byref(h)), "zd_batch_create_prefix")
            create.append((time.perf_counter() - t0) * 1e3)
            decode += self.decode(h)
            self.L.zd_batch_destroy(h)
        if timed:
            self.create_ms.append(sum(create))
            self.create_each.append(statistics.median(create))
            self.decode_ms.append(decode)


def race(sides):
    keys = list(sides)
    for rep in range(WARMUP + args.reps):
        for k in keys[rep % len(keys):] + keys[:rep % len(keys)]:
            sides[k].dst.zero_()
            sides[k].run(rep >= WARMUP)
    sums = {k: s.check() for k, s in sides.items()}
    if len(set(sums.values())) != 1:
        raise SystemExit(f"the sides' outputs differ: {sums}")
    res = {}
    for k, s in sides.items():
        res[k] = {"create_ms": stats(s.create_ms), "decode_ms": stats(s.decode_ms)}
        if s.create_each:
            res[k]["one_creation_ms"] = stats(s.create_each)
    return res


def emit(res):
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def main():
    L = _lib.lib()
    LP = load(args.parent) if args.parent else None
    n = max(1, int(8192 * args.scale))
    W = Work(n, min(n, args.unique))
    common = {"chains": n, "depth": DEPTH, "chunks": DEPTH * n, "decoded_bytes": DEPTH * n * PAGE,
              "compressed_bytes": W.compressed, "reps": args.reps, "warmup": WARMUP}
    sides = {"A_one_chain_batch": ChainSide(L, W, DEPTH), "B_four_prefix_batches": LinkSide(L, W, DEPTH)}
    if LP:
        sides["B_four_prefix_batches_parent_build"] = LinkSide(LP, W, DEPTH)
    ms = race(sides)
    a, b = ms["A_one_chain_batch"], ms["B_four_prefix_batches"]
    out = {"comparison": f"A/B: {n} chains of depth {DEPTH}, 16 KiB pages, 1 % edited per version: one chain batch / "
                         "four prefix batches one after another", **common, "ms": ms,
           "expectation": "A decode below B's four decodes (K1-K3 once at four times the width); A's creation about one "
                          "of B's four",
           "A_over_B_decode": round(a["decode_ms"]["median"] / b["decode_ms"]["median"], 4),
           "A_over_B_create": round(a["create_ms"]["median"] / b["create_ms"]["median"], 4),
           "A_create_over_one_B_creation": round(a["create_ms"]["median"] / b["one_creation_ms"]["median"], 4),
           "A_decoded_gbps": round(DEPTH * n * PAGE / a["decode_ms"]["median"] / 1e6, 1),
           "B_decoded_gbps": round(DEPTH * n * PAGE / b["decode_ms"]["median"] / 1e6, 1)}
    if LP:
        p = ms["B_four_prefix_batches_parent_build"]
        out["B_new_over_parent_decode"] = round(b["decode_ms"]["median"] / p["decode_ms"]["median"], 4)
    emit(out)
    del sides
    ms = race({"C_chain_batch_no_links": ChainSide(L, W, 1), "C_prefix_batch": LinkSide(L, W, 1)})
    c, p = ms["C_chain_batch_no_links"], ms["C_prefix_batch"]
    emit({"comparison": f"C: the {n} first-level chunks: a chain batch with every parent -1 / the prefix batch",
          "chunks": n, "decoded_bytes": n * PAGE, "reps": args.reps, "warmup": WARMUP, "ms": ms,
          "expectation": "within each side's min-max",
          "chain_over_prefix_decode": round(c["decode_ms"]["median"] / p["decode_ms"]["median"], 4),
          "chain_over_prefix_create": round(c["create_ms"]["median"] / p["create_ms"]["median"], 4)})


if __name__ == "__main__":
    main()
