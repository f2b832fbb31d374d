"""Times prefix batches on the block-parallel executor (ZD_F_BLOCK_PARALLEL on zd_batch_create_prefix: K4J with
zd_k_jscatter<true>) against the streaming one (zd_k_execute_prefix), and this build against the parent commit's:
  (a) big       one 100 MB text delta (1 % of the bytes edited, compressed against its old version with a
                128 MiB window, as `zstd --patch-from` does: ZD_F_LONG_WINDOW on both sides), flagged against
                unflagged on this build
  (b) pages     8,192 page deltas of 16 KiB (1 % edited), flagged against unflagged on this build
  (c) parent    this build against --parent (the parent commit's library) where nothing was asked for: the
                unflagged page deltas, the plain and the dictionary batch of scripts/time_prefix.py, and one
                prefix-less 100 MB frame on K4J (its zd_k_jscatter<false> must be the parent's kernel)
Every side is a library file loaded into this one process, the sides of a comparison alternate inside every
repetition, --reps repetitions after warm-up, min / median / max between device events around
zd_batch_decode_async.  Every decode's statuses are checked and every side's bytes compared with the records;
a step that fails ends the script.  `within` is the project's criterion: each side's median inside the other
side's min-max.  Appends one JSON line per comparison to the output file.
usage: python scripts/time_prefix_big.py OUT.jsonl --parent LIB [--reps 9] [--scale F] [--only a|b|c]"""
import argparse
import concurrent.futures as cf
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zstd-decompressor_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corpus import gen, libzstd, zdict  # noqa: E402
from zstd_decompressor import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--parent", help="libzd.so of the parent commit (comparison c)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's size")
ap.add_argument("--unique", type=int, default=4096, help="distinct pages / records compressed; the rest repeat them")
ap.add_argument("--only", choices=("a", "b", "c"))
args = ap.parse_args()
WARMUP = 2
PAGE = 16 << 10
BIG = 100_000_000
F_LONG_WINDOW = getattr(_lib, "F_LONG_WINDOW", 2048)
ZSTD_c_windowLog, ZSTD_c_enableLongDistanceMatching = 101, 160
dev = torch.device("cuda", 0)


def load(path):
    L = C.CDLL(path)
    for name, (res, argt) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, argt
    return L


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def within(a, b):
    return bool(b["min"] <= a["median"] <= b["max"] and a["min"] <= b["median"] <= a["max"])


def compress_all(items, fn):
    with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:      # ctypes drops the GIL
        return list(ex.map(fn, items, chunksize=32))


def patch_compress(data, prefix, level, window_log):
    """zdict.prefix_compress with the window `zstd --patch-from` sets (one that covers the old file) and its
    long-distance matcher"""
    L = zdict.lib()
    cap = L.ZSTD_compressBound(len(data))
    dst = C.create_string_buffer(cap)
    cctx = L.ZSTD_createCCtx()
    try:
        libzstd._chk(L.ZSTD_CCtx_setParameter(cctx, libzstd.ZSTD_c_compressionLevel, level))
        libzstd._chk(L.ZSTD_CCtx_setParameter(cctx, ZSTD_c_windowLog, window_log))
        libzstd._chk(L.ZSTD_CCtx_setParameter(cctx, ZSTD_c_enableLongDistanceMatching, 1))
        libzstd._chk(L.ZSTD_CCtx_refPrefix(cctx, prefix, len(prefix)))
        n = libzstd._chk(L.ZSTD_compress2(cctx, dst, cap, data, len(data)))
    finally:
        L.ZSTD_freeCCtx(cctx)
    return dst.raw[:n]


def upload(b):
    t = torch.empty(len(b) + 64, dtype=torch.uint8, device=dev)
    t[: len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return t


def upload_repeated(b, times, total):
    t = upload(b)[: len(b)].repeat(times)
    return t[:total] if total <= t.numel() else t


def u64(v):
    return (C.c_uint64 * len(v))(*v)


class Side:
    """One batch of library L over frames in one device tensor, the outputs packed in another."""

    def __init__(self, L, frames, sizes, prefix=None, dictionary=None, flags=0):
        self.L, n = L, len(frames)
        self.n, self.sizes = n, sizes
        self.src = upload(b"".join(frames))
        self.dst = torch.zeros(sum(sizes) + 64, dtype=torch.uint8, device=dev)
        so, do = np.cumsum([0] + [len(f) for f in frames]), np.cumsum([0] + list(sizes))
        self.do = do
        vpp = C.POINTER(C.c_void_p)
        sp, ss = u64([self.src.data_ptr() + int(o) for o in so[:-1]]), u64([len(f) for f in frames])
        dp, dc = u64([self.dst.data_ptr() + int(o) for o in do[:-1]]), u64(list(sizes))
        self.h, self.d = C.c_void_p(), C.c_void_p()
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        if prefix is not None:
            pp, ps = u64(prefix[0]), u64(prefix[1])
            _lib.check(L.zd_batch_create_prefix(C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, C.cast(pp, vpp), ps, n, flags,
                                                s, C.byref(self.h)), "zd_batch_create_prefix")
        else:
            if dictionary is not None:
                p, m, self.dkeep = _lib.buf(dictionary)
                _lib.check(L.zd_dict_create(p, m, C.byref(self.d)), "zd_dict_create")
            _lib.check(L.zd_batch_create(C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, n, flags, self.d, s,
                                         C.byref(self.h)), "zd_batch_create")
        info = _lib.BatchInfoEx()
        _lib.check(L.zd_batch_info_get_sized(self.h, C.byref(info), C.sizeof(info)), "zd_batch_info_get_sized")
        self.executors = int(info.executors)
        self.ms = []

    def decode(self, timed):
        s = torch.cuda.current_stream(dev)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        _lib.check(self.L.zd_batch_decode_async(self.h, C.c_void_p(s.cuda_stream)), "zd_batch_decode_async")
        e1.record(s)
        e1.synchronize()
        bad = C.c_uint64()
        _lib.check(self.L.zd_batch_results(self.h, C.c_void_p(s.cuda_stream), None, None, 0, C.byref(bad)))
        if bad.value:
            raise SystemExit(f"{bad.value} chunks failed")
        if timed:
            self.ms.append(e0.elapsed_time(e1))

    def check(self, records):
        """the first and last 64 chunks' bytes, and a digest of everything, against the records"""
        out = self.dst[: int(self.do[-1])].cpu().numpy()
        for i in list(range(min(64, self.n))) + list(range(max(0, self.n - 64), self.n)):
            if bytes(out[int(self.do[i]):int(self.do[i + 1])]) != records(i):
                raise SystemExit(f"chunk {i} differs from its record")
        return int(out.sum(dtype=np.uint64))

    def close(self):
        self.L.zd_batch_destroy(self.h)
        if self.d:
            self.L.zd_dict_destroy(self.d)


def race(sides, records):
    """The sides alternating, the order rotated every repetition; their outputs' digests must agree."""
    keys = list(sides)
    for rep in range(WARMUP + args.reps):
        for k in keys[rep % len(keys):] + keys[:rep % len(keys)]:
            sides[k].decode(rep >= WARMUP)
    sums = {k: s.check(records) for k, s in sides.items()}
    if len(set(sums.values())) != 1:
        raise SystemExit(f"the sides' outputs differ: {sums}")
    res = {k: stats(s.ms) for k, s in sides.items()}
    ex = {k: s.executors for k, s in sides.items()}
    for s in sides.values():
        s.close()
    return res, ex


def emit(res):
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def versus(name, ms, ex, a, b, extra):
    res = {"comparison": name, "reps": args.reps, "warmup": WARMUP, "ms": ms, "executors": ex,
           f"{a}_over_{b}": round(ms[a]["median"] / ms[b]["median"], 4), "within": within(ms[a], ms[b])}
    res.update(extra)
    emit(res)


_big = {}


def big_pair():
    if not _big:
        n = max(1 << 20, int(BIG * args.scale))
        old = gen.text(n, seed=0xB160)
        new = bytearray(old)
        rng = np.random.default_rng(0xB161)
        at = rng.choice(n, n // 100, replace=False)
        arr = np.frombuffer(new, dtype=np.uint8)
        arr[at] ^= rng.integers(1, 256, len(at), dtype=np.uint8)
        _big.update(old=old, new=bytes(new))
    return _big["old"], _big["new"]


def big(L):
    old, new = big_pair()
    n = len(new)
    wlog = max(21, (max(len(old), n) - 1).bit_length())
    frame = patch_compress(new, old, 3, wlog)
    if zdict.prefix_decompress(frame, old, n) != new:
        raise SystemExit("libzstd does not return the record")
    d_old = upload(old)
    prefix = ([d_old.data_ptr()], [len(old)])
    sides = {"flagged": Side(L, [frame], [n], prefix=prefix, flags=_lib.F_BLOCK_PARALLEL | F_LONG_WINDOW),
             "unflagged": Side(L, [frame], [n], prefix=prefix, flags=F_LONG_WINDOW)}
    ms, ex = race(sides, lambda i: new)
    a, b = ms["flagged"]["median"], ms["unflagged"]["median"]
    versus(f"a: one {n} byte text delta, 1 % edited, against its old version: ZD_F_BLOCK_PARALLEL / streaming",
           ms, ex, "flagged", "unflagged",
           {"compressed_bytes": len(frame), "decoded_bytes": n, "prefix_bytes": len(old), "window_log": wlog,
            "flagged_decoded_gbps": round(n / a / 1e6, 2), "unflagged_decoded_gbps": round(n / b / 1e6, 2)})


def edited_pages(nu, seed):
    text = gen.text(nu * PAGE + PAGE, seed=seed)
    rng = np.random.default_rng(seed + 1)
    old, new = [], []
    for i in range(nu):
        o = text[i * PAGE:(i + 1) * PAGE]
        b = bytearray(o)
        for p in rng.choice(PAGE, PAGE // 100, replace=False):
            b[p] ^= int(rng.integers(1, 256))
        old.append(o)
        new.append(bytes(b))
    return old, new


_pages = {}


def page_sides(L, LB, fa, fb):
    n = max(1, int(8192 * args.scale))
    nu = min(n, args.unique)
    if not _pages:
        old, new = edited_pages(nu, 0x9A6E0)
        _pages.update(old=old, new=new,
                      frames=compress_all(list(range(nu)), lambda i: zdict.prefix_compress(new[i], old[i], 3)))
    old, new, frames = _pages["old"], _pages["new"], _pages["frames"]
    rep = (n + nu - 1) // nu
    d_old = upload_repeated(b"".join(old), rep, n * PAGE)
    prefix = ([d_old.data_ptr() + i * PAGE for i in range(n)], [PAGE] * n)
    a = Side(L, (frames * rep)[:n], [PAGE] * n, prefix=prefix, flags=fa)
    b = Side(LB, (frames * rep)[:n], [PAGE] * n, prefix=prefix, flags=fb)
    return n, a, b, (lambda i: new[i % nu]), d_old


def pages(L):
    n, a, b, recs, keep = page_sides(L, L, _lib.F_BLOCK_PARALLEL, 0)
    ms, ex = race({"flagged": a, "unflagged": b}, recs)
    versus(f"b: {n} page deltas of 16 KiB, 1 % edited: ZD_F_BLOCK_PARALLEL / streaming", ms, ex, "flagged", "unflagged",
           {"chunks": n, "decoded_bytes": n * PAGE,
            "flagged_decoded_gbps": round(n * PAGE / ms["flagged"]["median"] / 1e6, 1),
            "unflagged_decoded_gbps": round(n * PAGE / ms["unflagged"]["median"] / 1e6, 1)})


def parent(L, LP):
    n, a, b, recs, keep = page_sides(L, LP, 0, 0)
    ms, ex = race({"new": a, "parent": b}, recs)
    versus(f"c: {n} page deltas, unflagged prefix batch: this build against the parent commit's", ms, ex, "new",
           "parent", {"chunks": n, "decoded_bytes": n * PAGE})
    del keep
    chunk, n = 128 << 10, max(1, int(8192 * args.scale))
    nu = min(n, max(1, args.unique // 8))
    text = gen.text(nu * chunk, seed=0xBA7C0)
    recs = [text[i:i + chunk] for i in range(0, nu * chunk, chunk)]
    frames = (compress_all(recs, lambda r: libzstd.compress(r, 3)) * ((n + nu - 1) // nu))[:n]
    ms, ex = race({"new": Side(L, frames, [chunk] * n), "parent": Side(LP, frames, [chunk] * n)}, lambda i: recs[i % nu])
    versus("c: plain batch, 8192 x 128 KiB frames, zstd -3: this build against the parent commit's", ms, ex, "new",
           "parent", {"chunks": n, "decoded_bytes": n * chunk})
    rec, n = 4096, max(1, int(65536 * args.scale))
    train = gen.text(2048 * rec, seed=0xD1C2)
    dct = zdict.train([train[i:i + rec] for i in range(0, len(train), rec)], 112 << 10)
    nu = min(n, args.unique * 4)
    text = gen.text(nu * rec, seed=0xD1C5)
    recs = [text[i:i + rec] for i in range(0, nu * rec, rec)]
    frames = (compress_all(recs, lambda r: zdict.compress(r, dct, 3)) * ((n + nu - 1) // nu))[:n]
    ms, ex = race({"new": Side(L, frames, [rec] * n, dictionary=dct),
                   "parent": Side(LP, frames, [rec] * n, dictionary=dct)}, lambda i: recs[i % nu])
    versus("c: dictionary batch, 65536 x 4 KiB records, 112 KiB dictionary: this build against the parent's", ms, ex,
           "new", "parent", {"chunks": n, "decoded_bytes": n * rec})
    # the prefix-less frame on K4J: its scatter now has a template argument
    old, new = big_pair()
    frame = libzstd.compress(new, 3)
    ms, ex = race({"new": Side(L, [frame], [len(new)], flags=_lib.F_BLOCK_PARALLEL),
                   "parent": Side(LP, [frame], [len(new)], flags=_lib.F_BLOCK_PARALLEL)}, lambda i: new)
    versus(f"c: one prefix-less {len(new)} byte frame on K4J: this build against the parent commit's", ms, ex, "new",
           "parent", {"decoded_bytes": len(new), "new_decoded_gbps": round(len(new) / ms["new"]["median"] / 1e6, 2)})


def main():
    L = _lib.lib()
    if args.only in (None, "a"):
        big(L)
    if args.only in (None, "b"):
        pages(L)
    if args.only in (None, "c"):
        if not args.parent:
            raise SystemExit("comparison c needs --parent LIB")
        parent(L, load(args.parent))


if __name__ == "__main__":
    main()
