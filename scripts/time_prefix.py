"""Times prefix batches (zd_batch_create_prefix, zd_k_execute_prefix):
  (a) variant   8,192 chunks of 16 KiB whose prefixes are 8,192 COPIES of one 16 KiB buffer, through the
                prefix batch, against the same frames through a batch with that one buffer as a raw-content
                dictionary: the per-chunk pointer, the exact-bounds edges, and 128 MiB of distinct prefix
                lines against one cache-resident 16 KiB
  (b) deltas    16 KiB pages with 1 % of their bytes edited, each against its own old page, at 8,192 and
                65,536 pages: decode ms, decoded GB/s, compressed bytes; beside them the same pages compressed
                alone, in a plain batch
  (c) parent    the README's two batch workloads (8,192 x 128 KiB frames; 65,536 x 4 KiB records with a
                112 KiB dictionary) on this build against --parent (the parent commit's library)
Every side is a library file loaded into this one process, the sides of a comparison alternate inside every
repetition, --reps repetitions after warm-up, min / median / max between device events around
zd_batch_decode_async.  Every decode's statuses are checked and every side's bytes compared with the records;
a step that fails ends the script.  Appends one JSON line per comparison to the output file.
usage: python scripts/time_prefix.py OUT.jsonl [--parent LIB] [--reps 9] [--scale F] [--only a|b|c]"""
import argparse
import concurrent.futures as cf
import ctypes as C
import functools
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
ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's chunk count")
ap.add_argument("--unique", type=int, default=4096, help="distinct pages / records compressed; the rest repeat them")
ap.add_argument("--only", choices=("a", "b", "c"))
args = ap.parse_args()
WARMUP = 2
PAGE = 16 << 10
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


def compress_all(items, fn):
    with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:      # ctypes drops the GIL
        return list(ex.map(fn, items, chunksize=32))


def upload(b):
    t = torch.empty(len(b) + 64, dtype=torch.uint8, device=dev)
    t[: len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return t


def upload_repeated(b, times, total):
    """`b` repeated on the device, cut to `total` bytes"""
    t = upload(b)[: len(b)].repeat(times)
    return t[:total] if total <= t.numel() else t


def u64(v):
    return (C.c_uint64 * len(v))(*v)


class Side:
    """One batch of library L over frames in one device tensor, the outputs packed in another."""

    def __init__(self, L, frames, sizes, prefix=None, dictionary=None):
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
            _lib.check(L.zd_batch_create_prefix(C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, C.cast(pp, vpp), ps, n, 0, s,
                                                C.byref(self.h)), "zd_batch_create_prefix")
        else:
            if dictionary is not None:
                p, m, self.dkeep = _lib.buf(dictionary)
                _lib.check(L.zd_dict_create(p, m, C.byref(self.d)), "zd_dict_create")
            _lib.check(L.zd_batch_create(C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, n, 0, self.d, s, C.byref(self.h)),
                       "zd_batch_create")
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
    for s in sides.values():
        s.close()
    return res


def emit(res):
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def edited_pages(nu, seed):
    """nu seeded text pages and each with 1 % of its bytes edited"""
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


@functools.lru_cache(maxsize=None)
def page_frames(nu):
    old, new = edited_pages(nu, 0x9A6E0)
    dframes = compress_all(list(range(nu)), lambda i: zdict.prefix_compress(new[i], old[i], 3))
    aframes = compress_all(new, lambda r: libzstd.compress(r, 3))
    return old, new, dframes, aframes


def variant(L):
    n = max(1, int(8192 * args.scale))
    nu = min(n, args.unique)
    base = gen.text(2 * PAGE, seed=0xA11CE)[:PAGE]
    rng = np.random.default_rng(0xA11CF)
    news = []
    for _ in range(nu):
        b = bytearray(base)
        for p in rng.choice(PAGE, PAGE // 100, replace=False):
            b[p] ^= int(rng.integers(1, 256))
        news.append(bytes(b))
    frames = compress_all(news, lambda r: zdict.prefix_compress(r, base, 3))
    frames = (frames * ((n + nu - 1) // nu))[:n]
    copies = upload_repeated(base, n, n * PAGE)                   # n copies: every chunk its own 16 KiB of lines
    prefix = ([copies.data_ptr() + i * PAGE for i in range(n)], [PAGE] * n)
    sides = {"prefix_batch": Side(L, frames, [PAGE] * n, prefix=prefix),
             "raw_dictionary_batch": Side(L, frames, [PAGE] * n, dictionary=base)}
    ms = race(sides, lambda i: news[i % nu])
    a, b = ms["prefix_batch"]["median"], ms["raw_dictionary_batch"]["median"]
    emit({"comparison": "a: 8192 x 16 KiB, prefixes = copies of one buffer, against that buffer as a raw dictionary",
          "chunks": n, "compressed_bytes": sum(map(len, frames)), "decoded_bytes": n * PAGE, "prefix_bytes": n * PAGE,
          "reps": args.reps, "warmup": WARMUP, "ms": ms, "prefix_over_dictionary": round(a / b, 4),
          "prefix_decoded_gbps": round(n * PAGE / a / 1e6, 1), "dictionary_decoded_gbps": round(n * PAGE / b / 1e6, 1)})


def deltas(L, pages):
    n = max(1, int(pages * args.scale))
    nu = min(n, args.unique)
    old, new, dframes, aframes = page_frames(nu)
    rep = (n + nu - 1) // nu
    d_old = upload_repeated(b"".join(old), rep, n * PAGE)         # every chunk its own old page
    prefix = ([d_old.data_ptr() + i * PAGE for i in range(n)], [PAGE] * n)
    sides = {"page_deltas_prefix_batch": Side(L, (dframes * rep)[:n], [PAGE] * n, prefix=prefix),
             "pages_alone_plain_batch": Side(L, (aframes * rep)[:n], [PAGE] * n)}
    ms = race(sides, lambda i: new[i % nu])
    a, b = ms["page_deltas_prefix_batch"]["median"], ms["pages_alone_plain_batch"]["median"]
    emit({"comparison": f"b: {n} pages of 16 KiB, 1 % edited: deltas against the old pages / the pages alone",
          "chunks": n, "decoded_bytes": n * PAGE, "prefix_bytes": n * PAGE,
          "delta_compressed_bytes": sum(map(len, (dframes * rep)[:n])),
          "alone_compressed_bytes": sum(map(len, (aframes * rep)[:n])), "reps": args.reps, "warmup": WARMUP, "ms": ms,
          "delta_decoded_gbps": round(n * PAGE / a / 1e6, 1), "alone_decoded_gbps": round(n * PAGE / b / 1e6, 1)})


def parent(L, LP):
    chunk, n = 128 << 10, max(1, int(8192 * args.scale))
    nu = min(n, max(1, args.unique // 8))
    text = gen.text(nu * chunk, seed=0xBA7C0)
    recs = [text[i:i + chunk] for i in range(0, nu * chunk, chunk)]
    frames = (compress_all(recs, lambda r: libzstd.compress(r, 3)) * ((n + nu - 1) // nu))[:n]
    ms = race({"new": Side(L, frames, [chunk] * n), "parent": Side(LP, frames, [chunk] * n)}, lambda i: recs[i % nu])
    emit({"comparison": "c: plain batch, 8192 x 128 KiB frames, zstd -3: this build against the parent commit's",
          "chunks": n, "decoded_bytes": n * chunk, "reps": args.reps, "warmup": WARMUP, "ms": ms,
          "new_over_parent": round(ms["new"]["median"] / ms["parent"]["median"], 4)})
    rec, n = 4096, max(1, int(65536 * args.scale))
    train = gen.text(2048 * rec, seed=0xD1C2)
    dct = zdict.train([train[i:i + rec] for i in range(0, len(train), rec)], 112 << 10)
    nu = min(n, args.unique * 4)
    text = gen.text(nu * rec, seed=0xD1C5)
    recs = [text[i:i + rec] for i in range(0, nu * rec, rec)]
    frames = (compress_all(recs, lambda r: zdict.compress(r, dct, 3)) * ((n + nu - 1) // nu))[:n]
    ms = race({"new": Side(L, frames, [rec] * n, dictionary=dct), "parent": Side(LP, frames, [rec] * n, dictionary=dct)},
              lambda i: recs[i % nu])
    emit({"comparison": "c: dictionary batch, 65536 x 4 KiB records, 112 KiB dictionary: this build against the parent's",
          "chunks": n, "decoded_bytes": n * rec, "reps": args.reps, "warmup": WARMUP, "ms": ms,
          "new_over_parent": round(ms["new"]["median"] / ms["parent"]["median"], 4)})


def main():
    L = _lib.lib()
    if args.only in (None, "a"):
        variant(L)
    if args.only in (None, "b"):
        deltas(L, 8192)
        deltas(L, 65536)
    if args.only in (None, "c"):
        if not args.parent:
            raise SystemExit("comparison c needs --parent LIB")
        parent(L, load(args.parent))


if __name__ == "__main__":
    main()
