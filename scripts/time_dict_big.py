"""Times dictionary batches on the block-parallel executor (ZD_F_DICT_BLOCK_PARALLEL: K4J with
zd_k_jscatter<true, false, true>) against the streaming one (zd_k_execute_dict), and this build against the parent
commit's where nothing was asked for:
  (a) big       one 100 MB text frame compressed with a 112 KiB trained dictionary: flag | ZD_F_BLOCK_PARALLEL
                against unflagged on this build
  (b) tail      65,536 records of 4 KiB and four records of 8 MiB in one dictionary batch: the flag alone (the
                ZD_AUTO_* rule), flag | ZD_F_BLOCK_PARALLEL, and unflagged
  (c) grid      N frames x B blocks of 128 KiB, N in 64, 256, 1,024 and B in 2, 4, 16: forced K4J, forced streaming
                (flag | ZD_F_FRAME_SERIAL) and the rule; `auto_outside_better` names the points where the rule's
                median lies outside the better forced side's min-max
  (d) parent    this build against --parent (the parent commit's library) on routes the flag does not touch: the
                unflagged dictionary batch (65,536 x 4 KiB), a plain batch, a prefix batch with
                ZD_F_BLOCK_PARALLEL, one prefix-less 100 MB frame on K4J
Every side is a library file loaded into this one process, the sides of a comparison alternate inside every
repetition, --reps repetitions after warm-up, min / median / max between device events around
zd_batch_decode_async.  Every decode's statuses are checked and every side's bytes compared with the records;
a step that fails ends the script.  `within`: each side's median inside the other side's min-max.  Appends one
JSON line per comparison to the output file.
usage: python scripts/time_dict_big.py OUT.jsonl --parent LIB [--reps 9] [--scale F] [--only a|b|c|d]
       [--frames 64,256,1024] [--blocks 2,4,16]"""
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
ap.add_argument("--parent", help="libzd.so of the parent commit (comparison d)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's size")
ap.add_argument("--unique", type=int, default=4096, help="distinct records compressed; the rest repeat them")
ap.add_argument("--only", choices=("a", "b", "c", "d"))
ap.add_argument("--frames", default="64,256,1024", help="comparison c: the frame counts N")
ap.add_argument("--blocks", default="2,4,16", help="comparison c: the block counts B")
args = ap.parse_args()
WARMUP = 2
REC, BLOCK, PAGE = 4096, 128 << 10, 16 << 10
BIG = 100_000_000
DJ, BP, FS = _lib.F_DICT_BLOCK_PARALLEL, _lib.F_BLOCK_PARALLEL, _lib.F_FRAME_SERIAL
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
        return list(ex.map(fn, items, chunksize=8))


def upload(b):
    t = torch.empty(len(b) + 64, dtype=torch.uint8, device=dev)
    t[: len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return t


def u64(v):
    return (C.c_uint64 * len(v))(*v)


_dict = {}


def dictionary():
    if not _dict:
        train = gen.text(2048 * REC, seed=0xD1C2)
        _dict["d"] = zdict.train([train[i:i + REC] for i in range(0, len(train), REC)], 112 << 10)
    return _dict["d"]


class Side:
    """One batch of library L over frames in one device tensor, the outputs packed in another."""

    def __init__(self, L, frames, sizes, prefix=None, dct=None, flags=0):
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
            if dct is not None:
                p, m, self.dkeep = _lib.buf(dct)
                _lib.check(L.zd_dict_create(p, m, C.byref(self.d)), "zd_dict_create")
            _lib.check(L.zd_batch_create(C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, n, flags, self.d, s,
                                         C.byref(self.h)), "zd_batch_create")
        info = _lib.BatchInfo2()
        _lib.check(L.zd_batch_info_get_sized(self.h, C.byref(info), C.sizeof(info)), "zd_batch_info_get_sized")
        self.executors, self.k4j_chunks = int(info.executors), int(info.k4j_chunks)
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
        self.src = self.dst = None


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
    kj = {k: s.k4j_chunks for k, s in sides.items()}
    for s in sides.values():
        s.close()
    torch.cuda.empty_cache()
    return res, ex, kj


def emit(res):
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def versus(name, ms, ex, kj, a, b, extra):
    res = {"comparison": name, "reps": args.reps, "warmup": WARMUP, "ms": ms, "executors": ex, "k4j_chunks": kj,
           f"{a}_over_{b}": round(ms[a]["median"] / ms[b]["median"], 4), "within": within(ms[a], ms[b])}
    res.update(extra)
    emit(res)


_big = {}


def big_text():
    if not _big:
        _big["t"] = gen.text(max(1 << 20, int(BIG * args.scale)), seed=0xB160)
    return _big["t"]


def big(L):
    dct, rec = dictionary(), big_text()
    n = len(rec)
    frame = zdict.compress(rec, dct, 3)
    sides = {"flagged": Side(L, [frame], [n], dct=dct, flags=DJ | BP), "unflagged": Side(L, [frame], [n], dct=dct)}
    ms, ex, kj = race(sides, lambda i: rec)
    a, b = ms["flagged"]["median"], ms["unflagged"]["median"]
    versus(f"a: one {n} byte text frame behind a {len(dct)} byte dictionary: flag | ZD_F_BLOCK_PARALLEL / unflagged",
           ms, ex, kj, "flagged", "unflagged",
           {"compressed_bytes": len(frame), "decoded_bytes": n,
            "flagged_decoded_gbps": round(n / a / 1e6, 2), "unflagged_decoded_gbps": round(n / b / 1e6, 2)})


_recs = {}


def small_records(n):
    """n records of 4 KiB (the distinct ones compressed once) with the dictionary: (frames, record of chunk i)"""
    nu = min(n, args.unique * 4)
    if _recs.get("nu") != nu:
        text = gen.text(nu * REC, seed=0xD1C5)
        recs = [text[i:i + REC] for i in range(0, nu * REC, REC)]
        dct = dictionary()
        _recs.update(nu=nu, recs=recs, frames=compress_all(recs, lambda r: zdict.compress(r, dct, 3)))
    recs, frames = _recs["recs"], _recs["frames"]
    return (frames * ((n + nu - 1) // nu))[:n], (lambda i: recs[i % nu])


def tail(L):
    dct = dictionary()
    n = max(1, int(65536 * args.scale))
    frames, rec_of = small_records(n)
    bigs = [gen.text(max(BLOCK, int((8 << 20) * args.scale)), seed=0x8B16 + k) for k in range(4)]
    bframes = compress_all(bigs, lambda r: zdict.compress(r, dct, 3))
    # the large records spread through the batch
    at = [n // 5 * (k + 1) + k for k in range(4)]
    sizes = [REC] * n
    for k, i in enumerate(at):
        frames.insert(i, bframes[k])
        sizes.insert(i, len(bigs[k]))
    where = {i: k for k, i in enumerate(at)}

    def records(i):
        if i in where:
            return bigs[where[i]]
        return rec_of(i - sum(1 for j in at if j < i))
    sides = {"auto": Side(L, frames, sizes, dct=dct, flags=DJ), "forced": Side(L, frames, sizes, dct=dct, flags=DJ | BP),
             "unflagged": Side(L, frames, sizes, dct=dct)}
    ms, ex, kj = race(sides, records)
    versus(f"b: {n} records of 4 KiB and four of {len(bigs[0])} bytes in one dictionary batch: the rule / unflagged "
           "(and every frame forced to K4J)", ms, ex, kj, "auto", "unflagged",
           {"chunks": n + 4, "decoded_bytes": sum(sizes),
            "forced_over_unflagged": round(ms["forced"]["median"] / ms["unflagged"]["median"], 4)})


def grid(L):
    dct = dictionary()
    outside = []
    for B in [int(v) for v in args.blocks.split(",")]:
        nu = 16
        text = gen.text(nu * B * BLOCK, seed=0x6E1D + B)
        recs = [text[i * B * BLOCK:(i + 1) * B * BLOCK] for i in range(nu)]
        uframes = compress_all(recs, lambda r: zdict.compress(r, dct, 3))
        for N in [int(v) for v in args.frames.split(",")]:
            n = max(1, int(N * args.scale))
            frames, sizes = [uframes[i % nu] for i in range(n)], [B * BLOCK] * n
            sides = {"k4j": Side(L, frames, sizes, dct=dct, flags=DJ | BP),
                     "streaming": Side(L, frames, sizes, dct=dct, flags=DJ | FS),
                     "auto": Side(L, frames, sizes, dct=dct, flags=DJ)}
            ms, ex, kj = race(sides, lambda i: recs[i % nu])
            better = "k4j" if ms["k4j"]["median"] <= ms["streaming"]["median"] else "streaming"
            out = not (ms[better]["min"] <= ms["auto"]["median"] <= ms[better]["max"])
            if out:
                outside.append([n, B])
            versus(f"c: {n} frames x {B} blocks of 128 KiB behind the dictionary: forced K4J / forced streaming / the rule",
                   ms, ex, kj, "k4j", "streaming",
                   {"frames": n, "blocks": B, "decoded_bytes": n * B * BLOCK, "better": better,
                    "auto_took": "k4j" if kj["auto"] else "streaming", "auto_outside_better": out})
    emit({"comparison": "c: points where the rule's median is outside the better forced side's min-max",
          "points_frames_blocks": outside})


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


def parent(L, LP):
    dct = dictionary()
    n = max(1, int(65536 * args.scale))
    frames, rec_of = small_records(n)
    ms, ex, kj = race({"new": Side(L, frames, [REC] * n, dct=dct), "parent": Side(LP, frames, [REC] * n, dct=dct)}, rec_of)
    versus(f"d: unflagged dictionary batch, {n} x 4 KiB records: this build against the parent commit's", ms, ex, kj,
           "new", "parent", {"chunks": n, "decoded_bytes": n * REC})
    n = max(1, int(8192 * args.scale))
    nu = min(n, max(1, args.unique // 8))
    text = gen.text(nu * BLOCK, seed=0xBA7C0)
    recs = [text[i:i + BLOCK] for i in range(0, nu * BLOCK, BLOCK)]
    frames = (compress_all(recs, lambda r: libzstd.compress(r, 3)) * ((n + nu - 1) // nu))[:n]
    ms, ex, kj = race({"new": Side(L, frames, [BLOCK] * n), "parent": Side(LP, frames, [BLOCK] * n)},
                      lambda i: recs[i % nu])
    versus(f"d: plain batch, {n} x 128 KiB frames, zstd -3: this build against the parent commit's", ms, ex, kj, "new",
           "parent", {"chunks": n, "decoded_bytes": n * BLOCK})
    nu = min(n, args.unique)
    old, new = edited_pages(nu, 0x9A6E0)
    frames = compress_all(list(range(nu)), lambda i: zdict.prefix_compress(new[i], old[i], 3))
    rep = (n + nu - 1) // nu
    d_old = upload(b"".join(old))[: nu * PAGE].repeat(rep)
    prefix = ([d_old.data_ptr() + i * PAGE for i in range(n)], [PAGE] * n)
    ms, ex, kj = race({"new": Side(L, (frames * rep)[:n], [PAGE] * n, prefix=prefix, flags=BP),
                       "parent": Side(LP, (frames * rep)[:n], [PAGE] * n, prefix=prefix, flags=BP)},
                      lambda i: new[i % nu])
    versus(f"d: prefix batch with ZD_F_BLOCK_PARALLEL, {n} page deltas of 16 KiB: this build against the parent "
           "commit's", ms, ex, kj, "new", "parent", {"chunks": n, "decoded_bytes": n * PAGE})
    del d_old
    rec = big_text()
    frame = libzstd.compress(rec, 3)
    ms, ex, kj = race({"new": Side(L, [frame], [len(rec)], flags=BP), "parent": Side(LP, [frame], [len(rec)], flags=BP)},
                      lambda i: rec)
    versus(f"d: one prefix-less {len(rec)} byte frame on K4J: this build against the parent commit's", ms, ex, kj,
           "new", "parent", {"decoded_bytes": len(rec), "new_decoded_gbps": round(len(rec) / ms["new"]["median"] / 1e6, 2)})


def main():
    L = _lib.lib()
    if args.only in (None, "a"):
        big(L)
    if args.only in (None, "b"):
        tail(L)
    if args.only in (None, "c"):
        grid(L)
    if args.only in (None, "d"):
        if not args.parent:
            raise SystemExit("comparison d needs --parent LIB")
        parent(L, load(args.parent))


if __name__ == "__main__":
    main()
