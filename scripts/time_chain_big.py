"""Times chain batches on the block-parallel executor (ZD_F_CHAIN_BLOCK_PARALLEL on zd_batch_create_chain: K4J level
by level, zd_k_jscatter<true, true> and zd_k_jround<true>) against what there was before, and this build against the
parent commit's:
  (A) one flagged chain batch: 4 chains of depth 4 over an external base, every frame a 100 MB text delta (1 % of
      the bytes edited per version, compressed against the version before it with a 128 MiB window as
      `zstd --patch-from` does: ZD_F_LONG_WINDOW), creation and decode
  (B) the same links as four prefix batches with ZD_F_BLOCK_PARALLEL, one per level, created and decoded one after
      another (a host round trip between links), on this build and on --parent: the yardstick
  (C) the same chain batch without the flag (the streaming executor), ONE repetition: seconds
  (D) page chains: 8,192 chains of depth 4 of 16 KiB pages (scripts/time_chain.py's workload), flagged / unflagged
  (E) the existing routes on this build against --parent: the unflagged chain batch, the flagged and the unflagged
      prefix batch, the plain batch, the dictionary batch, one prefix-less 100 MB frame on K4J
Every side is a library file loaded into this one process, the sides of a comparison alternate inside every
repetition, --reps repetitions after warm-up, median (min-max): decodes between device events around
zd_batch_decode_async, creations by the host's clock around the creation call (the stream idle before it).  Every
decode's statuses are checked and every side's bytes are compared with the records on the device; a step that fails
ends the script.  `within`: each side's median inside the other side's min-max.  One JSON line per comparison.
usage: python scripts/time_chain_big.py OUT.jsonl --parent LIB [--reps 9] [--scale F] [--only A|B|C|D|E ...]"""
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

from corpus import gen, libzstd, zdict  # noqa: E402
from zstd_decompressor import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--parent", help="libzd.so of the parent commit (B's yardstick, E)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's size")
ap.add_argument("--unique", type=int, default=1024, help="distinct page chains / records compressed; the rest repeat them")
ap.add_argument("--only", nargs="*", choices=("A", "B", "C", "D", "E"))
args = ap.parse_args()
WARMUP = 2
PAGE = 16 << 10
BIG = 100_000_000
CHAINS, DEPTH = 4, 4
F_CJ = getattr(_lib, "F_CHAIN_BLOCK_PARALLEL", 4096)
F_LONG, F_BP = _lib.F_LONG_WINDOW, _lib.F_BLOCK_PARALLEL
ZSTD_c_windowLog, ZSTD_c_enableLongDistanceMatching = 101, 160
dev = torch.device("cuda", 0)
vpp = C.POINTER(C.c_void_p)


def want(k):
    return not args.only or k in args.only


def load(path):
    L = C.CDLL(path)
    for name, (res, argt) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, argt
    return L


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4), "n": len(v)}


def within(a, b):
    return bool(b["min"] <= a["median"] <= b["max"] and a["min"] <= b["median"] <= a["max"])


def compress_all(items, fn):
    with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:      # ctypes drops the GIL
        return list(ex.map(fn, items))


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


def u64(v):
    return (C.c_uint64 * len(v))(*v)


def stream():
    return torch.cuda.current_stream(dev)


class Batch:
    """One batch of library L: frames at device addresses sp / ss into dp / dc; prefix = (addresses, sizes) or None;
    parent = a chain batch's parents or None; dictionary = bytes or None.  create_ms: the host's clock."""

    def __init__(self, L, sp, ss, dp, dc, flags=0, prefix=None, parent=None, dictionary=None):
        self.L, self.n = L, len(sp)
        n = self.n
        self.h, self.d = C.c_void_p(), C.c_void_p()
        a = (C.cast(u64(sp), vpp), u64(ss), C.cast(u64(dp), vpp), u64(dc))
        s = C.c_void_p(stream().cuda_stream)
        if dictionary is not None:
            p, m, self.dkeep = _lib.buf(dictionary)
            _lib.check(L.zd_dict_create(p, m, C.byref(self.d)), "zd_dict_create")
        pf = (C.cast(u64(prefix[0]), vpp), u64(prefix[1])) if prefix is not None else (None, None)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        if parent is not None:
            par = (C.c_int64 * n)(*parent)
            _lib.check(L.zd_batch_create_chain(*a, *pf, par, n, flags, s, C.byref(self.h)), "zd_batch_create_chain")
        elif prefix is not None:
            _lib.check(L.zd_batch_create_prefix(*a, *pf, n, flags, s, C.byref(self.h)), "zd_batch_create_prefix")
        else:
            _lib.check(L.zd_batch_create(*a, n, flags, self.d, s, C.byref(self.h)), "zd_batch_create")
        self.create_ms = (time.perf_counter() - t0) * 1e3
        info = _lib.BatchInfoEx()
        _lib.check(L.zd_batch_info_get_sized(self.h, C.byref(info), C.sizeof(info)), "zd_batch_info_get_sized")
        self.executors = int(info.executors)

    def decode(self):
        """milliseconds between device events around zd_batch_decode_async; every chunk ZD_OK"""
        s = stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(s)
        _lib.check(self.L.zd_batch_decode_async(self.h, C.c_void_p(s.cuda_stream)), "zd_batch_decode_async")
        e1.record(s)
        e1.synchronize()
        bad = C.c_uint64()
        _lib.check(self.L.zd_batch_results(self.h, C.c_void_p(s.cuda_stream), None, None, 0, C.byref(bad)))
        if bad.value:
            raise SystemExit(f"{bad.value} chunks failed")
        return e0.elapsed_time(e1)

    def close(self):
        self.L.zd_batch_destroy(self.h)
        if self.d:
            self.L.zd_dict_destroy(self.d)


class Layout:
    """Frames in one device tensor, outputs packed in another, the records on the device for the comparison."""

    def __init__(self, frames, records, repeat=1):
        self.src = upload(b"".join(frames))
        sizes = [len(r) for r in records]
        so, do = np.cumsum([0] + [len(f) for f in frames]), np.cumsum([0] + sizes)
        self.rec = upload(b"".join(records))[: int(do[-1])]
        self.repeat, self.one = repeat, int(do[-1])
        self.dst = torch.zeros(self.one * repeat + 64, dtype=torch.uint8, device=dev)
        self.sp = [self.src.data_ptr() + int(o) for o in so[:-1]] * repeat
        self.ss = [len(f) for f in frames] * repeat
        self.dp = [self.dst.data_ptr() + r * self.one + int(o) for r in range(repeat) for o in do[:-1]]
        self.dc = sizes * repeat

    def clear(self):
        self.dst.zero_()

    def check(self, what):
        for r in range(self.repeat):
            if not torch.equal(self.dst[r * self.one:(r + 1) * self.one], self.rec):
                raise SystemExit(f"{what}: the decoded bytes differ from the records")


def emit(res):
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def race(sides, reps):
    """sides: name -> callable returning a dict of milliseconds; alternating, the order rotated every repetition"""
    keys = list(sides)
    got = {k: {} for k in keys}
    for rep in range(WARMUP + reps):
        for k in keys[rep % len(keys):] + keys[:rep % len(keys)]:
            ms = sides[k]()
            if rep >= WARMUP:
                for name, v in ms.items():
                    got[k].setdefault(name, []).append(v)
    return {k: {name: stats(v) for name, v in d.items()} for k, d in got.items()}


# ---------------------------------------------------------------------------
# A, B, C: chains of 100 MB deltas
# ---------------------------------------------------------------------------
def big_chains():
    n = max(1 << 20, int(BIG * args.scale))
    base = gen.text(n, seed=0xC4A10)
    rng = np.random.default_rng(0xC4A11)
    recs = []                                     # chunk c * DEPTH + k: version k of chain c
    for c in range(CHAINS):
        prev = base
        for k in range(DEPTH):
            arr = np.frombuffer(bytearray(prev), dtype=np.uint8).copy()
            at = rng.choice(n, n // 100, replace=False)
            arr[at] ^= rng.integers(1, 256, len(at), dtype=np.uint8)
            prev = arr.tobytes()
            recs.append(prev)
    wlog = max(21, (n - 1).bit_length())
    against = lambda i: base if i % DEPTH == 0 else recs[i - 1]
    frames = compress_all(list(range(len(recs))), lambda i: patch_compress(recs[i], against(i), 3, wlog))
    for i in (0, 1, len(recs) - 1):
        if zdict.prefix_decompress(frames[i], against(i), n) != recs[i]:
            raise SystemExit("libzstd does not return the record")
    return n, wlog, base, recs, frames


def chains_of_big_deltas(L, LP):
    n, wlog, base, recs, frames = big_chains()
    lay = Layout(frames, recs)
    d_base = upload(base)
    N = CHAINS * DEPTH
    parent = [-1 if i % DEPTH == 0 else i - 1 for i in range(N)]
    ext = ([d_base.data_ptr() if p < 0 else 0 for p in parent], [n if p < 0 else 0 for p in parent])
    extra = {"chains": CHAINS, "depth": DEPTH, "frame_bytes": n, "decoded_bytes": N * n, "window_log": wlog,
             "compressed_bytes": sum(len(f) for f in frames)}

    def chain(lib, flags):
        lay.clear()
        b = Batch(lib, lay.sp, lay.ss, lay.dp, lay.dc, flags=flags | F_LONG, prefix=ext, parent=parent)
        try:
            ms = {"create": b.create_ms, "decode": b.decode(), "executors": b.executors}
        finally:
            b.close()
        lay.check("chain batch")
        return ms

    def links(lib):
        """one flagged prefix batch per level: level k's prefixes are level k - 1's outputs"""
        lay.clear()
        ms = {"create": 0.0, "decode": 0.0, "first_create": 0.0}
        for k in range(DEPTH):
            idx = [c * DEPTH + k for c in range(CHAINS)]
            pf = ([d_base.data_ptr() if k == 0 else lay.dp[i - 1] for i in idx], [n] * CHAINS)
            pick = lambda v: [v[i] for i in idx]
            b = Batch(lib, pick(lay.sp), pick(lay.ss), pick(lay.dp), pick(lay.dc), flags=F_BP | F_LONG, prefix=pf)
            try:
                ms["create"] += b.create_ms
                if k == 0:
                    ms["first_create"] = b.create_ms
                ms["decode"] += b.decode()
            finally:
                b.close()
        lay.check("four prefix batches")
        return ms

    if want("A") or want("B"):
        sides = {"A_chain_flagged": lambda: chain(L, F_CJ), "B_four_prefix_batches": lambda: links(L)}
        if LP is not None:
            sides["B_on_parent"] = lambda: links(LP)
        ms = race(sides, args.reps)
        a, b = ms["A_chain_flagged"], ms["B_four_prefix_batches"]
        res = {"comparison": f"A / B: {CHAINS} chains of depth {DEPTH} of {n} byte text deltas, 1 % edited a version: one "
                             "chain batch with ZD_F_CHAIN_BLOCK_PARALLEL / four prefix batches with ZD_F_BLOCK_PARALLEL",
               "reps": args.reps, "warmup": WARMUP, "ms": ms,
               "A_decode_over_B_decode": round(a["decode"]["median"] / b["decode"]["median"], 4),
               "A_create_over_one_of_B": round(a["create"]["median"] / b["first_create"]["median"], 4),
               "A_total_over_B_total": round((a["create"]["median"] + a["decode"]["median"]) /
                                             (b["create"]["median"] + b["decode"]["median"]), 4),
               "A_decoded_gbps": round(N * n / a["decode"]["median"] / 1e6, 2)}
        if LP is not None:
            p = ms["B_on_parent"]
            res["B_decode_over_parent"] = round(b["decode"]["median"] / p["decode"]["median"], 4)
            res["B_within_parent"] = within(b["decode"], p["decode"])
        res.update(extra)
        emit(res)
    if want("C"):
        ms = chain(L, 0)
        res = {"comparison": "C: the same chain batch without the flag (zd_k_execute_chain), one repetition", "reps": 1,
               "ms": {k: round(v, 3) for k, v in ms.items()}}
        res.update(extra)
        emit(res)
    return n, recs, frames


# ---------------------------------------------------------------------------
# D, E: page chains and the existing routes
# ---------------------------------------------------------------------------
def page_chains():
    n = max(1, int(8192 * args.scale))
    nu = min(n, args.unique)
    text = gen.text(nu * PAGE + PAGE, seed=0xC4A20)
    rng = np.random.default_rng(0xC4A21)
    bases = [text[i * PAGE:(i + 1) * PAGE] for i in range(nu)]
    recs = []
    for c in range(nu):
        prev = bases[c]
        for k in range(DEPTH):
            b = bytearray(prev)
            for p in rng.choice(PAGE, PAGE // 100, replace=False):
                b[p] ^= int(rng.integers(1, 256))
            prev = bytes(b)
            recs.append(prev)
    against = lambda i: bases[i // DEPTH] if i % DEPTH == 0 else recs[i - 1]
    frames = compress_all(list(range(len(recs))), lambda i: zdict.prefix_compress(recs[i], against(i), 3))
    return n, nu, bases, recs, frames


def versus(name, sides, a, b, extra, reps=None):
    ms = race(sides, reps or args.reps)
    res = {"comparison": name, "reps": reps or args.reps, "warmup": WARMUP, "ms": ms,
           f"{a}_over_{b}": round(ms[a]["decode"]["median"] / ms[b]["decode"]["median"], 4),
           "within": within(ms[a]["decode"], ms[b]["decode"])}
    res.update(extra)
    emit(res)


def decoder(lay, batch, what):
    def run():
        lay.clear()
        ms = batch.decode()
        lay.check(what)
        return {"decode": ms}
    return run


def pages_and_routes(L, LP, big):
    n, nu, bases, recs, frames = page_chains()
    rep = (n + nu - 1) // nu
    lay = Layout(frames, recs, repeat=rep)
    d_bases = upload(b"".join(bases))
    N = nu * DEPTH * rep
    parent = [-1 if i % DEPTH == 0 else i - 1 for i in range(N)]
    ext = ([d_bases.data_ptr() + ((i // DEPTH) % nu) * PAGE if p < 0 else 0 for i, p in enumerate(parent)],
           [PAGE if p < 0 else 0 for p in parent])
    mk = lambda lib, flags: Batch(lib, lay.sp, lay.ss, lay.dp, lay.dc, flags=flags, prefix=ext, parent=parent)
    shape = {"chains": nu * rep, "depth": DEPTH, "chunks": N, "decoded_bytes": N * PAGE}
    if want("D"):
        f, u = mk(L, F_CJ), mk(L, 0)
        shape["executors"] = {"flagged": f.executors, "unflagged": u.executors}
        versus(f"D: {nu * rep} page chains of depth {DEPTH}, 16 KiB pages, 1 % edited: ZD_F_CHAIN_BLOCK_PARALLEL / streaming",
               {"flagged": decoder(lay, f, "flagged page chains"), "unflagged": decoder(lay, u, "page chains")},
               "flagged", "unflagged", shape)
        f.close(), u.close()
    if not want("E"):
        return
    if LP is None:
        raise SystemExit("comparison E needs --parent LIB")

    def pair(name, make, lay_, extra):
        a, b = make(L), make(LP)
        extra = dict(extra, executors={"new": a.executors, "parent": b.executors})
        versus("E: " + name + ": this build against the parent commit's",
               {"new": decoder(lay_, a, name), "parent": decoder(lay_, b, name + " (parent)")}, "new", "parent", extra)
        a.close(), b.close()

    shape.pop("executors", None)
    pair("unflagged chain batch of page chains", lambda lib: mk(lib, 0), lay, shape)
    # prefix batches: the chains' first links
    idx = [i for i in range(N) if parent[i] < 0]
    pick = lambda v: [v[i] for i in idx]
    pf = (pick(ext[0]), pick(ext[1]))
    play = Layout([frames[i] for i in range(0, nu * DEPTH, DEPTH)], [recs[i] for i in range(0, nu * DEPTH, DEPTH)], repeat=rep)
    for flags, name in ((F_BP, "flagged prefix batch of page deltas (K4J)"), (0, "unflagged prefix batch of page deltas")):
        pair(name, lambda lib: Batch(lib, play.sp, play.ss, play.dp, play.dc, flags=flags, prefix=pf), play,
             {"chunks": len(idx), "decoded_bytes": len(idx) * PAGE})
    del lay, play
    chunk, n = 128 << 10, max(1, int(8192 * args.scale))
    nu = min(n, max(1, args.unique // 2))
    text = gen.text(nu * chunk, seed=0xBA7C0)
    recs = [text[i:i + chunk] for i in range(0, nu * chunk, chunk)]
    lay = Layout(compress_all(recs, lambda r: libzstd.compress(r, 3)), recs, repeat=(n + nu - 1) // nu)
    pair("plain batch of 128 KiB frames, zstd -3", lambda lib: Batch(lib, lay.sp, lay.ss, lay.dp, lay.dc), lay,
         {"chunks": len(lay.sp), "decoded_bytes": len(lay.sp) * chunk})
    rec, n = 4096, max(1, int(65536 * args.scale))
    train = gen.text(2048 * rec, seed=0xD1C2)
    dct = zdict.train([train[i:i + rec] for i in range(0, len(train), rec)], 112 << 10)
    nu = min(n, args.unique * 4)
    text = gen.text(nu * rec, seed=0xD1C5)
    recs = [text[i:i + rec] for i in range(0, nu * rec, rec)]
    lay = Layout(compress_all(recs, lambda r: zdict.compress(r, dct, 3)), recs, repeat=(n + nu - 1) // nu)
    pair("dictionary batch of 4 KiB records, 112 KiB dictionary",
         lambda lib: Batch(lib, lay.sp, lay.ss, lay.dp, lay.dc, dictionary=dct), lay,
         {"chunks": len(lay.sp), "decoded_bytes": len(lay.sp) * rec})
    # the prefix-less frame on K4J: zd_k_jscatter<false> and zd_k_jround<false> must be the parent's kernels
    one = big[1][0] if big else gen.text(max(1 << 20, int(BIG * args.scale)), seed=0xC4A30)
    lay = Layout([libzstd.compress(one, 3)], [one])
    pair(f"one prefix-less {len(one)} byte frame on K4J",
         lambda lib: Batch(lib, lay.sp, lay.ss, lay.dp, lay.dc, flags=F_BP), lay, {"decoded_bytes": len(one)})


def main():
    L = _lib.lib()
    LP = load(args.parent) if args.parent else None
    big = None
    if want("A") or want("B") or want("C"):
        big = chains_of_big_deltas(L, LP)
    if want("D") or want("E"):
        pages_and_routes(L, LP, big)


if __name__ == "__main__":
    main()
