"""Times ZD_F_AUTO_EXECUTOR (each chunk of a prefix or chain batch routed to K4J or to the streaming executor by
rule) against the two forced routes, and this build against the parent commit's:
  (1) sweep     prefix batches of N text deltas of B x 128 KiB (1 % of the bytes edited), B in 1..32, N in 16..4096
                (points above 8 GiB decoded are skipped), decoded three ways: forced K4J (ZD_F_BLOCK_PARALLEL), forced
                streaming (no flag), automatic; and chain batches of N chains of depth 4 at a few of these points
                (ZD_F_CHAIN_BLOCK_PARALLEL / no flag / automatic).  The automatic side is judged against the better
                forced side of the same run: `auto_ok` is false when its median is above that side's by more than the
                margin, the larger min-max spread of the two.
  (2) mixed     8,192 page deltas of 16 KiB plus four 100 MB deltas (128 MiB window, ZD_F_LONG_WINDOW) in one prefix
                batch, the three ways; and the same as a chain batch, each kind in chains of depth 4 (2,048 page
                chains, one chain of 100 MB deltas).  The four large chunks of the prefix batch share one frame and
                one prefix (their destinations differ).
  (3) parent    the existing routes on this build against --parent: the unflagged and the ZD_F_BLOCK_PARALLEL prefix
                batch, the unflagged and the ZD_F_CHAIN_BLOCK_PARALLEL chain batch, the plain and the dictionary batch
Every side is a library file loaded into this one process, the sides of a comparison alternate inside every
repetition (the order rotated), --reps repetitions after warm-up, median (min-max) between device events around
zd_batch_decode_async.  Every decode's statuses are checked, and every side's bytes are compared with the records on
the device after a decode into a cleared buffer; a step that fails ends the script.  Run each part as a process of
its own (--only) under a time limit.  One JSON line per point.
usage: python scripts/time_auto_exec.py OUT.jsonl --parent LIB [--reps 9] [--scale F] [--only sweep|chains|mixed|parent]"""
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
ap.add_argument("--parent", help="libzd.so of the parent commit (part 3)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of the mixed batch's sizes")
ap.add_argument("--only", choices=("sweep", "chains", "mixed", "parent"))
ap.add_argument("--max-bytes", type=int, default=8 << 30, help="sweep points above this many decoded bytes are skipped")
args = ap.parse_args()
WARMUP = 2
PAGE, BLOCK, BIG = 16 << 10, 128 << 10, 100_000_000
UNIQUE = 8
F_BP, F_CBP, F_LONG, F_AUTO = _lib.F_BLOCK_PARALLEL, _lib.F_CHAIN_BLOCK_PARALLEL, _lib.F_LONG_WINDOW, _lib.F_AUTO_EXECUTOR
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
        return list(ex.map(fn, items))


def patch_compress(data, prefix, level, window_log):
    """zdict.prefix_compress with the window `zstd --patch-from` sets and its long-distance matcher"""
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


def edited(data, seed):
    rng = np.random.default_rng(seed)
    arr = np.frombuffer(bytearray(data), dtype=np.uint8).copy()
    at = rng.choice(len(arr), max(1, len(arr) // 100), replace=False)
    arr[at] ^= rng.integers(1, 256, len(at), dtype=np.uint8)
    return arr.tobytes()


def upload(b):
    t = torch.empty(len(b) + 64, dtype=torch.uint8, device=dev)
    t[: len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return t


def u64(v):
    return (C.c_uint64 * len(v))(*v)


class Work:
    """The chunks of one batch: frames (bytes, shared by every side through one device tensor), decoded sizes,
    prefixes (device addresses, sizes) or None, parents or None, `expect`: the device tensor the packed outputs must
    equal, `keep`: what must stay alive."""

    def __init__(self, frames, sizes, prefix=None, parents=None, expect=None, keep=None, dictionary=None):
        self.frames, self.sizes, self.prefix, self.parents = frames, list(sizes), prefix, parents
        self.expect, self.keep, self.dictionary = expect, keep, dictionary
        self.n = len(frames)
        self.total = sum(self.sizes)
        self.src = upload(b"".join(frames))
        self.dst = torch.zeros(self.total + 64, dtype=torch.uint8, device=dev)
        self.so = np.cumsum([0] + [len(f) for f in frames])
        self.do = np.cumsum([0] + self.sizes)


class Side:
    """One batch of library L over a Work (the sides of a comparison share its source and destination tensors)."""

    def __init__(self, L, w, flags):
        self.L, self.w, n = L, w, w.n
        vpp = C.POINTER(C.c_void_p)
        sp, ss = u64([w.src.data_ptr() + int(o) for o in w.so[:-1]]), u64([len(f) for f in w.frames])
        dp, dc = u64([w.dst.data_ptr() + int(o) for o in w.do[:-1]]), u64(w.sizes)
        self.h, self.d = C.c_void_p(), C.c_void_p()
        s = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        pp = ps = None
        if w.prefix is not None:
            self.pa, ps = u64(w.prefix[0]), u64(w.prefix[1])
            pp = C.cast(self.pa, vpp)
        if w.parents is not None:
            par = (C.c_int64 * n)(*w.parents)
            _lib.check(L.zd_batch_create_chain(C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, pp, ps, par, n, flags, s,
                                               C.byref(self.h)), "zd_batch_create_chain")
        elif w.prefix is not None:
            _lib.check(L.zd_batch_create_prefix(C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, pp, ps, n, flags, s,
                                                C.byref(self.h)), "zd_batch_create_prefix")
        else:
            if w.dictionary is not None:
                p, m, self.dkeep = _lib.buf(w.dictionary)
                _lib.check(L.zd_dict_create(p, m, C.byref(self.d)), "zd_dict_create")
            _lib.check(L.zd_batch_create(C.cast(sp, vpp), ss, C.cast(dp, vpp), dc, n, flags, self.d, s,
                                         C.byref(self.h)), "zd_batch_create")
        info = _lib.BatchInfo2()
        _lib.check(L.zd_batch_info_get_sized(self.h, C.byref(info), C.sizeof(info)), "zd_batch_info_get_sized")
        self.executors, self.k4j_chunks = int(info.executors), int(info.k4j_chunks)   # (the parent's: k4j_chunks 0)
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

    def check(self):
        """a decode into the cleared buffer, compared with the records on the device"""
        w = self.w
        w.dst.zero_()
        self.decode(False)
        if not torch.equal(w.dst[: w.total], w.expect[: w.total]):
            raise SystemExit("a side's bytes differ from the records")

    def close(self):
        self.L.zd_batch_destroy(self.h)
        if self.d:
            self.L.zd_dict_destroy(self.d)


def race(sides):
    """The sides alternating, the order rotated every repetition; every side's bytes checked first."""
    keys = list(sides)
    for k in keys:
        sides[k].check()
    for rep in range(WARMUP + args.reps):
        for k in keys[rep % len(keys):] + keys[:rep % len(keys)]:
            sides[k].decode(rep >= WARMUP)
    ms = {k: stats(s.ms) for k, s in sides.items()}
    ex = {k: s.executors for k, s in sides.items()}
    kj = {k: s.k4j_chunks for k, s in sides.items()}
    for s in sides.values():
        s.close()
    return ms, ex, kj


def emit(res):
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(line + "\n")


def three_ways(name, w, forced, base, extra):
    """forced K4J / forced streaming / automatic over one Work; the automatic side against the better forced one"""
    L = _lib.lib()
    ms, ex, kj = race({"k4j": Side(L, w, forced | base), "streaming": Side(L, w, base), "auto": Side(L, w, F_AUTO | base)})
    best = "k4j" if ms["k4j"]["median"] <= ms["streaming"]["median"] else "streaming"
    spread = lambda m: m["max"] - m["min"]
    margin = max(spread(ms["auto"]), spread(ms[best]))
    res = {"comparison": name, "reps": args.reps, "warmup": WARMUP, "ms": ms, "executors": ex, "k4j_chunks": kj["auto"],
           "chunks": w.n, "decoded_bytes": w.total, "better_forced": best,
           "k4j_over_streaming": round(ms["k4j"]["median"] / ms["streaming"]["median"], 3),
           "auto_over_better": round(ms["auto"]["median"] / ms[best]["median"], 3), "margin_ms": round(margin, 4),
           "auto_ok": bool(ms["auto"]["median"] <= ms[best]["median"] + margin)}
    res.update(extra)
    emit(res)


# ---------------------------------------------------------------------------
# the sweep's deltas: UNIQUE distinct chains of `depth` versions of B blocks, repeated
# ---------------------------------------------------------------------------
def versions(B, depth):
    size = B * BLOCK
    nu = UNIQUE
    base = [gen.text(size, seed=0xA5E00 + 64 * B + u) for u in range(nu)]
    recs = [[None] * depth for _ in range(nu)]
    prev = list(base)
    for j in range(depth):
        cur = compress_all(range(nu), lambda u: edited(prev[u], 0xA5F00 + 64 * B + 8 * j + u))
        for u in range(nu):
            recs[u][j] = cur[u]
        prev = cur
    frames = compress_all([(u, j) for u in range(nu) for j in range(depth)],
                          lambda a: zdict.prefix_compress(recs[a[0]][a[1]], recs[a[0]][a[1] - 1] if a[1] else base[a[0]], 3))
    for u in range(nu):
        if zdict.prefix_decompress(frames[u * depth], base[u], size) != recs[u][0]:
            raise SystemExit("libzstd does not return the record")
    return base, recs, frames


def sweep_work(N, B, depth, data):
    base, recs, frames = data
    size, nu = B * BLOCK, min(UNIQUE, N)
    d_base = upload(b"".join(base[:nu]))
    d_new = upload(b"".join(recs[u][j] for u in range(nu) for j in range(depth)))
    expect = d_new[: nu * depth * size].repeat(N // nu)
    fr, pp, ps, par = [], [], [], []
    for c in range(N):
        u = c % nu
        for j in range(depth):
            fr.append(frames[u * depth + j])
            pp.append(d_base.data_ptr() + u * size if j == 0 else 0)
            ps.append(size if j == 0 else 0)
            par.append(len(par) - 1 if j else -1)
    return Work(fr, [size] * (N * depth), prefix=(pp, ps), parents=par if depth > 1 else None, expect=expect,
                keep=(d_base, d_new))


def sweep(chains):
    points = ([(16, 2), (256, 2), (1024, 4), (16, 16), (256, 16)] if chains else
              [(N, B) for B in (1, 2, 4, 8, 16, 32) for N in (16, 64, 256, 1024, 4096)])
    depth = 4 if chains else 1
    data = {}
    for N, B in points:
        if N * B * BLOCK * depth > args.max_bytes:
            print(f"skipped: N {N} B {B} depth {depth}", flush=True)
            continue
        if B not in data:
            data = {B: versions(B, depth)}
        w = sweep_work(N, B, depth, data[B])
        kind = "chains of depth 4" if chains else "prefix batch"
        three_ways(f"sweep, {kind}: N {N} x B {B} blocks", w, F_CBP if chains else F_BP, 0,
                   {"N": N, "B": B, "depth": depth})
        del w
        torch.cuda.empty_cache()


# ---------------------------------------------------------------------------
# the mixed batch
# ---------------------------------------------------------------------------
def page_versions(nu, depth, seed):
    text = gen.text(nu * PAGE, seed=seed)
    base = [text[i * PAGE:(i + 1) * PAGE] for i in range(nu)]
    recs, prev = [], list(base)
    for j in range(depth):
        prev = [edited(p, seed + 1 + 8192 * j + i) for i, p in enumerate(prev)]
        recs.append(prev)
    return base, recs


def big_versions(depth):
    n = max(1 << 20, int(BIG * args.scale)) // 16 * 16
    base = gen.text(n, seed=0xB160)
    recs, prev = [], base
    for j in range(depth):
        prev = edited(prev, 0xB161 + j)
        recs.append(prev)
    wlog = max(21, (n - 1).bit_length())
    frames = compress_all(range(depth), lambda j: patch_compress(recs[j], recs[j - 1] if j else base, 3, wlog))
    if zdict.prefix_decompress(frames[0], base, n) != recs[0]:
        raise SystemExit("libzstd does not return the record")
    return base, recs, frames


def mixed_works():
    npages = max(4, int(8192 * args.scale))
    # the prefix batch: npages page deltas, then four large chunks of one frame
    nu = min(npages, 4096)
    pbase, precs = page_versions(nu, 1, 0x9A6E0)
    pframes = compress_all(range(nu), lambda i: zdict.prefix_compress(precs[0][i], pbase[i], 3))
    bbase, brecs, bframes = big_versions(4)
    n = len(bbase)
    d_pold, d_pnew = upload(b"".join(pbase)), upload(b"".join(precs[0]))
    d_bold = upload(bbase)
    d_bnew = [upload(r) for r in brecs]
    rep = (npages + nu - 1) // nu
    fr = (pframes * rep)[:npages] + [bframes[0]] * 4
    pp = [d_pold.data_ptr() + (i % nu) * PAGE for i in range(npages)] + [d_bold.data_ptr()] * 4
    ps = [PAGE] * npages + [n] * 4
    expect = torch.cat([d_pnew[: nu * PAGE].repeat(rep)[: npages * PAGE]] + [d_bnew[0][:n]] * 4)
    prefix_w = Work(fr, [PAGE] * npages + [n] * 4, prefix=(pp, ps), expect=expect, keep=(d_pold, d_bold))
    del expect
    # the chain batch: npages / 4 page chains of depth 4, then one chain of depth 4 of large deltas
    nc = max(1, npages // 4)
    ncu = min(nc, 1024)
    cbase, crecs = page_versions(ncu, 4, 0x9A7E0)
    cframes = compress_all([(i, j) for i in range(ncu) for j in range(4)],
                           lambda a: zdict.prefix_compress(crecs[a[1]][a[0]], crecs[a[1] - 1][a[0]] if a[1] else cbase[a[0]], 3))
    d_cold = upload(b"".join(cbase))
    d_cnew = upload(b"".join(crecs[j][i] for i in range(ncu) for j in range(4)))
    fr, pp, ps, par = [], [], [], []
    for c in range(nc):
        for j in range(4):
            fr.append(cframes[(c % ncu) * 4 + j])
            pp.append(d_cold.data_ptr() + (c % ncu) * PAGE if j == 0 else 0)
            ps.append(PAGE if j == 0 else 0)
            par.append(len(par) - 1 if j else -1)
    for j in range(4):
        fr.append(bframes[j])
        pp.append(d_bold.data_ptr() if j == 0 else 0)
        ps.append(n if j == 0 else 0)
        par.append(len(par) - 1 if j else -1)
    crep = (nc + ncu - 1) // ncu
    expect = torch.cat([d_cnew[: ncu * 4 * PAGE].repeat(crep)[: nc * 4 * PAGE]] + [t[:n] for t in d_bnew])
    chain_w = Work(fr, [PAGE] * (4 * nc) + [n] * 4, prefix=(pp, ps), parents=par, expect=expect, keep=(d_cold, d_bold))
    return prefix_w, chain_w, npages, n


def mixed():
    pw, cw, npages, n = mixed_works()
    three_ways(f"mixed prefix batch: {npages} page deltas of 16 KiB + 4 deltas of {n} bytes", pw, F_BP, F_LONG,
               {"pages": npages, "large_bytes": n})
    three_ways(f"mixed chain batch: {npages // 4} page chains + 1 chain of {n} byte deltas, depth 4", cw, F_CBP, F_LONG,
               {"pages": npages, "large_bytes": n})


# ---------------------------------------------------------------------------
# the existing routes against the parent commit's library
# ---------------------------------------------------------------------------
def versus(name, w, flags, LP):
    ms, ex, _ = race({"new": Side(_lib.lib(), w, flags), "parent": Side(LP, w, flags)})
    emit({"comparison": name, "reps": args.reps, "warmup": WARMUP, "ms": ms, "executors": ex, "chunks": w.n,
          "decoded_bytes": w.total, "new_over_parent": round(ms["new"]["median"] / ms["parent"]["median"], 4),
          "within": within(ms["new"], ms["parent"])})


def parent():
    if not args.parent:
        raise SystemExit("part 3 needs --parent LIB")
    LP = load(args.parent)
    pw, cw, npages, n = mixed_works()
    # (the pages alone: the mixed works without their four large chunks)
    pages_w = Work(pw.frames[:npages], pw.sizes[:npages], prefix=(pw.prefix[0][:npages], pw.prefix[1][:npages]),
                   expect=pw.expect, keep=pw.keep)
    versus(f"parent: {npages} page deltas, unflagged prefix batch", pages_w, 0, LP)
    versus(f"parent: {npages} page deltas + 4 deltas of {n} bytes, prefix batch with ZD_F_BLOCK_PARALLEL", pw,
           F_BP | F_LONG, LP)
    m = 4 * (npages // 4)
    chains_w = Work(cw.frames[:m], cw.sizes[:m], prefix=(cw.prefix[0][:m], cw.prefix[1][:m]), parents=cw.parents[:m],
                    expect=cw.expect, keep=cw.keep)
    versus(f"parent: {npages // 4} page chains of depth 4, unflagged chain batch", chains_w, 0, LP)
    versus(f"parent: {npages // 4} page chains + 1 chain of {n} byte deltas, chain batch with ZD_F_CHAIN_BLOCK_PARALLEL",
           cw, F_CBP | F_LONG, LP)
    del pw, cw, pages_w, chains_w
    torch.cuda.empty_cache()
    chunk, k = 128 << 10, max(1, int(8192 * args.scale))
    nu = min(k, 512)
    text = gen.text(nu * chunk, seed=0xBA7C0)
    recs = [text[i:i + chunk] for i in range(0, nu * chunk, chunk)]
    frames = (compress_all(recs, lambda r: libzstd.compress(r, 3)) * ((k + nu - 1) // nu))[:k]
    expect = upload(text)[: nu * chunk].repeat((k + nu - 1) // nu)
    versus(f"parent: plain batch, {k} x 128 KiB frames, zstd -3", Work(frames, [chunk] * k, expect=expect), 0, LP)
    rec, k = 4096, max(1, int(65536 * args.scale))
    train = gen.text(2048 * rec, seed=0xD1C2)
    dct = zdict.train([train[i:i + rec] for i in range(0, len(train), rec)], 112 << 10)
    nu = min(k, 16384)
    text = gen.text(nu * rec, seed=0xD1C5)
    recs = [text[i:i + rec] for i in range(0, nu * rec, rec)]
    frames = (compress_all(recs, lambda r: zdict.compress(r, dct, 3)) * ((k + nu - 1) // nu))[:k]
    expect = upload(text)[: nu * rec].repeat((k + nu - 1) // nu)
    versus(f"parent: dictionary batch, {k} x 4 KiB records, 112 KiB dictionary",
           Work(frames, [rec] * k, expect=expect, dictionary=dct), 0, LP)


def main():
    if args.only in (None, "sweep"):
        sweep(False)
    if args.only in (None, "chains"):
        sweep(True)
    if args.only in (None, "mixed"):
        mixed()
    if args.only in (None, "parent"):
        parent()


if __name__ == "__main__":
    main()
