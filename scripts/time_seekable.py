"""Times reads of seekable archives (zd_seekable_read_create, zd_seek_read_decode_async, zd_k_seek_finish):
  (a) sequential  one range over all of 1 GiB written as 1 MiB entries, against Batch.from_device
                  (zd_batch_create_device) over the same entries with the destinations computed on the host:
                  decode ms of both, the finish pass alone, creation ms of both
  (b) records     8,192 ranges of 4 KiB at random offsets of 1 GiB written as 128 KiB entries, against decoding
                  the whole archive in one plan (zd_plan_create_device + zd_decode_async): decode ms of both, the
                  distinct entries touched, the staged bytes, the finish pass alone
  (c) parent      the plain, dictionary, prefix and chain batch workloads of the earlier timing scripts on this
                  build against --parent (the parent commit's library)
Every side is a library file loaded into this one process, the sides of a comparison alternate inside every
repetition, --reps repetitions after warm-up, min / median / max between device events around the decode call.
Every decode's statuses are checked and every side's bytes compared with the source; a step that fails ends the
script.  Appends one JSON line per comparison to the output file.
usage: python scripts/time_seekable.py OUT.jsonl [--parent LIB] [--reps 9] [--scale F] [--only a|b|c]"""
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

from corpus import gen, libzstd, seekable, zdict  # noqa: E402
from zstd_decompressor import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--parent", help="libzd.so of the parent commit (comparison c)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's size")
ap.add_argument("--unique-mib", type=int, default=64, help="distinct content compressed (MiB); the rest repeats it")
ap.add_argument("--only", choices=("a", "b", "c"))
args = ap.parse_args()
WARMUP = 2
PAGE = 16 << 10
dev = torch.device("cuda", 0)
VPP = C.POINTER(C.c_void_p)


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
        return list(ex.map(fn, items, chunksize=8))


def upload(b):
    t = torch.empty(len(b) + 64, dtype=torch.uint8, device=dev)
    t[: len(b)].copy_(torch.frombuffer(bytearray(b), dtype=torch.uint8))
    return t


def u64(v):
    return (C.c_uint64 * len(v))(*v)


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
    """a device tensor's bytes against the source"""
    if not np.array_equal(t.cpu().numpy(), np.frombuffer(want, dtype=np.uint8)):
        raise SystemExit(f"{what}: bytes differ from the source")


# ---------------------------------------------------------------------------
# seekable archives
# ---------------------------------------------------------------------------
class Arc:
    """total bytes of content as entries of `entry` bytes: the distinct part compressed, then repeated."""

    def __init__(self, total, entry, seed):
        self.n = total // entry
        unique = min(self.n * entry, max(entry, (args.unique_mib << 20) // entry * entry))
        self.text = gen.text(unique + entry, seed=seed)[:unique]
        recs = [self.text[i:i + entry] for i in range(0, unique, entry)]
        frames = compress_all(recs, lambda r: libzstd.compress(r, 3))
        self.entry, self.total = entry, self.n * entry
        self.frames = (frames * ((self.n + len(frames) - 1) // len(frames)))[: self.n]
        self.unique = len(frames) * entry
        rows = [(len(f), entry, 0) for f in self.frames]
        self.blob = b"".join(self.frames) + seekable.seek_table(rows, False)
        self.src = upload(self.blob)
        self.c_off = np.cumsum([0] + [len(f) for f in self.frames])

    def content(self, off, n):
        """content bytes [off, off + n)"""
        out = bytearray()
        while n:
            o = off % self.unique
            k = min(n, self.unique - o)
            out += self.text[o:o + k]
            off += k
            n -= k
        return bytes(out)


class ReadSide:
    """zd_seekable_read_create over ranges of an Arc"""

    def __init__(self, L, arc, ranges):
        self.L, self.arc, self.ranges = L, arc, ranges
        s = C.c_void_p(stream().cuda_stream)
        self.z = C.c_void_p()
        t0 = time.perf_counter()
        _lib.check(L.zd_seekable_open_device(C.c_void_p(arc.src.data_ptr()), len(arc.blob), s, C.byref(self.z)), "open")
        self.open_ms = (time.perf_counter() - t0) * 1e3
        lens = [n for _, n in ranges]
        self.do = np.cumsum([0] + lens)
        self.dst = torch.zeros(int(self.do[-1]) + 64, dtype=torch.uint8, device=dev)
        t = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
        self.arrs = (t([o for o, _ in ranges]), t(lens), t([self.dst.data_ptr() + int(o) for o in self.do[:-1]]))
        torch.cuda.synchronize()
        self.create_ms = []
        self.h = None
        for _ in range(3):
            if self.h:
                L.zd_seek_read_destroy(self.h)
            self.h = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.zd_seekable_read_create(self.z, *[C.c_void_p(a.data_ptr()) for a in self.arrs], len(ranges), 0, s,
                                                 C.byref(self.h)), "zd_seekable_read_create")
            self.create_ms.append((time.perf_counter() - t0) * 1e3)
        self.info = _lib.SeekReadInfo()
        _lib.check(L.zd_seek_read_info_get(self.h, C.byref(self.info)))
        self.ms, self.finish_ms = [], []

    def decode(self, keep):
        s = C.c_void_p(stream().cuda_stream)
        ms = timed(lambda: _lib.check(self.L.zd_seek_read_decode_async(self.h, s), "zd_seek_read_decode_async"))
        bad = C.c_uint64()
        _lib.check(self.L.zd_seek_read_results(self.h, s, None, None, 0, C.byref(bad)))
        if bad.value:
            raise SystemExit(f"{bad.value} ranges failed")
        fin = timed(lambda: _lib.check(self.L.zd_seek_read_finish_async(self.h, s), "zd_seek_read_finish_async"))
        if keep:
            self.ms.append(ms)
            self.finish_ms.append(fin)

    def check(self):
        idx = list(range(min(64, len(self.ranges)))) + list(range(max(0, len(self.ranges) - 64), len(self.ranges)))
        for i in idx:
            o, n = self.ranges[i]
            k = min(n, 1 << 20)
            at = int(self.do[i])
            same(self.dst[at:at + k], self.arc.content(o, k), f"range {i}")
            same(self.dst[at + n - k:at + n], self.arc.content(o + n - k, k), f"range {i}'s end")

    def close(self):
        self.L.zd_seek_read_destroy(self.h)
        self.L.zd_seekable_close(self.z)


class DeviceBatchSide:
    """zd_batch_create_device over every entry of an Arc, the destinations computed on the host"""

    def __init__(self, L, arc):
        self.L, self.arc = L, arc
        self.dst = torch.zeros(arc.total + 64, dtype=torch.uint8, device=dev)
        t = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
        base = arc.src.data_ptr()
        self.arrs = (t([base + int(o) for o in arc.c_off[:-1]]), t([len(f) for f in arc.frames]),
                     t([self.dst.data_ptr() + i * arc.entry for i in range(arc.n)]), t([arc.entry] * arc.n))
        torch.cuda.synchronize()
        s = C.c_void_p(stream().cuda_stream)
        self.create_ms = []
        self.h = None
        for _ in range(3):
            if self.h:
                L.zd_batch_destroy(self.h)
            self.h = C.c_void_p()
            t0 = time.perf_counter()
            _lib.check(L.zd_batch_create_device(*[C.c_void_p(a.data_ptr()) for a in self.arrs], arc.n, 0, None, s,
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

    def check(self):
        k = min(self.arc.total, 1 << 20)
        same(self.dst[:k], self.arc.content(0, k), "the batch's first bytes")
        same(self.dst[self.arc.total - k:self.arc.total], self.arc.content(self.arc.total - k, k), "the batch's last bytes")

    def close(self):
        self.L.zd_batch_destroy(self.h)


class PlanSide:
    """zd_plan_create_device over the whole archive (the seek table is a skippable frame: skipped)"""

    def __init__(self, L, arc):
        self.L, self.arc = L, arc
        self.dst = torch.zeros(arc.total + 64, dtype=torch.uint8, device=dev)
        self.h = C.c_void_p()
        s = C.c_void_p(stream().cuda_stream)
        _lib.check(L.zd_plan_create_device(C.c_void_p(arc.src.data_ptr()), len(arc.blob), 0, s, C.byref(self.h)),
                   "zd_plan_create_device")
        self.ms = []

    def decode(self, keep):
        s = C.c_void_p(stream().cuda_stream)
        ms = timed(lambda: _lib.check(self.L.zd_decode_async(self.h, C.c_void_p(self.arc.src.data_ptr()),
                                                             C.c_void_p(self.dst.data_ptr()), self.arc.total, s)))
        total, first = C.c_uint64(), C.c_int32()
        st = self.L.zd_plan_results(self.h, C.c_void_p(self.dst.data_ptr()), s, None, None, C.byref(total), C.byref(first))
        if st or total.value != self.arc.total:
            raise SystemExit(f"the plan failed: {st}, {total.value} bytes")
        if keep:
            self.ms.append(ms)

    def check(self):
        k = min(self.arc.total, 1 << 20)
        same(self.dst[:k], self.arc.content(0, k), "the plan's first bytes")
        same(self.dst[self.arc.total - k:self.arc.total], self.arc.content(self.arc.total - k, k), "the plan's last bytes")

    def close(self):
        self.L.zd_plan_destroy(self.h)


def sequential(L):
    total = max(2 << 20, int((1 << 30) * args.scale))
    arc = Arc(total, 1 << 20, 0x5EE4A)
    sides = {"seekable_read": ReadSide(L, arc, [(0, arc.total)]), "device_batch": DeviceBatchSide(L, arc)}
    ms = race(sides)
    for s in sides.values():
        s.check()
    r = sides["seekable_read"]
    emit({"comparison": "a: one range over 1 GiB of 1 MiB entries / zd_batch_create_device over the same entries",
          "entries": arc.n, "content_bytes": arc.total, "compressed_bytes": int(arc.c_off[-1]), "reps": args.reps,
          "warmup": WARMUP, "ms": ms, "finish_pass_ms": stats(r.finish_ms),
          "read_over_batch": round(ms["seekable_read"]["median"] / ms["device_batch"]["median"], 4),
          "read_gbps": round(arc.total / ms["seekable_read"]["median"] / 1e6, 1),
          "open_ms": round(r.open_ms, 3), "read_create_ms": stats(r.create_ms),
          "batch_create_ms": stats(sides["device_batch"].create_ms),
          "frames_decoded": r.info.frames_decoded, "frames_in_place": r.info.frames_in_place,
          "staged_bytes": r.info.staged_bytes, "copy_pieces": r.info.copy_pieces,
          "executors": r.info.batch.executors, "k4j_chunks": r.info.batch.k4j_chunks})
    for s in sides.values():
        s.close()


def records(L):
    total = max(2 << 20, int((1 << 30) * args.scale))
    arc = Arc(total, 128 << 10, 0x5EE4B)
    rng = np.random.default_rng(0x5EE4C)
    n = max(1, int(8192 * args.scale))
    ranges = [(int(o), 4096) for o in rng.integers(0, arc.total - 4096, size=n)]
    sides = {"seekable_read": ReadSide(L, arc, ranges), "whole_archive_plan": PlanSide(L, arc)}
    ms = race(sides)
    for s in sides.values():
        s.check()
    r = sides["seekable_read"]
    emit({"comparison": "b: 8192 ranges of 4 KiB at random offsets of 1 GiB of 128 KiB entries / the whole archive in one plan",
          "entries": arc.n, "ranges": n, "content_bytes": arc.total, "read_bytes": 4096 * n, "reps": args.reps,
          "warmup": WARMUP, "ms": ms, "finish_pass_ms": stats(r.finish_ms),
          "read_over_plan": round(ms["seekable_read"]["median"] / ms["whole_archive_plan"]["median"], 4),
          "read_create_ms": stats(r.create_ms), "frames_decoded": r.info.frames_decoded,
          "frames_in_place": r.info.frames_in_place, "staged_bytes": r.info.staged_bytes,
          "copy_pieces": r.info.copy_pieces, "decoded_bytes": r.info.frames_decoded * arc.entry,
          "decoded_gbps": round(r.info.frames_decoded * arc.entry / ms["seekable_read"]["median"] / 1e6, 1)})
    for s in sides.values():
        s.close()


# ---------------------------------------------------------------------------
# (c) the existing batch routes, this build against the parent's
# ---------------------------------------------------------------------------
class BatchSide:
    """One host-array batch of library L: plain, with a dictionary, with prefixes, or a chain."""

    def __init__(self, L, frames, sizes, dictionary=None, prefix=None, parents=None):
        self.L, n = L, len(frames)
        self.n, self.sizes = n, sizes
        self.src = upload(b"".join(frames))
        self.dst = torch.zeros(sum(sizes) + 64, dtype=torch.uint8, device=dev)
        so, self.do = np.cumsum([0] + [len(f) for f in frames]), np.cumsum([0] + list(sizes))
        sp, ss = u64([self.src.data_ptr() + int(o) for o in so[:-1]]), u64([len(f) for f in frames])
        dp, dc = u64([self.dst.data_ptr() + int(o) for o in self.do[:-1]]), u64(list(sizes))
        self.h, self.d = C.c_void_p(), C.c_void_p()
        s = C.c_void_p(stream().cuda_stream)
        if parents is not None:
            pp, ps = u64(prefix[0]), u64(prefix[1])
            par = (C.c_int64 * n)(*parents)
            _lib.check(L.zd_batch_create_chain(C.cast(sp, VPP), ss, C.cast(dp, VPP), dc, C.cast(pp, VPP), ps, par, n, 0, s,
                                               C.byref(self.h)), "zd_batch_create_chain")
        elif prefix is not None:
            pp, ps = u64(prefix[0]), u64(prefix[1])
            _lib.check(L.zd_batch_create_prefix(C.cast(sp, VPP), ss, C.cast(dp, VPP), dc, C.cast(pp, VPP), ps, n, 0, s,
                                                C.byref(self.h)), "zd_batch_create_prefix")
        else:
            if dictionary is not None:
                p, m, self.dkeep = _lib.buf(dictionary)
                _lib.check(L.zd_dict_create(p, m, C.byref(self.d)), "zd_dict_create")
            _lib.check(L.zd_batch_create(C.cast(sp, VPP), ss, C.cast(dp, VPP), dc, n, 0, self.d, s, C.byref(self.h)),
                       "zd_batch_create")
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

    def check(self, record):
        out = self.dst[: int(self.do[-1])].cpu().numpy()
        for i in list(range(min(64, self.n))) + list(range(max(0, self.n - 64), self.n)):
            if bytes(out[int(self.do[i]):int(self.do[i + 1])]) != record(i):
                raise SystemExit(f"chunk {i} differs from its record")
        return int(out.sum(dtype=np.uint64))

    def close(self):
        self.L.zd_batch_destroy(self.h)
        if self.d:
            self.L.zd_dict_destroy(self.d)


def versus(name, make, record, extra):
    sides = {"new": make(_lib.lib()), "parent": make(PARENT)}
    ms = race(sides)
    sums = {k: s.check(record) for k, s in sides.items()}
    if len(set(sums.values())) != 1:
        raise SystemExit(f"the sides' outputs differ: {sums}")
    for s in sides.values():
        s.close()
    emit(dict({"comparison": "c: " + name + ": this build against the parent commit's", "reps": args.reps,
               "warmup": WARMUP, "ms": ms, "new_over_parent": round(ms["new"]["median"] / ms["parent"]["median"], 4)},
              **extra))


def edited(pages, rng):
    out = []
    for o in pages:
        b = bytearray(o)
        for p in rng.choice(PAGE, PAGE // 100, replace=False):
            b[p] ^= int(rng.integers(1, 256))
        out.append(bytes(b))
    return out


def parent():
    # plain: 8,192 x 128 KiB frames
    chunk, n = 128 << 10, max(1, int(8192 * args.scale))
    nu = min(n, 512)
    text = gen.text(nu * chunk, seed=0xBA7C0)
    recs = [text[i:i + chunk] for i in range(0, nu * chunk, chunk)]
    frames = (compress_all(recs, lambda r: libzstd.compress(r, 3)) * ((n + nu - 1) // nu))[:n]
    versus("plain batch, 8192 x 128 KiB frames, zstd -3", lambda L: BatchSide(L, frames, [chunk] * n),
           lambda i: recs[i % nu], {"chunks": n, "decoded_bytes": n * chunk})
    # dictionary: 65,536 x 4 KiB records, a 112 KiB dictionary
    rec, n = 4096, max(1, int(65536 * args.scale))
    train = gen.text(2048 * rec, seed=0xD1C2)
    dct = zdict.train([train[i:i + rec] for i in range(0, len(train), rec)], 112 << 10)
    nu = min(n, 16384)
    text = gen.text(nu * rec, seed=0xD1C5)
    recs2 = [text[i:i + rec] for i in range(0, nu * rec, rec)]
    frames2 = (compress_all(recs2, lambda r: zdict.compress(r, dct, 3)) * ((n + nu - 1) // nu))[:n]
    versus("dictionary batch, 65536 x 4 KiB records, 112 KiB dictionary",
           lambda L: BatchSide(L, frames2, [rec] * n, dictionary=dct), lambda i: recs2[i % nu],
           {"chunks": n, "decoded_bytes": n * rec})
    # prefix: 8,192 pages of 16 KiB, 1 % edited, each against its own old page
    n = max(1, int(8192 * args.scale))
    nu = min(n, 4096)
    text = gen.text(nu * PAGE + PAGE, seed=0x9A6E0)
    rng = np.random.default_rng(0x9A6E1)
    old = [text[i * PAGE:(i + 1) * PAGE] for i in range(nu)]
    new = edited(old, rng)
    dframes = compress_all(list(range(nu)), lambda i: zdict.prefix_compress(new[i], old[i], 3))
    rep = (n + nu - 1) // nu
    d_old = upload(b"".join(old))[: nu * PAGE].repeat(rep)[: n * PAGE].contiguous()
    prefix = ([d_old.data_ptr() + i * PAGE for i in range(n)], [PAGE] * n)
    versus("prefix batch, 8192 pages of 16 KiB, 1 % edited, against the old pages",
           lambda L: BatchSide(L, (dframes * rep)[:n], [PAGE] * n, prefix=prefix), lambda i: new[i % nu],
           {"chunks": n, "decoded_bytes": n * PAGE})
    # chain: the same pages, four versions deep; chunk (level l, chain c) is chunk l * n + c
    depth, n = 4, max(1, int(2048 * args.scale))
    nu = min(n, 1024)
    vers, prev = [], old[:nu]
    for _ in range(depth):
        prev = edited(prev, rng)
        vers.append(prev)
    lv = [compress_all(list(range(nu)), lambda i, l=l: zdict.prefix_compress(vers[l][i], (old if l == 0 else vers[l - 1])[i], 3))
          for l in range(depth)]
    rep = (n + nu - 1) // nu
    flat = [f for l in range(depth) for f in (lv[l] * rep)[:n]]
    d_base = upload(b"".join(old[:nu]))[: nu * PAGE].repeat(rep)[: n * PAGE].contiguous()
    cpre = ([d_base.data_ptr() + i * PAGE if i < n else 0 for i in range(depth * n)],
            [PAGE if i < n else 0 for i in range(depth * n)])
    parents = [-1 if i < n else i - n for i in range(depth * n)]
    versus("chain batch, 2048 chains of 16 KiB pages, 4 versions deep",
           lambda L: BatchSide(L, flat, [PAGE] * (depth * n), prefix=cpre, parents=parents),
           lambda i: vers[i // n][(i % n) % nu], {"chunks": depth * n, "decoded_bytes": depth * n * PAGE})


PARENT = None


def main():
    global PARENT
    L = _lib.lib()
    if args.only in (None, "a"):
        sequential(L)
    if args.only in (None, "b"):
        records(L)
    if args.only in (None, "c"):
        if not args.parent:
            raise SystemExit("comparison c needs --parent LIB")
        PARENT = load(args.parent)
        parent()


if __name__ == "__main__":
    main()
