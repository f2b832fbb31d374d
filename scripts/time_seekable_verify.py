"""Times verified reads of seekable archives (zd_seekable_read_create_ex with ZD_SEEK_VERIFY_TABLE: zd_k_seek_verify
between the inner batch's decode and zd_k_seek_finish):
  (a) sequential  one range over 1 GiB written as 1,024 entries of 1 MiB, with the option and without: decode ms of
                  both, and zd_seek_read_finish_async alone on both (their difference is the verify pass)
  (b) records     8,192 ranges of 4 KiB at random offsets of 1 GiB written as 8,192 entries of 128 KiB, the same two
  (c) own sums    the archives of (a) and (b) with a Content_Checksum in every frame: ZD_F_VERIFY_CHECKSUM alone
                  against the same plus the option (the entries are compared by the inner batch's digests)
  (d) parent      the unverified reads of (a) and (b) and a plain device batch over (b)'s entries on this build
                  against --parent (the parent commit's library)
Every side is a library file loaded into this one process, the sides of a comparison alternate inside every
repetition with the order rotated, --reps repetitions after warm-up, min / median / max between device events.
Every decode's statuses are checked (a verified side: every verdict 1 as well) and every side's bytes compared with
the source; a step that fails ends the script.  Appends one JSON line per comparison to the output file.
usage: python scripts/time_seekable_verify.py OUT.jsonl --parent LIB [--reps 9] [--scale F] [--only a|b|c|d]"""
import argparse
import concurrent.futures as cf
import ctypes as C
import json
import os
import statistics
import struct
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zstd-decompressor_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

from corpus import gen, libzstd, seekable  # noqa: E402
from zstd_decompressor import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--parent", help="libzd.so of the parent commit (comparison d)")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's size")
ap.add_argument("--unique-mib", type=int, default=64, help="distinct content compressed (MiB); the rest repeats it")
ap.add_argument("--only", choices=("a", "b", "c", "d"))
args = ap.parse_args()
WARMUP = 2
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


class Arc:
    """total bytes of content as entries of `entry` bytes, the table with checksums (the writer's: the 32 bits
    libzstd stores as the frame's Content_Checksum): the distinct part compressed, then repeated.  `blob`: frames
    without a Content_Checksum; `blob_own`: the same entries, every frame with its own."""

    def __init__(self, total, entry, seed):
        self.n = total // entry
        unique = min(self.n * entry, max(entry, (args.unique_mib << 20) // entry * entry))
        self.text = gen.text(unique + entry, seed=seed)[:unique]
        recs = [self.text[i:i + entry] for i in range(0, unique, entry)]
        plain = compress_all(recs, lambda r: libzstd.compress(r, 3))
        own = compress_all(recs, lambda r: libzstd.compress(r, 3, checksum=True))
        sums = [struct.unpack("<I", f[-4:])[0] for f in own]
        self.entry, self.total, self.unique = entry, self.n * entry, len(plain) * entry
        rep = (self.n + len(plain) - 1) // len(plain)
        self.frames, self.frames_own, sums = (plain * rep)[: self.n], (own * rep)[: self.n], (sums * rep)[: self.n]
        self.blob = b"".join(self.frames) + seekable.seek_table(
            [(len(f), entry, k) for f, k in zip(self.frames, sums)], True)
        self.blob_own = b"".join(self.frames_own) + seekable.seek_table(
            [(len(f), entry, k) for f, k in zip(self.frames_own, sums)], True)
        self.src, self.src_own = upload(self.blob), upload(self.blob_own)
        self.c_off = np.cumsum([0] + [len(f) for f in self.frames])

    def content(self, off, n):
        out = bytearray()
        while n:
            o = off % self.unique
            k = min(n, self.unique - o)
            out += self.text[o:o + k]
            off += k
            n -= k
        return bytes(out)


class ReadSide:
    """A read over ranges of an Arc: zd_seekable_read_create_ex when the library has it (read_flags), else
    zd_seekable_read_create."""

    def __init__(self, L, arc, ranges, flags=0, read_flags=0, own=False):
        self.L, self.arc, self.ranges, self.read_flags = L, arc, ranges, read_flags
        s = C.c_void_p(stream().cuda_stream)
        src, blob = (arc.src_own, arc.blob_own) if own else (arc.src, arc.blob)
        self.z = C.c_void_p()
        _lib.check(L.zd_seekable_open_device(C.c_void_p(src.data_ptr()), len(blob), s, C.byref(self.z)), "open")
        lens = [n for _, n in ranges]
        self.do = np.cumsum([0] + lens)
        self.dst = torch.zeros(int(self.do[-1]) + 64, dtype=torch.uint8, device=dev)
        t = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
        self.arrs = (t([o for o, _ in ranges]), t(lens), t([self.dst.data_ptr() + int(o) for o in self.do[:-1]]))
        torch.cuda.synchronize()
        self.h = C.c_void_p()
        a = [C.c_void_p(x.data_ptr()) for x in self.arrs]
        if hasattr(L, "zd_seekable_read_create_ex"):
            _lib.check(L.zd_seekable_read_create_ex(self.z, *a, len(ranges), flags, read_flags, s, C.byref(self.h)),
                       "zd_seekable_read_create_ex")
        else:
            assert not read_flags
            _lib.check(L.zd_seekable_read_create(self.z, *a, len(ranges), flags, s, C.byref(self.h)),
                       "zd_seekable_read_create")
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
        if self.read_flags:
            ok, n = C.c_void_p(), C.c_uint64()
            _lib.check(self.L.zd_seek_read_device_verdicts(self.h, None, C.byref(ok), None, C.byref(n)))
            torch.cuda.synchronize()
            from zstd_decompressor.seekable import _read_device
            v = _read_device(ok.value or 0, C.c_int8, n.value)
            if n.value != self.info.frames_decoded or any(x != 1 for x in v):
                raise SystemExit("a verified read whose verdicts are not all 1")

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
        self.h = C.c_void_p()
        _lib.check(L.zd_batch_create_device(*[C.c_void_p(a.data_ptr()) for a in self.arrs], arc.n, 0, None,
                                            C.c_void_p(stream().cuda_stream), C.byref(self.h)), "zd_batch_create_device")
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


def run(name, sides, extra):
    ms = race(sides)
    for s in sides.values():
        s.check()
    res = dict({"comparison": name, "reps": args.reps, "warmup": WARMUP, "ms": ms}, **extra)
    fin = {k: stats(s.finish_ms) for k, s in sides.items() if getattr(s, "finish_ms", None)}
    if fin:
        res["finish_async_ms"] = fin
    first = next(iter(sides.values()))
    if isinstance(first, ReadSide):
        res.update(frames_decoded=first.info.frames_decoded, frames_in_place=first.info.frames_in_place,
                   staged_bytes=first.info.staged_bytes)
    keys = list(sides)
    res["first_over_second"] = round(ms[keys[0]]["median"] / ms[keys[1]]["median"], 4)
    if len(fin) == 2:
        res["finish_async_difference_ms"] = round(fin[keys[0]]["median"] - fin[keys[1]]["median"], 4)
    emit(res)
    for s in sides.values():
        s.close()


def workloads():
    total = max(2 << 20, int((1 << 30) * args.scale))
    seq = Arc(total, 1 << 20, 0x5EE4A)
    rec = Arc(total, 128 << 10, 0x5EE4B)
    rng = np.random.default_rng(0x5EE4C)
    n = max(1, int(8192 * args.scale))
    return seq, [(0, seq.total)], rec, [(int(o), 4096) for o in rng.integers(0, rec.total - 4096, size=n)]


def main():
    L = _lib.lib()
    V, F = _lib.SEEK_VERIFY_TABLE, _lib.F_VERIFY_CHECKSUM
    seq, seq_ranges, rec, rec_ranges = workloads()
    A = "one range over 1 GiB of 1 MiB entries"
    B = "8192 ranges of 4 KiB at random offsets of 1 GiB of 128 KiB entries"
    if args.only in (None, "a"):
        run("a: " + A + ": ZD_SEEK_VERIFY_TABLE / without",
            {"verified": ReadSide(L, seq, seq_ranges, 0, V), "plain": ReadSide(L, seq, seq_ranges)},
            {"entries": seq.n, "content_bytes": seq.total})
    if args.only in (None, "b"):
        run("b: " + B + ": ZD_SEEK_VERIFY_TABLE / without",
            {"verified": ReadSide(L, rec, rec_ranges, 0, V), "plain": ReadSide(L, rec, rec_ranges)},
            {"entries": rec.n, "ranges": len(rec_ranges), "content_bytes": rec.total})
    if args.only in (None, "c"):
        for name, arc, ranges in ((A, seq, seq_ranges), (B, rec, rec_ranges)):
            run("c: " + name + ", a Content_Checksum in every frame: ZD_F_VERIFY_CHECKSUM with ZD_SEEK_VERIFY_TABLE / alone",
                {"both": ReadSide(L, arc, ranges, F, V, own=True), "frames_only": ReadSide(L, arc, ranges, F, 0, own=True)},
                {"entries": arc.n, "content_bytes": arc.total})
    if args.only in (None, "d"):
        if not args.parent:
            raise SystemExit("comparison d needs --parent LIB")
        P = load(args.parent)
        run("d: " + A + ", unverified: this build / the parent commit's",
            {"new": ReadSide(L, seq, seq_ranges), "parent": ReadSide(P, seq, seq_ranges)}, {"entries": seq.n})
        run("d: " + B + ", unverified: this build / the parent commit's",
            {"new": ReadSide(L, rec, rec_ranges), "parent": ReadSide(P, rec, rec_ranges)}, {"entries": rec.n})
        run("d: plain device batch, 8192 x 128 KiB frames: this build / the parent commit's",
            {"new": DeviceBatchSide(L, rec), "parent": DeviceBatchSide(P, rec)}, {"chunks": rec.n})


if __name__ == "__main__":
    main()
