"""Times ZD_F_VERIFY_CHECKSUM (zd_k_verify, the checksum pass inside the decode
launch) on three checksummed workloads:
  frames   8,192 frames of 128 KiB of gen.text, zstd -3
  records  65,536 records of 4 KiB with a 112 KiB trained dictionary
  single   one 100 MB frame
Every side is a library file loaded into this one process (the same ctypes
calls on each), the sides alternating inside every repetition, --reps
repetitions after warm-up, min / median / max:
  decode            zd_decode_async without the flag: this build against --parent
                    (the parent commit built with `make variant`); expected ratio 1
  decode_verified   the same plan made with the flag: the added time per decode
  zd_k_verify       the pass alone, profiling mode 1's entry: this build against
                    --words (this commit built with -DZD_VERIFY_WORDS: zd_k_xxh64's
                    8-byte loads 32 bytes apart as the body)
  parent_checksums  events around the parent's zd_plan_checksums (zd_k_xxh64 with
                    its two uploads and its download: what a caller paid before)
Each GPU step of a workload runs between its own device events; a step that
fails ends the script.  Appends one JSON line per workload to the output file.
usage: python scripts/time_verify.py OUT.jsonl --parent LIB [--words LIB] [--reps 9] [--scale F] [--only NAME]
                                      [--prewarm]"""
import argparse
import concurrent.futures as cf
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "zstd-decompressor_amd")]

import torch  # noqa: E402

from corpus import gen, libzstd, zdict  # noqa: E402
from zstd_decompressor import _lib  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("out")
ap.add_argument("--parent", required=True, help="libzd.so of the parent commit")
ap.add_argument("--words", help="libzd.so of this commit built with -DZD_VERIFY_WORDS")
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's size")
ap.add_argument("--unique-mib", type=int, default=64)
ap.add_argument("--only", choices=("frames", "records", "single"))
ap.add_argument("--prewarm", action="store_true", help="an untimed decode of the same plan before every timed one")
args = ap.parse_args()
WARMUP = 2
dev = torch.device("cuda", 0)
VERIFY = _lib.F_VERIFY_CHECKSUM


def load(path):
    """A library file with include/zd.h's signatures (the parent lacks the newest entry points)."""
    L = C.CDLL(path)
    for name, (res, argt) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, argt
    return L


class Plan:
    """zd_plan of library L over host bytes (dictionary: the raw bytes of one, or None)."""

    def __init__(self, L, data, flags, dictionary=None):
        self.L, self.h, self.d = L, C.c_void_p(), C.c_void_p()
        p, n, self.keep = _lib.buf(data)
        if dictionary is not None:
            dp, dn, self.dkeep = _lib.buf(dictionary)
            _lib.check(L.zd_dict_create(dp, dn, C.byref(self.d)), "zd_dict_create")
            _lib.check(L.zd_plan_create_dict(p, n, flags, self.d, C.byref(self.h)), "zd_plan_create_dict")
        else:
            _lib.check(L.zd_plan_create(p, n, flags, C.byref(self.h)), "zd_plan_create")
        self.info = _lib.PlanInfo()
        _lib.check(L.zd_plan_info_get(self.h, C.byref(self.info)))

    def decode(self, d_src, d_dst, stream):
        _lib.check(self.L.zd_decode_async(self.h, C.c_void_p(d_src), C.c_void_p(d_dst), self.info.out_bytes,
                                          C.c_void_p(stream)), "zd_decode_async")

    def results(self, d_dst, stream):
        total, first = C.c_uint64(), C.c_int32()
        st = self.L.zd_plan_results(self.h, C.c_void_p(d_dst), C.c_void_p(stream), None, None, C.byref(total),
                                    C.byref(first))
        return st, total.value

    def checksums(self, d_dst, stream):
        nf = self.info.nframes
        ok = (C.c_int32 * nf)()
        _lib.check(self.L.zd_plan_checksums(self.h, C.c_void_p(d_dst), C.c_void_p(stream), ok, None))
        return list(ok)

    def kernel_times(self):
        names, ms, n = (C.c_char_p * 8)(), (C.c_float * 8)(), C.c_int()
        _lib.check(self.L.zd_plan_kernel_times(self.h, names, ms, 8, C.byref(n)))
        return {names[i].decode(): ms[i] for i in range(n.value)}

    def close(self):
        self.L.zd_plan_destroy(self.h)
        if self.d:
            self.L.zd_dict_destroy(self.d)


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def timed(fn, stream):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    fn()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def compress_all(pieces, fn):
    with cf.ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:      # ctypes drops the GIL
        return list(ex.map(fn, pieces, chunksize=64))


def workload(name, frames, sources_bytes, libs, dictionary):
    data = b"".join(frames)
    d_src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    d_src[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    d_dst = torch.zeros(sources_bytes + 64, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev)
    sp, dp, st = d_src.data_ptr(), d_dst.data_ptr(), s.cuda_stream
    # the sides: (library, flags, profiling mode)
    sides = {"decode/new": ("new", 0, 0), "decode/parent": ("parent", 0, 0), "decode_verified/new": ("new", VERIFY, 0),
             "zd_k_verify/new": ("new", VERIFY, 1)}
    if "words" in libs:
        sides["zd_k_verify/words"] = ("words", VERIFY, 1)
    plans = {k: Plan(libs[lib], data, flags, dictionary) for k, (lib, flags, _) in sides.items()}
    for k, (_, _, mode) in sides.items():
        if mode:
            _lib.check(plans[k].L.zd_plan_set_profiling(plans[k].h, mode))
    ms = {k: [] for k in sides}
    ms["parent_checksums/parent"] = []
    keys = list(plans)
    for rep in range(WARMUP + args.reps):
        # alternating, the order rotated every repetition.  --prewarm: every timed decode behind
        # an untimed one of the same plan (the side that runs behind the single frame's 0.2-0.4 s
        # pass, one busy wave on an idle chip, measures 1-2 % slower than the side behind a decode)
        for k in keys[rep % len(keys):] + keys[:rep % len(keys)]:
            p = plans[k]
            if args.prewarm:
                p.decode(sp, dp, st)
                p.results(dp, st)
            t = timed(lambda: p.decode(sp, dp, st), s)
            r, total = p.results(dp, st)
            if r != 0 or total != sources_bytes:
                raise SystemExit(f"{name}: {k}: status {r}, {total} bytes")
            if sides[k][2]:
                t = p.kernel_times()["zd_k_verify"]
            if rep >= WARMUP:
                ms[k].append(t)
            if k == "decode/parent":
                t = timed(lambda: p.checksums(dp, st), s)
                if rep >= WARMUP:
                    ms["parent_checksums/parent"].append(t)
    ok = plans["decode/new"].checksums(dp, st)
    if any(v != 1 for v in ok):
        raise SystemExit(f"{name}: a checksum does not match")
    executors = plans["decode/new"].info.executors
    for p in plans.values():
        p.close()
    med = {k: statistics.median(v) for k, v in ms.items()}
    res = {"workload": name, "frames": len(frames), "compressed_bytes": len(data), "decoded_bytes": sources_bytes,
           "reps": args.reps, "warmup": WARMUP, "prewarm": args.prewarm, "executors": executors, "ms": {k: stats(v) for k, v in ms.items()},
           "decode_new_over_parent": round(med["decode/new"] / med["decode/parent"], 4),
           "verify_added_ms": round(med["decode_verified/new"] - med["decode/new"], 4),
           "verify_added_share_of_decode": round((med["decode_verified/new"] - med["decode/new"]) / med["decode/new"], 4),
           "zd_k_verify_gbps": round(sources_bytes / med["zd_k_verify/new"] / 1e6, 1),
           "parent_checksums_over_zd_k_verify": round(med["parent_checksums/parent"] / med["zd_k_verify/new"], 3)}
    if "words" in libs:
        res["words_over_lines"] = round(med["zd_k_verify/words"] / med["zd_k_verify/new"], 3)
        res["zd_k_verify_words_gbps"] = round(sources_bytes / med["zd_k_verify/words"] / 1e6, 1)
    return res


def main():
    libs = {"new": _lib.lib(), "parent": load(args.parent)}
    if args.words:
        libs["words"] = load(args.words)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(res):
        line = json.dumps(res)
        print(line, flush=True)
        with open(args.out, "a") as f:
            f.write(line + "\n")
    if args.only in (None, "frames"):
        chunk, n = 128 << 10, max(1, int(8192 * args.scale))
        nu = min(n, max(1, (args.unique_mib << 20) // chunk))
        text = gen.text(nu * chunk, seed=0xBA7C0)
        unique = compress_all([text[i:i + chunk] for i in range(0, nu * chunk, chunk)],
                              lambda r: libzstd.compress(r, 3, checksum=True))
        emit(workload("8192 x 128 KiB gen.text, zstd -3, checksummed", (unique * ((n + nu - 1) // nu))[:n], n * chunk,
                      libs, None))
    if args.only in (None, "records"):
        rec, n = 4096, max(1, int(65536 * args.scale))
        train = gen.text(2048 * rec, seed=0xD1C2)
        dct = zdict.train([train[i:i + rec] for i in range(0, len(train), rec)], 112 << 10)
        nu = min(n, max(1, (args.unique_mib << 20) // rec))
        text = gen.text(nu * rec, seed=0xD1C5)
        unique = compress_all([text[i:i + rec] for i in range(0, nu * rec, rec)],
                              lambda r: zdict.compress(r, dct, 3, checksum=True))
        emit(workload("65536 x 4 KiB gen.text, zstd -3, 112 KiB dictionary, checksummed",
                      (unique * ((n + nu - 1) // nu))[:n], n * rec, libs, dct))
    if args.only in (None, "single"):
        size = max(1 << 20, int(100_000_000 * args.scale))
        text = gen.text(size, seed=0x51461)[:size]
        emit(workload("one 100 MB frame, zstd -3, checksummed", [libzstd.compress(text, 3, checksum=True)], size, libs,
                      None))


if __name__ == "__main__":
    main()
