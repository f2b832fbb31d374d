"""Times ZD_F_RFC's cost on two workloads that hold no frame the flag changes
(plain text, zstd -3: the flag must cost nothing there):
  frames   8,192 frames of 128 KiB of gen.text
  records  65,536 records of 4 KiB with a 112 KiB trained dictionary
as scripts/time_verify.py does it: every side is a plan of a library file loaded
into this one process (the same ctypes calls on each), the sides alternating
inside every repetition with the order rotated, --reps repetitions after
warm-up, median (min-max) of zd_decode_async between two device events:
  decode/new       this build, no flag
  decode/parent    --parent (the parent commit's libzd.so), no flag: expected ratio 1,
                   K3 / K4 being the parent's instructions, K1 / K2 one uniform branch more
  decode_rfc/new   this build, the plan made with ZD_F_RFC
Every decode's status and length are checked, and the flagged plan's bytes
against the unflagged plan's once.  Appends one JSON line per workload.
usage: python scripts/time_rfc.py OUT.jsonl --parent LIB [--reps 9] [--scale F] [--only NAME]"""
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
ap.add_argument("--reps", type=int, default=9)
ap.add_argument("--scale", type=float, default=1.0, help="fraction of each workload's size")
ap.add_argument("--unique-mib", type=int, default=64)
ap.add_argument("--only", choices=("frames", "records"))
args = ap.parse_args()
WARMUP = 2
dev = torch.device("cuda", 0)


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


def inside(a, b):
    """a's median within b's min-max"""
    return b["min"] <= a["median"] <= b["max"]


def workload(name, frames, sources_bytes, libs, dictionary):
    data = b"".join(frames)
    d_src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    d_src[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    d_dst = torch.zeros(sources_bytes + 64, dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev)
    sp, dp, st = d_src.data_ptr(), d_dst.data_ptr(), s.cuda_stream
    sides = {"decode/new": ("new", 0), "decode/parent": ("parent", 0), "decode_rfc/new": ("new", _lib.F_RFC)}
    plans = {k: Plan(libs[lib], data, flags, dictionary) for k, (lib, flags) in sides.items()}
    ms = {k: [] for k in sides}
    keys = list(plans)
    digest = {}
    for rep in range(WARMUP + args.reps):
        for k in keys[rep % len(keys):] + keys[:rep % len(keys)]:
            p = plans[k]
            t = timed(lambda: p.decode(sp, dp, st), s)
            r, total = p.results(dp, st)
            if r != 0 or total != sources_bytes:
                raise SystemExit(f"{name}: {k}: status {r}, {total} bytes")
            if rep == 0:
                digest[k] = int(d_dst[:sources_bytes].view(torch.int64)[: sources_bytes // 8].sum().item())
            if rep >= WARMUP:
                ms[k].append(t)
    if len(set(digest.values())) != 1:
        raise SystemExit(f"{name}: the sides' outputs differ: {digest}")
    executors = plans["decode/new"].info.executors
    for p in plans.values():
        p.close()
    S = {k: stats(v) for k, v in ms.items()}
    return {"workload": name, "frames": len(frames), "compressed_bytes": len(data), "decoded_bytes": sources_bytes,
            "reps": args.reps, "warmup": WARMUP, "executors": executors, "ms": S,
            "decode_new_over_parent": round(S["decode/new"]["median"] / S["decode/parent"]["median"], 4),
            "new_and_parent_medians_inside_each_other": inside(S["decode/new"], S["decode/parent"]) and
            inside(S["decode/parent"], S["decode/new"]),
            "rfc_over_unflagged": round(S["decode_rfc/new"]["median"] / S["decode/new"]["median"], 4),
            "rfc_and_unflagged_medians_inside_each_other": inside(S["decode_rfc/new"], S["decode/new"]) and
            inside(S["decode/new"], S["decode_rfc/new"])}


def main():
    libs = {"new": _lib.lib(), "parent": load(args.parent)}
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
        unique = compress_all([text[i:i + chunk] for i in range(0, nu * chunk, chunk)], lambda r: libzstd.compress(r, 3))
        emit(workload("8192 x 128 KiB gen.text, zstd -3", (unique * ((n + nu - 1) // nu))[:n], n * chunk, libs, None))
    if args.only in (None, "records"):
        rec, n = 4096, max(1, int(65536 * args.scale))
        train = gen.text(2048 * rec, seed=0xD1C2)
        dct = zdict.train([train[i:i + rec] for i in range(0, len(train), rec)], 112 << 10)
        nu = min(n, max(1, (args.unique_mib << 20) // rec))
        text = gen.text(nu * rec, seed=0xD1C5)
        unique = compress_all([text[i:i + rec] for i in range(0, nu * rec, rec)], lambda r: zdict.compress(r, dct, 3))
        emit(workload("65536 x 4 KiB gen.text, zstd -3, 112 KiB dictionary", (unique * ((n + nu - 1) // nu))[:n],
                      n * rec, libs, dct))


if __name__ == "__main__":
    main()
