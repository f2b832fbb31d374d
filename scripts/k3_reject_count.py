"""Blocks K3Q hands to the exact chain, counted by a ZD_K3_COUNT variant build.

    make -C zstd-decompressor_amd variant NAME=c_b24 DEFS="-DZD_K3_COUNT -DZD_K3H_BITS=24"
    ZD_LIB_PATH=zstd-decompressor_amd/lib/variants/libzd_c_b24.so \
        python scripts/k3_reject_count.py c4:1024 c5:256:1 c5:256:9 c5:256:19

Each argument is workload:unique MiB[:level], the corpus bench.py makes for
it (one replica; corpus/cache/ is used when it holds the frames).  Every plan
is made with ZD_F_SEQ_NO_LATENCY | ZD_F_NO_FUSE, so K3Q runs whatever the
plan's size (neither K3L nor zd_k_fused, whose chains are not counted).
Prints one JSON line per corpus: blocks run by K3Q, blocks on the half-window
chain, rejects of seq_chainq and of seq_chainqh.
"""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "zstd-decompressor_amd")):
    sys.path.insert(0, p)


def main():
    import torch
    import bench
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Plan
    L = _lib.lib()
    L.zd_debug_k3_count.restype = C.c_int
    L.zd_debug_k3_count.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    dev = torch.device("cuda", 0)
    for spec in sys.argv[1:]:
        w, mib, *lv = spec.split(":")
        level = int(lv[0]) if lv else 9
        data = bench.cached_corpus(w, int(mib), 0x5EED, level, cache_dir=bench.default_corpus_cache())[0]
        plan = Plan(data, flags=_lib.F_SEQ_NO_LATENCY | _lib.F_NO_FUSE)
        assert not plan.info.executors & _lib.EXEC_FUSED
        info = plan.info
        d_src = torch.empty(len(data) + 64, dtype=torch.uint8, device=dev)
        d_src[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        d_dst = torch.empty(info.out_bytes + 64, dtype=torch.uint8, device=dev)
        sptr = torch.cuda.current_stream(dev).cuda_stream
        v = (C.c_ulonglong * 4)()
        torch.cuda.synchronize(dev)
        assert L.zd_debug_k3_count(v, 1) == 0
        plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), info.out_bytes, sptr)
        torch.cuda.synchronize(dev)
        st, total, _, _, _ = plan.results(d_dst.data_ptr(), sptr)
        assert L.zd_debug_k3_count(v, 1) == 0
        print(json.dumps({"lib": os.path.basename(_lib.LIB_PATH), "corpus": spec, "status": st,
                          "compressed_blocks": info.ncompressed, "k3q_blocks": v[0], "half_window_blocks": v[1],
                          "rejects_full": v[2], "rejects_half": v[3]}), flush=True)
        plan.close()
        del d_src, d_dst


if __name__ == "__main__":
    main()
