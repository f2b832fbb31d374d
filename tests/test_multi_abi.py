"""CPU-side checks of the multi-frame batch's calls (include/zd.h zd_multi_*):
the symbols are declared, exported and bound, the ABI version stays 8,
ZD_SIZES_MULTI_FRAME is 8 and the size query still refuses bits 2 and 4, and
every whole-call argument error comes back before any HIP call -- this file
runs without a GPU, on made-up addresses that nothing reads."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zd_multi_create_device", "zd_multi_decode_async", "zd_multi_finish_async", "zd_multi_device_results",
       "zd_multi_results", "zd_multi_device_frames", "zd_multi_info_get_sized", "zd_multi_destroy")
FAKE = [0x10000, 0x20000, 0x30000, 0x40000]      # "device arrays": never dereferenced by these calls
FAKE_HANDLE = 0x50000                            # a "dictionary" and a "set": looked at only when both are given


def create(L, arrs, n, flags=0, dict_=None, set_=None, out=True):
    h = C.c_void_p()
    st = L.zd_multi_create_device(*[C.c_void_p(a) if a else None for a in arrs], n, flags,
                                  C.c_void_p(dict_) if dict_ else None, C.c_void_p(set_) if set_ else None, None,
                                  C.byref(h) if out else None)
    return st, h


def test_new_symbols_declared_exported_and_bound():
    from zstd_decompressor import _lib
    L = _lib.lib()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "zd.h")).read(), flags=re.S)
    for n in NEW:
        assert re.search(r"\b%s\s*\(" % n, header), n
        assert n in _lib.SIGNATURES, n
        fn = getattr(L, n)
        assert fn.argtypes == _lib.SIGNATURES[n][1] and fn.restype == _lib.SIGNATURES[n][0], n
    assert len(_lib.SIGNATURES["zd_multi_create_device"][1]) == 10
    assert len(_lib.SIGNATURES["zd_multi_results"][1]) == 6
    assert len(_lib.SIGNATURES["zd_multi_device_frames"][1]) == 4
    assert "typedef struct zd_multi zd_multi;" in header
    import zstd_decompressor
    assert callable(zstd_decompressor.MultiFrameBatch) and callable(zstd_decompressor.decode_multi)
    assert "MultiFrameBatch" in zstd_decompressor.__all__ and "decode_multi" in zstd_decompressor.__all__


def test_abi_version_flag_value_and_struct_sizes():
    from zstd_decompressor import _lib
    L = _lib.lib()
    assert L.zd_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "zd.h")).read()
    assert re.search(r"#define\s+ZD_SIZES_MULTI_FRAME\s+8u\b", header)
    assert re.search(r"#define\s+ZD_ABI_VERSION\s+8\b", header)
    assert _lib.SIZES_MULTI_FRAME == 8
    assert C.sizeof(_lib.BatchInfo) == 80
    assert _lib.MultiInfo.batch.offset == 48 and C.sizeof(_lib.MultiInfo) == 48 + C.sizeof(_lib.BatchInfo2)


def test_create_whole_call_argument_errors_need_no_gpu():
    from zstd_decompressor import _lib
    L = _lib.lib()
    st, h = create(L, FAKE, 1, out=False)
    assert st == _lib.INVALID_ARG                                          # NULL out
    for k in range(4):                                                     # a NULL array with nchunks = 1
        arrs = list(FAKE)
        arrs[k] = None
        st, h = create(L, arrs, 1)
        assert st == _lib.INVALID_ARG and not h.value, k
    for n in (1 << 31, 1 << 40):
        st, h = create(L, FAKE, n)
        assert st == _lib.INVALID_ARG and not h.value, n                   # nchunks >= 2^31
    for n in (0, 1):
        st, h = create(L, FAKE, n, dict_=FAKE_HANDLE, set_=FAKE_HANDLE)
        assert st == _lib.INVALID_ARG and not h.value, n                   # both dict and set
    for flags in (_lib.F_SKIPPABLE, _lib.F_SKIPPABLE | _lib.F_RFC, 16, 1 << 15, 1 << 31):
        for n in (0, 1):
            st, h = create(L, FAKE, n, flags=flags)
            assert st == _lib.INVALID_ARG and not h.value, (flags, n)      # ZD_F_SKIPPABLE, unknown bits


def test_a_batch_of_no_chunks_needs_no_gpu():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for flags in (0, _lib.F_RFC | _lib.F_VERIFY_CHECKSUM | _lib.F_LONG_WINDOW | _lib.F_BLOCK_PARALLEL):
        st, h = create(L, [None] * 4, 0, flags=flags)
        assert st == 0 and h.value
        assert L.zd_multi_decode_async(h, None) == 0
        assert L.zd_multi_finish_async(h, None) == 0
        bad = C.c_uint64(7)
        assert L.zd_multi_results(h, None, None, None, 0, C.byref(bad)) == 0 and bad.value == 0
        info = _lib.MultiInfo()
        assert L.zd_multi_info_get_sized(h, C.byref(info), C.sizeof(info)) == 0
        assert (info.nchunks, info.frames, info.staged_bytes, info.copy_pieces) == (0, 0, 0, 0)
        assert L.zd_multi_info_get_sized(h, C.byref(info), 47) == _lib.INVALID_ARG
        assert L.zd_multi_info_get_sized(h, C.byref(info), 48) == 0
        first, fs, fl = C.c_void_p(1), C.c_void_p(1), C.c_void_p(1)
        assert L.zd_multi_device_frames(h, C.byref(first), C.byref(fs), C.byref(fl)) == 0
        assert not fs.value and not fl.value
        L.zd_multi_destroy(h)


def test_calls_on_no_object():
    from zstd_decompressor import _lib
    L = _lib.lib()
    assert L.zd_multi_decode_async(None, None) == _lib.INVALID_ARG
    assert L.zd_multi_finish_async(None, None) == _lib.INVALID_ARG
    assert L.zd_multi_results(None, None, None, None, 0, None) == _lib.INVALID_ARG
    assert L.zd_multi_device_results(None, None, None) == _lib.INVALID_ARG
    assert L.zd_multi_device_frames(None, None, None, None) == _lib.INVALID_ARG
    info = _lib.MultiInfo()
    assert L.zd_multi_info_get_sized(None, C.byref(info), C.sizeof(info)) == _lib.INVALID_ARG
    L.zd_multi_destroy(None)


def test_size_query_flag_bits_need_no_gpu():
    """ZD_SIZES_MULTI_FRAME (8) is a flag of zd_chunk_sizes_device now; bits 2
    and 4 stay ZD_E_INVALID_ARG, with or without it.  nchunks = 0 is ZD_OK
    without a HIP call."""
    from zstd_decompressor import _lib
    L = _lib.lib()
    q = lambda flags, n: L.zd_chunk_sizes_device(C.c_void_p(FAKE[0]), C.c_void_p(FAKE[1]), n, flags,
                                                 C.c_void_p(FAKE[2]), None, None, None)
    for extra in (0, _lib.SIZES_DICT, _lib.SIZES_RFC | _lib.SIZES_LONG_WINDOW):
        assert q(_lib.SIZES_MULTI_FRAME | extra, 0) == 0
    for bad in (2, 4, 16):
        assert q(bad, 0) == _lib.INVALID_ARG and q(bad | _lib.SIZES_MULTI_FRAME, 0) == _lib.INVALID_ARG
    assert q(_lib.SIZES_MULTI_FRAME, 1 << 31) == _lib.INVALID_ARG
    assert L.zd_chunk_sizes_device(None, C.c_void_p(FAKE[1]), 1, _lib.SIZES_MULTI_FRAME, C.c_void_p(FAKE[2]), None,
                                   None, None) == _lib.INVALID_ARG


def test_chunk_sizes_takes_multi_frame():
    import inspect
    from zstd_decompressor import chunk_sizes
    assert inspect.signature(chunk_sizes).parameters["multi_frame"].default is False
