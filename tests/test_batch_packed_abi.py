"""CPU-side checks of the size query and the packed batches (include/zd.h
zd_chunk_sizes_device, zd_batch_create_device_packed / _dicts,
zd_batch_output_layout, zd_batch_bind_output): the symbols are exported and
bound, the ABI version stays 8 and zd_batch_info its 80 bytes, and every
whole-call argument error comes back before any HIP call -- this file runs
without a GPU, on made-up device addresses that nothing reads."""
import ctypes as C

import pytest

NEW = ("zd_chunk_sizes_device", "zd_batch_create_device_packed", "zd_batch_create_device_packed_dicts",
       "zd_batch_output_layout", "zd_batch_bind_output")
CREATE = ("zd_batch_create_device_packed", "zd_batch_create_device_packed_dicts")
FAKE = [0x10000, 0x20000]                 # "device arrays": never dereferenced by these calls
FAKE_OUT = [0x30000, 0x40000, 0x50000]


def vp(a):
    return C.c_void_p(a) if a else None


def create(L, arrs, n, align=16, flags=0, out=True, fn=CREATE[0], handle=None):
    h = C.c_void_p()
    st = getattr(L, fn)(vp(arrs[0]), vp(arrs[1]), n, align, flags, handle, None, C.byref(h) if out else None)
    return st, h


def sizes(L, arrs, n, flags=0, outs=FAKE_OUT):
    return L.zd_chunk_sizes_device(vp(arrs[0]), vp(arrs[1]), n, flags, vp(outs[0]), vp(outs[1]), vp(outs[2]), None)


def test_new_symbols_exported_and_bound():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for n in NEW:
        assert n in _lib.SIGNATURES, n
        fn = getattr(L, n)
        assert fn.argtypes == _lib.SIGNATURES[n][1] and fn.restype == _lib.SIGNATURES[n][0], n
    assert L.zd_abi_version() == 8
    assert C.sizeof(_lib.BatchInfo) == 80
    import zstd_decompressor
    assert callable(zstd_decompressor.Batch.packed) and callable(zstd_decompressor.chunk_sizes)
    assert callable(zstd_decompressor.decompress_tensors)
    assert _lib.SIZES_DICT == 1


def test_packed_creation_argument_errors_need_no_gpu():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for fn in CREATE:
        # (the _dicts entry point: a NULL set is ZD_E_INVALID_ARG whatever the rest)
        st, h = create(L, FAKE, 1, out=False, fn=fn)
        assert st == _lib.INVALID_ARG, fn                                  # NULL out
        for flags in (_lib.F_SKIPPABLE, _lib.F_SKIPPABLE | _lib.F_FRAME_SERIAL):
            st, h = create(L, FAKE, 1, flags=flags, fn=fn)
            assert st == _lib.INVALID_ARG and not h.value, (fn, flags)
        st, h = create(L, FAKE, 1 << 31, fn=fn)
        assert st == _lib.INVALID_ARG and not h.value, fn                  # nchunks = 2^31
        for k in range(2):                                                 # a NULL array with nchunks = 1
            arrs = list(FAKE)
            arrs[k] = None
            st, h = create(L, arrs, 1, fn=fn)
            assert st == _lib.INVALID_ARG and not h.value, (fn, k)
    for align in (0, 3, 8192, 48, 1 << 31):
        for n in (0, 1):
            st, h = create(L, FAKE, n, align=align)
            assert st == _lib.INVALID_ARG and not h.value, (align, n)
    st, h = create(L, [None] * 2, 0, fn=CREATE[1])
    assert st == _lib.INVALID_ARG and not h.value                          # no set


def test_size_query_argument_errors_need_no_gpu():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for k in range(2):
        arrs = list(FAKE)
        arrs[k] = None
        assert sizes(L, arrs, 1) == _lib.INVALID_ARG, k
    assert sizes(L, FAKE, 1, outs=[None, 0x40000, 0x50000]) == _lib.INVALID_ARG     # NULL d_size
    assert sizes(L, FAKE, 1 << 31) == _lib.INVALID_ARG
    for flags in (2, 4, 0x80000000, _lib.SIZES_DICT | 2):
        assert sizes(L, FAKE, 1, flags=flags) == _lib.INVALID_ARG, flags
        assert sizes(L, FAKE, 0, flags=flags) == _lib.INVALID_ARG, flags
    # no chunks: ZD_OK without a HIP call, whatever the arrays
    assert sizes(L, [None] * 2, 0, outs=[None] * 3) == 0
    assert sizes(L, FAKE, 0, flags=_lib.SIZES_DICT) == 0


@pytest.mark.parametrize("align", [1, 16, 4096])
def test_no_chunks_is_an_empty_packed_batch(align):
    from zstd_decompressor import _lib
    L = _lib.lib()
    st, h = create(L, [None] * 2, 0, align=align)
    assert st == 0 and h.value
    try:
        info = _lib.BatchInfo()
        assert L.zd_batch_info_get(h, C.byref(info)) == 0
        assert info.nchunks == 0 and info.gathered_bytes == 0 and info.device_built == 1
        ob, off, cap = C.c_uint64(7), C.c_void_p(), C.c_void_p()
        assert L.zd_batch_output_layout(h, C.byref(ob), C.byref(off), C.byref(cap)) == 0
        assert ob.value == 0
        assert L.zd_batch_output_layout(h, None, None, None) == 0
        assert L.zd_batch_decode_async(h, None) == 0                       # nothing to bind
        assert L.zd_batch_bind_output(h, None, 0) == 0
        assert L.zd_batch_bind_output(h, C.c_void_p(0x1001), 5) == 0
        assert L.zd_batch_bind_output(h, C.c_void_p((1 << 64) - 8), 16) == _lib.INVALID_ARG   # the range wraps
        assert L.zd_batch_decode_async(h, None) == 0
        bad = C.c_uint64(7)
        assert L.zd_batch_results(h, None, None, None, 0, C.byref(bad)) == 0 and bad.value == 0
        assert L.zd_batch_checksums(h, None, None, None) == 0
    finally:
        L.zd_batch_destroy(h)


def test_layout_and_binding_refuse_other_batches():
    from zstd_decompressor import _lib
    L = _lib.lib()
    ob = C.c_uint64()
    assert L.zd_batch_output_layout(None, C.byref(ob), None, None) == _lib.INVALID_ARG
    assert L.zd_batch_bind_output(None, C.c_void_p(0x1000), 16) == _lib.INVALID_ARG
    # a batch that was not made packed (an empty one needs no GPU)
    h = C.c_void_p()
    assert L.zd_batch_create_device(None, None, None, None, 0, 0, None, None, C.byref(h)) == 0
    try:
        assert L.zd_batch_output_layout(h, C.byref(ob), None, None) == _lib.INVALID_ARG
        assert L.zd_batch_bind_output(h, None, 0) == _lib.INVALID_ARG
    finally:
        L.zd_batch_destroy(h)


def test_packed_without_chunks():
    from zstd_decompressor import Batch
    b = Batch.packed(0, 0, nchunks=0)
    try:
        assert b.nchunks == 0 and b.info.device_built == 1 and b.out_bytes == 0
        b.bind_output(0, 0)
        b.decode_async(0)
        assert b.results(0) == ([], [])
        assert b.checksums(0) == ([], [])
    finally:
        b.close()
