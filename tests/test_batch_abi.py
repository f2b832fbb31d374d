"""CPU-side checks of the batch additions to the C ABI (include/zd.h zd_batch):
the seven symbols are exported and bound, the ABI version stays 8, and
zd_batch_create's argument checks come before any HIP call -- this file runs
without a GPU, on made-up pointer values that nothing dereferences."""
import ctypes as C

NEW = ("zd_batch_create", "zd_batch_info_get", "zd_batch_decode_async", "zd_batch_device_results",
       "zd_batch_results", "zd_batch_checksums", "zd_batch_destroy")


def arrays(srcs, sizes, dsts, caps):
    n = len(srcs)
    return ((C.c_void_p * n)(*srcs), (C.c_uint64 * n)(*sizes), (C.c_void_p * n)(*dsts), (C.c_uint64 * n)(*caps), n)


def create(L, sp, ss, dp, dc, n, flags=0):
    h = C.c_void_p()
    st = L.zd_batch_create(sp, ss, dp, dc, n, flags, None, None, C.byref(h))
    assert st != 0 and not h.value
    return st


def test_new_symbols_exported_and_bound():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for n in NEW:
        assert n in _lib.SIGNATURES, n
        fn = getattr(L, n)
        assert fn.argtypes == _lib.SIGNATURES[n][1] and fn.restype == _lib.SIGNATURES[n][0], n
    import zstd_decompressor
    assert zstd_decompressor.Batch is zstd_decompressor.batch.Batch
    assert zstd_decompressor.decode_tensors is zstd_decompressor.batch.decode_tensors
    assert C.sizeof(_lib.BatchInfo) == 80


def test_abi_version_unchanged():
    from zstd_decompressor import _lib
    assert _lib.lib().zd_abi_version() == 8


def test_null_arrays_are_invalid():
    from zstd_decompressor import _lib
    L = _lib.lib()
    sp, ss, dp, dc, n = arrays([0x10000, 0x20000], [64, 64], [0x30000, 0x40000], [128, 128])
    for k in range(4):
        args = [sp, ss, dp, dc]
        args[k] = None
        assert create(L, *args, n) == _lib.INVALID_ARG, k
    assert L.zd_batch_create(sp, ss, dp, dc, n, 0, None, None, None) == _lib.INVALID_ARG


def test_null_entries_are_invalid():
    from zstd_decompressor import _lib
    L = _lib.lib()
    # a NULL source with bytes, a NULL destination with capacity
    assert create(L, *arrays([0x10000, None], [64, 64], [0x30000, 0x40000], [128, 128])) == _lib.INVALID_ARG
    assert create(L, *arrays([0x10000, 0x20000], [64, 64], [0x30000, None], [128, 128])) == _lib.INVALID_ARG


def test_skippable_flag_is_invalid():
    from zstd_decompressor import _lib
    L = _lib.lib()
    a = arrays([0x10000, 0x20000], [64, 64], [0x30000, 0x40000], [128, 128])
    assert create(L, *a, flags=_lib.F_SKIPPABLE) == _lib.INVALID_ARG
    assert create(L, *a, flags=_lib.F_SKIPPABLE | _lib.F_FRAME_SERIAL) == _lib.INVALID_ARG


def test_overlapping_destinations_are_invalid():
    from zstd_decompressor import _lib
    L = _lib.lib()
    src, sz = [0x10000, 0x20000, 0x28000], [64, 64, 64]
    # the second range starts inside the first, given in either order, and
    # with a third range between them in the arrays
    for dsts, caps in (([0x30000, 0x30040, 0x50000], [128, 128, 16]),
                       ([0x30040, 0x50000, 0x30000], [128, 16, 128]),
                       ([0x30000, 0x50000, 0x3007F], [128, 16, 1]),
                       ([0x30000, 0x30000, 0x50000], [1, 1, 16])):
        assert create(L, *arrays(src, sz, dsts, caps)) == _lib.INVALID_ARG, (dsts, caps)


def test_destroy_null_is_harmless():
    from zstd_decompressor import _lib
    L = _lib.lib()
    L.zd_batch_destroy(None)
    assert L.zd_batch_info_get(None, None) == _lib.INVALID_ARG
    assert L.zd_batch_decode_async(None, None) == _lib.INVALID_ARG
    assert L.zd_batch_results(None, None, None, None, 0, None) == _lib.INVALID_ARG
    assert L.zd_batch_checksums(None, None, None, None) == _lib.INVALID_ARG
    assert L.zd_batch_device_results(None, None, None) == _lib.INVALID_ARG
