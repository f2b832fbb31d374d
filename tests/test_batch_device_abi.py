"""CPU-side checks of zd_batch_create_device / zd_batch_create_device_dicts
(include/zd.h): the two symbols are exported and bound, the ABI version stays
8 and zd_batch_info keeps its 80 bytes with device_built where `reserved` was,
and every whole-call argument error comes back before any HIP call -- this
file runs without a GPU, on made-up device addresses that nothing reads."""
import ctypes as C

NEW = ("zd_batch_create_device", "zd_batch_create_device_dicts")
FAKE = [0x10000, 0x20000, 0x30000, 0x40000]          # "device arrays": never dereferenced by these calls


def create(L, arrs, n, flags=0, out=True, fn="zd_batch_create_device", handle=None):
    h = C.c_void_p()
    st = getattr(L, fn)(*[C.c_void_p(a) if a else None for a in arrs], n, flags, handle, None,
                        C.byref(h) if out else None)
    return st, h


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
    assert callable(zstd_decompressor.Batch.from_device)


def test_device_built_sits_where_reserved_was():
    from zstd_decompressor import _lib
    names = [f[0] for f in _lib.BatchInfo._fields_]
    assert "reserved" not in names
    # uint32_t executors at 40, then the old `reserved` word at 44, the four phases from 48
    assert _lib.BatchInfo.executors.offset == 40
    assert _lib.BatchInfo.device_built.offset == 44 and _lib.BatchInfo.device_built.size == 4
    assert _lib.BatchInfo.gather_ns.offset == 48 and _lib.BatchInfo.upload_ns.offset == 72


def test_whole_call_argument_errors_need_no_gpu():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for fn in NEW:
        # (the _dicts entry point: a NULL set is ZD_E_INVALID_ARG whatever the rest)
        st, h = create(L, FAKE, 1, out=False, fn=fn)
        assert st == _lib.INVALID_ARG, fn                                  # NULL out
        for flags in (_lib.F_SKIPPABLE, _lib.F_SKIPPABLE | _lib.F_FRAME_SERIAL):
            st, h = create(L, FAKE, 1, flags=flags, fn=fn)
            assert st == _lib.INVALID_ARG and not h.value, (fn, flags)
        st, h = create(L, FAKE, 1 << 31, fn=fn)
        assert st == _lib.INVALID_ARG and not h.value, fn                  # nchunks = 2^31
        for k in range(4):                                                 # a NULL array with nchunks = 1
            arrs = list(FAKE)
            arrs[k] = None
            st, h = create(L, arrs, 1, fn=fn)
            assert st == _lib.INVALID_ARG and not h.value, (fn, k)
    st, h = create(L, [None] * 4, 0, fn="zd_batch_create_device_dicts")
    assert st == _lib.INVALID_ARG and not h.value                          # no set


def test_no_chunks_is_an_empty_batch():
    from zstd_decompressor import _lib
    L = _lib.lib()
    st, h = create(L, [None] * 4, 0)
    assert st == 0 and h.value
    try:
        info = _lib.BatchInfo()
        assert L.zd_batch_info_get(h, C.byref(info)) == 0
        assert info.nchunks == 0 and info.gathered_bytes == 0 and info.device_built == 1
        assert L.zd_batch_decode_async(h, None) == 0
        bad = C.c_uint64(7)
        assert L.zd_batch_results(h, None, None, None, 0, C.byref(bad)) == 0 and bad.value == 0
        assert L.zd_batch_checksums(h, None, None, None) == 0
        st_p, ln_p = C.c_void_p(), C.c_void_p()
        assert L.zd_batch_device_results(h, C.byref(st_p), C.byref(ln_p)) == 0
    finally:
        L.zd_batch_destroy(h)


def test_from_device_without_chunks():
    from zstd_decompressor import Batch
    b = Batch.from_device(0, 0, 0, 0, nchunks=0)
    try:
        assert b.nchunks == 0 and b.info.device_built == 1
        b.decode_async(0)
        assert b.results(0) == ([], [])
        assert b.checksums(0) == ([], [])
    finally:
        b.close()
