"""CPU-side checks of the verified seekable reads (include/zd.h
zd_seekable_read_create_ex, ZD_SEEK_VERIFY_TABLE, zd_seek_read_device_verdicts,
zd_seek_read_info_get_sized): the symbols are exported and bound, the info
struct grew behind its 136 bytes and the ABI version stays 8, and every
whole-call argument error comes back before any HIP call -- this file runs
without a GPU, on made-up addresses that nothing reads."""
import ctypes as C

NEW = ("zd_seekable_read_create_ex", "zd_seek_read_device_verdicts", "zd_seek_read_info_get_sized")
FAKE = [0x10000, 0x20000, 0x30000]        # "device arrays": never dereferenced by these calls
FAKE_ARCHIVE = 0x50000                    # an "open archive": never dereferenced before the arguments are checked


def create_ex(L, z, arrs, n, flags=0, read_flags=0, out=True):
    h = C.c_void_p()
    st = L.zd_seekable_read_create_ex(C.c_void_p(z) if z else None, *[C.c_void_p(a) if a else None for a in arrs], n,
                                      flags, read_flags, None, C.byref(h) if out else None)
    return st, h


def test_new_symbols_exported_and_bound():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for n in NEW:
        assert n in _lib.SIGNATURES, n
        fn = getattr(L, n)
        assert fn.argtypes == _lib.SIGNATURES[n][1] and fn.restype == _lib.SIGNATURES[n][0], n
    assert len(_lib.SIGNATURES["zd_seekable_read_create_ex"][1]) == 9
    assert len(_lib.SIGNATURES["zd_seek_read_device_verdicts"][1]) == 5
    assert _lib.SEEK_VERIFY_TABLE == 1
    from zstd_decompressor import SeekableArchive, seekable
    assert callable(SeekableArchive.verify_all) and callable(seekable.SeekReader.verdicts)


def test_struct_sizes_and_abi_version():
    from zstd_decompressor import _lib
    L = _lib.lib()
    assert L.zd_abi_version() == 8
    assert C.sizeof(_lib.SeekReadInfo) == 136
    assert C.sizeof(_lib.SeekReadInfo2) == C.sizeof(_lib.SeekReadInfo) + 16
    assert _lib.SeekReadInfo2.read_flags.offset == 136 and _lib.SeekReadInfo2.verify_entries.offset == 144


def test_create_ex_whole_call_argument_errors_need_no_gpu():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for rf in (0, _lib.SEEK_VERIFY_TABLE):
        st, h = create_ex(L, FAKE_ARCHIVE, FAKE, 1, read_flags=rf, out=False)
        assert st == _lib.INVALID_ARG                                      # NULL out
        for k in range(3):                                                 # a NULL array with nranges = 1
            arrs = list(FAKE)
            arrs[k] = None
            st, h = create_ex(L, FAKE_ARCHIVE, arrs, 1, read_flags=rf)
            assert st == _lib.INVALID_ARG and not h.value, k
        st, h = create_ex(L, FAKE_ARCHIVE, FAKE, 1 << 31, read_flags=rf)
        assert st == _lib.INVALID_ARG and not h.value                      # nranges = 2^31
        for flags in (_lib.F_SKIPPABLE, _lib.F_SKIPPABLE | _lib.F_VERIFY_CHECKSUM, 16, 1 << 14, 1 << 31):
            st, h = create_ex(L, FAKE_ARCHIVE, FAKE, 1, flags=flags, read_flags=rf)
            assert st == _lib.INVALID_ARG and not h.value, flags           # ZD_F_SKIPPABLE, unknown bits
        for n in (0, 1):                                                   # a NULL archive
            st, h = create_ex(L, None, FAKE, n, read_flags=rf)
            assert st == _lib.INVALID_ARG and not h.value, n
    for rf in (2, 1 << 31, 3, _lib.SEEK_VERIFY_TABLE | (1 << 31)):         # unknown read_flags bits
        for n in (0, 1):
            st, h = create_ex(L, FAKE_ARCHIVE, FAKE, n, read_flags=rf)
            assert st == _lib.INVALID_ARG and not h.value, rf


def test_new_calls_on_no_read():
    from zstd_decompressor import _lib
    L = _lib.lib()
    e, ok, h32 = C.c_void_p(), C.c_void_p(), C.c_void_p()
    n = C.c_uint64(7)
    assert L.zd_seek_read_device_verdicts(None, C.byref(e), C.byref(ok), C.byref(h32), C.byref(n)) == _lib.INVALID_ARG
    assert L.zd_seek_read_device_verdicts(None, None, None, None, None) == _lib.INVALID_ARG
    info = _lib.SeekReadInfo2()
    assert L.zd_seek_read_info_get_sized(None, C.cast(C.byref(info), C.POINTER(_lib.SeekReadInfo)),
                                         C.sizeof(info)) == _lib.INVALID_ARG
