"""CPU-side checks of the seekable-archive calls (include/zd.h zd_seekable_*,
zd_seek_read_*): the symbols are exported and bound, the ABI version stays 8
and zd_batch_info keeps its 80 bytes, the new status has its name, and every
whole-call argument error comes back before any HIP call -- this file runs
without a GPU, on made-up addresses that nothing reads."""
import ctypes as C

NEW = ("zd_seekable_open_device", "zd_seekable_info_get", "zd_seekable_table", "zd_seekable_close",
       "zd_seekable_read_create", "zd_seek_read_decode_async", "zd_seek_read_finish_async",
       "zd_seek_read_device_results",
       "zd_seek_read_results", "zd_seek_read_info_get", "zd_seek_read_destroy")
FAKE = [0x10000, 0x20000, 0x30000]        # "device arrays": never dereferenced by these calls
FAKE_ARCHIVE = 0x50000                    # an "open archive": never dereferenced before the arguments are checked


def read_create(L, z, arrs, n, flags=0, out=True):
    h = C.c_void_p()
    st = L.zd_seekable_read_create(C.c_void_p(z) if z else None, *[C.c_void_p(a) if a else None for a in arrs], n,
                                   flags, None, C.byref(h) if out else None)
    return st, h


def test_new_symbols_exported_and_bound():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for n in NEW:
        assert n in _lib.SIGNATURES, n
        fn = getattr(L, n)
        assert fn.argtypes == _lib.SIGNATURES[n][1] and fn.restype == _lib.SIGNATURES[n][0], n
    assert len(_lib.SIGNATURES["zd_seekable_open_device"][1]) == 4
    assert len(_lib.SIGNATURES["zd_seekable_read_create"][1]) == 8
    import zstd_decompressor
    assert callable(zstd_decompressor.SeekableArchive) and callable(zstd_decompressor.SeekableArchive.reader)


def test_abi_version_and_struct_sizes():
    from zstd_decompressor import _lib
    L = _lib.lib()
    assert L.zd_abi_version() == 8
    assert C.sizeof(_lib.BatchInfo) == 80
    assert C.sizeof(_lib.SeekableInfo) == 40
    assert _lib.SeekReadInfo.batch.offset == 40 and C.sizeof(_lib.SeekReadInfo) == 40 + C.sizeof(_lib.BatchInfo2)
    assert _lib.SEEK_TABLE == -101 and _lib.status_name(-101) == "SeekTableWrong"
    assert _lib.status_name(-102) == "Unknown"


def test_open_argument_errors_need_no_gpu():
    from zstd_decompressor import _lib
    L = _lib.lib()
    h = C.c_void_p()
    for n in (0, 1, 16):                                                   # n < 17: before any HIP call
        assert L.zd_seekable_open_device(C.c_void_p(FAKE_ARCHIVE), n, None, C.byref(h)) == _lib.NOT_ENOUGH_BYTES
        assert not h.value
    assert L.zd_seekable_open_device(C.c_void_p(FAKE_ARCHIVE), 100, None, None) == _lib.INVALID_ARG   # NULL out
    assert L.zd_seekable_open_device(None, 100, None, C.byref(h)) == _lib.INVALID_ARG and not h.value  # NULL archive
    info = _lib.SeekableInfo()
    assert L.zd_seekable_info_get(None, C.byref(info)) == _lib.INVALID_ARG
    assert L.zd_seekable_table(None, None, None, None) == _lib.INVALID_ARG
    L.zd_seekable_close(None)


def test_read_whole_call_argument_errors_need_no_gpu():
    from zstd_decompressor import _lib
    L = _lib.lib()
    st, h = read_create(L, FAKE_ARCHIVE, FAKE, 1, out=False)
    assert st == _lib.INVALID_ARG                                          # NULL out
    for k in range(3):                                                     # a NULL array with nranges = 1
        arrs = list(FAKE)
        arrs[k] = None
        st, h = read_create(L, FAKE_ARCHIVE, arrs, 1)
        assert st == _lib.INVALID_ARG and not h.value, k
    st, h = read_create(L, FAKE_ARCHIVE, FAKE, 1 << 31)
    assert st == _lib.INVALID_ARG and not h.value                          # nranges = 2^31
    for flags in (_lib.F_SKIPPABLE, _lib.F_SKIPPABLE | _lib.F_VERIFY_CHECKSUM, 16, 1 << 14, 1 << 31):
        st, h = read_create(L, FAKE_ARCHIVE, FAKE, 1, flags=flags)
        assert st == _lib.INVALID_ARG and not h.value, flags               # ZD_F_SKIPPABLE, unknown bits
    for n in (0, 1):                                                       # a closed archive
        st, h = read_create(L, None, FAKE, n)
        assert st == _lib.INVALID_ARG and not h.value, n


def test_calls_on_no_read():
    from zstd_decompressor import _lib
    L = _lib.lib()
    assert L.zd_seek_read_decode_async(None, None) == _lib.INVALID_ARG
    assert L.zd_seek_read_finish_async(None, None) == _lib.INVALID_ARG
    assert L.zd_seek_read_results(None, None, None, None, 0, None) == _lib.INVALID_ARG
    assert L.zd_seek_read_device_results(None, None, None) == _lib.INVALID_ARG
    info = _lib.SeekReadInfo()
    assert L.zd_seek_read_info_get(None, C.byref(info)) == _lib.INVALID_ARG
    L.zd_seek_read_destroy(None)


def test_closed_python_archive_raises():
    import pytest
    from zstd_decompressor import SeekableArchive
    a = SeekableArchive.__new__(SeekableArchive)
    a._h = None
    with pytest.raises(ValueError):
        a.reader([0], [1])
    with pytest.raises(ValueError):
        a.table()
    a.close()


def test_written_archive_is_a_zst_with_a_table():
    """corpus/seekable.py: the archive decodes front to back to the data on the
    CPU oracle (the table is a skippable frame), and the table's fields are the
    entries' sizes."""
    import struct
    from corpus import gen, seekable
    from oracle import oracle
    data = gen.text(10000, seed=7)[:9001]
    for sizes, n in ((1000, 10), ([1, 4000, 0, 5000], 4)):
        for sums in (False, True):
            blob = seekable.write_seekable(data, sizes, checksums=sums, frame_checksums={1})
            assert oracle.decompress(blob) == data
            e = 12 if sums else 8
            assert struct.unpack("<IBI", blob[-9:]) == (n, 0x80 if sums else 0, 0x8F92EAB1)
            table = blob[-(17 + n * e):]
            assert struct.unpack("<II", table[:8]) == (0x184D2A5E, n * e + 9)
            rows = [struct.unpack("<III" if sums else "<II", table[8 + i * e:8 + (i + 1) * e]) for i in range(n)]
            assert sum(r[0] for r in rows) == len(blob) - len(table) and sum(r[1] for r in rows) == len(data)
            assert [r[1] for r in rows] == (sizes if isinstance(sizes, list) else [1000] * 9 + [1])
