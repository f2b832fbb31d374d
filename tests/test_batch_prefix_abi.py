"""CPU-side checks of the prefix batches' additions to the C ABI (include/zd.h
zd_batch_create_prefix, zd_batch_create_device_prefix): the header declares
them, the library exports them and the bindings match, the ABI version stays 8,
zd_batch_info keeps its field offsets with prefix_bytes_total at its end, and
every whole-call argument error comes back before any HIP call -- this file
runs without a GPU, on made-up device addresses that nothing dereferences."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zd.h")).read()
NEW = ("zd_batch_create_prefix", "zd_batch_create_device_prefix", "zd_batch_info_get_sized")


def arrays(srcs, sizes, dsts, caps, pfx, psz):
    n = len(srcs)
    return ((C.c_void_p * n)(*srcs), (C.c_uint64 * n)(*sizes), (C.c_void_p * n)(*dsts), (C.c_uint64 * n)(*caps),
            (C.c_void_p * n)(*pfx), (C.c_uint64 * n)(*psz), n)


def create(L, sp, ss, dp, dc, pp, ps, n, flags=0, out=True):
    h = C.c_void_p()
    st = L.zd_batch_create_prefix(sp, ss, dp, dc, pp, ps, n, flags, None, C.byref(h) if out else None)
    return st, h


# two chunks: sources, destinations [0x30000, +128) and [0x40000, +128), prefixes well away from them
GOOD = dict(srcs=[0x10000, 0x20000], sizes=[64, 64], dsts=[0x30000, 0x40000], caps=[128, 128],
            pfx=[0x60000, 0x70000], psz=[100, 4096])


def with_(**kw):
    a = dict(GOOD)
    a.update(kw)
    return arrays(a["srcs"], a["sizes"], a["dsts"], a["caps"], a["pfx"], a["psz"])


def test_header_declares_and_library_exports_the_calls():
    from zstd_decompressor import _lib
    L = _lib.lib()
    assert re.search(r"^#define\s+ZD_ABI_VERSION\s+8\b", HEADER, re.M)
    assert L.zd_abi_version() == 8
    for name, arrays_ in (("zd_batch_create_prefix", r"const void\* const\* d_prefix, const uint64_t\* prefix_bytes"),
                          ("zd_batch_create_device_prefix",
                           r"const void\* const\* d_prefix_ptrs, const uint64_t\* d_prefix_bytes")):
        assert re.search(r"^int\s+%s\(" % name, HEADER, re.M), name
        decl = re.search(r"^int\s+%s\(([^;]*)\);" % name, HEADER, re.M | re.S).group(1)
        assert re.search(arrays_, decl), name
        assert re.search(r"size_t nchunks,\s*uint32_t flags,\s*void\* stream,\s*zd_batch\*\* out", decl), name
    for n in NEW:
        assert n in _lib.SIGNATURES, n
        fn = getattr(L, n)                     # (AttributeError: not exported)
        assert fn.argtypes == _lib.SIGNATURES[n][1] and fn.restype == _lib.SIGNATURES[n][0], n
    assert len(_lib.SIGNATURES["zd_batch_create_prefix"][1]) == 10
    assert len(_lib.SIGNATURES["zd_batch_create_device_prefix"][1]) == 10


def test_batch_info_keeps_its_offsets_and_ends_with_the_new_field():
    from zstd_decompressor import _lib
    old = [("nchunks", 0), ("gathered_bytes", 8), ("nblocks", 16), ("nsequences", 24), ("workspace_bytes", 32),
           ("executors", 40), ("device_built", 44), ("gather_ns", 48), ("walk_ns", 56), ("host_ns", 64),
           ("upload_ns", 72)]
    for cls in (_lib.BatchInfo, _lib.BatchInfoEx):
        for name, off in old:
            assert getattr(cls, name).offset == off, (cls.__name__, name)
    assert C.sizeof(_lib.BatchInfo) == 80
    assert _lib.BatchInfoEx.prefix_bytes_total.offset == 80 and C.sizeof(_lib.BatchInfoEx) == 88
    # the header's struct: the new field last
    body = re.search(r"typedef struct zd_batch_info \{(.*?)\} zd_batch_info;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"uint(?:32|64)_t\s+(\w+);", body)
    assert fields == [n for n, _ in old] + ["prefix_bytes_total"]


def test_info_of_an_empty_prefix_batch_through_both_getters():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for dev in (False, True):
        h = C.c_void_p()
        if dev:
            st = L.zd_batch_create_device_prefix(None, None, None, None, None, None, 0, 0, None, C.byref(h))
        else:
            st = L.zd_batch_create_prefix(None, None, None, None, None, None, 0, 0, None, C.byref(h))
        assert st == 0 and h.value, dev                        # nchunks == 0: ZD_OK, no HIP call
        try:
            # the old call writes 80 bytes and no more: a guard word behind the struct survives
            class Guarded(C.Structure):
                _fields_ = [("info", _lib.BatchInfo), ("guard", C.c_uint64)]
            g = Guarded()
            g.guard = 0x5A5A5A5A5A5A5A5A
            assert L.zd_batch_info_get(h, C.byref(g.info)) == 0
            assert g.guard == 0x5A5A5A5A5A5A5A5A and g.info.nchunks == 0 and g.info.device_built == int(dev)
            ex = _lib.BatchInfoEx()
            ex.prefix_bytes_total = 77
            assert L.zd_batch_info_get_sized(h, C.byref(ex), C.sizeof(ex)) == 0
            assert ex.prefix_bytes_total == 0 and ex.nchunks == 0 and ex.executors == 0
            ex.prefix_bytes_total = 77
            assert L.zd_batch_info_get_sized(h, C.byref(ex), 80) == 0 and ex.prefix_bytes_total == 77
            assert L.zd_batch_info_get_sized(h, C.byref(ex), 79) == _lib.INVALID_ARG
            assert L.zd_batch_info_get_sized(h, None, 88) == _lib.INVALID_ARG
            assert L.zd_batch_decode_async(h, None) == 0
            bad = C.c_uint64(7)
            assert L.zd_batch_results(h, None, None, None, 0, C.byref(bad)) == 0 and bad.value == 0
        finally:
            L.zd_batch_destroy(h)


def test_what_batch_create_refuses_is_refused():
    from zstd_decompressor import _lib
    L = _lib.lib()
    a = with_()
    assert create(L, *a, out=False)[0] == _lib.INVALID_ARG                       # NULL out
    for flags in (_lib.F_SKIPPABLE, _lib.F_SKIPPABLE | _lib.F_VERIFY_CHECKSUM):
        st, h = create(L, *a, flags=flags)
        assert st == _lib.INVALID_ARG and not h.value, flags
    for k in range(4):                                                            # a NULL array of the old four
        args = list(a)
        args[k] = None
        st, h = create(L, *args)
        assert st == _lib.INVALID_ARG and not h.value, k
    st, h = create(L, *with_(srcs=[0x10000, None]))
    assert st == _lib.INVALID_ARG and not h.value                                 # NULL source with bytes
    st, h = create(L, *with_(dsts=[0x30000, None]))
    assert st == _lib.INVALID_ARG and not h.value                                 # NULL destination with capacity
    st, h = create(L, *with_(dsts=[0x30000, 0x30040]))
    assert st == _lib.INVALID_ARG and not h.value                                 # destinations overlap
    args = list(a)
    args[6] = 1 << 31
    st, h = create(L, *args)
    assert st == _lib.INVALID_ARG and not h.value                                 # nchunks = 2^31


def test_null_prefix_arrays_are_invalid():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for k in (4, 5):
        args = list(with_())
        args[k] = None
        st, h = create(L, *args)
        assert st == _lib.INVALID_ARG and not h.value, k
    # the device call: its whole-call checks (the entries are a per-chunk matter there)
    fake = [C.c_void_p(0x1000 * (k + 1)) for k in range(6)]
    for k in range(6):
        args = list(fake)
        args[k] = None
        h = C.c_void_p()
        st = L.zd_batch_create_device_prefix(*args, 1, 0, None, C.byref(h))
        assert st == _lib.INVALID_ARG and not h.value, k
    h = C.c_void_p()
    assert L.zd_batch_create_device_prefix(*fake, 1, _lib.F_SKIPPABLE, None, C.byref(h)) == _lib.INVALID_ARG
    assert L.zd_batch_create_device_prefix(*fake, 1 << 31, 0, None, C.byref(h)) == _lib.INVALID_ARG
    assert L.zd_batch_create_device_prefix(*fake, 1, 0, None, None) == _lib.INVALID_ARG


def test_null_prefix_entry_with_a_size_is_invalid():
    from zstd_decompressor import _lib
    L = _lib.lib()
    st, h = create(L, *with_(pfx=[0x60000, None], psz=[100, 1]))
    assert st == _lib.INVALID_ARG and not h.value


def test_prefix_range_that_wraps_is_invalid():
    from zstd_decompressor import _lib
    L = _lib.lib()
    st, h = create(L, *with_(pfx=[0x60000, (1 << 64) - 8], psz=[100, 16]))
    assert st == _lib.INVALID_ARG and not h.value


def test_prefix_that_overlaps_a_destination_is_invalid():
    from zstd_decompressor import _lib
    L = _lib.lib()
    # destinations [0x30000, 0x30080) and [0x40000, 0x40080)
    for pfx, psz in (([0x30000, 0x70000], [1, 4096]),          # a destination's first byte (its own chunk's)
                     ([0x60000, 0x3007F], [100, 1]),            # the other chunk's last byte
                     ([0x2FFF0, 0x70000], [17, 4096]),          # ends one byte inside
                     ([0x60000, 0x20000], [100, 0x30000]),      # covers both destinations whole
                     ([0x4007F, 0x60000], [0x1000, 0]),         # starts at a destination's last byte
                     ([0x30010, 0x30020], [8, 8])):             # inside a destination
        st, h = create(L, *with_(pfx=pfx, psz=psz))
        assert st == _lib.INVALID_ARG and not h.value, (pfx, psz)


def test_python_refuses_prefixes_with_a_dictionary():
    import pytest
    from zstd_decompressor import Batch

    class Open:            # stands for an open Dictionary: the check comes before anything reads it
        _h = 1
    with pytest.raises(ValueError):
        Batch([0x10000], [64], [0x30000], [128], dictionary=Open(), prefixes=([0x60000], [100]))
    with pytest.raises(ValueError):
        Batch.from_device(0x1000, 0x2000, 0x3000, 0x4000, nchunks=1, dictionary=Open(),
                          prefixes=(0x5000, 0x6000))


def test_cli_takes_patch_from():
    from zstd_decompressor.__main__ import _parser
    a = _parser().parse_args(["new.zst", "--patch-from", "old.bin", "-o", "out"])
    assert a.patch_from == "old.bin" and a.output == "out" and a.dictionary is None
    assert _parser().parse_args(["new.zst"]).patch_from is None
