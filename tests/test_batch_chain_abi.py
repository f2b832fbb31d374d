"""CPU-side checks of the chain batches' additions to the C ABI (include/zd.h
zd_batch_create_chain, zd_batch_create_device_chain, zd_batch_chain_info): the
header declares them, the library exports them and the bindings match, the ABI
version stays 8, zd_batch_info is what it was, and every whole-call argument
error comes back before any HIP call -- this file runs without a GPU, on
made-up device addresses that nothing dereferences (a HIP call would fail with
ZD_E_HIP here, never with ZD_E_INVALID_ARG)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zd.h")).read()
NEW = ("zd_batch_create_chain", "zd_batch_create_device_chain", "zd_batch_chain_info")


def arrays(srcs, sizes, dsts, caps, pfx, psz, parent):
    n = len(srcs)
    return ((C.c_void_p * n)(*srcs), (C.c_uint64 * n)(*sizes), (C.c_void_p * n)(*dsts), (C.c_uint64 * n)(*caps),
            (C.c_void_p * n)(*pfx) if pfx is not None else None,
            (C.c_uint64 * n)(*psz) if psz is not None else None,
            (C.c_int64 * n)(*parent) if parent is not None else None, n)


def create(L, sp, ss, dp, dc, pp, ps, par, n, flags=0, out=True):
    h = C.c_void_p()
    st = L.zd_batch_create_chain(sp, ss, dp, dc, pp, ps, par, n, flags, None, C.byref(h) if out else None)
    return st, h


# three chunks: destinations [0x30000, +128), [0x40000, +128), [0x50000, +128); chunk 0 has an external prefix,
# chunk 1 decodes against chunk 0's output, chunk 2 against chunk 1's
GOOD = dict(srcs=[0x10000, 0x20000, 0x28000], sizes=[64, 64, 64], dsts=[0x30000, 0x40000, 0x50000],
            caps=[128, 128, 128], pfx=[0x60000, None, None], psz=[100, 0, 0], parent=[-1, 0, 1])


def with_(**kw):
    a = dict(GOOD)
    a.update(kw)
    return arrays(a["srcs"], a["sizes"], a["dsts"], a["caps"], a["pfx"], a["psz"], a["parent"])


def refused(L, **kw):
    st, h = create(L, *with_(**kw))
    return st == -93 and not h.value                       # ZD_E_INVALID_ARG, and no batch


def test_header_declares_and_library_exports_the_calls():
    from zstd_decompressor import _lib
    L = _lib.lib()
    assert re.search(r"^#define\s+ZD_ABI_VERSION\s+8\b", HEADER, re.M)
    assert L.zd_abi_version() == 8
    assert re.search(r"^#define\s+ZD_CHAIN_MAX_DEPTH\s+255\b", HEADER, re.M) and _lib.CHAIN_MAX_DEPTH == 255
    for name, arrays_ in (("zd_batch_create_chain",
                           r"const void\* const\* d_prefix, const uint64_t\* prefix_bytes,\s*const int64_t\* parent"),
                          ("zd_batch_create_device_chain",
                           r"const void\* const\* d_prefix_ptrs, const uint64_t\* d_prefix_bytes,\s*"
                           r"const int64_t\* d_parent")):
        decl = re.search(r"^int\s+%s\(([^;]*)\);" % name, HEADER, re.M | re.S).group(1)
        assert re.search(arrays_, decl), name
        assert re.search(r"size_t nchunks,\s*uint32_t flags,\s*void\* stream,\s*zd_batch\*\* out", decl), name
    decl = re.search(r"^int\s+zd_batch_chain_info\(([^;]*)\);", HEADER, re.M | re.S).group(1)
    assert re.sub(r"\s+", " ", decl) == "const zd_batch* batch, uint32_t* levels, uint64_t* links"
    for n in NEW:
        assert n in _lib.SIGNATURES, n
        fn = getattr(L, n)                     # (AttributeError: not exported)
        assert fn.argtypes == _lib.SIGNATURES[n][1] and fn.restype == _lib.SIGNATURES[n][0], n
    assert len(_lib.SIGNATURES["zd_batch_create_chain"][1]) == 11
    assert len(_lib.SIGNATURES["zd_batch_create_device_chain"][1]) == 11
    assert len(_lib.SIGNATURES["zd_batch_chain_info"][1]) == 3


def test_batch_info_is_unchanged():
    from zstd_decompressor import _lib
    body = re.search(r"typedef struct zd_batch_info \{(.*?)\} zd_batch_info;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint(?:32|64)_t)\s+(\w+);", body)
    assert fields == [("uint64_t", "nchunks"), ("uint64_t", "gathered_bytes"), ("uint64_t", "nblocks"),
                      ("uint64_t", "nsequences"), ("uint64_t", "workspace_bytes"), ("uint32_t", "executors"),
                      ("uint32_t", "device_built"), ("uint64_t", "gather_ns"), ("uint64_t", "walk_ns"),
                      ("uint64_t", "host_ns"), ("uint64_t", "upload_ns"), ("uint64_t", "prefix_bytes_total")]
    assert C.sizeof(_lib.BatchInfo) == 80 and C.sizeof(_lib.BatchInfoEx) == 88


def test_an_empty_chain_batch_is_ok_with_one_level_and_no_links():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for dev in (False, True):
        h = C.c_void_p()
        fn = L.zd_batch_create_device_chain if dev else L.zd_batch_create_chain
        st = fn(None, None, None, None, None, None, None, 0, 0, None, C.byref(h))
        assert st == 0 and h.value, dev                        # nchunks == 0: ZD_OK, no HIP call
        try:
            levels, links = C.c_uint32(9), C.c_uint64(9)
            assert L.zd_batch_chain_info(h, C.byref(levels), C.byref(links)) == 0
            assert (levels.value, links.value) == (1, 0)
            assert L.zd_batch_chain_info(h, None, None) == 0
            # the 80-byte getter writes 80 bytes and no more, the sized one the whole struct
            class Guarded(C.Structure):
                _fields_ = [("info", _lib.BatchInfo), ("guard", C.c_uint64)]
            g = Guarded()
            g.guard = 0x5A5A5A5A5A5A5A5A
            assert L.zd_batch_info_get(h, C.byref(g.info)) == 0
            assert g.guard == 0x5A5A5A5A5A5A5A5A and g.info.nchunks == 0 and g.info.device_built == int(dev)
            ex = _lib.BatchInfoEx()
            ex.prefix_bytes_total = 77
            assert L.zd_batch_info_get_sized(h, C.byref(ex), C.sizeof(ex)) == 0 and ex.prefix_bytes_total == 0
            assert L.zd_batch_info_get_sized(h, C.byref(ex), 79) == _lib.INVALID_ARG
            assert L.zd_batch_decode_async(h, None) == 0
            bad = C.c_uint64(7)
            assert L.zd_batch_results(h, None, None, None, 0, C.byref(bad)) == 0 and bad.value == 0
        finally:
            L.zd_batch_destroy(h)


def test_chain_info_refuses_a_batch_that_is_no_chain():
    from zstd_decompressor import _lib
    L = _lib.lib()
    assert L.zd_batch_chain_info(None, None, None) == _lib.INVALID_ARG
    for make in (lambda h: L.zd_batch_create(None, None, None, None, 0, 0, None, None, C.byref(h)),
                 lambda h: L.zd_batch_create_prefix(None, None, None, None, None, None, 0, 0, None, C.byref(h))):
        h = C.c_void_p()
        assert make(h) == 0 and h.value
        try:
            levels = C.c_uint32(9)
            assert L.zd_batch_chain_info(h, C.byref(levels), None) == _lib.INVALID_ARG and levels.value == 9
        finally:
            L.zd_batch_destroy(h)


def test_what_batch_create_prefix_refuses_is_refused():
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
    assert refused(L, srcs=[0x10000, None, 0x28000])                              # NULL source with bytes
    assert refused(L, dsts=[0x30000, None, 0x50000])                              # NULL destination with capacity
    assert refused(L, dsts=[0x30000, 0x30040, 0x50000])                           # destinations overlap
    args = list(a)
    args[7] = 1 << 31
    st, h = create(L, *args)
    assert st == _lib.INVALID_ARG and not h.value                                 # nchunks = 2^31
    assert refused(L, pfx=[None, None, None])                                     # NULL prefix entry with a size
    assert refused(L, pfx=[(1 << 64) - 8, None, None], psz=[16, 0, 0])            # a prefix range that wraps
    # an EXTERNAL prefix that overlaps a destination (any chunk's)
    for p, z in ((0x30000, 1), (0x4007F, 1), (0x2FFF0, 17), (0x20000, 0x40000), (0x50010, 8)):
        assert refused(L, pfx=[p, None, None], psz=[z, 0, 0]), (p, z)


def test_exactly_one_null_prefix_array_and_a_null_parent_array_are_invalid():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for k in (4, 5, 6):
        args = list(with_())
        args[k] = None
        st, h = create(L, *args)
        assert st == _lib.INVALID_ARG and not h.value, k
    # the device call's whole-call checks (the entries are a per-chunk matter there)
    fake = [C.c_void_p(0x1000 * (k + 1)) for k in range(7)]
    for k in range(7):
        args = list(fake)
        args[k] = None
        h = C.c_void_p()
        st = L.zd_batch_create_device_chain(*args, 1, 0, None, C.byref(h))
        assert st == _lib.INVALID_ARG and not h.value, k
    h = C.c_void_p()
    assert L.zd_batch_create_device_chain(*fake, 1, _lib.F_SKIPPABLE, None, C.byref(h)) == _lib.INVALID_ARG
    assert L.zd_batch_create_device_chain(*fake, 1 << 31, 0, None, C.byref(h)) == _lib.INVALID_ARG
    assert L.zd_batch_create_device_chain(*fake, 1, 0, None, None) == _lib.INVALID_ARG
    args = list(fake)
    args[4] = args[5] = None                                    # both prefix arrays NULL, the parent array too
    args[6] = None
    assert L.zd_batch_create_device_chain(*args, 1, 0, None, C.byref(h)) == _lib.INVALID_ARG and not h.value


def test_parent_entries_are_checked_before_any_hip_call():
    from zstd_decompressor import _lib
    L = _lib.lib()
    assert refused(L, parent=[-1, 3, 1])                        # index n
    assert refused(L, parent=[-1, -2, 1])                       # below -1
    assert refused(L, parent=[-1, 1 << 40, 1])                  # far outside
    assert refused(L, parent=[-1, 1, 0])                        # parent[i] == i
    assert refused(L, pfx=[None, None, None], psz=[0, 0, 0], parent=[1, 0, -1])       # a 2-cycle
    assert refused(L, pfx=[None, None, None], psz=[0, 0, 0], parent=[2, 0, 1])        # a 3-cycle
    assert refused(L, psz=[100, 0, 8], pfx=[0x60000, None, 0x70000])                  # a prefix size on a chained chunk
    assert refused(L, psz=[100, 1, 0], pfx=[0x60000, 0x70000, None])
    # NULL prefix arrays, but the cycle is still found
    assert refused(L, pfx=None, psz=None, parent=[1, 0, -1])


def test_null_prefix_arrays_pass_the_checks_when_no_root_has_a_prefix():
    # chunks of no bytes and no destination, so that nothing is dereferenced where there is a GPU: the call passes
    # every argument check (without a GPU its first HIP call then fails, ZD_E_HIP)
    from zstd_decompressor import _lib
    L = _lib.lib()
    a = arrays([None, None, None], [0, 0, 0], [None, None, None], [0, 0, 0], None, None, [-1, 0, 1])
    st, h = create(L, *a)
    try:
        assert st in (0, _lib.HIP), st
        if st == 0:
            levels, links = C.c_uint32(), C.c_uint64()
            assert L.zd_batch_chain_info(h, C.byref(levels), C.byref(links)) == 0
            assert (levels.value, links.value) == (3, 2)
    finally:
        if h.value:
            L.zd_batch_destroy(h)
    # the same with the prefix arrays given and every size 0
    a = arrays([None, None, None], [0, 0, 0], [None, None, None], [0, 0, 0], [None] * 3, [0] * 3, [-1, 0, 1])
    st, h = create(L, *a)
    if h.value:
        L.zd_batch_destroy(h)
    assert st in (0, _lib.HIP), st


def test_a_chunk_with_more_than_255_ancestors_is_refused():
    from zstd_decompressor import _lib
    L = _lib.lib()
    n = 257
    a = arrays([0x100000 + 64 * i for i in range(n)], [16] * n, [0x900000 + 64 * i for i in range(n)], [64] * n,
               None, None, [i - 1 for i in range(n)])
    st, h = create(L, *a)
    assert st == _lib.INVALID_ARG and not h.value


def test_python_refuses_parents_with_a_dictionary_and_checks_lengths():
    from zstd_decompressor import Batch

    class Open:            # stands for an open Dictionary: the check comes before anything reads it
        _h = 1
    with pytest.raises(ValueError):
        Batch([0x10000], [64], [0x30000], [128], dictionary=Open(), parents=[-1])
    with pytest.raises(ValueError):
        Batch.from_device(0x1000, 0x2000, 0x3000, 0x4000, nchunks=1, dictionary=Open(), parents=0x5000)
    with pytest.raises(ValueError):
        Batch([0x10000], [64], [0x30000], [128], parents=[-1, 0])
    # the whole-call refusal reaches Python as a ZdError(INVALID_ARG), with and without prefixes
    from zstd_decompressor import _lib
    for pfx in (None, ([0, 0], [0, 0])):
        with pytest.raises(_lib.ZdError) as e:
            Batch([0x10000, 0x20000], [64, 64], [0x30000, 0x40000], [128, 128], prefixes=pfx, parents=[1, 0])
        assert e.value.code == _lib.INVALID_ARG
