"""CPU-side checks of ZD_F_CHAIN_BLOCK_PARALLEL (include/zd.h): the constant's
value, the header and the binding agree, the ABI version stays 8, every
zd_batch_create* argument check that runs before any HIP call accepts the flag,
and ZD_F_SKIPPABLE is still refused with it.  This file runs without a GPU: the
chunks have no bytes and no destination, so nothing is dereferenced where there
is one (without a GPU the first HIP call then fails, ZD_E_HIP, never
ZD_E_INVALID_ARG)."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zd.h")).read()


def _flag(name):
    return int(re.search(r"^#define\s+%s\s+(\d+)u\b" % name, HEADER, re.M).group(1))


def test_the_constant_is_bit_4096_in_the_header_and_the_binding():
    from zstd_decompressor import _lib
    assert _flag("ZD_F_CHAIN_BLOCK_PARALLEL") == 4096 == _lib.F_CHAIN_BLOCK_PARALLEL
    assert re.search(r"^#define\s+ZD_ABI_VERSION\s+8\b", HEADER, re.M)
    assert _lib.lib().zd_abi_version() == 8


def test_the_bit_was_free():
    mine = _flag("ZD_F_CHAIN_BLOCK_PARALLEL")
    others = {n: int(v) for n, v in re.findall(r"^#define\s+(ZD_F_\w+)\s+(\d+)u\b", HEADER, re.M)
              if n != "ZD_F_CHAIN_BLOCK_PARALLEL"}
    assert len(others) >= 11
    for n, v in others.items():
        assert v & mine == 0, n


def test_the_header_says_where_the_flag_means_something():
    text = re.sub(r"\s*\n \*\s*", " ", HEADER)
    assert "Everywhere else the flag is accepted and ignored" in text
    assert "keeps ignoring ZD_F_BLOCK_PARALLEL and ZD_F_FRAME_SERIAL" in text


def _empty(n):
    return ((C.c_void_p * n)(), (C.c_uint64 * n)(), (C.c_void_p * n)(), (C.c_uint64 * n)())


def _creators(L, n, flags):
    """Every host-array creation call over n chunks of no bytes and no destination, and every call with n == 0."""
    sp, ss, dp, dc = _empty(max(n, 1))
    pp, ps = (C.c_void_p * max(n, 1))(), (C.c_uint64 * max(n, 1))()
    par = (C.c_int64 * max(n, 1))(*([-1] + list(range(max(n, 1) - 1))))
    yield "create", lambda h: L.zd_batch_create(sp, ss, dp, dc, n, flags, None, None, C.byref(h))
    yield "prefix", lambda h: L.zd_batch_create_prefix(sp, ss, dp, dc, pp, ps, n, flags, None, C.byref(h))
    yield "chain", lambda h: L.zd_batch_create_chain(sp, ss, dp, dc, pp, ps, par, n, flags, None, C.byref(h))
    yield "chain_no_prefixes", lambda h: L.zd_batch_create_chain(sp, ss, dp, dc, None, None, par, n, flags, None,
                                                                 C.byref(h))
    if n == 0:      # (device arrays would be read on the device: only the call of no chunks runs here)
        yield "device", lambda h: L.zd_batch_create_device(None, None, None, None, 0, flags, None, None, C.byref(h))
        yield "device_prefix", lambda h: L.zd_batch_create_device_prefix(None, None, None, None, None, None, 0, flags,
                                                                         None, C.byref(h))
        yield "device_chain", lambda h: L.zd_batch_create_device_chain(None, None, None, None, None, None, None, 0,
                                                                       flags, None, C.byref(h))
        yield "device_packed", lambda h: L.zd_batch_create_device_packed(None, None, 0, 16, flags, None, None,
                                                                         C.byref(h))


def test_every_creation_call_accepts_the_flag():
    from zstd_decompressor import _lib
    L = _lib.lib()
    F = _lib.F_CHAIN_BLOCK_PARALLEL
    for flags in (F, F | _lib.F_BLOCK_PARALLEL, F | _lib.F_FRAME_SERIAL, F | _lib.F_VERIFY_CHECKSUM | _lib.F_LONG_WINDOW):
        for n in (0, 3):
            for name, make in _creators(L, n, flags):
                h = C.c_void_p()
                st = make(h)
                try:
                    assert st in ((0,) if n == 0 else (0, _lib.HIP)), (name, n, flags, st)
                finally:
                    if h.value:
                        L.zd_batch_destroy(h)


def test_an_empty_flagged_chain_batch_is_a_chain_batch():
    from zstd_decompressor import _lib
    L = _lib.lib()
    h = C.c_void_p()
    assert L.zd_batch_create_chain(None, None, None, None, None, None, None, 0, _lib.F_CHAIN_BLOCK_PARALLEL, None,
                                   C.byref(h)) == 0 and h.value
    try:
        levels, links = C.c_uint32(9), C.c_uint64(9)
        assert L.zd_batch_chain_info(h, C.byref(levels), C.byref(links)) == 0
        assert (levels.value, links.value) == (1, 0)
        ex = _lib.BatchInfoEx()
        assert L.zd_batch_info_get_sized(h, C.byref(ex), C.sizeof(ex)) == 0 and ex.executors == 0
        assert L.zd_batch_decode_async(h, None) == 0
    finally:
        L.zd_batch_destroy(h)


def test_skippable_is_still_refused_with_the_flag():
    from zstd_decompressor import _lib
    L = _lib.lib()
    flags = _lib.F_CHAIN_BLOCK_PARALLEL | _lib.F_SKIPPABLE
    for n in (0, 3):
        for name, make in _creators(L, n, flags):
            h = C.c_void_p()
            assert make(h) == _lib.INVALID_ARG and not h.value, (name, n)


def test_the_whole_call_checks_of_a_chain_are_what_they_were_with_the_flag():
    from zstd_decompressor import _lib
    L = _lib.lib()
    F = _lib.F_CHAIN_BLOCK_PARALLEL
    sp, ss, dp, dc = _empty(3)
    for parent in ([-1, 3, 1], [-1, 1, 0], [1, 0, -1], [2, 0, 1]):       # index n, itself, cycles
        h = C.c_void_p()
        st = L.zd_batch_create_chain(sp, ss, dp, dc, None, None, (C.c_int64 * 3)(*parent), 3, F, None, C.byref(h))
        assert st == _lib.INVALID_ARG and not h.value, parent
    h = C.c_void_p()
    assert L.zd_batch_create_chain(sp, ss, dp, dc, None, None, None, 3, F, None, C.byref(h)) == _lib.INVALID_ARG
