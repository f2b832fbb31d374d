"""CPU-side checks of ZD_F_AUTO_EXECUTOR (include/zd.h): the flag's and the four
constants' values and their presence in the header, the binding, the ABI version
(still 8), that every zd_batch_create* argument check accepts the flag, and
zd_batch_info2.k4j_chunks behind zd_batch_info through the sized info call.  This
file runs without a GPU: batches of no chunks make no HIP call."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zd.h")).read()


def _define(name):
    return int(re.search(r"^#define\s+%s\s+(\d+)u?\b" % name, HEADER, re.M).group(1))


def test_the_flag_is_bit_8192_in_the_header_and_the_binding():
    from zstd_decompressor import _lib
    assert _define("ZD_F_AUTO_EXECUTOR") == 8192 == _lib.F_AUTO_EXECUTOR
    assert re.search(r"^#define\s+ZD_ABI_VERSION\s+8\b", HEADER, re.M)
    assert _lib.lib().zd_abi_version() == 8
    others = {n: int(v) for n, v in re.findall(r"^#define\s+(ZD_F_\w+)\s+(\d+)u\b", HEADER, re.M)
              if n != "ZD_F_AUTO_EXECUTOR"}
    assert len(others) >= 12
    for n, v in others.items():
        assert v & 8192 == 0, n


def test_the_four_constants_are_public_macros():
    v = {n: _define(n) for n in ("ZD_AUTO_MIN_BLOCKS", "ZD_AUTO_MIN_BLOCKS_FEW", "ZD_AUTO_FEW_CHUNKS",
                                 "ZD_AUTO_MAX_CANDIDATES")}
    assert 1 <= v["ZD_AUTO_MIN_BLOCKS_FEW"] <= v["ZD_AUTO_MIN_BLOCKS"]
    assert v["ZD_AUTO_FEW_CHUNKS"] >= 1 and v["ZD_AUTO_MAX_CANDIDATES"] >= 1


def test_the_header_says_what_the_flag_does_and_no_longer_that_no_rule_exists():
    text = re.sub(r"\s*\n \*\s*", " ", HEADER)
    assert "Everywhere else the flag is accepted and ignored: plain, dictionary and dictionary-set batches" in text
    assert "The forcing flags win" in text
    assert "no automatic rule" not in text and "no rule sets this flag" not in text


def _creators(L, flags):
    yield "create", lambda h: L.zd_batch_create(None, None, None, None, 0, flags, None, None, C.byref(h))
    yield "prefix", lambda h: L.zd_batch_create_prefix(None, None, None, None, None, None, 0, flags, None, C.byref(h))
    yield "chain", lambda h: L.zd_batch_create_chain(None, None, None, None, None, None, None, 0, flags, None,
                                                     C.byref(h))
    yield "device", lambda h: L.zd_batch_create_device(None, None, None, None, 0, flags, None, None, C.byref(h))
    yield "device_prefix", lambda h: L.zd_batch_create_device_prefix(None, None, None, None, None, None, 0, flags,
                                                                     None, C.byref(h))
    yield "device_chain", lambda h: L.zd_batch_create_device_chain(None, None, None, None, None, None, None, 0,
                                                                   flags, None, C.byref(h))
    yield "device_packed", lambda h: L.zd_batch_create_device_packed(None, None, 0, 16, flags, None, None, C.byref(h))


def test_every_creation_call_accepts_the_flag_and_still_refuses_skippable():
    from zstd_decompressor import _lib
    L = _lib.lib()
    F = _lib.F_AUTO_EXECUTOR
    for flags in (F, F | _lib.F_BLOCK_PARALLEL, F | _lib.F_FRAME_SERIAL, F | _lib.F_CHAIN_BLOCK_PARALLEL,
                  F | _lib.F_VERIFY_CHECKSUM | _lib.F_LONG_WINDOW | _lib.F_J_ONE_ROUND):
        for name, make in _creators(L, flags):
            h = C.c_void_p()
            try:
                assert make(h) == 0 and h.value, (name, flags)
            finally:
                if h.value:
                    L.zd_batch_destroy(h)
    for name, make in _creators(L, F | _lib.F_SKIPPABLE):
        h = C.c_void_p()
        assert make(h) == _lib.INVALID_ARG and not h.value, name


def test_k4j_chunks_follows_the_struct_and_old_callers_keep_their_bytes():
    from zstd_decompressor import _lib
    assert C.sizeof(_lib.BatchInfo) == 80 and C.sizeof(_lib.BatchInfoEx) == 88
    assert _lib.BatchInfo2.k4j_chunks.offset == 88 and C.sizeof(_lib.BatchInfo2) == 96
    assert _lib.BatchInfo2.prefix_bytes_total.offset == 80
    # the header: zd_batch_info2 is zd_batch_info and then the new field
    body = re.search(r"typedef struct zd_batch_info2 \{(.*?)\} zd_batch_info2;", HEADER, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    assert re.findall(r"(\w+)\s+(\w+);", body) == [("zd_batch_info", "info"), ("uint64_t", "k4j_chunks")]
    L = _lib.lib()
    for dev in (False, True):
        h = C.c_void_p()
        if dev:
            st = L.zd_batch_create_device_prefix(None, None, None, None, None, None, 0, _lib.F_AUTO_EXECUTOR, None,
                                                 C.byref(h))
        else:
            st = L.zd_batch_create_prefix(None, None, None, None, None, None, 0, _lib.F_AUTO_EXECUTOR, None, C.byref(h))
        assert st == 0 and h.value
        try:
            x = _lib.BatchInfo2()
            x.k4j_chunks = x.prefix_bytes_total = 77
            assert L.zd_batch_info_get_sized(h, C.byref(x), C.sizeof(x)) == 0
            assert x.k4j_chunks == 0 and x.prefix_bytes_total == 0 and x.executors == 0 and x.device_built == int(dev)
            # a caller of the 88-byte struct, and one of the 80-byte struct: nothing behind their sizes is written
            for size in (88, 80):
                x.k4j_chunks = x.prefix_bytes_total = 77
                assert L.zd_batch_info_get_sized(h, C.byref(x), size) == 0
                assert x.k4j_chunks == 77 and x.prefix_bytes_total == (0 if size == 88 else 77)

            class Guarded(C.Structure):
                _fields_ = [("info", _lib.BatchInfo), ("guard", C.c_uint64 * 2)]
            g = Guarded()
            g.guard[0] = g.guard[1] = 0x5A5A5A5A5A5A5A5A
            assert L.zd_batch_info_get(h, C.byref(g.info)) == 0          # the exported old call: 80 bytes
            assert list(g.guard) == [0x5A5A5A5A5A5A5A5A] * 2
            # a size past the struct writes the struct and no more
            class Wide(C.Structure):
                _fields_ = [("info", _lib.BatchInfo2), ("guard", C.c_uint64)]
            w = Wide()
            w.guard = 0x5A5A5A5A5A5A5A5A
            assert L.zd_batch_info_get_sized(h, C.cast(C.byref(w), C.POINTER(_lib.BatchInfoEx)), C.sizeof(w)) == 0
            assert w.guard == 0x5A5A5A5A5A5A5A5A
        finally:
            L.zd_batch_destroy(h)
