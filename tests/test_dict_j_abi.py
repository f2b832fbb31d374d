"""CPU-side checks of ZD_F_DICT_BLOCK_PARALLEL (include/zd.h): the flag's value in
the header and the binding, distinct from every other ZD_F_*; every
zd_batch_create* argument check that needs no dictionary handle accepts it
(batches of no chunks make no HIP call); a seekable read's plan flags refuse it.
This file runs without a GPU."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zd.h")).read()


def test_the_flag_is_bit_32768_distinct_from_every_other_flag():
    from zstd_decompressor import _lib
    flags = {n: int(v) for n, v in re.findall(r"^#define\s+(ZD_F_\w+)\s+(\d+)u\b", HEADER, re.M)}
    assert flags["ZD_F_DICT_BLOCK_PARALLEL"] == 32768 == _lib.F_DICT_BLOCK_PARALLEL
    assert len(flags) >= 14
    for n, v in flags.items():
        assert n == "ZD_F_DICT_BLOCK_PARALLEL" or v & 32768 == 0, n
    # the first free bit: every bit below it but 16 (never a plan flag) is taken
    assert sum(v for n, v in flags.items() if n != "ZD_F_DICT_BLOCK_PARALLEL") == 32767 - 16


def test_the_header_states_the_rule_and_the_limits():
    text = re.sub(r"\s*\n \*\s*", " ", HEADER)
    for words in ("with ZD_F_FRAME_SERIAL no frame goes to K4J", "with ZD_F_BLOCK_PARALLEL every such frame does",
                  "a capacity within K4J's 32 GiB and dictionary content of at most 0x7FFF0000 bytes",
                  "against ZD_AUTO_DICT_MAX_CANDIDATES in ZD_AUTO_MAX_CANDIDATES' place",
                  "Without the flag nothing changes"):
        assert words in text, words


def test_the_dictionary_plans_cap_is_a_public_macro_within_the_prefix_batches():
    cap = int(re.search(r"^#define\s+ZD_AUTO_DICT_MAX_CANDIDATES\s+(\d+)\b", HEADER, re.M).group(1))
    assert 1 <= cap <= int(re.search(r"^#define\s+ZD_AUTO_MAX_CANDIDATES\s+(\d+)\b", HEADER, re.M).group(1))


def _creators(L, flags):
    # (the *_dicts calls need a dictionary set, which is made on a GPU: tests/test_dict_j_gpu.py creates them)
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
    F = _lib.F_DICT_BLOCK_PARALLEL
    for flags in (F, F | _lib.F_BLOCK_PARALLEL, F | _lib.F_FRAME_SERIAL, F | _lib.F_AUTO_EXECUTOR,
                  F | _lib.F_CHAIN_BLOCK_PARALLEL, F | _lib.F_VERIFY_CHECKSUM | _lib.F_LONG_WINDOW | _lib.F_RFC |
                  _lib.F_J_ONE_ROUND):
        for name, make in _creators(L, flags):
            h = C.c_void_p()
            try:
                assert make(h) == 0 and h.value, (name, flags)
                x = _lib.BatchInfo2()
                assert L.zd_batch_info_get_sized(h, C.byref(x), C.sizeof(x)) == 0
                assert x.k4j_chunks == 0 and x.executors == 0, name
            finally:
                if h.value:
                    L.zd_batch_destroy(h)
    for name, make in _creators(L, F | _lib.F_SKIPPABLE):
        h = C.c_void_p()
        assert make(h) == _lib.INVALID_ARG and not h.value, name


def test_a_seekable_read_refuses_the_bit_in_its_plan_flags():
    from zstd_decompressor import _lib
    L = _lib.lib()
    fake = C.c_void_p(0x1000)          # (the flags are checked before anything is read)
    for flags in (_lib.F_DICT_BLOCK_PARALLEL, _lib.F_DICT_BLOCK_PARALLEL | _lib.F_BLOCK_PARALLEL):
        for ex in (False, True):
            h = C.c_void_p()
            if ex:
                st = L.zd_seekable_read_create_ex(fake, None, None, None, C.c_size_t(0), C.c_uint32(flags),
                                                  C.c_uint32(0), None, C.byref(h))
            else:
                st = L.zd_seekable_read_create(fake, None, None, None, C.c_size_t(0), C.c_uint32(flags), None,
                                               C.byref(h))
            assert st == _lib.INVALID_ARG and not h.value, (flags, ex)
