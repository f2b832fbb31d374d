"""CPU-side checks of the dictionary-set additions to the C ABI (include/zd.h
zd_dict_set_*, zd_plan_create_dicts, zd_decompress_dicts,
zd_batch_create_dicts): the symbols are exported and bound, argument checks
come before any HIP call (this file runs without a GPU), the CLI takes -D more
than once, and the planner's per-frame pass picks each frame's dictionary from
the plan's table (tests/native/plan_dicts.cpp drives zd_plan.h plan_frame with
g++)."""
import ctypes as C
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("zd_dict_set_create", "zd_dict_set_destroy", "zd_dict_set_info", "zd_plan_create_dicts",
       "zd_decompress_dicts", "zd_batch_create_dicts")


def test_new_symbols_exported_and_bound():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for n in NEW:
        assert n in _lib.SIGNATURES, n
        fn = getattr(L, n)
        assert fn.argtypes == _lib.SIGNATURES[n][1] and fn.restype == _lib.SIGNATURES[n][0], n
    import zstd_decompressor
    assert zstd_decompressor.DictionarySet is zstd_decompressor.batch.DictionarySet
    assert "DictionarySet" in zstd_decompressor.__all__


def test_abi_version_and_set_limit():
    from zstd_decompressor import _lib
    assert _lib.lib().zd_abi_version() == 8
    header = open(os.path.join(ROOT, "include", "zd.h")).read()
    assert "#define ZD_ABI_VERSION 8" in header
    assert "#define ZD_DICT_SET_MAX %d\n" % _lib.DICT_SET_MAX in header
    assert _lib.DICT_SET_MAX >= 256


def test_argument_checks_come_first():
    """NULL, zero-count and bad-fallback arguments: ZD_E_INVALID_ARG with no
    device present (a NULL entry stands for a destroyed dictionary too: the
    Python Dictionary's handle is NULL once closed)."""
    from zstd_decompressor import _lib
    L = _lib.lib()
    bad = _lib.INVALID_ARG
    h = C.c_void_p()
    one = (C.c_void_p * 1)(None)
    two = (C.c_void_p * 2)(None, None)
    assert L.zd_dict_set_create(None, 1, 0, C.byref(h)) == bad
    assert L.zd_dict_set_create(one, 0, -1, C.byref(h)) == bad          # ndicts == 0
    assert L.zd_dict_set_create(one, 1, 0, None) == bad
    assert L.zd_dict_set_create(one, 1, 0, C.byref(h)) == bad           # a NULL entry
    assert L.zd_dict_set_create(two, 2, -1, C.byref(h)) == bad
    for fb in (-2, 1, 2, 1 << 20):                                      # fallback outside [-1, ndicts)
        assert L.zd_dict_set_create(one, 1, fb, C.byref(h)) == bad, fb
    assert L.zd_dict_set_create(one, _lib.DICT_SET_MAX + 1, -1, C.byref(h)) == bad
    assert not h.value
    L.zd_dict_set_destroy(None)
    n, fb = C.c_size_t(), C.c_int()
    assert L.zd_dict_set_info(None, C.byref(n), C.byref(fb)) == bad
    x = C.c_char_p(b"x")
    assert L.zd_plan_create_dicts(x, 1, 0, None, C.byref(h)) == bad     # no set
    assert L.zd_plan_create_dicts(None, 16, 0, None, C.byref(h)) == bad
    assert L.zd_plan_create_dicts(x, 1, 0, None, None) == bad
    ol = C.c_size_t()
    out = (C.c_uint8 * 16)()
    assert L.zd_decompress_dicts(x, 1, out, 16, C.byref(ol), 0, None) == bad
    vpp = C.POINTER(C.c_void_p)
    p = (C.c_void_p * 1)(None)
    z = (C.c_uint64 * 1)(0)
    assert L.zd_batch_create_dicts(C.cast(p, vpp), z, C.cast(p, vpp), z, 1, 0, None, None, C.byref(h)) == bad
    assert L.zd_batch_create_dicts(C.cast(p, vpp), z, C.cast(p, vpp), z, 0, 0, None, None, C.byref(h)) == bad
    assert not h.value


def test_python_set_refuses_what_is_not_a_dictionary():
    from zstd_decompressor import DictionarySet, ZdError
    with pytest.raises(TypeError):
        DictionarySet([b"raw bytes"])
    with pytest.raises(ZdError) as e:
        DictionarySet([])
    assert e.value.name == "InvalidArg" or e.value.code == -93


def test_cli_accepts_repeated_dictionary_option():
    from zstd_decompressor.__main__ import _parser
    a = _parser().parse_args(["in.zst", "-D", "a.dict", "-o", "out", "-D", "b.dict", "-D", "c.raw"])
    assert a.dictionary == ["a.dict", "b.dict", "c.raw"] and a.output == "out"
    assert _parser().parse_args(["in.zst", "-D", "a.dict"]).dictionary == ["a.dict"]
    assert _parser().parse_args(["in.zst"]).dictionary is None


# ---------------------------------------------------------------------------
# plan_frame with a dictionary table
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def plan_dicts(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_dicts")
    exe = d / "plan_dicts"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "plan_dicts.cpp")])

    def run(fallback):
        out = subprocess.run([str(exe), str(fallback)], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        return [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    return run


# (out_len0, rep x 3, huf_src, tab_src x 3, status, dictionary index); the
# table: 0 = raw 5000 B, 1 = ID 300 / 3000 B / comp 0, 2 = ID 70000 / 16 KiB / comp 1
ID300 = (3000, 11, 12, 13, 0, 0, 0, 0, 0, 1)
ID70000 = (16384, 21, 22, 23, 1, 1, 1, 1, 0, 2)
HUFFMAN_DECODER_MISSING, DICT_MISMATCH = -20, -99
NONE = (0, 1, 4, 8, -1, -1, -1, -1, HUFFMAN_DECODER_MISSING, 3)     # what a plan without a dictionary gives it
RAW = (5000, 1, 4, 8, -1, -1, -1, -1, HUFFMAN_DECODER_MISSING, 0)   # content, but no tables for a Treeless block
UNKNOWN = (0, 1, 4, 8, -1, -1, -1, -1, DICT_MISMATCH, 3)
SKIPPABLE = (0, 1, 4, 8, -9, -9, -9, -9, 0, 3)


def test_plan_frame_takes_each_frames_dictionary(plan_dicts):
    """Frames with IDs 300, absent, 70000, 0, 5 (unknown), a skippable frame,
    300 again: by ID from the sorted table; absent or 0 -> the fallback."""
    assert plan_dicts(-1) == [ID300, NONE, ID70000, NONE, UNKNOWN, SKIPPABLE, ID300]
    assert plan_dicts(0) == [ID300, RAW, ID70000, RAW, UNKNOWN, SKIPPABLE, ID300]
    assert plan_dicts(2) == [ID300, ID70000, ID70000, ID70000, UNKNOWN, SKIPPABLE, ID300]
