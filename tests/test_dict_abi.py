"""CPU-side checks of the dictionary additions to the C ABI (include/zd.h):
the symbols are exported and bound, the two status codes have names, argument
checks come before any HIP call (this file runs without a GPU), and the
corpus helper that makes the GPU tests' frames round-trips through libzstd."""
import ctypes as C

import numpy as np
import pytest

from corpus import gen, libzstd, zdict

NEW = ("zd_dict_create", "zd_dict_destroy", "zd_dict_info", "zd_plan_create_dict", "zd_decompress_dict")


def test_new_symbols_exported_and_bound():
    from zstd_decompressor import _lib
    L = _lib.lib()
    for n in NEW:
        assert n in _lib.SIGNATURES, n
        fn = getattr(L, n)
        assert fn.argtypes == _lib.SIGNATURES[n][1] and fn.restype == _lib.SIGNATURES[n][0], n
    import zstd_decompressor
    assert zstd_decompressor.Dictionary is zstd_decompressor.batch.Dictionary


def test_new_status_names_and_abi_version():
    from zstd_decompressor import _lib
    assert (_lib.DICT_CORRUPTED, _lib.DICT_MISMATCH) == (-98, -99)
    assert _lib.status_name(_lib.DICT_CORRUPTED) == "DictionaryCorrupted"
    assert _lib.status_name(_lib.DICT_MISMATCH) == "DictionaryMismatch"
    assert _lib.lib().zd_abi_version() == 8


def test_argument_checks_come_first():
    from zstd_decompressor import _lib
    L = _lib.lib()
    one = C.c_char_p(b"x")
    h = C.c_void_p()
    bad = _lib.INVALID_ARG
    assert L.zd_dict_create(None, 16, C.byref(h)) == bad
    assert L.zd_dict_create(one, 0, C.byref(h)) == bad
    assert L.zd_dict_create(one, 1, None) == bad
    assert not h.value
    assert L.zd_dict_info(None, None, None, None, None) == bad
    L.zd_dict_destroy(None)
    assert L.zd_plan_create_dict(None, 16, 0, None, C.byref(h)) == bad
    assert L.zd_plan_create_dict(one, 1, 0, None, None) == bad
    ol = C.c_size_t()
    out = (C.c_uint8 * 16)()
    assert L.zd_decompress_dict(None, 16, out, 16, C.byref(ol), 0, None) == bad
    assert not h.value


@pytest.mark.skipif(not libzstd.available(), reason="no libzstd")
def test_zdict_round_trips():
    text = gen.text(96 * 2048, seed=0xD1CA)
    recs = [text[i:i + 2048] for i in range(0, len(text), 2048)]
    trained = zdict.train(recs[:64], 8 << 10)
    assert trained[:4] == b"\x37\xa4\x30\xec" and zdict.dict_id(trained) != 0
    raw = np.random.default_rng(0xD1CB).integers(0, 256, 3000, dtype=np.uint8).tobytes()
    assert zdict.dict_id(raw) == 0
    for d, rec in ((trained, recs[70]), (raw, raw[-64:] * 20 + recs[71])):
        for kw in ({}, {"checksum": True}, {"content_size": False}):
            f = zdict.compress(rec, d, 3, **kw)
            assert zdict.decompress(f, d, len(rec)) == rec
            has_fcs = libzstd.frame_content_size(f) == len(rec)
            assert has_fcs == kw.get("content_size", True)
    # the trained dictionary's frame names its ID and needs it
    f = zdict.compress(recs[70], trained, 3)
    from zstd_decompressor.batch import frames_index
    frames, _, st, _ = frames_index(f)
    assert st == 0 and frames[0]["dict_id"] == zdict.dict_id(trained)
    with pytest.raises(RuntimeError):
        libzstd.decompress_frame(f, len(recs[70]))
