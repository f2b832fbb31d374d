"""Frames compressed with a zstd dictionary (RFC 8878 5) on the GPU path:
zd_dict_create / zd_plan_create_dict (include/zd.h), the streaming K4's
dictionary variant (zd_k_execute_dict) and the dictionary's tables
(zd_k_dict_tables).

The reference parses a frame's Dictionary_ID and ignores it, and the oracle has
no dictionaries: the expected bytes here are the source records, which
libzstd's ZSTD_decompress_usingDict reproduces from the same frames
(corpus/zdict.py).  Every test first checks, from the frames' own bytes, that
the frames have the shape it is about (one sequence, Treeless + Repeat, ...),
so it cannot pass on some other shape.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from corpus import gen, libzstd, zdict
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dict")


# ---------------------------------------------------------------------------
# the frames' own bytes
# ---------------------------------------------------------------------------
def header_layout(frame: bytes):
    """Offsets inside a zstd frame header: (dict_id offset, its size, FCS
    offset, its size, first block header offset)."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    single = (fhd >> 5) & 1
    did_size = [0, 1, 2, 4][fhd & 3]
    fcs_size = [1 if single else 0, 2, 4, 8][fhd >> 6]
    did_at = 5 + (0 if single else 1)
    fcs_at = did_at + did_size
    return did_at, did_size, fcs_at, fcs_size, fcs_at + fcs_size


def first_block_shape(frame: bytes):
    """The first block of a frame: (block type, literals type, nseq, (LL, OF,
    ML) modes); literals type / nseq / modes None unless it is compressed."""
    at = header_layout(frame)[4]
    bh = frame[at] | frame[at + 1] << 8 | frame[at + 2] << 16
    btype = (bh >> 1) & 3
    if btype != 2:
        return btype, None, None, None
    p = at + 3
    b0 = frame[p]
    lt, sf = b0 & 3, (b0 >> 2) & 3
    if lt in (0, 1):                      # Raw / RLE
        hs = [1, 2, 1, 3][sf]
        v = int.from_bytes(frame[p:p + hs], "little")
        regen = v >> 3 if hs == 1 else v >> 4
        p += hs + (regen if lt == 0 else 1)
    else:                                 # Compressed / Treeless
        hs = [3, 3, 4, 5][sf]
        v = int.from_bytes(frame[p:p + hs], "little")
        bits = [10, 10, 14, 18][sf]
        comp = (v >> (4 + bits)) & ((1 << bits) - 1)
        p += hs + comp
    n0 = frame[p]
    if n0 == 0:
        return btype, lt, 0, None
    if n0 < 128:
        nseq, p = n0, p + 1
    elif n0 < 255:
        nseq, p = ((n0 - 128) << 8) + frame[p + 1], p + 2
    else:
        nseq, p = frame[p + 1] + (frame[p + 2] << 8) + 0x7F00, p + 3
    m = frame[p]
    return btype, lt, nseq, (m >> 6, (m >> 4) & 3, (m >> 2) & 3)


def treeless_repeat(frame: bytes) -> bool:
    bt, lt, nseq, modes = first_block_shape(frame)
    return bt == 2 and lt == 3 and bool(nseq) and modes == (3, 3, 3)


def ncount_bytes(d: bytes, at: int) -> int:
    """Bytes an FSE table description takes from d[at] (RFC 8878 4.1.1)."""
    bit = 0

    def take(n):
        nonlocal bit
        v = 0
        for i in range(n):
            v |= ((d[at + ((bit + i) >> 3)] >> ((bit + i) & 7)) & 1) << i
        bit += n
        return v

    al = take(4) + 5
    remaining, nsym = 1 << al, 0
    while remaining > 0 and nsym < 256:
        bits = (remaining + 1).bit_length()
        save = bit
        pk = take(bits)
        low_mask = (1 << (bits - 1)) - 1
        thr = (1 << bits) - 1 - (remaining + 1)
        low = pk & low_mask
        if low < thr:
            bit = save + bits - 1
            val = low
        else:
            val = pk - thr if pk > low_mask else pk
        proba = val - 1
        remaining -= abs(proba)
        nsym += 1
        if proba == 0:
            while True:
                r = take(2)
                nsym += r
                if r != 3:
                    break
    assert remaining == 0
    return (bit + 7) // 8


def entropy_layout(d: bytes):
    """A formatted dictionary's sections: (Huffman description offset, the
    three FSE descriptions' offsets, repeat offsets' offset, content offset)."""
    assert d[:4] == b"\x37\xa4\x30\xec"
    h = d[8]
    p = 8 + 1 + (h if h < 128 else (h - 127 + 1) // 2)
    fse = []
    for _ in range(3):
        fse.append(p)
        p += ncount_bytes(d, p)
    return 8, fse, p, p + 12


# ---------------------------------------------------------------------------
# corpora (seeded; built once per session)
# ---------------------------------------------------------------------------
def records_of(text: bytes, size: int):
    return [text[i:i + size] for i in range(0, len(text) - size + 1, size)]


@functools.lru_cache(maxsize=None)
def raw5000() -> bytes:
    return np.random.default_rng(0xD1C7).integers(0, 256, 5000, dtype=np.uint8).tobytes()


@functools.lru_cache(maxsize=None)
def trained16():
    """16 KiB dictionary trained on 512 records of 4 KiB of gen.text; 128 other
    records of 512 B, 1 KiB, 4 KiB and 8 KiB and their frames."""
    d = zdict.train(records_of(gen.text(512 * 4096, seed=0xD1C0), 4096), 16 << 10)
    other = gen.text(32 * (512 + 1024 + 4096 + 8192), seed=0xD1C1)
    recs, at = [], 0
    for i in range(128):
        n = (512, 1024, 4096, 8192)[i % 4]
        recs.append(other[at:at + n])
        at += n
    frames = [zdict.compress(r, d, 3) for r in recs]
    return d, recs, frames


@functools.lru_cache(maxsize=None)
def trained112():
    return zdict.train(records_of(gen.text(2048 * 4096, seed=0xD1C2), 4096), 112 << 10)


# ---------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------
def decode_host(data: bytes, dictionary, flags: int = 0):
    """zd_plan_decompress (host in, host out): (status, bytes, plan info)."""
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Plan, run_plan
    plan = Plan(data, False, flags, dictionary=dictionary)
    try:
        p, n, keep = _lib.buf(data)
        st, out = run_plan(plan, p, n)
        info = plan.refresh_info()
        return st, out, {"replans": info.replans, "executors": info.executors, "nframes": info.nframes}
    finally:
        plan.close()


def decode_device(data: bytes, dictionary, flags: int = 0, checksums: bool = False):
    """zd_decode_async + zd_plan_results (+ zd_plan_checksums) on torch
    buffers: (status, [frame statuses], [frame bytes], checksum oks, info)."""
    import torch
    from zstd_decompressor.batch import Plan
    plan = Plan(data, False, flags, dictionary=dictionary)
    try:
        n = int(plan.info.out_bytes)
        dev = torch.device("cuda", 0)
        d_src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
        d_src[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        d_dst = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, s)
        st, total, fst, flen, first = plan.results(d_dst.data_ptr(), s)
        ok = plan.checksums(d_dst.data_ptr(), s)[0] if checksums else None
        out = bytes(d_dst[:total].cpu().numpy().tobytes())
        parts, at = [], 0
        for code, ln in zip(fst, flen):
            parts.append(out[at:at + ln] if code == 0 else None)
            at += ln if code == 0 else 0
        assert at == total
        return st, fst, parts, ok, plan.refresh_info()
    finally:
        plan.close()


@pytest.fixture(scope="module")
def Dictionary():
    from zstd_decompressor.batch import Dictionary
    return Dictionary


# ---------------------------------------------------------------------------
# 1. a match source that starts in the dictionary and runs into the frame
# ---------------------------------------------------------------------------
def test_straddle_one_sequence(Dictionary):
    D = raw5000()
    record = D[-100:] * 30
    frame = zdict.compress(record, D, 3)
    assert first_block_shape(frame)[2] == 1, first_block_shape(frame)
    assert zdict.decompress(frame, D, len(record)) == record
    with pytest.raises(RuntimeError):
        libzstd.decompress_frame(frame, len(record))
    d = Dictionary(D)
    assert (d.dict_id, d.content_size, d.raw_content, d.repeat_offsets) == (0, 5000, True, (1, 4, 8))
    st, out, info = decode_host(frame, d)
    assert st == 0 and out == record and info["executors"] == 0
    st, fst, parts, _, _ = decode_device(frame, d)
    assert st == 0 and parts == [record]
    d.close()


def test_straddle_two_sequences(Dictionary):
    D = raw5000()
    rnd = np.random.default_rng(0xD1C8).integers(0, 256, 50, dtype=np.uint8).tobytes()
    record = D[-100:] * 30 + rnd + D[100:900]
    assert len(record) == 3850
    frame = zdict.compress(record, D, 3)
    assert first_block_shape(frame)[2] == 2, first_block_shape(frame)
    assert zdict.decompress(frame, D, len(record)) == record
    d = Dictionary(D)
    st, out, _ = decode_host(frame, d)
    assert st == 0 and out == record
    d.close()


def test_straddle_batch_of_periods(Dictionary):
    """64 frames whose records repeat the dictionary's last k bytes: pieces
    that begin before the boundary at every alignment, periods below 16."""
    D = raw5000()
    recs = []
    for i in range(64):
        k = (1, 7, 15, 16, 17, 33, 100)[i % 7]
        recs.append((D[-k:] * (3200 // k + 1))[:200 + 47 * i])
    frames = [zdict.compress(r, D, 3) for r in recs]
    for r, f in zip(recs, frames):
        assert zdict.decompress(f, D, len(r)) == r
    assert all(first_block_shape(f)[2] == 1 for f in frames)
    d = Dictionary(D)
    st, fst, parts, _, _ = decode_device(b"".join(frames), d)
    assert st == 0 and fst == [0] * 64
    for i, (r, got) in enumerate(zip(recs, parts)):
        assert got == r, i
    st, out, _ = decode_host(b"".join(frames), d)
    assert st == 0 and out == b"".join(recs)
    d.close()


# ---------------------------------------------------------------------------
# 2. matches far into the dictionary (past K4's LDS window)
# ---------------------------------------------------------------------------
def test_far_into_the_dictionary(Dictionary):
    rng = np.random.default_rng(0xD1C9)
    D = rng.integers(0, 256, 64 << 10, dtype=np.uint8).tobytes()
    recs = []
    for _ in range(64):
        parts = []
        for _ in range(40):
            n = int(rng.integers(20, 300))
            at = int(rng.integers(0, len(D) - n))
            parts.append(D[at:at + n])
            parts.append(rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8).tobytes())
        recs.append(b"".join(parts))
    frames = [zdict.compress(r, D, 3) for r in recs]
    src_total, comp_total = sum(map(len, recs)), sum(map(len, frames))
    assert comp_total * 10 < src_total, (src_total, comp_total)
    d = Dictionary(D)
    st, fst, parts, _, _ = decode_device(b"".join(frames), d)
    assert st == 0
    for i, (r, got) in enumerate(zip(recs, parts)):
        assert got == r, i
    d.close()


# ---------------------------------------------------------------------------
# 3. a trained dictionary: Treeless literals and Repeat tables from it
# ---------------------------------------------------------------------------
def _flag(name):
    from zstd_decompressor import _lib
    return getattr(_lib, name) if name else 0


@pytest.mark.parametrize("flag", ["", "F_SEQ_NO_LATENCY", "F_SEQ_ONE_LANE", "F_K1_LANES", "F_K1_SPLIT"])
def test_trained_dictionary_tables(Dictionary, flag):
    dct, recs, frames = trained16()
    assert sum(treeless_repeat(f) for f in frames) >= 64
    failing = 0
    for f, r in zip(frames[:16], recs[:16]):
        try:
            libzstd.decompress_frame(f, len(r))
        except RuntimeError:
            failing += 1
    assert failing == 16                           # (no frame decodes without the dictionary)
    d = Dictionary(dct)
    assert d.dict_id == zdict.dict_id(dct) != 0 and not d.raw_content
    assert d.content_size == len(dct) - entropy_layout(dct)[3]
    st, fst, parts, _, info = decode_device(b"".join(frames), d, _flag(flag))
    assert st == 0 and info.executors == 0 and info.nframes == 128
    for i, (r, got) in enumerate(zip(recs, parts)):
        assert got == r, i
    d.close()


# ---------------------------------------------------------------------------
# 4. a plan past the small-plan thresholds (K3Q, several K4 rounds)
# ---------------------------------------------------------------------------
def test_large_plan_with_checksums(Dictionary):
    dct = trained112()
    recs = records_of(gen.text(2400 * 2048, seed=0xD1C3), 2048)
    assert len(recs) == 2400
    frames = [zdict.compress(r, dct, 3, checksum=True) for r in recs]
    assert sum(treeless_repeat(f) for f in frames) >= 1200
    data, want = b"".join(frames), b"".join(recs)
    d = Dictionary(dct)
    st, out, info = decode_host(data, d)
    assert st == 0 and out == want and info["executors"] == 0 and info["replans"] == 0
    st, fst, parts, ok, _ = decode_device(data, d, checksums=True)
    assert st == 0 and ok == [1] * 2400
    assert b"".join(parts) == want
    d.close()


# ---------------------------------------------------------------------------
# 5. frames of several blocks; frames without a Frame_Content_Size
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 3, 19])
def test_multi_block_frames(Dictionary, level):
    dct = trained112()
    record = gen.text(300 << 10, seed=0xD1C4)
    frame = zdict.compress(record, dct, level)
    assert zdict.decompress(frame, dct, len(record)) == record
    from zstd_decompressor.batch import frames_index
    frames, _, ist, _ = frames_index(frame)
    assert ist == 0 and frames[0]["num_blocks"] == 3
    assert first_block_shape(frame)[1] == 2           # the first block brings its own tree
    d = Dictionary(dct)
    st, out, _ = decode_host(frame, d)
    assert st == 0 and out == record
    d.close()


def test_frames_without_content_size(Dictionary):
    """No Frame_Content_Size: capacities are bounds and zd_plan_results
    compacts the frames in place."""
    dct = trained112()
    record = gen.text(300 << 10, seed=0xD1C4)
    recs = [record[i:i + 8192] for i in range(0, len(record), 8192)]
    frames = [zdict.compress(r, dct, 3, content_size=False) for r in recs]
    assert all(header_layout(f)[3] == 0 for f in frames)
    d = Dictionary(dct)
    st, fst, parts, _, info = decode_device(b"".join(frames), d)
    assert st == 0 and info.out_exact == 0
    assert parts == recs
    st, out, _ = decode_host(b"".join(frames), d)
    assert st == 0 and out == record
    d.close()


# ---------------------------------------------------------------------------
# 6. the committed fixture (made with libzstd; no trainer at test time)
# ---------------------------------------------------------------------------
def test_pinned_fixture(Dictionary):
    idx = json.load(open(os.path.join(GOLDEN, "index.json")))
    dct = open(os.path.join(GOLDEN, "dict.bin"), "rb").read()
    frames = open(os.path.join(GOLDEN, "frames.bin"), "rb").read()
    records = open(os.path.join(GOLDEN, "records.bin"), "rb").read()
    assert len(idx["frames"]) == 8 and sum(idx["frames"]) == len(frames) and sum(idx["records"]) == len(records)
    d = Dictionary(dct)
    assert d.dict_id == idx["dict_id"]
    st, fst, parts, _, _ = decode_device(frames, d)
    assert st == 0 and [len(p) for p in parts] == idx["records"]
    assert b"".join(parts) == records
    d.close()


def test_cli_dictionary_option(tmp_path, capsys):
    """python -m zstd_decompressor FILE -D DICT -o OUT (zstd's own -D)."""
    from zstd_decompressor.__main__ import main
    dct, recs, frames = trained16()
    (tmp_path / "in.zst").write_bytes(b"".join(frames[:8]))
    (tmp_path / "dict").write_bytes(dct)
    out = tmp_path / "out.txt"
    assert main([str(tmp_path / "in.zst"), "-D", str(tmp_path / "dict"), "-o", str(out)]) == 0
    assert out.read_bytes() == b"".join(recs[:8])
    assert main([str(tmp_path / "in.zst"), "-o", str(out)]) == 1          # without it: the reference's answer
    assert "Error: frame 0" in capsys.readouterr().err
    (tmp_path / "bad").write_bytes(dct[:40])
    assert main([str(tmp_path / "in.zst"), "-D", str(tmp_path / "bad"), "-o", str(out)]) == 1
    assert "DictionaryCorrupted" in capsys.readouterr().err


# ---------------------------------------------------------------------------
# 7. errors
# ---------------------------------------------------------------------------
def test_offset_past_dictionary_and_position(Dictionary):
    from zstd_decompressor import _lib
    D = raw5000()
    record = D[-100:] * 30
    frame = zdict.compress(record, D, 3)
    with pytest.raises(RuntimeError):                  # libzstd: "Corrupted block detected"
        zdict.decompress(frame, D[-50:], len(record))
    d = Dictionary(D[-50:])
    st, out, _ = decode_host(frame, d)
    assert st == _lib.IMPOSSIBLE_VALUE and out == b""
    d.close()


def test_dictionary_id_mismatch(Dictionary):
    from zstd_decompressor import _lib
    dct, recs, frames = trained16()
    bad = bytearray(frames[5])
    at, size = header_layout(frames[5])[:2]
    assert size > 0 and int.from_bytes(bad[at:at + size], "little") == zdict.dict_id(dct)
    bad[at] ^= 1
    assert int.from_bytes(bad[at:at + size], "little") != 0
    data = b"".join(frames[:5]) + bytes(bad) + b"".join(frames[6:8])
    d = Dictionary(dct)
    st, fst, parts, _, _ = decode_device(data, d)
    assert st == _lib.DICT_MISMATCH
    assert fst == [0] * 5 + [_lib.DICT_MISMATCH] + [_lib.NOT_DECODED] * 2
    assert parts[:5] == recs[:5]
    st, out, _ = decode_host(data, d)
    assert st == _lib.DICT_MISMATCH and out == b"".join(recs[:5])
    d.close()


def test_without_a_dictionary_status_is_unchanged():
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import decompress_status
    dct, recs, frames = trained16()
    f = next(f for f in frames if treeless_repeat(f))
    want_st, want_out = oracle.decompress_status(f)
    st, out = decompress_status(f)
    assert (st, out) == (want_st, want_out)
    assert st in (_lib.HUFFMAN_DECODER_MISSING, _lib.NO_PREVIOUS_DECODER)


def _create_status(data: bytes) -> int:
    from zstd_decompressor import _lib
    L = _lib.lib()
    p, n, keep = _lib.buf(data)
    h = C.c_void_p()
    st = L.zd_dict_create(p, n, C.byref(h))
    if st == 0:
        L.zd_dict_destroy(h)
    else:
        assert not h.value
    return st


def test_damaged_dictionaries():
    from zstd_decompressor import _lib
    dct = trained16()[0]
    huf, fse, rep, content = entropy_layout(dct)
    assert _create_status(dct) == 0
    assert _create_status(dct[:(huf + fse[0]) // 2]) == _lib.DICT_CORRUPTED     # inside the Huffman description
    assert _create_status(dct[:(fse[1] + fse[2]) // 2]) == _lib.DICT_CORRUPTED  # inside the second FSE description
    assert _create_status(dct[:rep + 6]) == _lib.DICT_CORRUPTED                 # inside the repeat offsets
    assert _create_status(dct[:content]) == _lib.DICT_CORRUPTED                 # no content
    size = len(dct) - content
    for v in (0, size + 1):
        bad = dct[:rep] + v.to_bytes(4, "little") + dct[rep + 4:]
        assert _create_status(bad) == _lib.DICT_CORRUPTED, v
    ok = dct[:rep] + size.to_bytes(4, "little") + dct[rep + 4:]
    assert _create_status(ok) == 0
    # a description that fails as it would in a block keeps its code: an
    # accuracy log of 5 + 15 in the first FSE description
    bad = bytearray(dct)
    bad[fse[0]] |= 0x0F
    assert _create_status(bytes(bad)) == _lib.LARGE_ACCURACY_LOG


# ---------------------------------------------------------------------------
# 8. a frame that overruns its declared size is planned again, with the dictionary
# ---------------------------------------------------------------------------
def test_capacity_replan_keeps_the_dictionary(Dictionary):
    dct, recs, frames = trained16()
    i = next(i for i, r in enumerate(recs) if len(r) == 4096 and treeless_repeat(frames[i]))
    f = bytearray(frames[i])
    _, _, at, size, _ = header_layout(frames[i])
    assert size == 2 and int.from_bytes(f[at:at + 2], "little") + 256 == 4096
    f[at:at + 2] = (2048 - 256).to_bytes(2, "little")
    d = Dictionary(dct)
    st, out, info = decode_host(bytes(f), d)
    assert st == 0 and out == recs[i] and info["replans"] >= 1
    d.close()


# ---------------------------------------------------------------------------
# 9. zd_decode_async of a dictionary plan in a HIP graph
# ---------------------------------------------------------------------------
def test_hip_graph_capture_replay_with_dictionary(Dictionary):
    import torch
    from zstd_decompressor.batch import Plan
    dct, recs, frames = trained16()
    data, want = b"".join(frames), b"".join(recs)
    d = Dictionary(dct)
    plan = Plan(data, dictionary=d)
    n = plan.info.out_bytes
    dev = torch.device("cuda", 0)
    d_src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    d_src[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    d_dst = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):          # warm-up outside the capture
        plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, s.cuda_stream)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, s.cuda_stream)
    for _ in range(2):
        d_dst.zero_()
        torch.cuda.synchronize(dev)
        g.replay()
        torch.cuda.synchronize(dev)
        st, total, _, _, _ = plan.results(d_dst.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
        assert st == 0 and total == len(want)
        assert bytes(d_dst[:total].cpu().numpy().tobytes()) == want
    plan.close()
    d.close()


# ---------------------------------------------------------------------------
# 10. the plan keeps its dictionary alive
# ---------------------------------------------------------------------------
def test_dictionary_destroyed_before_the_plan(Dictionary):
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Plan, run_plan
    dct, recs, frames = trained16()
    data = b"".join(frames[:32])
    d = Dictionary(dct)
    plan = Plan(data, dictionary=d)
    d.close()
    p, n, keep = _lib.buf(data)
    st, out = run_plan(plan, p, n)
    assert st == 0 and out == b"".join(recs[:32])
    plan.close()
