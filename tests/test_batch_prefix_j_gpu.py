"""Prefix batches on the block-parallel executor (K4J): a prefix batch created
with F_BLOCK_PARALLEL sends every frame with a compressed block through
zd_k_jsum .. zd_k_jscatter<true> .. zd_k_jround, the scatter writing the match
bytes whose sources lie in the frame's prefix as final words; the frames
without a compressed block stay on zd_k_execute_prefix.

Expected bytes are always the original record AND corpus.zdict.prefix_decompress
of the same frame with the same prefix (delta() checks the second when it makes
a chunk); a chunk that must fail has one exact expected status, the status the
same batch gives without the flag.  The harness (Arena, Run, Chunk: ranges inside
0xA5-filled tensors, 64 bytes of slack on every side, the slack, the prefixes and
the sources compared after each decode) is tests/test_batch_prefix_gpu.py's, and
every case runs through both creation calls."""
import functools

import numpy as np
import pytest

from corpus import gen, libzstd, zdict
from test_batch_prefix_gpu import (FILL, LL_DIST, ML_DIST, OF_DIST, PAGE, Chunk, Run, big_pair, delta, edge_records,
                                   hand_frame, ml_code, needs_its_prefix, page_chunks, pages, rnd, spread_symbols,
                                   trained)

pytestmark = pytest.mark.gpu


def flag_j():
    from zstd_decompressor import _lib
    return _lib.F_BLOCK_PARALLEL


def both_j(chunks, flags=0, shift=0, want_j=True):
    """The chunks through both creation calls with F_BLOCK_PARALLEL | flags:
    (statuses, lengths, outputs), the two calls agreeing on all of it."""
    from zstd_decompressor import _lib
    res = []
    for device in (False, True):
        r = Run(chunks, device, flags=flags | flag_j(), shift=shift)
        try:
            st, ln = r.decode()
            assert bool(r.b.info.executors & _lib.EXEC_K4J) == want_j, r.b.info.executors
            assert r.b.info.prefix_bytes_total == r.prefix_total
            res.append((st, ln, r.out))
        finally:
            r.close()
    assert res[0] == res[1], "the host-array and the device-array batch differ"
    return res[0]


def expect_all_ok_j(chunks, flags=0, shift=0):
    st, ln, out = both_j(chunks, flags, shift)
    assert st == [0] * len(chunks), [(i, s) for i, s in enumerate(st) if s]
    for i, c in enumerate(chunks):
        assert ln[i] == len(c.record), i
        assert out[i] == c.record, i


# ---------------------------------------------------------------------------
# 1. page deltas; 8. the same batch without the flag
# ---------------------------------------------------------------------------
def test_page_deltas_block_parallel():
    chunks = page_chunks()[:64]                 # prefix alignments 0-15, destination alignments 0-15
    assert {c.palign for c in chunks} == set(range(16)) and {c.dalign for c in chunks} == set(range(16))
    assert all(needs_its_prefix(c.frame, PAGE) for c in chunks)
    expect_all_ok_j(chunks)


def test_unflagged_batch_stays_on_the_streaming_executor():
    chunks = page_chunks()[:64]
    for device in (False, True):
        r = Run(chunks, device)
        try:
            st, ln = r.decode()
            assert r.b.info.executors == 0
            assert st == [0] * 64 and all(o == c.record for o, c in zip(r.out, chunks))
        finally:
            r.close()


# ---------------------------------------------------------------------------
# 2. the prefix boundary
# ---------------------------------------------------------------------------
def test_periods_across_the_boundary():
    """Matches that start in the prefix and run into the frame's own bytes with
    a period below the match length: the record repeats its prefix's last o
    bytes, at every piece alignment (the record lengths move the destinations'
    pieces against the periods) and every prefix alignment."""
    chunks = []
    for i in range(96):
        o = (1, 2, 3, 15, 16, 17)[i % 6]
        P = rnd(0x9E820D00 + i, 5000)
        rec = (P[-o:] * (3200 // o + 1))[:200 + 31 * i]
        chunks.append(delta(rec, P, palign=i % 16, dalign=(3 * i) % 16))
        # a period that starts further back in the prefix and crosses the boundary mid-piece
        if i < 16:
            back = 40 + i
            rec2 = P[-back:] + (P[-o:] * 64)[:300 + i] + rnd(0x9E830000 + i, 9) + P[-o - 7:] * 5
            chunks.append(delta(rec2, P, palign=(5 * i) % 16, dalign=i))
    # (libzstd finds the periods of 15 and more in the prefix; the shorter ones it starts from the frame's own
    # literals, so those records decode alone: the hand-assembled frames below cross the boundary with them)
    assert sum(needs_its_prefix(c.frame, len(c.record)) for c in chunks) >= 60
    expect_all_ok_j(chunks)


def hand_period_frame(lits, off, ml):
    """One frame of one compressed block: Raw literals `lits` (at most 15), one
    sequence in Predefined mode -- literal length len(lits), offset `off`, match
    length `ml` (at most 66): with off > len(lits) the match starts in the prefix,
    with ml > off it runs on with period `off` into its own bytes."""
    ll = len(lits)
    assert ll < 16 and 3 <= ml <= 66 and ll + ml < 256
    ov = off + 3
    ofc = ov.bit_length() - 1
    mlc, mlx, mlb = ml_code(ml)
    st_ll = spread_symbols(6, LL_DIST).index(ll)          # literal lengths below 16: the code is the length
    st_of = spread_symbols(5, OF_DIST).index(ofc)
    st_ml = spread_symbols(6, ML_DIST).index(mlc)
    acc, nb = 0, 0
    for v, n in ((0, 0), (mlx, mlb), (ov - (1 << ofc), ofc), (st_ml, 6), (st_of, 5), (st_ll, 6), (1, 1)):
        acc |= v << nb
        nb += n
    bits = acc.to_bytes((nb + 7) // 8, "little")
    block = bytes([ll << 3]) + lits + bytes([1, 0]) + bits
    hdr = (1 | (2 << 1) | (len(block) << 3)).to_bytes(3, "little")
    return bytes.fromhex("28b52ffd") + bytes([0x20, ll + ml]) + hdr + block


PERIOD_CASES = [(o, ll) for o in (1, 2, 3, 15, 16, 17) for ll in (0, 1, 2, 5, 14) if ll < o]


def test_hand_assembled_periods_across_the_boundary():
    """Periods 1, 2, 3, 15, 16, 17 below the match length, the match starting
    o - ll bytes before the frame's first byte: behind a 64-byte prefix, and
    behind one of exactly o - ll bytes (the match reaches prefix byte 0)."""
    chunks = []
    for k, (o, ll) in enumerate(PERIOD_CASES):
        ml = 40 if o < 15 else 66
        lits = rnd(0x4C00 + k, ll)
        frame = hand_period_frame(lits, o, ml)
        for P in (rnd(0x4C40 + k, 64), rnd(0x4C80 + k, o - ll)):
            want = zdict.prefix_decompress(frame, P, ll + ml)        # libzstd accepts the frame
            hist = bytearray(P + lits)
            for _ in range(ml):
                hist.append(hist[len(hist) - o])                      # the reference's byte-by-byte push
            assert want == bytes(hist[len(P):]) and len(want) == ll + ml, (o, ll)
            for a in (0, 5, 11, 15):
                chunks.append(Chunk(frame, P, record=want, palign=(a + k) % 16, dalign=(3 * a + k) % 16))
    assert len(chunks) == 8 * len(PERIOD_CASES) and len(PERIOD_CASES) == 21
    expect_all_ok_j(chunks)


def test_tiny_prefixes():
    """Prefix sizes 1, 15, 16, 17 (and 2..14), and 0 with a null address."""
    chunks = []
    for K in (1, 15, 16, 17) + tuple(range(2, 15)):
        P = rnd(0x7291 + K, K)
        rec = (P * 40)[:300] + rnd(0x7292 + K, 30) + P * 3
        for a in (0, 7):
            chunks.append(delta(rec, P, palign=(K * 5 + a) % 16, dalign=(K + a) % 16))
    plain_rec = gen.text(3000, seed=0x7293)
    chunks.append(Chunk(libzstd.compress(plain_rec, 3), None, record=plain_rec, dalign=3))     # size 0, address NULL
    expect_all_ok_j(chunks)


@pytest.mark.parametrize("K", [1, 2, 8, 14])
def test_first_sequence_reaches_prefix_byte_0(K):
    """The hand-assembled frames: one sequence whose match starts at prefix byte
    0 and runs through the prefix and the literals into its own bytes."""
    P = rnd(0x4B9D + K, K)
    lits = rnd(0x4B9E + K, 5)
    frame = hand_frame(K, lits)
    n = 5 + 3 * K + 7
    want = zdict.prefix_decompress(frame, P, n)
    hist = bytearray(P + lits)
    for j in range(3 * K + 7):
        hist.append(hist[j])
    assert want == bytes(hist[K:]) and len(want) == n
    chunks = [Chunk(frame, P, record=want, palign=a, dalign=(a + K) % 16) for a in range(16)]
    expect_all_ok_j(chunks)


@pytest.mark.parametrize("shift", range(16))
def test_edges(shift):
    recs = edge_records()
    chunks = [delta(r, P, dalign=(7 * i) % 16) for i, (P, r) in enumerate(recs)]
    assert all(needs_its_prefix(c.frame, len(c.record)) for c in chunks)
    expect_all_ok_j(chunks, shift=shift)


# ---------------------------------------------------------------------------
# 3. far sources
# ---------------------------------------------------------------------------
def test_far_sources():
    rng = np.random.default_rng(0xFA46)
    chunks = []
    for i in range(16):
        P = rng.integers(0, 256, 64 << 10, dtype=np.uint8).tobytes()
        parts = []
        for _ in range(40):
            n = int(rng.integers(20, 300))
            at = int(rng.integers(0, len(P) - n))
            parts.append(P[at:at + n])
            parts.append(rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8).tobytes())
        chunks.append(delta(b"".join(parts), P, palign=(i * 7) % 16, dalign=(i * 11) % 16))
    expect_all_ok_j(chunks)


# ---------------------------------------------------------------------------
# 4. multi-block frames
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("level", [1, 19])
def test_multi_block(level):
    old, new = big_pair()
    c = delta(new, old, level, palign=9, dalign=3)
    expect_all_ok_j([c, delta(new[:1000], old[:700], level)])


def test_frame_without_content_size():
    old, new = big_pair()
    c = delta(new, old, 3, content_size=False, palign=1, dalign=15)
    assert libzstd.frame_content_size(c.frame) == (1 << 64) - 1
    expect_all_ok_j([c])


@functools.lru_cache(maxsize=None)
def delta_2m5():
    n = 2560 << 10
    old = gen.text(n, seed=0xB26)
    new = bytearray(old)
    rng = np.random.default_rng(0xB27)
    for p in rng.choice(n, n // 100, replace=False):
        new[p] ^= int(rng.integers(1, 256))
    return delta(bytes(new), old, 3, palign=13, dalign=6)


def test_delta_of_twenty_blocks():
    from zstd_decompressor.batch import frames_index
    c = delta_2m5()
    _, blocks, st, _ = frames_index(c.frame)
    assert st == 0 and sum(b["type"] == 2 for b in blocks) >= 16
    assert len(c.frame) * 4 < len(c.record)
    expect_all_ok_j([c])


def test_block_of_many_scatter_segments():
    """One block of more than J_SEG (512) sequences, every one a match into the
    prefix: the later segments start from their checkpoints and read the prefix."""
    from zstd_decompressor.batch import frames_index
    rng = np.random.default_rng(0x75E6)
    P = rng.integers(0, 256, 64 << 10, dtype=np.uint8).tobytes()
    parts = []
    for _ in range(2600):
        n = int(rng.integers(20, 40))
        at = int(rng.integers(0, len(P) - n))
        parts.append(P[at:at + n])
        parts.append(rng.integers(0, 256, int(rng.integers(0, 3)), dtype=np.uint8).tobytes())
    rec = b"".join(parts)
    assert len(rec) < 128 << 10
    c = delta(rec, P, palign=11, dalign=5)
    frames, blocks, st, _ = frames_index(c.frame)
    assert st == 0 and len(blocks) == 1 and blocks[0]["type"] == 2
    for device in (False, True):
        r = Run([c], device, flags=flag_j())
        try:
            st, ln = r.decode()
            assert r.b.info.nsequences > 3 * 512
            assert st == [0] and r.out[0] == rec
        finally:
            r.close()


# ---------------------------------------------------------------------------
# 5. one mixed batch
# ---------------------------------------------------------------------------
def test_mixed_batch_statuses_equal_the_unflagged_ones():
    from zstd_decompressor import _lib
    P5 = rnd(0x58A0, 5000)
    good = lambda i: delta((P5[100 * i:100 * i + 900] + bytes([i]) * 7) * 2, P5, palign=i, dalign=2 * i)
    plain_rec = gen.text(3000, seed=0x58A1)
    plain = Chunk(libzstd.compress(plain_rec, 3), None, record=plain_rec)                  # no prefix, NULL address
    raw_rec = rnd(0x58A2, 2000)
    raw = Chunk(libzstd.compress(raw_rec, 1), P5, record=raw_rec, palign=3)               # a Raw block only
    rle_rec = b"\x00" * 70000
    rle_frame = libzstd.compress(rle_rec, 1)
    empty = Chunk(b"", None, cap=0, record=b"")
    with_id = Chunk(zdict.compress(plain_rec, trained(), 3), P5, record=plain_rec)
    K = 8
    Pk = rnd(0x58A3, K)
    hf = hand_frame(K, rnd(0x58A4, 5))
    hand_ok = Chunk(hf, Pk, record=zdict.prefix_decompress(hf, Pk, 5 + 3 * K + 7), palign=9)
    hand_short = Chunk(hf, Pk[1:], cap=5 + 3 * K + 7, record=None, palign=4)              # one byte short
    g = good(9)
    truncated = Chunk(g.frame[:-3], P5, cap=len(g.record), record=g.record)
    chunks = [good(0), plain, good(1), raw, Chunk(rle_frame, P5, record=rle_rec), good(2), empty, with_id, good(3),
              hand_ok, hand_short, good(4), truncated, good(5)]
    failing = {7: _lib.DICT_MISMATCH, 10: _lib.IMPOSSIBLE_VALUE, 12: None}
    from zstd_decompressor.batch import frames_index
    assert all(b["type"] != 2 for b in frames_index(raw.frame)[1])
    # without the flag: the route the existing suite pins
    unflagged = []
    for device in (False, True):
        r = Run(chunks, device)
        try:
            st0, ln0 = r.decode()
            assert r.b.info.executors == 0
            unflagged.append((st0, ln0))
        finally:
            r.close()
    assert unflagged[0] == unflagged[1]
    st0, ln0 = unflagged[0]
    st, ln, out = both_j(chunks)
    assert st == st0 and ln == ln0
    for i, c in enumerate(chunks):
        if i in failing:
            assert st[i] != 0 and ln[i] == 0, i
            if failing[i] is not None:
                assert st[i] == failing[i], (i, st[i])
        else:
            assert st[i] == 0 and ln[i] == len(c.record) and out[i] == c.record, (i, st[i])


# ---------------------------------------------------------------------------
# 6. verification, relaunch with changed prefix contents, graph capture
# ---------------------------------------------------------------------------
def test_verified_and_relaunched_with_a_changed_prefix():
    from zstd_decompressor import _lib
    chunks = page_chunks(True, 64)
    old, new, edited = pages()[7]
    gaps = np.diff(edited)
    k = int(np.argmax(gaps))
    assert gaps[k] > 80
    pos = int(edited[k]) + int(gaps[k]) // 2      # a prefix byte inside a matched region
    for device in (False, True):
        r = Run(chunks, device, flags=_lib.F_VERIFY_CHECKSUM | _lib.F_BLOCK_PARALLEL)
        try:
            st, ln = r.decode()
            assert r.b.info.executors & _lib.EXEC_K4J
            assert st == [0] * 64 and all(o == c.record for o, c in zip(r.out, chunks))
            at = r.po[7] + pos
            r.P.t[at] ^= 0xFF
            r.P.host[at] ^= 0xFF
            st, ln = r.decode()
            assert st[7] == _lib.CHECKSUM_WRONG and ln[7] == 0
            assert [s for i, s in enumerate(st) if i != 7] == [0] * 63
            assert all(r.out[i] == chunks[i].record for i in range(64) if i != 7)
            r.P.t[at] ^= 0xFF
            r.P.host[at] ^= 0xFF
            st, ln = r.decode()
            assert st == [0] * 64 and all(o == c.record for o, c in zip(r.out, chunks))
        finally:
            r.close()


def test_hip_graph_capture_replay():
    import torch
    chunks = page_chunks()[:64]
    dev = torch.device("cuda", 0)
    for device in (False, True):
        r = Run(chunks, device, flags=flag_j())
        try:
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):          # warm-up outside the capture
                r.b.decode_async(s.cuda_stream)
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                r.b.decode_async(s.cuda_stream)
            for _ in range(2):
                r.D.t.fill_(FILL)
                torch.cuda.synchronize(dev)
                g.replay()
                torch.cuda.synchronize(dev)
                r.status, r.length = r.b.results(torch.cuda.current_stream(dev).cuda_stream)
                r.read_back()
                assert r.status == [0] * 64
                assert all(o == c.record for o, c in zip(r.out, chunks))
            del g
        finally:
            r.close()


# ---------------------------------------------------------------------------
# 7. the redo path: chunks whose pointer jumping did not converge
# ---------------------------------------------------------------------------
def deep_chain_chunk(i):
    """A record that needs its prefix AND more than one hop: X (bytes that are
    not in the prefix) eight times over with separators of growing lengths (no
    one overlapping match), so each copy's words point at the copy before it,
    whose words are pending themselves."""
    P = rnd(0x8ED0 + i, 4000)
    X = rnd(0x8EE0 + i, 1500)
    rec = P[100:1100] + b"".join(X + rnd(0x8EF0 + 16 * i + k, 3 + 2 * k) for k in range(8)) + P[2000:3000]
    return delta(rec, P, palign=i % 16, dalign=(7 * i) % 16)


def test_redo_keeps_the_prefixes():
    import torch
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import _read_u64
    chunks = page_chunks()[:64] + [deep_chain_chunk(i) for i in range(4)]
    n = len(chunks)
    assert all(needs_its_prefix(c.frame, len(c.record)) for c in chunks)
    for device in (False, True):
        r = Run(chunks, device, flags=_lib.F_J_ONE_ROUND | _lib.F_BLOCK_PARALLEL)
        try:
            r.b.decode_async(torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            # the launch's own statuses, before results() decodes anything again
            words = _read_u64(r.b.device_results()[0], (n + 1) // 2)
            dev_st = np.array(words, dtype=np.uint64).view(np.int32)[:n]
            assert all(dev_st[64 + i] == _lib.OUT_OF_DOMAIN for i in range(4)), dev_st[64:]
            r.status, r.length = r.b.results(torch.cuda.current_stream().cuda_stream)
            r.read_back()
            assert r.status == [0] * n, [(i, s) for i, s in enumerate(r.status) if s]
            assert all(o == c.record for o, c in zip(r.out, chunks))
        finally:
            r.close()
