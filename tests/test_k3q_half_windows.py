"""K3Q's half-window chain (seq_chainqh: a ring of three bitstream windows,
each used by two FSE steps and loaded again one step after the second)
against the oracle, through the C ABI.

zd_k_sequences_q picks the chain per wave of 16 blocks: the half-window
chain when every block of the wave has 8 * bitstream bytes / sequences at or
below K3H_BITS (26), else seq_chainq for the whole wave.  ZD_F_SEQ_NO_LATENCY
with ZD_F_NO_FUSE makes small plans take K3Q (assert_parity checks the
plan's route).  Every case asks for the oracle's status and the oracle's
bytes; the host walk of the inputs (zd_frames_index, then the
literals and sequences headers) tells which chain a plan's waves take and
which table modes occur, and the tests fail when the inputs miss what they
are there for.
"""
import random

import pytest

from corpus import gen, libzstd
from oracle import oracle

pytestmark = pytest.mark.gpu

OUT_OF_DOMAIN = -91
K3H_BITS = 26                       # zd_kernels.hip ZD_K3H_BITS
CHAINS = 16                         # blocks per K3Q wave
MODES = ("Predefined", "RLE", "FSE", "Repeat")


def ncount_bytes(data, o):
    """Bytes of the FSE table description at data[o:] (the format's
    normalized-count header: 4 bits of accuracy log, then one variable-width
    value per symbol, 2-bit repeat flags after a zero probability)."""
    pos = [8 * o]

    def read(n):
        v = (int.from_bytes(data[pos[0] >> 3:(pos[0] >> 3) + 5], "little") >> (pos[0] & 7)) & ((1 << n) - 1)
        pos[0] += n
        return v

    remaining = 1 << (read(4) + 5)
    while remaining > 0:
        bits = (remaining + 1).bit_length()
        val = read(bits)
        low = (1 << (bits - 1)) - 1
        thr = (1 << bits) - 1 - (remaining + 1)
        if (val & low) < thr:
            pos[0] -= 1
            val &= low
        elif val > low:
            val -= thr
        remaining -= abs(val - 1)
        assert remaining >= 0, "table description does not add up"
        if val == 1:
            rep = read(2)
            while rep == 3:
                rep = read(2)
    return (pos[0] + 7 >> 3) - o


def seq_blocks(data):
    """[(nseq, 8 * bitstream bytes / nseq, (LL, OF, ML modes))] of the
    compressed blocks with sequences, in plan order: the value the kernel
    compares with K3H_BITS, from the header walk."""
    from zstd_decompressor.batch import frames_index
    _, blocks, st, _ = frames_index(data)
    assert st == 0
    out = []
    for b in blocks:
        if b["type"] != 2:
            continue
        o, end = b["src_offset"], b["src_offset"] + b["block_size"]
        b0 = data[o]
        kind, sf = b0 & 3, (b0 >> 2) & 3
        if kind < 2:                                   # Raw / RLE literals
            hl = (1, 2, 1, 3)[sf]
            v = int.from_bytes(data[o:o + hl], "little")
            size = v >> (3 if hl == 1 else 4)
            o += hl + (size if kind == 0 else 1)
        else:                                          # Compressed / Treeless
            hl, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
            v = int.from_bytes(data[o:o + hl], "little")
            o += hl + ((v >> (4 + bits)) & ((1 << bits) - 1))
        s0 = data[o]
        if s0 == 0:
            continue
        if s0 < 128:
            nseq, o = s0, o + 1
        elif s0 < 255:
            nseq, o = ((s0 - 128) << 8) + data[o + 1], o + 2
        else:
            nseq, o = data[o + 1] + (data[o + 2] << 8) + 0x7F00, o + 3
        m = data[o]
        o += 1
        modes = (m >> 6, (m >> 4) & 3, (m >> 2) & 3)
        for mode in modes:                             # descriptions in the order LL, OF, ML
            o += 1 if mode == 1 else (ncount_bytes(data, o) if mode == 2 else 0)
        assert o <= end
        out.append((nseq, 8 * (end - o) / nseq, modes))
    return out


def waves(data):
    """Per K3Q wave (16 consecutive blocks with sequences): True when every
    block is at or below K3H_BITS (the wave takes the half-window chain)."""
    sb = seq_blocks(data)
    return [all(r <= K3H_BITS for _, r, _ in sb[i:i + CHAINS]) for i in range(0, len(sb), CHAINS)]


def assert_parity(data, what):
    """The oracle's status and bytes from a plan that runs K3 as
    zd_k_sequences_q: ZD_F_SEQ_NO_LATENCY keeps it off K3L, ZD_F_NO_FUSE off
    zd_k_fused (whose chains are seq_chainq whatever the bit rate; plans of
    256-1024 single-block frames fuse by default), and the plan's executors
    are asserted to say so."""
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Plan, run_plan
    ost, oout = oracle.decompress_status(data, False)
    plan = Plan(data, False, _lib.F_SEQ_NO_LATENCY | _lib.F_NO_FUSE)
    try:
        assert not plan.info.executors & _lib.EXEC_FUSED, f"{what}: the plan runs zd_k_fused, not K3Q"
        p, n, keep = _lib.buf(data)
        gst, gout = run_plan(plan, p, n)
    finally:
        plan.close()
    assert gst != OUT_OF_DOMAIN, f"{what}: out of the GPU path's domain (oracle status {ost})"
    assert gst == ost, f"{what}: oracle status {ost}, gpu status {gst}"
    assert gout == oout, f"{what}: output differs (len {len(gout)} vs {len(oout)})"
    return ost


@pytest.fixture(scope="module")
def text_plan():
    return gen.frames(gen.text(300 * 4096, seed=41), 4096, 3)


@pytest.fixture(scope="module")
def binary_plan():
    return gen.frames(gen.binary(8 * (128 << 10), seed=42), 128 << 10, 19)


def test_low_rate_text_takes_half_windows(text_plan):
    """300 x 4 KiB text frames at L3: every wave is under the limit."""
    w = waves(text_plan)
    assert len(w) >= 300 // CHAINS and all(w), f"{w.count(False)} of {len(w)} waves over the limit"
    assert assert_parity(text_plan, "text 4 KiB L3") == 0


def far_matches(count, seed, size=128 << 10, n=200):
    """`count` frames of random bytes with n 8-byte copies from the first
    quarter into the last: few sequences of long literal runs and far offsets,
    the most bits a sequence that libzstd writes here (25-27.5 at L19).  Kept
    are the frames whose walk reports a block over the limit."""
    out = []
    for k in range(4 * count):
        r = random.Random(seed + k)
        d = bytearray(r.randbytes(size))
        for _ in range(n):
            a, b = r.randrange(0, size // 4), r.randrange(size * 3 // 4, size - 16)
            d[b:b + 8] = d[a:a + 8]
        f = libzstd.compress(bytes(d), 19)
        sb = seq_blocks(f)
        if len(sb) == 1 and sb[0][1] > K3H_BITS:
            out.append(f)
            if len(out) == count:
                return out
    raise AssertionError(f"{len(out)} of {count} far-match frames over the limit")


def test_binary_l19_and_blocks_over_the_limit(binary_plan):
    """8 x 128 KiB binary frames at L19 (long offset codes; 21 bits a sequence
    by the walk, so their wave takes the half-window chain like the text),
    and 16 blocks of far matches over the limit, whose wave keeps seq_chainq."""
    sb = seq_blocks(binary_plan)
    assert len(sb) == 8 and waves(binary_plan) == [True], sb   # the half-window chain
    assert assert_parity(binary_plan, "binary 128 KiB L19") == 0
    high = b"".join(far_matches(CHAINS, 600))
    sb = seq_blocks(high)
    assert len(sb) == CHAINS and min(r for _, r, _ in sb) > K3H_BITS, sb
    assert assert_parity(high, "far matches L19") == 0


def test_mixed_wave_keeps_full_windows():
    """Consecutive blocks alternate text (under the limit) and far matches
    (over it), so every wave holds both and takes seq_chainq as a whole."""
    far = far_matches(24, 500)
    parts = []
    for i in range(48):
        parts.append(gen.frames(gen.text(4096, seed=500 + i), 4096, 3) if i % 2 == 0 else far[i // 2])
    data = b"".join(parts)
    sb = seq_blocks(data)
    assert len(sb) == 48
    lo = [r <= K3H_BITS for _, r, _ in sb]
    assert lo == [i % 2 == 0 for i in range(48)], lo
    assert assert_parity(data, "text | far matches alternating") == 0


def test_one_to_nine_sequences():
    """Blocks of 1, 2, ..., 9 sequences (the pair store, the six-step trip and
    the spare pair): tiny inputs (text, and eight random bytes four times over,
    which is one sequence in three bitstream bytes), kept by the count their
    header walk reports when they are under the limit, up to eight frames of
    each count in one plan whose waves all take the half-window chain."""
    keep = {n: [] for n in range(1, 10)}
    r = random.Random(6)
    cands = [r.randbytes(8) * 4 for _ in range(8)]
    cands += [gen.text(24 + (i * 7) % 400, seed=7000 + i) for i in range(600)]
    for c in cands:
        f = libzstd.compress(c, 3)
        sb = seq_blocks(f)
        if len(sb) == 1 and sb[0][0] in keep and sb[0][1] <= K3H_BITS and len(keep[sb[0][0]]) < 8:
            keep[sb[0][0]].append(f)
    missing = [n for n, v in keep.items() if not v]
    assert not missing, f"no block of {missing} sequences under the limit among the inputs"
    frames = [f for n in range(1, 10) for f in keep[n]]
    random.Random(5).shuffle(frames)
    data = b"".join(frames)
    assert sorted({n for n, _, _ in seq_blocks(data)}) == list(range(1, 10))
    assert all(waves(data))
    assert assert_parity(data, "1..9 sequences") == 0


def test_rate_spike_under_a_low_average():
    """Text with an 8 KiB run of binary in the middle: the block's average is
    under the limit, so its wave takes the half-window chain, and the run's
    sequences read more bits each than the text's.  Where a window does not
    cover its step (ymin < 0) the block goes to the exact chain; either way
    the output is the oracle's."""
    t = gen.text(120 << 10, seed=43)
    src = t[:60 << 10] + gen.binary(8 << 10, seed=44) + t[60 << 10:]
    data = libzstd.compress(src, 3)
    sb = seq_blocks(data)
    assert len(sb) == 1 and sb[0][1] <= K3H_BITS, sb
    assert assert_parity(data, "text with a binary run") == 0


def test_table_modes_and_multi_block():
    """Eight-block frames under the limit (Repeat tables), blocks whose match
    lengths share one code (an RLE table beside Predefined ones), and the
    FSE tables of 4 KiB text frames: all four modes run through the
    half-window chain."""
    multi = gen.frames(gen.text(1 << 20, seed=45), 1 << 20, 9)
    r = random.Random(46)
    d = bytearray(r.randbytes(400))
    for _ in range(20):                                # 10 fresh bytes, then 6 from 300 back
        d += r.randbytes(10)
        d += d[-300:-294]
    rle = libzstd.compress(bytes(d), 3)
    text = gen.frames(gen.text(14 * 4096, seed=48), 4096, 3)
    data = multi + rle + text + rle
    sb = seq_blocks(data)
    seen = set()
    for _, _, m in sb:
        seen.update(m)
    assert seen == {0, 1, 2, 3}, f"table modes missing: {[MODES[k] for k in {0, 1, 2, 3} - seen]}"
    assert all(waves(data)), [round(x, 1) for _, x, _ in sb]
    assert assert_parity(data, "table modes") == 0


def test_corruptions(text_plan):
    """Ten seeded 1-3 byte corruptions of the text plan: the oracle's status
    and the output of the frames before the failure."""
    r = random.Random(49)
    for it in range(10):
        d = bytearray(text_plan)
        for _ in range(r.randrange(1, 4)):
            d[r.randrange(len(d))] = r.randrange(256)
        assert_parity(bytes(d), f"corrupt #{it}")
