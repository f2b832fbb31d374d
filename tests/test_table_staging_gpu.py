"""Table staging: the LDS table fills of K3Q (zd_k_sequences_q: a wave fills
its quads' tables together, eight quads a round), K2 (zd_k_huffman: a block's
four lanes copy its pair table) and K4 (k4_body: the block's three symbol
tables) against the oracle, through the C ABI.

Every case asks for the oracle's status, first failing frame and partial
output (test_gpu_parity.assert_parity).  What a case is there for -- a count
of blocks, a table mode, a stream count, a tree depth -- is read back from
its input's block headers, and the test fails when the input misses it.
"""
import random

import pytest

from corpus import gen, libzstd
from oracle import oracle
from test_gpu_parity import _deep_tree_frame, _ncount, assert_parity
from test_k3q_half_windows import seq_blocks

pytestmark = pytest.mark.gpu

CHAINS = 16                         # blocks per K3Q wave
K2_BLOCKS = 8                       # blocks per K2 workgroup
K2_LUT_BITS = 11                    # deeper trees have no pair table
PREDEFINED, RLE, FSE, REPEAT = 0, 1, 2, 3
MAGIC = b"\x28\xb5\x2f\xfd"


def k3q_flags():
    """K3 as zd_k_sequences_q in a plan of any size: off K3L, off zd_k_fused."""
    from zstd_decompressor import _lib
    return _lib.F_SEQ_NO_LATENCY | _lib.F_NO_FUSE


def text_frames(n, seed):
    """n frames of 4 KiB text at level 3, one compressed block with sequences each."""
    data = gen.frames(gen.text(n * 4096, seed=seed), 4096, 3)
    assert len(seq_blocks(data)) == n
    return data


def modes_of(data):
    """The (LL, OF, ML) table modes of the blocks with sequences, in plan order."""
    return [m for _, _, m in seq_blocks(data)]


def lit_blocks(data):
    """[(literals kind, streams)] of the compressed blocks in plan order:
    kind 0 Raw, 1 RLE, 2 Compressed, 3 Treeless; streams 1 or 4 of a Huffman
    block, 0 of the others."""
    from zstd_decompressor.batch import frames_index
    _, blocks, st, _ = frames_index(data)
    assert st == 0
    out = []
    for b in blocks:
        if b["type"] != 2:
            continue
        b0 = data[b["src_offset"]]
        kind, sf = b0 & 3, (b0 >> 2) & 3
        out.append((kind, (1 if sf == 0 else 4) if kind >= 2 else 0))
    return out


def huffman_blocks(data):
    return [x for x in lit_blocks(data) if x[0] >= 2]


def splice(frames, window_exp=13):
    """One frame (no content size, an 8 MiB window) holding the blocks of the
    given frames in order.  A block taken from another frame still decodes:
    its offsets reach its own bytes or, through the repeat offsets it finds,
    bytes before them; the oracle says what comes out."""
    from zstd_decompressor.batch import frames_index
    body = []
    for f in frames:
        _, blocks, st, _ = frames_index(f)
        assert st == 0
        for b in blocks:
            o, n = b["src_offset"], b["block_size"]
            stored = {0: n, 1: 1, 2: n}[b["type"]]
            body.append((b["type"], n, f[o:o + stored]))
    out = [MAGIC, bytes([0x00, window_exp << 3])]
    for i, (t, n, payload) in enumerate(body):
        out.append(((n << 3) | (t << 1) | (i == len(body) - 1)).to_bytes(3, "little"))
        out.append(payload)
    return b"".join(out)


@pytest.fixture(scope="module")
def rle_frame():
    """Match lengths that share one code: an RLE table beside Predefined ones."""
    r = random.Random(46)
    d = bytearray(r.randbytes(400))
    for _ in range(20):                                # 10 fresh bytes, then 6 from 300 back
        d += r.randbytes(10)
        d += d[-300:-294]
    f = libzstd.compress(bytes(d), 3)
    assert any(RLE in m for m in modes_of(f))
    return f


@pytest.fixture(scope="module")
def predefined_frames():
    """Tiny text frames whose one block uses the three Predefined tables."""
    out = []
    for i in range(200):
        f = libzstd.compress(gen.text(24 + (i * 7) % 400, seed=7000 + i), 3)
        if modes_of(f) == [(PREDEFINED, PREDEFINED, PREDEFINED)]:
            out.append(f)
    assert len(out) >= CHAINS + 1, f"{len(out)} all-Predefined frames among the inputs"
    return out


@pytest.fixture(scope="module")
def multi_frames():
    """Two 1 MiB text frames at level 9: eight blocks each, later ones with
    Repeat tables (whose source is an earlier block) and Treeless literals."""
    data = gen.frames(gen.text(2 << 20, seed=45), 1 << 20, 9)
    assert any(REPEAT in m for m in modes_of(data))
    return data


# --------------------------------------------------------------------------
# K3Q
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 15, 16, 17, 33, 65])
def test_k3q_block_counts(n):
    """Plans of n blocks: a full wave, a partial last wave, quads with nothing to do."""
    assert assert_parity(text_frames(n, 300 + n), False, f"{n} text blocks", flags=k3q_flags())[0] == 0


def test_k3q_predefined_tables(predefined_frames):
    """Accuracy logs 6 / 5 / 6: 64-, 32- and 64-entry tables, a wave and one block more."""
    data = b"".join(predefined_frames[:CHAINS + 1])
    assert modes_of(data) == [(PREDEFINED,) * 3] * (CHAINS + 1)
    assert assert_parity(data, False, "Predefined tables", flags=k3q_flags())[0] == 0


def test_k3q_rle_table(rle_frame):
    """An RLE table has one entry (accuracy log 0): the fill's entry-by-entry path,
    alone, and in a wave beside tables of every other size."""
    assert assert_parity(rle_frame, False, "an RLE table alone", flags=k3q_flags())[0] == 0
    data = text_frames(5, 51) + rle_frame + text_frames(3, 52) + rle_frame
    assert sum(RLE in m for m in modes_of(data)) == 2 and len(modes_of(data)) == 10
    assert assert_parity(data, False, "RLE tables among text", flags=k3q_flags())[0] == 0


def test_k3q_repeat_tables(multi_frames):
    """Repeat mode: the quad's tables come from another block's slot."""
    assert assert_parity(multi_frames, False, "1 MiB level-9 frames", flags=k3q_flags())[0] == 0


def al9_offset_frames(count, seed):
    """Frames of one block whose offset table is FSE with accuracy log 9 (512
    states: past K3Q's 256-entry LDS table), LL / ML Predefined, three raw
    literals and one or two sequences from random bits; those the oracle decodes."""
    r = random.Random(seed)
    al = 9
    probs = [(1 << al) - 31] + [1] * 31                # 32 offset codes, most states code 0 (a repeat offset)
    table = _ncount(al, probs)
    assert (table[0] & 15) + 5 == al
    out = []
    for _ in range(4000):
        bitstream = bytes(r.randrange(256) for _ in range(r.randrange(3, 12))) + bytes([r.randrange(1, 256)])
        seqs = bytes([r.choice([1, 2]), 0x20]) + table + bitstream   # OF FSE, LL / ML Predefined
        content = bytes([(3 << 3) | 0]) + b"xyz" + seqs
        hdr = ((len(content) << 3) | (2 << 1) | 1).to_bytes(3, "little")
        f = MAGIC + bytes([0x00, 0x00]) + hdr + content
        if oracle.decompress_status(f, False)[0] == 0:
            out.append(f)
            if len(out) == count:
                return out
    raise AssertionError(f"{len(out)} of {count} AL 9 offset-table frames decode")


def test_k3q_al9_offset_table_in_the_wave():
    """One block with an AL 9 offset table among 15 ordinary ones: the whole
    wave leaves the LDS tables for the exact chain; the next wave keeps them."""
    deep = al9_offset_frames(2, 91)
    for f in deep:
        assert modes_of(f) == [(PREDEFINED, FSE, PREDEFINED)]
        assert_parity(f, False, "AL 9 offset table alone", flags=k3q_flags())
    data = text_frames(7, 61) + deep[0] + text_frames(8, 62) + text_frames(4, 63) + deep[1]
    m = modes_of(data)
    assert len(m) == 21 and m[7] == (PREDEFINED, FSE, PREDEFINED) and m[20] == (PREDEFINED, FSE, PREDEFINED)
    assert assert_parity(data, False, "AL 9 offset table in a wave", flags=k3q_flags())[0] == 0


def test_k3q_corruptions():
    """Ten seeded 1-3 byte corruptions of the 17-block plan."""
    plan = text_frames(17, 317)
    r = random.Random(49)
    for it in range(10):
        d = bytearray(plan)
        for _ in range(r.randrange(1, 4)):
            d[r.randrange(len(d))] = r.randrange(256)
        assert_parity(bytes(d), False, f"corrupt #{it}", flags=k3q_flags())


# --------------------------------------------------------------------------
# K2
# --------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 7, 8, 9])
def test_k2_block_counts(n):
    """Plans of n Huffman blocks: part of a workgroup, a whole one, one block more."""
    data = text_frames(n, 400 + n)
    assert len(huffman_blocks(data)) == n
    assert assert_parity(data, False, f"{n} Huffman blocks")[0] == 0


def test_k2_one_and_four_streams():
    """Single-stream blocks (libzstd writes them under 256 literals) and
    four-stream blocks in one workgroup."""
    small = [libzstd.compress(gen.text(250, seed=500 + i), 3) for i in range(4)]
    big = text_frames(4, 55)
    from zstd_decompressor.batch import frames_index
    spans = [(f["src_offset"], f["src_size"]) for f in frames_index(big)[0]]
    parts = []
    for i in range(4):
        parts += [small[i], big[spans[i][0]:spans[i][0] + spans[i][1]]]
    data = b"".join(parts)
    hb = huffman_blocks(data)
    assert len(hb) == K2_BLOCKS and [s for _, s in hb] == [1, 4] * 4, hb
    assert assert_parity(data, False, "one- and four-stream blocks")[0] == 0


def test_k2_treeless(multi_frames):
    """Treeless blocks: the pair table is an earlier block's slot."""
    assert any(k == 3 for k, _ in lit_blocks(multi_frames))
    assert assert_parity(multi_frames, False, "Treeless literals")[0] == 0


def test_k2_deep_tree_in_the_workgroup():
    """A 12-bit tree among seven blocks with pair tables: its workgroup skips
    the fill and reads every table from HBM; the next workgroup fills."""
    r = random.Random(9)
    deep = None
    for _ in range(400):
        f = _deep_tree_frame(r, r.randrange(20, 200))
        if oracle.decompress_status(f, False)[0] == 0:
            deep = f
            break
    assert deep is not None
    # the block: 3 bytes of literals header, then the tree description (direct weights 12..1)
    _, widths = oracle.huffman_widths(deep[12:12 + 7])
    assert max(widths) == 12 > K2_LUT_BITS
    data = text_frames(3, 71) + deep + text_frames(4, 72) + text_frames(5, 73)
    assert len(huffman_blocks(data)) == K2_BLOCKS + 5
    assert assert_parity(data, False, "a deep tree among pair tables")[0] == 0


# --------------------------------------------------------------------------
# K4
# --------------------------------------------------------------------------
def k4_parity(data, what):
    """Default flags, and once more with every frame on the streaming executor
    (a plan of few frames sends those of many blocks to K4J by itself)."""
    from zstd_decompressor import _lib
    ost, _ = assert_parity(data, False, what)
    assert_parity(data, False, what + " (frame-serial)", flags=_lib.F_FRAME_SERIAL)
    return ost


def test_k4_table_modes_in_consecutive_blocks(multi_frames, rle_frame, predefined_frames):
    """One frame whose consecutive blocks bring FSE, Repeat, RLE and Predefined
    tables: the block's three symbol tables are 512, 64, 32 entries or one."""
    from zstd_decompressor.batch import frames_index
    spans = [(f["src_offset"], f["src_size"]) for f in frames_index(multi_frames)[0]]
    first = multi_frames[spans[0][0]:spans[0][0] + spans[0][1]]
    frame = splice([first, rle_frame, predefined_frames[0], first, predefined_frames[1], rle_frame])
    m = modes_of(frame)
    seen = set()
    for x in m:
        seen.update(x)
    assert seen == {PREDEFINED, RLE, FSE, REPEAT}, seen
    nb = len(modes_of(first))
    assert RLE in m[nb] and m[nb + 1] == (PREDEFINED,) * 3 and REPEAT in m[nb - 1] + m[nb - 2], m
    k4_parity(frame, "table modes in consecutive blocks")
    assert k4_parity(multi_frames, "1 MiB level-9 frames") == 0


def test_k4_first_block_without_sequences(rle_frame):
    """A frame whose first compressed block has zero sequences (Huffman
    literals only), then blocks with sequences: the block skips the tables'
    fill, and the frame ends as the oracle says."""
    r = random.Random(83)
    lits = bytes(r.randrange(64) for _ in range(1500))    # 6 bits a byte: Huffman pays, no 4-byte match
    f0 = libzstd.compress(lits, 3)
    from zstd_decompressor.batch import frames_index
    _, blocks, st, _ = frames_index(f0)
    assert st == 0 and [b["type"] for b in blocks] == [2]
    assert lit_blocks(f0) == [(2, 4)] and seq_blocks(f0) == []   # compressed literals, Number_of_Sequences 0
    frame = splice([f0, text_frames(1, 84), rle_frame])
    assert len(lit_blocks(frame)) == 3 and len(seq_blocks(frame)) == 2
    k4_parity(frame, "first block without sequences")
    k4_parity(text_frames(2, 85) + frame + text_frames(2, 86), "first block without sequences, among frames")
