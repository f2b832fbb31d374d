"""ZD_F_RFC on the GPU: frames libzstd writes (or accepts) that the reference's
decoder fails or corrupts -- D1 the long-form Number_of_Sequences, D2 a
compressed block of 0 sequences, D3 Huffman weight totals, D8 Regenerated_Size
(include/zd.h) -- decode to their source with the flag.

Every test decodes its batch WITHOUT the flag first: at least one chunk of each
class must fail or differ there (else the fixture is stale and the test fails),
and the ordinary frames beside them must be ZD_OK both times.  Ground truth is
the source bytes, cross-checked with libzstd's decoder (corpus/libzstd.py); the
oracle has no RFC mode.

The classes (numpy default_rng(1), one frame each): 4,096 random letters a-z
(D2: Huffman literals, 0 sequences; levels 1 and 3, level 19 finds matches),
4,096 bytes over two symbols (D3: a weight total that is a power of two), 4,096
bytes half of them 0xFF (D3: the rest is truncated `as u8`), and the three-block
frame text / letters / text of 3 x 128 KiB (D2 in the middle block), which has
no 4 KiB form: one block of it decodes without the flag."""
import os
import struct

import numpy as np
import pytest

from corpus import libzstd, zdict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, CORRUPTED_TABLE, CORRUPTED_STREAMS_SIZE = 0, -13, -21
CANARY, FILL = 64, 0xA5
K = 128 << 10


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
def text(rng, n):
    vocab = [bytes(rng.integers(97, 123, int(rng.integers(2, 9)), dtype=np.uint8)) for _ in range(2000)]
    out = bytearray()
    while len(out) < n:
        out += vocab[int(rng.zipf(1.3)) % 2000] + b" "
    return bytes(out[:n])


def letters(rng, n):
    return bytes(rng.integers(97, 123, n, dtype=np.uint8))


def two(rng, n):
    return bytes(rng.integers(0, 2, n, dtype=np.uint8) + 65)


def half(rng, n):
    d = rng.integers(0, 256, n, dtype=np.uint8)
    d[rng.random(n) < 0.5] = 255
    return bytes(d)


def mix(rng, n=K):
    return text(rng, n) + letters(rng, n) + text(rng, n)


def make(fn, *a):
    return fn(np.random.default_rng(1), *a)


class Chunk:
    def __init__(self, cls, frame, want):
        self.cls, self.frame, self.want = cls, frame, want


_cache = {}


def small_classes():
    """letters / two / half at 4,096 bytes and levels 1, 3, 19: the frames and
    their sources, libzstd's decoder agreeing (computed once)."""
    if "small" not in _cache:
        out = []
        for name, fn in (("letters", letters), ("two", two), ("half", half)):
            d = make(fn, 4096)
            for lv in (1, 3, 19):
                f = libzstd.compress(d, lv)
                assert libzstd.decompress_frame(f, len(d)) == d
                out.append(Chunk(name, f, d))
        _cache["small"] = out
    return _cache["small"]


def mix_frames():
    if "mix" not in _cache:
        d = make(mix)
        out = []
        for lv in (1, 3):
            f = libzstd.compress(d, lv)
            assert libzstd.decompress_frame(f, len(d)) == d
            out.append(Chunk("mix", f, d))
        _cache["mix"] = out
    return _cache["mix"]


def plain_text():
    if "text" not in _cache:
        rng = np.random.default_rng(2)
        _cache["text"] = [Chunk("text", libzstd.compress(d, lv), d) for d, lv in ((text(rng, 4096), 1), (text(rng, 20000), 3))]
    return _cache["text"]


# --------------------------------------------------------------------------
# hand-assembled frames
# --------------------------------------------------------------------------
def _nseq(n):
    if n < 128:
        return bytes([n])
    if n < 0x7F00:
        return bytes([128 + (n >> 8), n & 255])
    return bytes([255]) + struct.pack("<H", n - 0x7F00)


def _bits(bits):
    """A backward bitstream holding `bits` (first read first), the marker above them"""
    v = 1
    for b in bits:
        v = (v << 1) | b
    return v.to_bytes(v.bit_length() // 8 + 1, "little").rstrip(b"\0") or b"\x01"


def _raw_block(data, last=False):
    return struct.pack("<I", (len(data) << 3) | int(last))[:3] + data


def _comp_block(lits, nseq, mode=None, tables=b"", bitstream=b"", last=False):
    assert len(lits) < 32
    body = bytes([len(lits) << 3]) + lits + _nseq(nseq)
    if nseq:
        body += bytes([mode]) + tables + bitstream
    return struct.pack("<I", (len(body) << 3) | (2 << 1) | int(last))[:3] + body


def _frame(blocks, total):
    return struct.pack("<I", 0xFD2FB528) + bytes([0xA0]) + struct.pack("<I", total) + b"".join(blocks)


def d1_frame(n):
    """A 16-byte Raw block, then one compressed block: 1 Raw literal, long-form
    Number_of_Sequences n, every table RLE (LL code 0, OF code 2, ML code 0):
    every sequence is ll 0, ml 3, offset_value 4 + two zero bits = offset 1."""
    raw = b"abcdefghijklmnop"
    want = raw + b"p" * (3 * n) + b"Z"
    assert (2 * n) % 8 == 0
    blk = _comp_block(b"Z", n, 0x54, bytes([0, 2, 0]), b"\0" * (2 * n // 8) + b"\x01", last=True)
    return _frame([_raw_block(raw), blk], len(want)), want


def _lz(out, rep, lits, seqs):
    """Sequences (ll, ml, offset_value) over `lits`, RFC 8878 3.1.1.5's repeat offsets"""
    cur = 0
    for ll, ml, ofv in seqs:
        out += lits[cur:cur + ll]
        cur += ll
        if ofv > 3:
            off = ofv - 3
            rep[:] = [off, rep[0], rep[1]]
        else:
            idx = ofv - (1 if ll else 0)
            off = rep[0] - 1 if idx == 3 else rep[idx]
            if idx == 1:
                rep[:] = [off, rep[0], rep[2]]
            elif idx >= 2:
                rep[:] = [off, rep[0], rep[1]]
        for _ in range(ml):
            out.append(out[-off])
    out += lits[cur:]


def d2_repeat_frame():
    """Raw block; block A: RLE tables (LL code 1: ll 1, OF code 1: offset_value 2
    or 3 by one bit, ML code 0: ml 3) and two sequences; block B: 0 sequences,
    Raw literals; block C: mode byte 0xFC, every table Repeat_Mode, two sequences
    whose first takes the third repeat offset -- 1 as A left them, 8 had B reset
    them -- and which has tables only if B left A's in place."""
    raw = b"abcdefghijklmnop"
    out, rep = bytearray(raw), [1, 4, 8]
    a_l, a_s = b"AB-", [(1, 3, 2), (1, 3, 3)]
    b_l = b"0123"
    c_l, c_s = b"XY.", [(1, 3, 3), (1, 3, 2)]
    _lz(out, rep, a_l, a_s)
    assert rep == [8, 4, 1]
    out += b_l
    _lz(out, rep, c_l, c_s)
    blocks = [_raw_block(raw),
              _comp_block(a_l, 2, 0x54, bytes([1, 1, 0]), _bits([s[2] - 2 for s in a_s])),
              _comp_block(b_l, 0),
              _comp_block(c_l, 2, 0xFC, b"", _bits([s[2] - 2 for s in c_s]), last=True)]
    return _frame(blocks, len(out)), bytes(out)


def hand_frames():
    if "hand" not in _cache:
        out = []
        for n in (0x7F00, 32600):
            f, want = d1_frame(n)
            out.append(Chunk("d1", f, want))
        f, want = d2_repeat_frame()
        out.append(Chunk("d2rep", f, want))
        for c in out:
            assert libzstd.decompress_frame(c.frame, len(c.want)) == c.want, c.cls
        _cache["hand"] = out
    return _cache["hand"]


# --------------------------------------------------------------------------
# one batch over chunks
# --------------------------------------------------------------------------
def run(chunks, flags=0, device=False, dictionary=None, prefixes=None):
    """(statuses, lengths, outputs) of one Batch over the chunks; every
    destination is followed by CANARY bytes that must come back intact."""
    import torch
    from zstd_decompressor import Batch
    dev = torch.device("cuda", 0)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    srcs = [up(c.frame) for c in chunks]
    caps = [len(c.want) for c in chunks]
    offs = np.concatenate(([0], np.cumsum([(cp + CANARY + 15) & ~15 for cp in caps]))).tolist()
    dst = torch.full((offs[-1] + 16,), FILL, dtype=torch.uint8, device=dev)
    sp, ss = [t.data_ptr() for t in srcs], [t.numel() for t in srcs]
    dp = [dst.data_ptr() + o for o in offs[:-1]]
    pf = keep = None
    if prefixes is not None:
        keep = [up(p) for p in prefixes]
        pf = ([t.data_ptr() for t in keep], [t.numel() for t in keep])
    s = torch.cuda.current_stream().cuda_stream
    if device:
        arr = [torch.tensor(v, dtype=torch.int64, device=dev) for v in (sp, ss, dp, caps)]
        parr = tuple(torch.tensor(v, dtype=torch.int64, device=dev) for v in pf) if pf else None
        torch.cuda.synchronize()
        b = Batch.from_device(*arr, flags=flags, dictionary=dictionary, stream=s, prefixes=parr)
    else:
        b = Batch(sp, ss, dp, caps, flags=flags, dictionary=dictionary, stream=s, prefixes=pf)
    try:
        assert b.info.device_built == int(device)
        b.decode_async(s)
        st, ln = b.results(s)
    finally:
        b.close()
    host = dst.cpu().numpy()
    outs = []
    for o, cp, n in zip(offs, caps, ln):
        assert n <= cp
        outs.append(bytes(host[o:o + n]))
        assert (host[o + cp:o + cp + CANARY] == FILL).all(), "a canary byte was written"
    return st, ln, outs


def check(chunks, flags=0, **kw):
    """The batch without the flag (each class trips, ordinary text does not),
    then with it (every chunk ZD_OK and equal to its source)."""
    from zstd_decompressor import _lib
    st0, _, out0 = run(chunks, flags, **kw)
    tripped = {}
    for c, s, o in zip(chunks, st0, out0):
        bad = s != OK or o != c.want
        if c.cls == "text":
            assert not bad, "an ordinary frame failed without the flag"
        else:
            tripped[c.cls] = tripped.get(c.cls, False) or bad
    assert tripped and all(tripped.values()), "stale fixture: a class decodes without ZD_F_RFC: %r" % tripped
    st1, ln1, out1 = run(chunks, flags | _lib.F_RFC, **kw)
    for i, c in enumerate(chunks):
        assert st1[i] == OK, (i, c.cls, _lib.status_name(st1[i]))
        assert out1[i] == c.want, (i, c.cls)
    return st0, (st1, ln1, out1)


# --------------------------------------------------------------------------
# 1. the libzstd-written classes in one batch
# --------------------------------------------------------------------------
def test_libzstd_classes_in_one_batch():
    st0, _ = check(small_classes() + mix_frames() + plain_text())
    # the statuses the reference gives (the issue's table)
    by = {}
    for c, s in zip(small_classes() + mix_frames(), st0):
        by.setdefault(c.cls, set()).add(s)
    assert -31 in by["letters"] and by["two"] == {-90} and by["half"] == {-90} and by["mix"] == {-4}


# --------------------------------------------------------------------------
# 2. every executor
# --------------------------------------------------------------------------
@pytest.mark.parametrize("exe", ["frame_serial", "block_parallel", "automatic"])
def test_three_block_frame_on_each_executor(exe):
    from zstd_decompressor import _lib
    check(mix_frames(), {"frame_serial": _lib.F_FRAME_SERIAL, "block_parallel": _lib.F_BLOCK_PARALLEL, "automatic": 0}[exe])


def _plan(data, flags):
    import torch
    from zstd_decompressor.batch import Plan
    plan = Plan(data, flags=flags)
    try:
        d_src = torch.frombuffer(bytearray(data + bytes(64)), dtype=torch.uint8).cuda()
        cap = max(int(plan.info.out_bytes), 1)
        d_dst = torch.zeros(cap + 64, dtype=torch.uint8, device="cuda")
        plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), cap)
        st, total, sts, lens, first = plan.results(d_dst.data_ptr())
        return st, bytes(d_dst[:total].cpu().numpy()), first, plan.info.executors
    finally:
        plan.close()


def test_plan_of_256_frames():
    """The 4 KiB classes in a plan of 256 single-block frames: the fused route
    (zd_k_fused) and, with ZD_F_NO_FUSE, K4F (which a plan of 256-768 small
    frames takes on its own: no environment switch, no child process)."""
    from zstd_decompressor import _lib
    cs = small_classes()
    rng = np.random.default_rng(3)
    filler = [libzstd.compress(text(rng, 4096), 3) for _ in range(8)]
    frames, want = [], []
    rng = np.random.default_rng(4)
    fill_src = [libzstd.decompress_frame(f, 4096) for f in filler]
    for i in range(256):
        if i % 4 == 1:
            c = cs[(i // 4) % len(cs)]
            frames.append(c.frame)
            want.append(c.want)
        else:
            frames.append(filler[i % 8])
            want.append(fill_src[i % 8])
    data = b"".join(frames)
    for flags in (0, _lib.F_NO_FUSE):
        st, out, first, ex = _plan(data, flags)
        assert st != OK and first == 1 and out == want[0], "stale fixture: the plan decodes without ZD_F_RFC"
        st, out, first, ex = _plan(data, flags | _lib.F_RFC)
        assert st == OK, (_lib.status_name(st), first)
        assert out == b"".join(want)
        assert ex & (_lib.EXEC_K4F if flags else _lib.EXEC_FUSED)  # (a plan of 256 frames: K4F behind K3's own launch)


# --------------------------------------------------------------------------
# 3. hand-assembled frames: D1, and Repeat_Mode across a D2 block
# --------------------------------------------------------------------------
@pytest.mark.parametrize("exe", ["streaming", "block_parallel"])
def test_hand_assembled_frames(exe):
    from zstd_decompressor import _lib
    cs = hand_frames()
    st0, _ = check(cs, _lib.F_FRAME_SERIAL if exe == "streaming" else _lib.F_BLOCK_PARALLEL)
    # D1 is silent without the flag: ZD_OK, 127 + (n - 0x7F00) sequences' worth of bytes
    assert st0[0] == OK and st0[1] == OK


def test_d1_lengths_without_the_flag():
    cs = hand_frames()[:2]
    st, ln, _ = run(cs)
    assert (st, ln) == ([OK, OK], [398, 662])


# --------------------------------------------------------------------------
# 4. a dictionary batch and a prefix batch
# --------------------------------------------------------------------------
def _records():
    return [(name, make(fn, 4096)) for name, fn in (("letters", letters), ("two", two), ("half", half))]


def test_dictionary_batch():
    """zd_k_execute_dict and zd_k_dict_tables.  With a trained dictionary libzstd
    writes the two-symbol record's few literals Raw (levels -7 to 19, 4 to 64
    KiB: it keeps the dictionary's tree valid and never describes a new one), so
    that record has no D3 block here and stands beside the text as an ordinary
    frame; letters (D2) and half-0xFF (D3) trip as they do without one."""
    from zstd_decompressor import Dictionary
    rng = np.random.default_rng(5)
    samples = [text(rng, 4096) for _ in range(256)]
    D = zdict.train(samples, 16 << 10)
    assert zdict.dict_id(D) != 0
    chunks = []
    for name, d in _records():
        for lv in (1, 3):
            f = zdict.compress(d, D, lv)
            assert zdict.decompress(f, D, len(d)) == d
            chunks.append(Chunk("text" if name == "two" else name, f, d))
    for d, lv in ((samples[0], 3), (samples[1], 1)):
        chunks.append(Chunk("text", zdict.compress(d, D, lv), d))
    dct = Dictionary(D)
    try:
        check(chunks, dictionary=dct)
    finally:
        dct.close()


def test_prefix_batch():
    rng = np.random.default_rng(6)
    P = text(rng, 16384)
    chunks, prefixes = [], []
    for name, d in _records():
        for lv in (1, 3):
            f = zdict.prefix_compress(d, P, lv)
            assert zdict.prefix_decompress(f, P, len(d)) == d
            chunks.append(Chunk(name, f, d))
            prefixes.append(P)
    for lv in (1, 3):
        d = P[1000:3000] + text(rng, 2000)
        chunks.append(Chunk("text", zdict.prefix_compress(d, P, lv), d))
        prefixes.append(P)
    check(chunks, prefixes=prefixes)


# --------------------------------------------------------------------------
# 5. a device-built batch and the size query
# --------------------------------------------------------------------------
def test_device_built_batch_and_chunk_sizes():
    import torch
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import chunk_sizes
    chunks = small_classes() + mix_frames() + plain_text() + hand_frames()
    host = run(chunks, _lib.F_RFC)
    st0, _, out0 = run(chunks, 0, device=True)
    assert any(s != OK or o != c.want for c, s, o in zip(chunks, st0, out0)), "stale fixture"
    assert run(chunks, _lib.F_RFC, device=True) == host
    assert host[0] == [OK] * len(chunks) and host[2] == [c.want for c in chunks]
    dev = torch.device("cuda", 0)
    srcs = [torch.frombuffer(bytearray(c.frame), dtype=torch.uint8).to(dev) for c in chunks]
    ptrs = torch.tensor([t.data_ptr() for t in srcs], dtype=torch.int64, device=dev)
    sizes = torch.tensor([t.numel() for t in srcs], dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    need, st, exact = (t.cpu().tolist() for t in chunk_sizes(ptrs, sizes, rfc=True))
    assert st == host[0] and need == host[1] and exact == [1] * len(chunks)


# --------------------------------------------------------------------------
# 6. invalid input in RFC mode
# --------------------------------------------------------------------------
def huf_frame(weights, bits, regen):
    """One compressed block of 0 sequences whose literals are one Huffman
    stream: a direct tree description of the listed `weights` (symbols 0, 1, ..;
    the last symbol's weight is implied), the stream holding `bits`, and
    Regenerated_Size `regen`."""
    w = list(weights) + [0] * (len(weights) & 1)
    desc = bytes([127 + len(weights)]) + bytes(w[i] << 4 | w[i + 1] for i in range(0, len(w), 2))
    stream = _bits(bits)
    h = 2 | (regen << 4) | ((len(desc) + len(stream)) << 14)       # Compressed, size format 0: one stream
    body = struct.pack("<I", h)[:3] + desc + stream + b"\0"
    blk = struct.pack("<I", (len(body) << 3) | (2 << 1) | 1)[:3] + body
    return _frame([blk], regen)


def crafted_huffman():
    """(a valid frame and its bytes, a remainder that is no power of two,
    a stream short of Regenerated_Size).  The valid tree lists one weight of 1:
    the total is 1, one bit a code, symbol 0 the code 0 and symbol 1 the code 1
    (D3: a power of two), so the stream's bits are the literals.  Weights 3 and
    1 total 5, and 8 - 5 = 3 is no power of two."""
    bits = [int(b) for b in np.random.default_rng(8).integers(0, 2, 16)]
    good = huf_frame([1], bits, 16)
    assert libzstd.decompress_frame(good, 16) == bytes(bits)
    bad_rest, short = huf_frame([3, 1], bits, 16), huf_frame([1], bits, 17)
    for f in (bad_rest, short):
        with pytest.raises(RuntimeError):
            libzstd.decompress_frame(f, 32)
    return Chunk("huf", good, bytes(bits)), bad_rest, short


def test_invalid_input():
    from zstd_decompressor import _lib
    small = small_classes()
    bases = [small[0], small[3], small[6], hand_frames()[2]]       # letters, two, half at level 1; the D2 repeat frame
    rng = np.random.default_rng(7)
    chunks, mutant = [], []
    for k in range(128):
        for c in bases:
            f = bytearray(c.frame)
            f[int(rng.integers(4, len(f)))] ^= int(rng.integers(1, 256))
            chunks.append(Chunk(c.cls, bytes(f), c.want))
            mutant.append(True)
        c = bases[k % 4]
        chunks.append(c)
        mutant.append(False)
    good, bad_rest, short = crafted_huffman()
    chunks.append(good)
    mutant.append(False)
    crafted = {len(chunks): CORRUPTED_TABLE, len(chunks) + 1: CORRUPTED_STREAMS_SIZE}
    chunks += [Chunk("huf", bad_rest, good.want + b"\0"), Chunk("huf", short, good.want + b"\0")]
    mutant += [True, True]
    st, ln, outs = run(chunks, _lib.F_RFC)
    L = libzstd.lib()
    import ctypes as C
    disagree, both_ok, we_reject = [], 0, 0
    for i, c in enumerate(chunks):
        if not mutant[i]:
            assert st[i] == OK and outs[i] == c.want, i
            continue
        dst = C.create_string_buffer(len(c.want) + 1)
        r = L.ZSTD_decompress(dst, len(c.want), c.frame, len(c.frame))
        z_ok = not L.ZSTD_isError(r)
        if st[i] == OK and z_ok:
            both_ok += 1
            if outs[i] != dst.raw[:r]:
                disagree.append(i)
        elif z_ok:
            we_reject += 1
    print("mutants: %d, both decode: %d, libzstd alone: %d, disagree: %r" % (sum(mutant), both_ok, we_reject, disagree))
    assert not disagree
    for i, code in crafted.items():
        assert st[i] == code, (i, _lib.status_name(st[i]))


# --------------------------------------------------------------------------
# 7. decompress(rfc=True) and the command line
# --------------------------------------------------------------------------
def test_decompress_and_command_line(tmp_path):
    import zstd_decompressor as zd
    from zstd_decompressor import _lib
    from zstd_decompressor.__main__ import main
    for c in (small_classes()[0], small_classes()[3]):            # D2 (letters), D3 (two symbols)
        with pytest.raises(_lib.ZdError):
            zd.decompress(c.frame)
        assert zd.decompress(c.frame, rfc=True) == c.want
        src, out = tmp_path / (c.cls + ".zst"), tmp_path / (c.cls + ".out")
        src.write_bytes(c.frame)
        assert main([str(src), "-o", str(out)]) == 1
        assert main([str(src), "--rfc", "-o", str(out)]) == 0
        assert out.read_bytes() == c.want


# --------------------------------------------------------------------------
# 8. a seekable read (the read option ZD_SEEK_RFC, which reader(flags=F_RFC) sets)
# --------------------------------------------------------------------------
def test_seekable_read():
    from corpus import seekable
    from zstd_decompressor import SeekableArchive, _lib
    rng = np.random.default_rng(9)
    data = text(rng, 4096) + make(letters, 4096) + make(two, 4096) + text(rng, 4096)
    arc = SeekableArchive(seekable.write_seekable(data, 4096, level=1, checksums=True))
    try:
        assert bytes(arc.read(100, 3000).cpu().numpy()) == data[100:3100]          # the text entry alone
        with pytest.raises(_lib.ZdError):
            arc.read(0, len(data))                                                  # D2 and D3 entries
        for vt in (False, True):
            got = arc.read(1000, len(data) - 2000, flags=_lib.F_RFC, verify_table=vt)
            assert bytes(got.cpu().numpy()) == data[1000:len(data) - 1000]
    finally:
        arc.close()
