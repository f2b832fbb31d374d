"""Dictionary and dictionary-set plans and batches on the block-parallel
executor (K4J): with F_DICT_BLOCK_PARALLEL a frame behind a dictionary may run
through zd_k_jsum .. zd_k_jscatter<true, false, true> .. zd_k_jround, the scatter
writing the match bytes whose sources lie in the dictionary's content as final
words -- every frame with a compressed block under F_BLOCK_PARALLEL, none under
F_FRAME_SERIAL, else the frames the ZD_AUTO_* rule names.  Without the flag a
dictionary plan keeps executors == 0.

Expected bytes are always the original record AND corpus.zdict.decompress
(ZSTD_decompress_usingDict) of the same frame with the same dictionary (dchunk()
checks the second when it makes a chunk); a chunk that must fail has the status
the same batch gives without the flag.  The harness (Arena, Chunk, Run's decode /
read_back: ranges inside 0xA5-filled tensors, 64 bytes of slack on every side,
the slack and the sources compared after each decode) and the hand-assembled
frames are tests/test_batch_prefix_gpu.py's and tests/test_batch_prefix_j_gpu.py's,
and every batch case runs through both creation calls, which must agree."""
import functools

import numpy as np
import pytest

from corpus import gen, libzstd, zdict
from test_batch_auto_gpu import BLOCK, FC, FEW, MIN, compressed_blocks, large
from test_batch_prefix_gpu import Arena, Chunk, Run, big_pair, rnd, trained
from test_batch_prefix_j_gpu import PERIOD_CASES, hand_period_frame

pytestmark = pytest.mark.gpu


def lib():
    from zstd_decompressor import _lib
    return _lib


def DJ():
    return lib().F_DICT_BLOCK_PARALLEL


def forced():
    return lib().F_DICT_BLOCK_PARALLEL | lib().F_BLOCK_PARALLEL


# ---------------------------------------------------------------------------
# the harness: test_batch_prefix_gpu.Run with a dictionary in the prefixes' place
# ---------------------------------------------------------------------------
class DRun(Run):
    def __init__(self, chunks, device, flags=0, dictionary=None):
        import torch
        from zstd_decompressor import Batch
        self.chunks, n = chunks, len(chunks)
        self.P, self.S, self.D = Arena(), Arena(), Arena()          # (P stays empty: read_back compares it too)
        so = [self.S.place(c.frame, (3 * i) % 16) for i, c in enumerate(chunks)]
        order = np.random.default_rng(n).permutation(n)
        do = [None] * n
        for i in order:
            do[i] = self.D.place(None, chunks[i].dalign, size=chunks[i].cap)
        self.P.upload()
        sb, db = self.S.upload(), self.D.upload()
        self.do = do
        sp, ss = [sb + o for o in so], [len(c.frame) for c in chunks]
        dp, dc = [db + o for o in do], [c.cap for c in chunks]
        if device:
            dev = torch.device("cuda", 0)
            arr = [torch.tensor(v, dtype=torch.int64, device=dev) for v in (sp, ss, dp, dc)]
            torch.cuda.synchronize()
            self.b = Batch.from_device(*arr, flags=flags, dictionary=dictionary)
        else:
            self.b = Batch(sp, ss, dp, dc, flags=flags, dictionary=dictionary)
        assert self.b.info.device_built == int(device)


def both_d(chunks, dictionary, flags, want_j):
    """The chunks through both creation calls: (statuses, lengths, outputs), the
    two agreeing on all of it and on k4j_chunks == want_j."""
    res = []
    for device in (False, True):
        r = DRun(chunks, device, flags, dictionary)
        try:
            st, ln = r.decode()
            assert r.b.info.k4j_chunks == want_j, (device, r.b.info.k4j_chunks)
            assert bool(r.b.info.executors & lib().EXEC_K4J) == (want_j > 0)
            assert r.b.info.executors & ~lib().EXEC_K4J == 0       # (no fused kernel, no K4F behind a dictionary)
            res.append((st, ln, r.out))
        finally:
            r.close()
    assert res[0] == res[1], "the host-array and the device-array batch differ"
    return res[0]


def expect_records(chunks, st, ln, out, failing=()):
    for i, c in enumerate(chunks):
        if i in failing:
            assert st[i] != 0 and ln[i] == 0, (i, st[i])
        else:
            assert st[i] == 0 and ln[i] == len(c.record) and out[i] == c.record, (i, st[i])


def dchunk(record, dictionary, level=3, checksum=False, **kw):
    """A chunk: `record` compressed with the dictionary's bytes; libzstd with them gives the record back."""
    frame = zdict.compress(record, dictionary, level, checksum)
    assert zdict.decompress(frame, dictionary, len(record)) == record
    return Chunk(frame, None, record=record, **kw)


def plan_run(data, dictionary, flags):
    """One plan over `data` decoded once: (status, per-frame statuses, per-frame
    lengths, first error frame, the output's bytes, executors)."""
    import torch
    from zstd_decompressor import Plan
    dev = torch.device("cuda", 0)
    plan = Plan(data, False, flags, dictionary=dictionary)
    try:
        d_src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
        d_src[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        cap = max(int(plan.info.out_bytes), 1)
        d_dst = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device=dev)
        s = torch.cuda.current_stream(dev).cuda_stream
        plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), cap, s)
        st, total, sts, lens, first = plan.results(d_dst.data_ptr(), s)
        host = d_dst.cpu().numpy()
        assert (host[cap:] == 0xA5).all(), "a byte past the plan's output was written"
        return st, sts, lens, first, bytes(host[:total]), plan.info.executors
    finally:
        plan.close()


@functools.lru_cache(maxsize=None)
def records():
    """Five records of 3-4 KB of the trained dictionary's kind of text, and one of 300 KiB (three blocks)."""
    text = gen.text(5 * 4096, seed=0xD1C7)
    small = [text[i * 4096:i * 4096 + 3000 + 200 * i] for i in range(5)]
    return small, big_pair()[1]


@functools.lru_cache(maxsize=None)
def parity_chunks(checksum=False):
    small, big = records()
    chunks = [dchunk(r, trained(), 3, checksum, dalign=(5 * i + 1) % 16) for i, r in enumerate(small)]
    chunks.append(dchunk(big, trained(), 3, checksum, dalign=7))
    assert compressed_blocks(chunks[5].frame) == 3 and all(compressed_blocks(c.frame) == 1 for c in chunks[:5])
    return chunks


# ---------------------------------------------------------------------------
# 1. parity (fails without the feature: k4j_chunks stays 0)
# ---------------------------------------------------------------------------
def test_parity_batch_plan_and_decompress():
    from zstd_decompressor import Dictionary, decompress
    chunks = parity_chunks()
    d = Dictionary(trained())
    try:
        st, ln, out = both_d(chunks, d, forced(), 6)
        expect_records(chunks, st, ln, out)
        # the same frames as one plan, and through decompress()
        data = b"".join(c.frame for c in chunks)
        want = b"".join(c.record for c in chunks)
        st, sts, lens, first, got, ex = plan_run(data, d, forced())
        assert ex & lib().EXEC_K4J and ex & ~lib().EXEC_K4J == 0
        assert (st, first, sts) == (0, -1, [0] * 6) and lens == [len(c.record) for c in chunks] and got == want
        assert decompress(data, dictionary=d, flags=forced()) == want
        # without the flag: the route the existing suite pins
        st, sts, lens, first, got, ex = plan_run(data, d, lib().F_BLOCK_PARALLEL)
        assert ex == 0 and st == 0 and got == want
    finally:
        d.close()


# ---------------------------------------------------------------------------
# 2. the dictionary boundary
# ---------------------------------------------------------------------------
RAW_N = 5000


@functools.lru_cache(maxsize=None)
def raw5000():
    d = rnd(0xD1C75000, RAW_N)
    assert zdict.dict_id(d) == 0
    return d


def hand_chunk(lits, off, ml, dalign, ok=True):
    """hand_period_frame behind the raw-content dictionary: one sequence whose
    match starts off - len(lits) bytes before the frame's first byte."""
    D = raw5000()
    frame = hand_period_frame(lits, off, ml)
    n = len(lits) + ml
    if not ok:
        return Chunk(frame, None, cap=n, record=None, dalign=dalign)
    hist = bytearray(D + lits)
    for _ in range(ml):
        hist.append(hist[len(hist) - off])                     # the reference's byte-by-byte push
    want = bytes(hist[RAW_N:])
    assert zdict.decompress(frame, D, n) == want and len(want) == n      # libzstd accepts the frame
    return Chunk(frame, None, record=want, dalign=dalign)


def test_the_dictionary_boundary():
    from zstd_decompressor import Dictionary
    chunks = []
    k = 0
    # the match starts at the dictionary's first byte; at its last byte (period ll + 1 into the frame)
    for ll in (0, 5, 14):
        for ml in (3, 40, 66):
            for a in range(0, 16, 5):
                chunks.append(hand_chunk(rnd(0xB0D0 + k, ll), RAW_N + ll, ml, (a + k) % 16))
                chunks.append(hand_chunk(rnd(0xB0E0 + k, ll), ll + 1, ml, (a + k + 2) % 16))
            k += 1
    # periods 1, 2, 3, 15, 16, 17 that start in the dictionary and run into the frame
    for k, (o, ll) in enumerate(PERIOD_CASES):
        for a in (0, 5, 11, 15):
            chunks.append(hand_chunk(rnd(0xB0F0 + k, ll), o, 40 if o < 15 else 66, (3 * a + k) % 16))
    assert {c.dalign for c in chunks} == set(range(16))
    d = Dictionary(raw5000())
    try:
        st, ln, out = both_d(chunks, d, forced(), len(chunks))
        expect_records(chunks, st, ln, out)
        # an offset one past content plus position: the streaming executor's status, for that chunk alone
        bad = [chunks[0], hand_chunk(rnd(0xB100, 5), RAW_N + 5 + 1, 40, 3, ok=False), chunks[1],
               hand_chunk(b"", RAW_N + 1, 40, 9, ok=False), chunks[2]]
        want = both_d(bad, d, 0, 0)
        got = both_d(bad, d, forced(), 5)
        assert got == want
        assert [got[0][i] for i in (1, 3)] == [lib().IMPOSSIBLE_VALUE] * 2
        expect_records(bad, *got, failing=(1, 3))
    finally:
        d.close()


# ---------------------------------------------------------------------------
# 3. the dictionary's entropy state
# ---------------------------------------------------------------------------
def first_block_sections(frame):
    """(literals type, Number_of_Sequences, (LL, OF, ML) modes or None) of the frame's first block, a compressed one
    (RFC 8878 3.1.1.3.1.1, 3.1.1.3.2.1)."""
    from zstd_decompressor.batch import frames_index
    _, blocks, st, _ = frames_index(frame)
    assert st == 0 and blocks[0]["type"] == 2
    o, size = blocks[0]["src_offset"], blocks[0]["block_size"]
    assert int.from_bytes(frame[o - 3:o], "little") >> 3 == size          # (src_offset is the block's content)
    body = frame[o:o + size]
    lt, sf = body[0] & 3, (body[0] >> 2) & 3
    if lt < 2:
        hdr = (1, 2, 1, 3)[sf]
        regen = int.from_bytes(body[:hdr], "little") >> (3 if hdr == 1 else 4)
        p = hdr + (regen if lt == 0 else 1)
    else:
        hdr = (3, 3, 4, 5)[sf]
        v = int.from_bytes(body[:hdr], "little")
        comp = ((v >> 14) & 0x3FF, (v >> 14) & 0x3FF, (v >> 18) & 0x3FFF, (v >> 22) & 0x3FFFF)[sf]
        p = hdr + comp
    n0 = body[p]
    if n0 == 0:
        return lt, 0, None
    nseq, p = (n0, p + 1) if n0 < 128 else (((n0 - 128) << 8) + body[p + 1], p + 2) if n0 < 255 else \
        (body[p + 1] + (body[p + 2] << 8) + 0x7F00, p + 3)
    m = body[p]
    return lt, nseq, ((m >> 6) & 3, (m >> 4) & 3, (m >> 2) & 3)


def test_frames_that_start_from_the_dictionarys_tables():
    from zstd_decompressor import Dictionary
    text = gen.text(96 * 2048, seed=0xE27A)
    chunks = []
    for i in range(96):
        rec = text[i * 2048:i * 2048 + 300 + 18 * i]
        c = dchunk(rec, trained(), (1, 3, 19)[i % 3], dalign=i % 16)
        lt, nseq, modes = first_block_sections(c.frame)
        # treeless literals (the dictionary's Huffman tree) or a Repeat_Mode table (the dictionary's FSE tables)
        if lt == 3 or (modes and 3 in modes):
            chunks.append(c)
    assert len(chunks) >= 8, len(chunks)
    chunks = chunks[:48]
    d = Dictionary(trained())
    try:
        st, ln, out = both_d(chunks, d, forced(), len(chunks))
        expect_records(chunks, st, ln, out)
    finally:
        d.close()


# ---------------------------------------------------------------------------
# 4. sets
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trained_other(seed):
    text = gen.text(256 * 4096, seed=seed)
    d = zdict.train([text[i:i + 4096] for i in range(0, len(text), 4096)], 16 << 10)
    assert zdict.dict_id(d) not in (0, zdict.dict_id(trained()))
    return d


def test_sets_each_frame_its_own_dictionary():
    from zstd_decompressor import Dictionary, DictionarySet
    A, B, R, X = trained(), trained_other(0x5E7B), raw5000(), trained_other(0x5E7C)
    assert len({zdict.dict_id(v) for v in (A, B, X)}) == 3
    text = gen.text(12 * 4096, seed=0x5E7D)
    rec = lambda i: text[i * 4096:i * 4096 + 2500 + 100 * i]
    raw_rec = lambda i: R[100 * i:100 * i + 900] + rec(i)[:700] + R[-600:]
    _, big = records()
    chunks = [dchunk(rec(0), A, dalign=1), dchunk(rec(1), B, dalign=6), dchunk(raw_rec(2), R, dalign=11),
              dchunk(big, B, dalign=3), dchunk(rec(3), A, dalign=15), dchunk(rec(4), X, dalign=2),
              dchunk(raw_rec(5), R, dalign=8), dchunk(rec(6), B, dalign=13)]
    assert all(compressed_blocks(c.frame) >= 1 for c in chunks)
    ds = [Dictionary(A), Dictionary(B), Dictionary(R)]
    s = DictionarySet(ds, fallback=2)
    try:
        want = both_d(chunks, s, 0, 0)
        got = both_d(chunks, s, forced(), 7)               # every decodable frame, in the one launch
        assert got == want and got[0][5] == lib().DICT_MISMATCH
        expect_records(chunks, *got, failing=(5,))
    finally:
        s.close()
    # no fallback: a frame without an ID decodes without a dictionary, on K4J too
    plain = Chunk(libzstd.compress(rec(7), 3), None, record=rec(7), dalign=5)
    chunks = [chunks[0], plain, chunks[1], chunks[5], chunks[3]]
    s = DictionarySet(ds[:2], fallback=-1)
    try:
        want = both_d(chunks, s, 0, 0)
        got = both_d(chunks, s, forced(), 4)
        assert got == want and got[0][3] == lib().DICT_MISMATCH
        expect_records(chunks, *got, failing=(3,))
    finally:
        s.close()
        for d in ds:
            d.close()


# ---------------------------------------------------------------------------
# 5. the rule
# ---------------------------------------------------------------------------
def test_the_rule_without_a_forcing_flag():
    from zstd_decompressor import Dictionary
    L = lib()
    assert (FEW, MIN, FC) == (2, 4, 64)               # (the shapes below are the rule's crossings at these values)
    six = parity_chunks()
    small, _ = records()
    many = [six[i % 5] for i in range(FC)]
    four = dchunk(gen.text(4 * BLOCK, seed=0x4B10), trained(), dalign=9)
    assert compressed_blocks(four.frame) == 4
    d = Dictionary(trained())
    try:
        st, ln, out = both_d(six, d, DJ(), 1)                              # 6 chunks, one 3-block frame
        expect_records(six, st, ln, out)
        c65 = many + [six[5]]
        expect_records(c65, *both_d(c65, d, DJ(), 0))                      # 65 chunks: 3 blocks are below the minimum
        c65 = many + [four]
        expect_records(c65, *both_d(c65, d, DJ(), 1))                      # ... 4 blocks are not
        expect_records(c65, *both_d(c65, d, DJ() | L.F_FRAME_SERIAL, 0))
        expect_records(six, *both_d(six, d, forced() | L.F_FRAME_SERIAL, 0))
        # without the flag: executors == 0 whatever the other flags
        for flags in (0, L.F_BLOCK_PARALLEL, L.F_AUTO_EXECUTOR, L.F_BLOCK_PARALLEL | L.F_AUTO_EXECUTOR):
            expect_records(six, *both_d(six, d, flags, 0))
    finally:
        d.close()


# ---------------------------------------------------------------------------
# 6. failure
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def corrupt_second_block():
    """The 300 KiB frame with the first FSE table description of its second
    block damaged (an Accuracy_Log past the format's limit): the walk keeps the
    block, K1 fails it."""
    from zstd_decompressor.batch import frames_index
    c = parity_chunks()[5]
    _, blocks, st, _ = frames_index(c.frame)
    assert st == 0 and [b["type"] for b in blocks] == [2, 2, 2]
    f = bytearray(c.frame)
    o = blocks[1]["src_offset"]
    body = bytes(f[o:o + blocks[1]["block_size"]])
    # (the same walk as first_block_sections, over the second block)
    lt, sf = body[0] & 3, (body[0] >> 2) & 3
    assert lt == 2
    hdr = (3, 3, 4, 5)[sf]
    v = int.from_bytes(body[:hdr], "little")
    p = hdr + ((v >> 14) & 0x3FF, (v >> 14) & 0x3FF, (v >> 18) & 0x3FFF, (v >> 22) & 0x3FFFF)[sf]
    n0 = body[p]
    assert n0 >= 128                                           # many sequences: a two- or three-byte count
    p += 2 if n0 < 255 else 3
    assert (body[p] >> 6) & 3 == 2                             # Literals_Length_Mode: FSE_Compressed_Mode
    f[o + p + 1] |= 0x0F                                       # Accuracy_Log 20
    return Chunk(bytes(f), None, cap=len(c.record), record=None, dalign=4)


def test_failing_frames_fail_alone_in_a_batch_and_end_a_plan():
    from zstd_decompressor import Dictionary
    L = lib()
    six = parity_chunks()
    truncated = Chunk(six[2].frame[:-3], None, cap=len(six[2].record), record=None, dalign=12)
    chunks = [six[0], truncated, six[1], corrupt_second_block(), six[5], six[3]]
    d = Dictionary(trained())
    try:
        want = both_d(chunks, d, 0, 0)
        got = both_d(chunks, d, forced(), 5)               # (the truncated frame fails to index: never a K4J frame)
        assert got == want
        expect_records(chunks, *got, failing=(1, 3))
        # a plan: the failing frame ends the output
        for frames in ([six[0].frame, corrupt_second_block().frame, six[1].frame, six[5].frame],
                       [six[0].frame, six[5].frame, truncated.frame]):
            data = b"".join(frames)
            plain = plan_run(data, d, 0)
            flagged = plan_run(data, d, forced())
            assert plain[5] == 0 and flagged[5] & L.EXEC_K4J
            assert flagged[:5] == plain[:5]
            st, sts, lens, first, out, _ = flagged
            assert st != 0 and first >= 1 and sts[first] != 0 and sts[:first] == [0] * first
            assert all(s == L.NOT_DECODED for s in sts[first + 1:])
            assert out.startswith(six[0].record) and len(out) == sum(lens[:first])
    finally:
        d.close()


# ---------------------------------------------------------------------------
# 7. the redo path: a frame whose pointer jumping does not converge
# ---------------------------------------------------------------------------
def test_redo_on_the_streaming_executor_with_the_dictionary_or_the_set():
    import torch
    from zstd_decompressor import Dictionary, DictionarySet
    from zstd_decompressor.batch import _read_u64
    L = lib()
    six = parity_chunks()
    deep = dchunk(large(0xD1C7A5), trained(), dalign=10)
    assert compressed_blocks(deep.frame) == 3
    chunks = [six[0], deep, six[1]]
    d = Dictionary(trained())
    other = Dictionary(trained_other(0x5E7B))
    s = DictionarySet([other, d], fallback=-1)
    try:
        for dictionary in (d, s):
            for device in (False, True):
                r = DRun(chunks, device, forced() | L.F_J_ONE_ROUND, dictionary)
                try:
                    r.b.decode_async(torch.cuda.current_stream().cuda_stream)
                    torch.cuda.synchronize()
                    # the launch's own statuses, before results() decodes anything again
                    words = _read_u64(r.b.device_results()[0], 2)
                    dev_st = np.array(words, dtype=np.uint64).view(np.int32)[:3]
                    assert dev_st[1] == L.OUT_OF_DOMAIN, dev_st
                    r.status, r.length = r.b.results(torch.cuda.current_stream().cuda_stream)
                    r.read_back()
                    assert r.status == [0] * 3, r.status
                    assert all(o == c.record for o, c in zip(r.out, chunks))
                finally:
                    r.close()
        # a plan: zd_plan_decompress's re-plan
        from zstd_decompressor.batch import decompress_status
        st, out = decompress_status(deep.frame, flags=forced() | L.F_J_ONE_ROUND, dictionary=d)
        assert st == 0 and out == deep.record
    finally:
        s.close()
        other.close()
        d.close()


# ---------------------------------------------------------------------------
# 8. verified checksums; 9. two launches
# ---------------------------------------------------------------------------
def test_verify_checksum_and_a_second_launch():
    from zstd_decompressor import Dictionary
    L = lib()
    chunks = list(parity_chunks(True))
    good = chunks[5]
    f = bytearray(good.frame)
    f[-1] ^= 0x5A                                              # the stored Content_Checksum
    chunks.append(Chunk(bytes(f), None, cap=len(good.record), record=None, dalign=14))
    d = Dictionary(trained())
    try:
        for device in (False, True):
            r = DRun(chunks, device, forced() | L.F_VERIFY_CHECKSUM, d)
            try:
                first = r.decode()
                assert r.b.info.k4j_chunks == 7
                assert first[0][6] == L.CHECKSUM_WRONG and first[1][6] == 0
                expect_records(chunks, first[0], first[1], r.out, failing=(6,))
                out1 = list(r.out)
                r.D.t.fill_(0xA5)
                again = r.decode()                             # the same batch launched once more
                assert again == first and r.out == out1
            finally:
                r.close()
    finally:
        d.close()


# ---------------------------------------------------------------------------
# 10. the other dictionary paths
# ---------------------------------------------------------------------------
def test_packed_batch_multi_frame_batch_and_rfc():
    import torch
    from zstd_decompressor import Batch, Dictionary
    from zstd_decompressor.batch import _read_u64
    from zstd_decompressor.multi import MultiFrameBatch
    L = lib()
    dev = torch.device("cuda", 0)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    six = parity_chunks()
    d = Dictionary(trained())
    try:
        # a packed batch lays its own outputs out
        srcs = [up(c.frame) for c in six]
        b = Batch.packed([t.data_ptr() for t in srcs], [t.numel() for t in srcs], flags=forced(), dictionary=d)
        try:
            assert b.info.k4j_chunks == 6 and b.info.executors & L.EXEC_K4J
            out = torch.full((b.out_bytes,), 0xA5, dtype=torch.uint8, device=dev)
            b.bind_output(out)
            s = torch.cuda.current_stream().cuda_stream
            b.decode_async(s)
            st, ln = b.results(s)
            offs = _read_u64(b.output_layout()[0], 6)
            host = out.cpu().numpy()
            assert st == [0] * 6
            assert all(bytes(host[offs[i]:offs[i] + ln[i]]) == six[i].record for i in range(6))
        finally:
            b.close()
        # a multi-frame batch hands the flag to its inner batch
        groups = [(0, 5), (1, 2), (3,), (5, 4)]
        srcs = [up(b"".join(six[i].frame for i in g)) for g in groups]
        want = [b"".join(six[i].record for i in g) for g in groups]
        dsts = [torch.full((len(w) + 64,), 0xA5, dtype=torch.uint8, device=dev) for w in want]
        m = MultiFrameBatch([t.data_ptr() for t in srcs], [t.numel() for t in srcs], [t.data_ptr() for t in dsts],
                            [len(w) for w in want], flags=forced(), dictionary=d)
        try:
            assert m.info.batch.k4j_chunks == 7 and m.info.batch.executors & L.EXEC_K4J
            m.decode_async()
            st, ln = m.results()
            assert st == [0] * 4 and ln == [len(w) for w in want]
            for t, w in zip(dsts, want):
                host = t.cpu().numpy()
                assert bytes(host[:len(w)]) == w and (host[len(w):] == 0xA5).all()
        finally:
            m.close()
    finally:
        d.close()
    # F_RFC with the flag: a compressed block without sequences (D2) behind a dictionary, on K4J
    R = Dictionary(raw5000())
    try:
        # (random letters: Huffman literals, and with this seed libzstd finds no match, which the assert below holds)
        rec = bytes(np.random.default_rng(0x2FF).integers(97, 123, 4096, dtype=np.uint8))
        c = dchunk(rec, raw5000(), 3, dalign=5)
        lt, nseq, _ = first_block_sections(c.frame)
        assert lt == 2 and nseq == 0
        chunks = [c, hand_chunk(b"abc", RAW_N + 3, 20, 2)]
        st, ln, out = both_d(chunks, R, forced() | L.F_RFC, 2)
        expect_records(chunks, st, ln, out)
        want = both_d(chunks, R, 0, 0)                       # (the reference's decoder fails such a block)
        assert want[0][0] != 0 and both_d(chunks, R, forced(), 2)[0] == want[0]
    finally:
        R.close()


def test_command_line_sets_the_flag_from_2_mib(tmp_path, monkeypatch):
    """-D with a frame whose Frame_Content_Size is at least 2 MiB: the plan gets
    the flag and the output is the record; a smaller frame's plan does not."""
    from zstd_decompressor import __main__ as cli
    seen = []

    class Recorder(cli.Plan):
        def __init__(self, data, print_skippable=False, flags=0, dictionary=None):
            super().__init__(data, print_skippable, flags, dictionary=dictionary)
            seen.append((flags, self.info.executors))
    monkeypatch.setattr(cli, "Plan", Recorder)
    (tmp_path / "dict").write_bytes(trained())
    small, _ = records()
    ascii_text = lambda t: bytes(np.where(np.frombuffer(t, dtype=np.uint8) < 128, np.frombuffer(t, dtype=np.uint8), 32)
                                 .astype(np.uint8))                  # (the command line writes UTF-8 text only)
    for name, rec, flagged in (("big", ascii_text(gen.text(2 << 20, seed=0xC11)), True),
                               ("small", ascii_text(small[0]), False)):
        (tmp_path / name).write_bytes(zdict.compress(rec, trained(), 3))
        out = tmp_path / (name + ".out")
        assert cli.main([str(tmp_path / name), "-D", str(tmp_path / "dict"), "-o", str(out)]) == 0
        assert out.read_bytes() == rec
        flags, executors = seen.pop()
        assert bool(flags & DJ()) == flagged and bool(executors & lib().EXEC_K4J) == flagged
