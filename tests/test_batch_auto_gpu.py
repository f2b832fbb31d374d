"""Prefix and chain batches with F_AUTO_EXECUTOR: each chunk's frame is routed
on its own -- to K4J when it has at least ZD_AUTO_MIN_BLOCKS compressed blocks
(ZD_AUTO_MIN_BLOCKS_FEW in a batch whose width is at most ZD_AUTO_FEW_CHUNKS),
else to the batch's streaming executor -- and `info.k4j_chunks` counts the former.
The four constants are read from include/zd.h, so moving one moves the shapes.

Expected bytes are always the original record AND libzstd's own decode with the
prefix (delta() / check_links_on_the_cpu check the second when a chunk is made);
a chunk that must fail has the status the same batch gives without the flag.  A
frame of exactly k compressed blocks is a text delta of k x 128 KiB, and k is
asserted with the package's own frame parser before any GPU run.  Which chunk
went to K4J is seen with F_J_ONE_ROUND: the `deep` frames hold match chains
that one hop cannot resolve, so on K4J -- and only there -- the launch leaves them
ZD_E_OUT_OF_DOMAIN until results() decodes them again.

The harnesses (ranges inside 0xA5-filled tensors, 64 bytes of slack on every
side, slack, sources and prefixes compared after each decode) are
tests/test_batch_prefix_gpu.py's and tests/test_batch_chain_gpu.py's; every case
runs through both creation calls, which must agree."""
import functools
import os
import re

import numpy as np
import pytest

import test_batch_chain_gpu as C
import test_batch_prefix_gpu as P
from corpus import gen, libzstd, zdict
from test_batch_chain_gpu import NOT_DECODED, check_links_on_the_cpu, edit, verify
from test_batch_prefix_gpu import FILL, PAGE, big_pair, needs_its_prefix, page_chunks, pages, rnd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "zd.h")).read()
BLOCK = 128 << 10


def const(name):
    return int(re.search(r"^#define\s+%s\s+(\d+)u?\b" % name, HEADER, re.M).group(1))


MIN, FEW = const("ZD_AUTO_MIN_BLOCKS"), const("ZD_AUTO_MIN_BLOCKS_FEW")
FC, MC = const("ZD_AUTO_FEW_CHUNKS"), const("ZD_AUTO_MAX_CANDIDATES")


def lib():
    from zstd_decompressor import _lib
    return _lib


def auto():
    return lib().F_AUTO_EXECUTOR


def compressed_blocks(frame):
    from zstd_decompressor.batch import frames_index
    if not frame:
        return 0
    _, blocks, st, _ = frames_index(frame)
    assert st == 0
    return sum(b["type"] == 2 for b in blocks)


def min_blocks(width):
    return FEW if width <= FC else MIN


def on_j(frames, width):
    """The chunks rule (a) sends to K4J in a batch of that width (good frames, small prefixes)."""
    got = [i for i, f in enumerate(frames) if compressed_blocks(f) >= min_blocks(width)]
    assert len(got) <= MC
    return got


def deep_chain(seed):
    """Bytes that are in no prefix, eight times over with separators of growing
    lengths: each copy's words point at the copy before it, whose words are
    pending themselves -- more than one hop of pointer jumping."""
    X = rnd(seed, 1500)
    return b"".join(X + rnd(seed + 1 + k, 3 + 2 * k) for k in range(8))


@functools.lru_cache(maxsize=None)
def k_blocks(k, deep=True):
    """(old, new): text of k x 128 KiB and the same with 1 % of its bytes edited
    (and a deep chain spliced in): the delta has exactly k compressed blocks."""
    n = k * BLOCK
    old = gen.text(n, seed=0xA070 + k)
    new = bytearray(edit(old, 0xA071 + k))
    if deep:
        d = deep_chain(0xA0D0 + 16 * k)
        new[1000:1000 + len(d)] = d
    return old, bytes(new)


def k_delta(k, checksum=False, **kw):
    old, new = k_blocks(k)
    c = P.delta(new, old, 3, checksum, **kw)
    assert compressed_blocks(c.frame) == k, (k, compressed_blocks(c.frame))
    return c


def raw_only_chunk():
    rec = rnd(0xA0F0, 2000)
    c = P.Chunk(libzstd.compress(rec, 1), rnd(0xA0F1, 5000), record=rec, palign=3)
    assert compressed_blocks(c.frame) == 0
    return c


def device_arrays(b, n):
    from zstd_decompressor.batch import _read_u64
    d_st, d_ln = b.device_results()
    st = np.array(_read_u64(d_st, (n + 1) // 2), dtype=np.uint64).view(np.int32)[:n]
    return [int(v) for v in st], [int(v) for v in _read_u64(d_ln, n)]


def both_prefix(chunks, flags, want_j):
    """The chunks through both prefix creation calls with `flags`: (statuses,
    lengths, outputs), the two agreeing; k4j_chunks and executors as `want_j` says."""
    res = []
    for device in (False, True):
        r = P.Run(chunks, device, flags=flags)
        try:
            st, ln = r.decode()
            assert r.b.info.k4j_chunks == want_j, (device, r.b.info.k4j_chunks, want_j)
            assert r.b.info.executors == (lib().EXEC_K4J if want_j else 0), r.b.info.executors
            assert r.b.info.prefix_bytes_total == r.prefix_total
            res.append((st, ln, r.out))
        finally:
            r.close()
    assert res[0] == res[1], "the host-array and the device-array batch differ"
    return res[0]


def expect_records(chunks, st, ln, out):
    assert st == [0] * len(chunks), [(i, s) for i, s in enumerate(st) if s]
    for i, c in enumerate(chunks):
        assert ln[i] == len(c.record) and out[i] == c.record, i


# ---------------------------------------------------------------------------
# 1. a mixed prefix batch above the few limit
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed(checksum=False):
    assert FC <= 250
    old, new = big_pair()
    chunks = list(page_chunks(checksum)[:FC])
    chunks.append(P.delta(new, old, 3, checksum, palign=9, dalign=3))
    chunks.append(k_delta(MIN + 1, checksum, palign=13, dalign=6))
    chunks.append(raw_only_chunk())
    return chunks


def test_mixed_prefix_batch_routes_each_chunk():
    chunks = mixed()
    n = len(chunks)
    assert n > FC and compressed_blocks(chunks[FC].frame) == 3 and compressed_blocks(chunks[FC + 1].frame) == MIN + 1
    assert all(compressed_blocks(c.frame) == 1 for c in chunks[:FC])
    assert all(needs_its_prefix(c.frame, len(c.record)) for c in chunks[:FC + 2])
    want = on_j([c.frame for c in chunks], n)
    assert FC + 1 in want and (MIN <= 3 or want == [FC + 1])
    st, ln, out = both_prefix(chunks, auto(), len(want))
    expect_records(chunks, st, ln, out)


# ---------------------------------------------------------------------------
# 2. the boundary: min - 1 blocks stays, min blocks goes
# ---------------------------------------------------------------------------
def test_the_block_minimum_is_exact():
    import torch
    L = lib()
    assert MIN >= 2
    chunks = [k_delta(MIN - 1, palign=1, dalign=7), k_delta(MIN, palign=6, dalign=11)] + list(page_chunks()[:FC - 1])
    n = len(chunks)
    assert n == FC + 1
    want = on_j([c.frame for c in chunks], n)
    assert want == ([1] if MIN > 1 else list(range(n)))
    st, ln, out = both_prefix(chunks, auto(), len(want))
    expect_records(chunks, st, ln, out)
    # which of the two: one round of one hop leaves a deep frame unconverged on K4J only
    for device in (False, True):
        r = P.Run(chunks, device, flags=auto() | L.F_J_ONE_ROUND)
        try:
            s = torch.cuda.current_stream().cuda_stream
            r.b.decode_async(s)
            torch.cuda.synchronize()
            dev_st, _ = device_arrays(r.b, n)
            assert dev_st[0] == 0 and dev_st[1] == L.OUT_OF_DOMAIN, dev_st[:2]
            assert dev_st[2:] == [0] * (n - 2)
            r.status, r.length = r.b.results(s)
            r.read_back()
            expect_records(chunks, r.status, r.length, r.out)
        finally:
            r.close()


# ---------------------------------------------------------------------------
# 3. few chunks
# ---------------------------------------------------------------------------
def test_few_chunks_take_the_lower_minimum():
    old, new = big_pair()
    npages = min(8, FC - 1)
    chunks = [P.delta(new, old, 3, palign=9, dalign=3)] + list(page_chunks()[:npages])
    assert len(chunks) <= FC and compressed_blocks(chunks[0].frame) == 3
    want = on_j([c.frame for c in chunks], len(chunks))
    assert want == ([0] if 1 < FEW <= 3 else want)
    st, ln, out = both_prefix(chunks, auto(), len(want))
    expect_records(chunks, st, ln, out)


# ---------------------------------------------------------------------------
# 4. precedence; the flag outside prefix and chain batches
# ---------------------------------------------------------------------------
def test_the_forcing_flags_win():
    L = lib()
    chunks = mixed()
    with_block = sum(compressed_blocks(c.frame) > 0 for c in chunks)
    assert with_block == len(chunks) - 1
    st, ln, out = both_prefix(chunks, auto() | L.F_BLOCK_PARALLEL, with_block)
    expect_records(chunks, st, ln, out)
    st, ln, out = both_prefix(chunks, auto() | L.F_FRAME_SERIAL, 0)
    expect_records(chunks, st, ln, out)


def plain_batch(frames, caps, flags, dictionary, device):
    """A plain or dictionary batch over `frames`: (statuses, lengths, outputs, executors, k4j_chunks)."""
    import torch
    from zstd_decompressor import Batch
    dev = torch.device("cuda", 0)
    srcs = [torch.frombuffer(bytearray(f), dtype=torch.uint8).to(dev) for f in frames]
    dsts = [torch.full((c,), FILL, dtype=torch.uint8, device=dev) for c in caps]
    cols = ([t.data_ptr() for t in srcs], [len(f) for f in frames], [t.data_ptr() for t in dsts], list(caps))
    if device:
        arr = [torch.tensor(v, dtype=torch.int64, device=dev) for v in cols]
        torch.cuda.synchronize()
        b = Batch.from_device(*arr, flags=flags, dictionary=dictionary)
    else:
        b = Batch(*cols, flags=flags, dictionary=dictionary)
    try:
        s = torch.cuda.current_stream().cuda_stream
        b.decode_async(s)
        st, ln = b.results(s)
        out = [bytes(t.cpu().numpy().tobytes())[:n] for t, n in zip(dsts, ln)]
        return st, ln, out, b.info.executors, b.info.k4j_chunks
    finally:
        b.close()


def test_the_flag_means_nothing_to_a_plain_or_a_dictionary_batch():
    from zstd_decompressor import Dictionary
    d = P.trained()
    old, new = big_pair()
    recs = [gen.text(3000 + 100 * k, seed=0xA1A0 + k) for k in range(5)] + [new]      # pages and a frame of three blocks
    for dictionary in (None, d):
        frames = [zdict.compress(x, d, 3) if dictionary else libzstd.compress(x, 3) for x in recs]
        frames[2] = frames[2][:-3]                                                  # a failing chunk among them
        handle = Dictionary(d) if dictionary else None
        try:
            res = [plain_batch(frames, [len(x) for x in recs], flags, handle, device)
                   for flags in (0, auto()) for device in (False, True)]
        finally:
            if handle is not None:
                handle.close()
        assert all(r == res[0] for r in res), [r[3:] for r in res]
        st, ln, out, executors, k4j = res[0]
        assert st[2] != 0 and [s for i, s in enumerate(st) if i != 2] == [0] * 5
        assert all(out[i] == recs[i] for i in range(6) if i != 2)
        assert bool(executors & lib().EXEC_K4J) == (k4j > 0)
        if dictionary:
            assert executors == 0 and k4j == 0


# ---------------------------------------------------------------------------
# 5. chain batches: large and page links in one chain
# ---------------------------------------------------------------------------
def large(seed, base=None):
    """A record of 300 KiB (three blocks) with a deep chain in it: text, or `base` edited."""
    n = 300 << 10
    rec = bytearray(edit(base, seed) if base is not None else gen.text(n, seed=seed))
    d = deep_chain(seed + 0x100)
    rec[2000:2000 + len(d)] = d
    return bytes(rec)


@functools.lru_cache(maxsize=None)
def mixed_chains():
    """Three chains of depth 3 (level 0, 1, 2 each):
       A  external base (300 KiB) <- large <- page (of the large parent's bytes) <- ... depth 3: large, page, large
       B  no base: a plain page <- large <- page
       C  no base: a plain large <- page <- page"""
    base = gen.text(300 << 10, seed=0xA5A0)
    a0 = large(0xA5A1, base)
    a1 = edit(a0[70000:70000 + PAGE], 0xA5A2)
    a2 = large(0xA5A3)
    b0 = gen.text(PAGE, seed=0xA5B0)
    b1 = large(0xA5B1)
    b2 = edit(b1[150000:150000 + PAGE], 0xA5B2)
    c0 = large(0xA5C0)
    c1 = edit(c0[200000:200000 + PAGE], 0xA5C1)
    c2 = edit(c1, 0xA5C2)
    chunks = [C.delta(a0, base, external=True, dalign=3, palign=7), C.delta(a1, a0, parent=0, dalign=9),
              C.delta(a2, a1, parent=1, dalign=14),
              C.plain(b0, dalign=1), C.delta(b1, b0, parent=3, dalign=6), C.delta(b2, b1, parent=4, dalign=11),
              C.plain(c0, dalign=5), C.delta(c1, c0, parent=6, dalign=12), C.delta(c2, c1, parent=7, dalign=2)]
    return chunks


LARGE_LINKS, PAGE_LINKS = [0, 2, 4, 6], [1, 3, 5, 7, 8]


def chain_runs(chunks, flags):
    """The chain batch through both creation calls: [(statuses, lengths, outputs, chain_info, k4j_chunks, executors)]."""
    res = []
    for device in (False, True):
        r = C.Run(chunks, device, flags=flags)
        try:
            st, ln = r.decode()
            assert r.b.info.prefix_bytes_total == r.prefix_total
            res.append((st, ln, r.out, r.b.chain_info, r.b.info.k4j_chunks, r.b.info.executors))
        finally:
            r.close()
    assert res[0] == res[1], "the host-array and the device-array batch differ"
    return res[0]


def test_chains_that_mix_large_and_page_links():
    chunks = mixed_chains()
    check_links_on_the_cpu(chunks)
    blocks = [compressed_blocks(c.frame) for c in chunks]
    assert [blocks[i] for i in LARGE_LINKS] == [3] * 4 and [blocks[i] for i in PAGE_LINKS] == [1] * 5, blocks
    assert needs_its_prefix(chunks[1].frame, PAGE) and needs_its_prefix(chunks[5].frame, PAGE)
    st0, ln0, out0, info0, k0, ex0 = chain_runs(chunks, 0)
    assert (k0, ex0) == (0, 0) and info0 == (3, 6)
    verify(chunks, st0, ln0, out0)
    want = on_j([c.frame for c in chunks], 3)                 # the widest level holds three chunks
    assert want == (LARGE_LINKS if 1 < FEW <= 3 else want)
    st, ln, out, info, k, ex = chain_runs(chunks, auto())
    assert (st, ln, out, info) == (st0, ln0, out0, info0)
    assert k == len(want) and ex == (lib().EXEC_K4J if want else 0)
    # the chain's forcing flag wins, the prefix batch's flags stay ignored
    L = lib()
    assert chain_runs(chunks, auto() | L.F_CHAIN_BLOCK_PARALLEL)[4] == 9
    assert chain_runs(chunks, auto() | L.F_FRAME_SERIAL)[4] == len(want)
    assert chain_runs(chunks, auto() | L.F_BLOCK_PARALLEL)[4] == len(want)


def test_a_chain_batch_none_of_whose_frames_goes_to_k4j():
    chunks = C.case1(PAGE)[:6] if FEW > 1 else []
    if not chunks:
        return
    assert all(compressed_blocks(c.frame) < FEW for c in chunks)
    st0, ln0, out0, info0, _, _ = chain_runs(chunks, 0)
    st, ln, out, info, k, ex = chain_runs(chunks, auto())
    assert (st, ln, out, info) == (st0, ln0, out0, info0) and (k, ex) == (0, 0)
    verify(chunks, st, ln, out)


# ---------------------------------------------------------------------------
# 6. failure crosses the executors
# ---------------------------------------------------------------------------
def corrupt_block(frame):
    """`frame` with the last one-bit flip that the frame walk accepts (the planner
    routes the frame like the intact one) and the oracle's decode rejects: a
    damaged bitstream inside the last block."""
    from oracle import oracle
    from zstd_decompressor.batch import frames_index
    for k in range(len(frame) - 6, 9, -1):
        for bit in (0, 3, 7):
            bad = frame[:k] + bytes([frame[k] ^ (1 << bit)]) + frame[k + 1:]
            st = oracle.decompress_status(bad)[0]
            if st != 0 and frames_index(bad)[2] == 0:
                return bad, st
    raise AssertionError("no flip the walk accepts and the oracle rejects")


@pytest.mark.parametrize("failing", ["large", "page"])
def test_failure_crosses_executors(failing):
    if failing == "large":
        rec = large(0xA6A0)
        parent = C.plain(rec, dalign=7)
        child = C.delta(edit(rec[5000:5000 + PAGE], 0xA6A1), rec, parent=0, want=NOT_DECODED, dalign=2)
    else:
        rec = gen.text(PAGE, seed=0xA6B0)
        parent = C.plain(rec, dalign=7)
        child = C.delta(large(0xA6B1), rec, parent=0, want=NOT_DECODED, dalign=2)
    assert compressed_blocks(parent.frame) == (3 if failing == "large" else 1)
    assert compressed_blocks(child.frame) == (1 if failing == "large" else 3)
    parent.frame, parent.want = corrupt_block(parent.frame)
    parent.against = None
    assert compressed_blocks(parent.frame) == (3 if failing == "large" else 1)
    chunks = [parent, child] + C.good_siblings(2, 0xA6C0)
    check_links_on_the_cpu(chunks)
    st0, ln0, out0, info0, _, _ = chain_runs(chunks, 0)
    verify(chunks, st0, ln0, out0)
    st, ln, out, info, k, ex = chain_runs(chunks, auto())
    assert (st, ln, out, info) == (st0, ln0, out0, info0)
    assert st[0] == parent.want and st[1] == NOT_DECODED and st[2:] == [0, 0, 0]
    assert k == (1 if 1 < FEW <= 3 else k) and bool(ex) == (k > 0)


# ---------------------------------------------------------------------------
# 7. pointer jumping that does not converge: decoded again behind results()
# ---------------------------------------------------------------------------
def test_unconverged_chunk_of_the_mixed_prefix_batch():
    import torch
    L = lib()
    chunks = mixed()
    n = len(chunks)
    want = on_j([c.frame for c in chunks], n)
    for device in (False, True):
        r = P.Run(chunks, device, flags=auto() | L.F_J_ONE_ROUND)
        try:
            assert r.b.info.k4j_chunks == len(want)
            s = torch.cuda.current_stream().cuda_stream
            r.b.decode_async(s)
            torch.cuda.synchronize()
            dev_st, dev_ln = device_arrays(r.b, n)
            assert dev_st[FC + 1] == L.OUT_OF_DOMAIN and dev_ln[FC + 1] == 0, dev_st[FC:]
            assert [s_ for i, s_ in enumerate(dev_st) if i not in want] == [0] * (n - len(want))
            r.status, r.length = r.b.results(s)
            r.read_back()
            expect_records(chunks, r.status, r.length, r.out)
            assert device_arrays(r.b, n) == (r.status, r.length)          # the device arrays are updated
        finally:
            r.close()


def test_unconverged_links_and_everything_behind_them():
    import torch
    L = lib()
    chunks = mixed_chains()
    n = len(chunks)
    if not 1 < FEW <= 3:
        return
    for device in (False, True):
        r = C.Run(chunks, device, flags=auto() | L.F_J_ONE_ROUND)
        try:
            assert r.b.info.k4j_chunks == 4
            s = torch.cuda.current_stream().cuda_stream
            r.b.decode_async(s)
            torch.cuda.synchronize()
            dev_st, dev_ln = device_arrays(r.b, n)
            # A: the large root and everything behind it; B: the page root is done, the large link and its child
            # are not; C: the large root and both pages behind it
            assert dev_st == [L.OUT_OF_DOMAIN, NOT_DECODED, NOT_DECODED, 0, L.OUT_OF_DOMAIN, NOT_DECODED,
                              L.OUT_OF_DOMAIN, NOT_DECODED, NOT_DECODED], dev_st
            assert dev_ln == [0, 0, 0, PAGE, 0, 0, 0, 0, 0]
            r.status, r.length = r.b.results(s)
            r.read_back()
            verify(chunks, r.status, r.length, r.out)
            assert r.status == [0] * n
            assert device_arrays(r.b, n) == (r.status, r.length)
        finally:
            r.close()


# ---------------------------------------------------------------------------
# 8. verification inside the launch, on both executors
# ---------------------------------------------------------------------------
def test_verified_mixed_batch_with_two_damaged_frames():
    L = lib()
    good = mixed(True)
    n = len(good)
    chunks = list(good)
    for i in (5, FC + 1):                                    # a page (streaming) and the large frame (K4J)
        f = bytearray(good[i].frame)
        f[-1] ^= 0x10                                        # one bit of the stored Content_Checksum
        chunks[i] = P.Chunk(bytes(f), good[i].prefix, record=good[i].record, palign=good[i].palign, dalign=good[i].dalign)
    want = on_j([c.frame for c in chunks], n)
    st, ln, out = both_prefix(chunks, auto() | L.F_VERIFY_CHECKSUM, len(want))
    for i, c in enumerate(chunks):
        if i in (5, FC + 1):
            assert st[i] == L.CHECKSUM_WRONG and ln[i] == 0, (i, st[i])
        else:
            assert st[i] == 0 and ln[i] == len(c.record) and out[i] == c.record, (i, st[i])


# ---------------------------------------------------------------------------
# 9. graph capture: replayed after a prefix's content changed
# ---------------------------------------------------------------------------
def test_hip_graph_capture_replay_with_a_changed_prefix():
    import torch
    chunks = mixed()
    n = len(chunks)
    old, new, edited = pages()[7]
    gaps = np.diff(edited)
    k = int(np.argmax(gaps))
    assert gaps[k] > 80
    pos = int(edited[k]) + int(gaps[k]) // 2                 # a prefix byte inside a matched region
    changed = old[:pos] + bytes([old[pos] ^ 0xFF]) + old[pos + 1:]
    want7 = zdict.prefix_decompress(chunks[7].frame, changed, PAGE)
    assert want7 != chunks[7].record and want7[pos] == chunks[7].record[pos] ^ 0xFF
    dev = torch.device("cuda", 0)
    for device in (False, True):
        r = P.Run(chunks, device, flags=auto())
        try:
            assert r.b.info.k4j_chunks >= 1
            s = torch.cuda.Stream(dev)
            with torch.cuda.stream(s):          # warm-up outside the capture
                r.b.decode_async(s.cuda_stream)
            s.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=s):
                r.b.decode_async(s.cuda_stream)
            at = r.po[7] + pos
            r.P.t[at] ^= 0xFF
            r.P.host[at] ^= 0xFF
            for _ in range(2):
                r.D.t.fill_(FILL)
                torch.cuda.synchronize(dev)
                g.replay()
                torch.cuda.synchronize(dev)
                r.status, r.length = r.b.results(torch.cuda.current_stream(dev).cuda_stream)
                r.read_back()
                assert r.status == [0] * n
                assert r.out[7] == want7
                assert all(r.out[i] == chunks[i].record for i in range(n) if i != 7)
            del g
        finally:
            r.close()
