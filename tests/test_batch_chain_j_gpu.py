"""Chain batches on the block-parallel executor (K4J): a chain batch created
with F_CHAIN_BLOCK_PARALLEL sends every frame with a compressed block through
zd_k_jsum .. zd_k_jprefix once and then, level by level, zd_k_jscatter<true, true>
over the level's segments and zd_k_jround<true> over the level's pieces, behind
the level's zd_k_execute_chain; the frames without a compressed block stay on
zd_k_execute_chain.

Expected bytes are always the original record AND corpus.zdict.prefix_decompress
of the same frame against its parent's record (check_links_on_the_cpu, libzstd on
the CPU); a chunk that must fail has the status the same batch gives WITHOUT the
flag.  The harness (Arena, Run, Chunk, verify: ranges inside 0xA5-filled tensors,
64 bytes of slack on every side, the slack, the sources and the external prefixes
compared after each decode) is tests/test_batch_chain_gpu.py's, the records come
from tests/test_batch_prefix_gpu.py and tests/test_batch_prefix_j_gpu.py, and
every case runs through both creation calls."""
import functools

import numpy as np
import pytest

import test_batch_chain_gpu as C
import test_batch_prefix_gpu as P
from corpus import gen, libzstd, zdict
from test_batch_chain_gpu import FILL, NOT_DECODED, OK, PAGE, Chunk, Run, check_links_on_the_cpu, delta, edit, plain, verify
from test_batch_prefix_gpu import big_pair, needs_its_prefix, pages, rnd
from test_batch_prefix_j_gpu import PERIOD_CASES, hand_period_frame

pytestmark = pytest.mark.gpu


def lib():
    from zstd_decompressor import _lib
    return _lib


def flag_cj():
    return lib().F_CHAIN_BLOCK_PARALLEL


def compressed_blocks(frame):
    from zstd_decompressor.batch import frames_index
    _, blocks, st, _ = frames_index(frame)
    assert st == 0
    return sum(b["type"] == 2 for b in blocks)


def unflagged(chunks, flags=0):
    """(statuses, lengths) of the same chain batch without the flag: the streaming executor only."""
    r = Run(chunks, False, flags=flags)
    try:
        st, ln = r.decode()
        assert r.b.info.executors == 0
        return st, ln
    finally:
        r.close()


def both_j(chunks, flags=0, levels=None, links=None, allowed=None, same_as_unflagged=False):
    """The chunks through both creation calls with F_CHAIN_BLOCK_PARALLEL | flags:
    K4J ran, every chunk has its expected status and bytes, the two calls agree,
    and (same_as_unflagged) statuses and lengths are the unflagged batch's."""
    res = []
    for device in (False, True):
        r = Run(chunks, device, flags=flags | flag_cj())
        try:
            st, ln = r.decode()
            assert r.b.info.executors & lib().EXEC_K4J, r.b.info.executors
            assert r.b.info.prefix_bytes_total == r.prefix_total
            lv, lk = r.b.chain_info
            if levels is not None:
                assert lv == levels, (device, lv)
            if links is not None:
                assert lk == links, (device, lk)
            verify(chunks, st, ln, r.out, allowed)
            res.append((st, ln, r.out, lv, lk))
        finally:
            r.close()
    assert res[0] == res[1], "the host-array and the device-array batch differ"
    if same_as_unflagged:
        st0, ln0 = unflagged(chunks, flags)
        assert (res[0][0], res[0][1]) == (st0, ln0), [(i, a, b) for i, (a, b) in enumerate(zip(res[0][0], st0)) if a != b]
    return res[0]


# ---------------------------------------------------------------------------
# 1. page chains
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def page_chains(n=16, depth=4, checksum=False):
    """n chains of `depth` 16 KiB page versions over external bases (tests/test_batch_prefix_gpu.py pages():
    text with 1 % of the bytes edited), every prefix and destination alignment 0-15."""
    chunks = []
    for k in range(n):
        base = pages()[k][0]
        al = tuple((5 * k + 3 * j) % 16 for j in range(depth))
        chunks += C.line(base, depth, 0xD1A0 + 8 * k, dalign=al, first=len(chunks), palign=k % 16, checksum=checksum)
    return chunks


def test_page_chains():
    chunks = page_chains()
    assert len(chunks) == 64
    check_links_on_the_cpu(chunks)
    assert {c.palign for c in chunks if c.prefix} == set(range(16)) and {c.dalign for c in chunks} == set(range(16))
    assert all(needs_its_prefix(c.frame, PAGE) for c in chunks)
    assert all(compressed_blocks(c.frame) for c in chunks)
    st, ln, out, lv, lk = both_j(chunks, levels=4, links=48)
    assert st == [0] * 64 and (lv, lk) == (4, 48)


# ---------------------------------------------------------------------------
# 2. order and shape
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shapes():
    base = gen.text(PAGE, seed=0xD2A0)
    v = [edit(base, 0xD2A1)]
    v += [edit(v[0], 0xD2A2)]
    v += [edit(v[1], 0xD2A3)]
    # children before their parents: chunk 0 needs chunk 1 needs chunk 2 needs the external base
    chunks = [delta(v[2], v[1], parent=1, dalign=5), delta(v[1], v[0], parent=2, dalign=11),
              delta(v[0], base, external=True, dalign=9, palign=7)]
    chunks.append(plain(gen.text(3000, seed=0xD2B0)))                               # unrelated, no prefix
    hub = len(chunks) + 8
    hub_rec = gen.text(PAGE, seed=0xD2C0)
    chunks += [delta(edit(hub_rec, 0xD2D0 + k), hub_rec, parent=hub, dalign=(7 * k) % 16) for k in range(8)]   # a star ...
    chunks.append(plain(hub_rec, dalign=13))                                        # ... whose parent comes last
    chunks.append(plain(rnd(0xD2F0, 700)))                                          # unrelated, raw blocks only
    e = len(chunks)
    chunks += [Chunk(b"", b"", cap=0), plain(gen.text(4000, seed=0xD2F1), parent=e, dalign=3)]   # an empty parent
    chunks.append(delta(edit(chunks[e + 1].record, 0xD2F2), chunks[e + 1].record, parent=e + 1))
    return chunks


def test_order_star_unrelated_and_an_empty_parent():
    chunks = shapes()
    check_links_on_the_cpu(chunks)
    st, ln, out, _, _ = both_j(chunks, levels=3, links=2 + 8 + 2, same_as_unflagged=True)
    assert st == [0] * len(chunks)


# ---------------------------------------------------------------------------
# 3. streaming and K4J frames in one chain
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_executors():
    """raw (streaming) <- J <- raw <- J <- raw (two blocks) <- J: every link crosses the two executors."""
    r0 = rnd(0xD3A0, 6000)                                         # incompressible: Raw blocks only
    j1 = r0[1000:4000] + gen.text(2000, seed=0xD3A1) + r0[:500]
    r2 = rnd(0xD3A2, 5000)
    j3 = r2[:2500] + j1[200:900] * 2 + r2[2500:]
    z4 = rnd(0xD3A4, 140000)
    j5 = z4[:3000] + gen.text(1500, seed=0xD3A3) + z4[-2000:]
    chunks = [plain(r0, level=1, dalign=1), delta(j1, r0, parent=0, dalign=6),
              delta(r2, j1, parent=1, level=1, dalign=11), delta(j3, r2, parent=2, dalign=4),
              delta(z4, j3, parent=3, level=1, dalign=9), delta(j5, z4, parent=4, dalign=15)]
    return chunks


def test_mixed_executors_inside_one_chain():
    chunks = mixed_executors()
    check_links_on_the_cpu(chunks)
    kinds = [compressed_blocks(c.frame) > 0 for c in chunks]
    assert kinds == [False, True, False, True, False, True], kinds
    assert needs_its_prefix(chunks[1].frame, len(chunks[1].record)) and needs_its_prefix(chunks[3].frame, len(chunks[3].record))
    st, ln, out, _, _ = both_j(chunks, levels=6, links=5, same_as_unflagged=True)
    assert st == [0] * 6


# ---------------------------------------------------------------------------
# 4. the boundary: periods that start in the parent's output
# ---------------------------------------------------------------------------
def push(prefix, lits, off, ml):
    hist = bytearray(prefix + lits)
    for _ in range(ml):
        hist.append(hist[len(hist) - off])                  # the reference's byte-by-byte push
    return bytes(hist[len(prefix):])


def hand_parent(seed, size):
    """A frame of one compressed block that needs no prefix and decodes to `size` bytes (5 literals, offset 5)."""
    lits = rnd(seed, 5)
    frame = hand_period_frame(lits, 5, size - 5)
    rec = push(b"", lits, 5, size - 5)
    assert libzstd.decompress_frame(frame, size) == rec and compressed_blocks(frame) == 1
    return Chunk(frame, rec, against=b"")


@functools.lru_cache(maxsize=None)
def boundary():
    chunks = []
    for k, (o, ll) in enumerate(PERIOD_CASES):
        ml = 40 if o < 15 else 66
        # behind a parent of 64 bytes, and (where a frame of a compressed block can be that small) behind one
        # of exactly o - ll bytes: the match source reaches the parent's first byte
        for size in (64,) + ((o - ll,) if o - ll >= 8 else ()):
            par = hand_parent(0xD4A0 + 2 * k + (size != 64), size)
            par.dalign = (3 * k + size) % 16
            lits = rnd(0xD4C0 + k, ll)
            frame = hand_period_frame(lits, o, ml)
            want = push(par.record, lits, o, ml)
            assert zdict.prefix_decompress(frame, par.record, ll + ml) == want and len(want) == ll + ml
            p = len(chunks)
            chunks += [par, Chunk(frame, want, parent=p, against=par.record, dalign=(5 * k + 1) % 16)]
    return chunks


def test_periods_across_the_boundary_behind_a_j_parent():
    chunks = boundary()
    assert sum(c.parent >= 0 and len(chunks[c.parent].record) < 64 for c in chunks) >= 3    # parent byte 0 reached
    check_links_on_the_cpu(chunks)
    st, ln, out, _, _ = both_j(chunks, levels=2, links=len(chunks) // 2, same_as_unflagged=True)
    assert st == [0] * len(chunks)


def test_an_offset_one_past_the_parents_first_byte():
    # parent of 12 bytes, child: 5 literals, offset 18 = 12 + 5 + 1, and two chunks behind it
    par = hand_parent(0xD4F0, 12)
    lits = rnd(0xD4F1, 5)
    bad = Chunk(hand_period_frame(lits, 18, 66), b"\x00" * 71, parent=0, against=None, want=lib().IMPOSSIBLE_VALUE)
    ok = Chunk(hand_period_frame(lits, 17, 66), push(par.record, lits, 17, 66), parent=0, against=par.record, dalign=7)
    behind = [delta(edit(gen.text(300, seed=0xD4F2), 0xD4F3 + k), b"\x00" * 71, parent=1 + k, want=NOT_DECODED)
              for k in range(2)]
    for c in behind:
        c.against = None
    chunks = [par, bad, behind[0], behind[1], ok]
    chunks[3].parent = 2
    check_links_on_the_cpu(chunks)
    st, ln, out, _, _ = both_j(chunks, levels=4, links=4, same_as_unflagged=True)
    assert st == [0, lib().IMPOSSIBLE_VALUE, NOT_DECODED, NOT_DECODED, 0]


# ---------------------------------------------------------------------------
# 5. multi-block frames
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_chain(level):
    old, new = big_pair()                                  # 300 KiB: three blocks each
    newer = edit(new, 0xD5A0 + level, 200)
    newer = newer[:90000] + rnd(0xD5A1, 2000) + newer[90000:len(newer) - 2000]
    return [plain(old, level=level, dalign=9), delta(new, old, parent=0, level=level, dalign=3),
            delta(newer, new, parent=1, level=level, dalign=14)]


@pytest.mark.parametrize("level", [1, 19])
def test_multi_block_chain(level):
    chunks = big_chain(level)
    check_links_on_the_cpu(chunks)
    assert all(compressed_blocks(c.frame) >= 3 for c in chunks)
    st, ln, out, _, _ = both_j(chunks, levels=3, links=2)
    assert st == [0, 0, 0]


@functools.lru_cache(maxsize=None)
def chain_2m5():
    n = 2560 << 10
    v = [gen.text(n, seed=0xD5B0)]
    for k in range(2):
        v.append(edit(v[-1], 0xD5B1 + k, 100))
    return [plain(v[0], dalign=13), delta(v[1], v[0], parent=0, dalign=6), delta(v[2], v[1], parent=1, dalign=1)]


def test_a_chain_of_twenty_block_versions():
    chunks = chain_2m5()
    check_links_on_the_cpu(chunks)
    assert all(compressed_blocks(c.frame) >= 16 for c in chunks)
    assert all(len(c.frame) * 4 < len(c.record) for c in chunks[1:])
    # (the frames' headers ask for no window past 8 MiB: no F_LONG_WINDOW)
    st, ln, out, _, _ = both_j(chunks, levels=3, links=2)
    assert st == [0, 0, 0]


# ---------------------------------------------------------------------------
# 6. depth: 256 levels, and a failing frame at level 100
# ---------------------------------------------------------------------------
def test_256_levels():
    chunks = C.case4()
    assert sum(compressed_blocks(c.frame) > 0 for c in chunks) >= 250
    st, ln, out, lv, lk = both_j(chunks, levels=256, links=255)
    assert st == [0] * 256 and (lv, lk) == (256, 255)


def test_a_corrupt_frame_at_level_100():
    line = C.case4()
    chunks = [Chunk(c.frame, c.record, parent=c.parent, dalign=c.dalign, against=c.against) for c in line]
    chunks[100].frame = chunks[100].frame[:-3]              # truncated: the walk's or the decode's own status
    chunks[100].against = None
    beside = C.good_siblings(len(chunks), 0xD6A0)           # a chain beside it
    chunks += beside
    st0, ln0 = unflagged(chunks)
    assert st0[100] not in (OK, NOT_DECODED) and ln0[100] == 0
    chunks[100].want = st0[100]
    for c in chunks[101:256]:
        c.want = NOT_DECODED
    st, ln, out, _, _ = both_j(chunks, levels=256, links=255 + 2)
    assert (st, ln) == (st0, ln0)
    assert st[:100] == [0] * 100 and st[101:256] == [NOT_DECODED] * 155 and ln[101:256] == [0] * 155
    assert st[256:] == [0, 0, 0]


# ---------------------------------------------------------------------------
# 7. failure propagation: the statuses of the unflagged batch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["table", "dst_cap", "checksum"])
def test_failing_j_parent(kind):
    chunks = C.case5(kind)
    assert compressed_blocks(plain(chunks[3].record).frame) > 0           # the failing parent is a K4J frame
    flags = C.F_VERIFY_CHECKSUM if kind == "checksum" else 0
    st, ln, out, _, _ = both_j(chunks, flags=flags, levels=3, same_as_unflagged=True)
    assert st[3] == chunks[3].want and st[4] == st[5] == st[9] == NOT_DECODED


def test_a_parent_whose_length_is_not_its_content_size():
    rec = gen.text(PAGE, seed=0xD7A0)
    par = plain(rec, dalign=7)
    f = bytearray(par.frame)
    assert f[4] >> 6 == 1 and (f[4] >> 5) & 1 and f[4] & 3 == 0          # single segment, a 2-byte Frame_Content_Size
    assert int.from_bytes(f[5:7], "little") + 256 == PAGE
    f[5:7] = (PAGE + 10 - 256).to_bytes(2, "little")                      # ten bytes more than the frame decodes to
    par.frame, par.cap, par.against = bytes(f), PAGE + 10, None
    child = delta(edit(rec, 0xD7A1), rec, parent=0, want=NOT_DECODED, dalign=3)
    grand = delta(edit(child.record, 0xD7A2), child.record, parent=1, want=NOT_DECODED)
    chunks = [par, child, grand] + C.good_siblings(3, 0xD7B0)
    st0, ln0 = unflagged(chunks)
    assert st0[1] == st0[2] == NOT_DECODED and st0[3:] == [0, 0, 0]
    par.want = st0[0]
    allowed = {0: (st0[0],)} if st0[0] else None
    if not st0[0]:
        par.record = rec
    st, ln, out, _, _ = both_j(chunks, levels=3, allowed=allowed)
    assert (st, ln) == (st0, ln0)


def test_a_frame_that_names_a_dictionary():
    rec = gen.text(3000, seed=0xD7C0)
    with_id = Chunk(zdict.compress(rec, P.trained(), 3), rec, against=None, want=lib().DICT_MISMATCH)
    child = delta(edit(rec, 0xD7C1), rec, parent=0, want=NOT_DECODED)
    # ... and as a child of a good K4J parent
    root = plain(gen.text(2000, seed=0xD7C2))
    with_id2 = Chunk(with_id.frame, rec, parent=2, against=None, want=lib().DICT_MISMATCH, dalign=5)
    chunks = [with_id, child, root, with_id2] + C.good_siblings(4, 0xD7D0)
    st, ln, out, _, _ = both_j(chunks, levels=3, same_as_unflagged=True)
    assert st[:4] == [lib().DICT_MISMATCH, NOT_DECODED, 0, lib().DICT_MISMATCH]


# ---------------------------------------------------------------------------
# 8. pointer jumping that does not converge: decoded again behind results()
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def unconverged():
    """root (raw blocks, streaming) <- middle (match chains deeper than one hop) <- leaf <- leaf2, and beside them
    a chain whose K4J frames copy from their prefixes only (final at the scatter: no hop needed)."""
    root = rnd(0xD8A0, 4000)
    X = rnd(0xD8A1, 1500)                                  # not in the prefix: each copy points at the copy before it
    mid = root[100:1100] + b"".join(X + rnd(0xD8B0 + k, 3 + 2 * k) for k in range(8)) + root[2000:3000]
    leaf = edit(mid, 0xD8A2)
    leaf2 = edit(leaf, 0xD8A3)
    chunks = [plain(root, level=1, dalign=3), delta(mid, root, parent=0, dalign=9), delta(leaf, mid, parent=1, dalign=14),
              delta(leaf2, leaf, parent=2, dalign=5)]
    r2 = rnd(0xD8C0, 8000)
    rng = np.random.default_rng(0xD8C1)
    far = b"".join(r2[a:a + 150] + bytes(rng.integers(0, 256, 4, dtype=np.uint8)) for a in range(0, 7500, 300))
    far2 = b"".join(far[a:a + 120] + bytes(rng.integers(0, 256, 3, dtype=np.uint8)) for a in range(0, 3600, 240))
    chunks += [plain(r2, level=1, dalign=1), delta(far, r2, parent=4, dalign=7), delta(far2, far, parent=5, dalign=12)]
    return chunks


def test_unconverged_frames_and_everything_behind_them_are_decoded_again():
    import torch
    from zstd_decompressor.batch import _read_u64
    L = lib()
    chunks = unconverged()
    check_links_on_the_cpu(chunks)
    n = len(chunks)
    assert [compressed_blocks(c.frame) > 0 for c in chunks] == [False, True, True, True, False, True, True]
    for device in (False, True):
        r = Run(chunks, device, flags=L.F_J_ONE_ROUND | L.F_CHAIN_BLOCK_PARALLEL)
        try:
            s = torch.cuda.current_stream().cuda_stream
            r.b.decode_async(s)
            torch.cuda.synchronize()
            # the launch's own statuses, before results() decodes anything again
            def device_arrays():
                d_st, d_ln = r.b.device_results()
                st = np.array(_read_u64(d_st, (n + 1) // 2), dtype=np.uint64).view(np.int32)[:n]
                return [int(v) for v in st], [int(v) for v in _read_u64(d_ln, n)]
            dev_st, dev_ln = device_arrays()
            assert dev_st[:4] == [0, L.OUT_OF_DOMAIN, NOT_DECODED, NOT_DECODED], dev_st
            assert dev_st[4:] == [0, 0, 0], dev_st
            assert dev_ln[1:4] == [0, 0, 0]
            # the chain beside it is complete already: its bytes do not change below
            before = r.D.download()
            for i in (4, 5, 6):
                assert bytes(before[r.do[i]:r.do[i] + dev_ln[i]]) == chunks[i].record, i
            r.status, r.length = r.b.results(s)
            r.read_back()
            assert r.status == [0] * n, r.status
            verify(chunks, r.status, r.length, r.out)
            assert device_arrays() == (r.status, r.length)            # the device arrays are updated
        finally:
            r.close()


# ---------------------------------------------------------------------------
# 9. relaunch, a changed base, graph capture
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def one_line():
    """One chain of depth 4 over an external base, and the position of a base byte every link copies."""
    base = pages()[40][0]
    rng = np.random.default_rng(0xD9A0)
    pos = 8000
    recs, prev = [], base
    for k in range(4):
        at = [int(p) for p in rng.choice(PAGE, PAGE // 100, replace=False) if abs(int(p) - pos) > 100]
        new = bytearray(prev)
        for p in at:
            new[p] ^= 0x5A
        recs.append(bytes(new))
        prev = recs[-1]
    chunks, prev = [], base
    for k, rec in enumerate(recs):
        chunks.append(delta(rec, prev, parent=k - 1 if k else -1, external=k == 0, dalign=(5 * k + 2) % 16, palign=11))
        prev = rec
    return chunks, pos


def test_relaunch_and_a_changed_base():
    chunks, pos = one_line()
    chunks = chunks + C.good_siblings(len(chunks), 0xD9B0)
    check_links_on_the_cpu(chunks)
    base = chunks[0].prefix
    base2 = base[:pos] + bytes([base[pos] ^ 0xFF]) + base[pos + 1:]
    want2, prev = [], base2
    for c in chunks[:4]:
        prev = zdict.prefix_decompress(c.frame, prev, PAGE)
        want2.append(prev)
        assert prev != c.record and prev[pos] == c.record[pos] ^ 0xFF      # every link copies that byte
    for device in (False, True):
        r = Run(chunks, device, flags=flag_cj())
        try:
            first = r.decode()
            verify(chunks, *first, r.out)
            r.D.t.fill_(FILL)
            again = r.decode()
            assert again == first
            verify(chunks, *again, r.out)
            at = r.P.items[0][0] + pos
            r.P.t[at] ^= 0xFF
            r.P.host[at] ^= 0xFF
            st, ln = r.decode()
            assert st == [0] * len(chunks)
            assert r.out[:4] == want2 and all(o == c.record for o, c in zip(r.out[4:], chunks[4:]))
        finally:
            r.close()


def test_graph_capture_replay():
    import torch
    chunks = page_chains(4, 4) + shapes()[-3:]
    off = 16
    chunks = chunks[:off] + [Chunk(c.frame, c.record, parent=c.parent - (len(shapes()) - 3) + off if c.parent >= 0 else -1,
                                   prefix=c.prefix, cap=c.cap, dalign=c.dalign, against=c.against) for c in chunks[off:]]
    check_links_on_the_cpu(chunks)
    dev = torch.device("cuda", 0)
    for device in (False, True):
        r = Run(chunks, device, flags=flag_cj())
        try:
            assert r.b.info.executors & lib().EXEC_K4J
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
                verify(chunks, r.status, r.length, r.out)
            del g
        finally:
            r.close()


# ---------------------------------------------------------------------------
# 10. nothing else moves
# ---------------------------------------------------------------------------
def test_without_the_flag_a_chain_stays_on_the_streaming_executor():
    chunks = page_chains(4, 4)
    for flags in (0, lib().F_BLOCK_PARALLEL):
        C.both(chunks, flags=flags, levels=4, links=12)            # (asserts executors == 0)


def test_the_flag_means_nothing_outside_a_chain_batch():
    import torch
    from zstd_decompressor import Dictionary, decode_tensors
    L = lib()
    F = L.F_CHAIN_BLOCK_PARALLEL
    # a prefix batch: tests/test_batch_prefix_gpu.py's harness
    pchunks = P.page_chunks()[:16]
    got = []
    for flags in (0, F):
        for device in (False, True):
            r = P.Run(pchunks, device, flags=flags)
            try:
                st, ln = r.decode()
                got.append((st, ln, r.out, r.b.info.executors))
            finally:
                r.close()
    assert all(g == got[0] for g in got) and got[0][3] == 0 and got[0][0] == [0] * 16
    assert all(o == c.record for o, c in zip(got[0][2], pchunks))
    # a plain batch and a dictionary batch, a failing chunk among them
    dev = torch.device("cuda", 0)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    recs = [gen.text(3000 + 100 * k, seed=0xDAA0 + k) for k in range(6)]
    d = P.trained()
    for dictionary in (None, d):
        frames = [zdict.compress(x, d, 3) if dictionary else libzstd.compress(x, 3) for x in recs]
        frames[2] = frames[2][:-3]
        handle = Dictionary(d) if dictionary else None
        res = []
        for flags in (0, F):
            srcs = [up(f) for f in frames]
            dsts = [torch.full((len(x),), FILL, dtype=torch.uint8, device=dev) for x in recs]
            st, ln = decode_tensors(srcs, dsts, dictionary=handle, flags=flags)
            res.append((st, ln, [bytes(t.cpu().numpy().tobytes()) for t in dsts]))
        assert res[0] == res[1]
        st, ln, out = res[0]
        assert st[2] != 0 and [s for i, s in enumerate(st) if i != 2] == [0] * 5
        assert all(out[i] == recs[i] for i in range(6) if i != 2)
        if handle is not None:
            handle.close()
