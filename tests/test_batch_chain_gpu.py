"""Chain batches on the GPU (include/zd.h zd_batch_create_chain /
zd_batch_create_device_chain, Batch(parents=...), zd_k_execute_chain): a chunk's
prefix is another chunk's decoded output of the same launch.

Expected bytes are always the original record AND corpus.zdict.prefix_decompress
(ZSTD_DCtx_refPrefix + ZSTD_decompressDCtx) of the same frame against its
parent's record (or its external prefix); a chunk that must fail has one exact
expected status.  test_fixtures_are_known_good builds every fixture and checks
every link that way on the CPU, so the inputs are known good before any GPU run.

Layout of every test (class Arena, as in test_batch_prefix_gpu.py): the external
prefixes, the sources and the destinations are carved out of the interior of
three single device tensors filled with 0xA5, with at least 64 bytes of slack on
every side of every range.  After every decode the slack of all three tensors,
the external prefixes and the sources are compared with what was uploaded.  No
test provokes a fault: every failing case is a status the decoder returns, with
all reads inside owned ranges.  Every case runs through both creation calls."""
import functools

import numpy as np
import pytest

from corpus import gen, libzstd, zdict
from oracle import oracle

gpu = pytest.mark.gpu
FILL = 0xA5
SLACK = 64
PAGE = 16 << 10
OK, OUT_OF_DOMAIN, DST_TOO_SMALL, INVALID_ARG, NOT_DECODED, CHECKSUM_WRONG = 0, -91, -92, -93, -96, -100
CORRUPTED_TABLE, LARGE_ACCURACY_LOG = -13, -12
F_VERIFY_CHECKSUM = 1024


def rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


def edit(data, seed, frac=100):
    """`data` with one byte in `frac` changed (at least one), seeded."""
    rng = np.random.default_rng(seed)
    out = bytearray(data)
    for p in rng.choice(len(data), max(1, len(data) // frac), replace=False):
        out[p] ^= int(rng.integers(1, 256))
    return bytes(out)


# ---------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------
class Arena:
    """Ranges inside one uint8 tensor filled with FILL: place(data or size,
    align) gives the range's offset, with offset % 16 == align % 16 (the
    tensor's base is 256-byte aligned) and SLACK bytes of FILL around it."""

    def __init__(self):
        self.at = 256
        self.items = []

    def place(self, data, align=0, size=None):
        n = len(data) if data is not None else size
        o = self.at + SLACK
        o += (align - o) % 16
        self.items.append((o, data, n))
        self.at = o + n
        return o

    def upload(self):
        import torch
        host = np.full(self.at + SLACK + 256, FILL, dtype=np.uint8)
        for o, data, n in self.items:
            if data is not None and n:
                host[o:o + n] = np.frombuffer(data, dtype=np.uint8)
        self.host = host
        self.t = torch.from_numpy(host.copy()).to(torch.device("cuda", 0))
        assert self.t.data_ptr() % 16 == 0
        return self.t.data_ptr()

    def download(self):
        return self.t.cpu().numpy()


class Chunk:
    """frame: the chunk's bytes; record: what it decodes to when `want` is OK;
    parent: -1 or the index in the batch (any integer, for the entries the
    device call must refuse); prefix: an external prefix (bytes) or None;
    against: the bytes libzstd needs as the prefix to give `record` back (the
    parent's record or the external prefix; None: the frame as it is cannot be
    checked that way, e.g. a corrupted one); psize: the prefix_bytes entry when
    there is no external prefix (a size on a chained chunk must be refused)."""

    def __init__(self, frame, record, parent=-1, prefix=None, cap=None, dalign=0, palign=0, want=OK, against=b"",
                 psize=0):
        self.frame, self.record, self.parent, self.prefix = frame, record, parent, prefix
        self.cap = len(record) if cap is None else cap
        self.dalign, self.palign, self.want, self.against, self.psize = dalign, palign, want, against, psize


def plain(record, level=3, checksum=False, content_size=True, **kw):
    return Chunk(libzstd.compress(record, level, checksum, 0, content_size), record, against=b"", **kw)


def delta(record, base, parent=-1, external=False, level=3, checksum=False, content_size=True, **kw):
    """`record` compressed against `base`: the parent's record (parent given), or an external prefix."""
    frame = zdict.prefix_compress(record, base, level, checksum, content_size)
    return Chunk(frame, record, parent=parent, prefix=base if external else None, against=base, **kw)


def check_links_on_the_cpu(chunks):
    """Every chunk that is expected to decode (and every failing one whose
    frame is intact) gives its record back through libzstd with its prefix."""
    for i, c in enumerate(chunks):
        if c.against is None:
            continue
        if 0 <= c.parent < len(chunks) and c.prefix is None and chunks[c.parent].want == OK and c.want == OK:
            assert c.against == chunks[c.parent].record, (i, "the link is not against its parent's record")
        if c.prefix is not None:
            assert c.against == c.prefix, i
        if len(c.frame):
            assert zdict.prefix_decompress(c.frame, c.against, len(c.record)) == c.record, i
        else:
            assert c.record == b"", i


class Run:
    """The chunks laid out on the device and one chain batch over them."""

    def __init__(self, chunks, device, flags=0, chain=True):
        import torch
        from zstd_decompressor import Batch
        self.chunks, n = chunks, len(chunks)
        self.P, self.S, self.D = Arena(), Arena(), Arena()
        po = [self.P.place(c.prefix, c.palign) if c.prefix else None for c in chunks]
        so = [self.S.place(c.frame, (3 * i) % 16) for i, c in enumerate(chunks)]
        order = np.random.default_rng(n).permutation(n)      # the lowest destination is not chunk 0's
        do = [None] * n
        for i in order:
            do[i] = self.D.place(None, chunks[i].dalign, size=chunks[i].cap)
        pb, sb, db = self.P.upload(), self.S.upload(), self.D.upload()
        self.do = do
        sp = [sb + o for o in so]
        ss = [len(c.frame) for c in chunks]
        dp = [db + o for o in do]
        dc = [c.cap for c in chunks]
        pp = [pb + o if o is not None else 0 for o in po]
        ps = [len(c.prefix) if c.prefix else c.psize for c in chunks]
        par = [c.parent for c in chunks]
        self.prefix_total = sum(len(c.prefix) for c in chunks if c.prefix and c.want != INVALID_ARG)
        external = any(ps)
        if device:
            dev = torch.device("cuda", 0)
            arr = [torch.tensor(v, dtype=torch.int64, device=dev) for v in (sp, ss, dp, dc, pp, ps, par)]
            torch.cuda.synchronize()
            self.b = Batch.from_device(*arr[:4], flags=flags, prefixes=(arr[4], arr[5]) if external or not chain else None,
                                       parents=arr[6] if chain else None)
        else:
            self.b = Batch(sp, ss, dp, dc, flags=flags, prefixes=(pp, ps) if external or not chain else None,
                           parents=par if chain else None)
        assert self.b.info.device_built == int(device)

    def decode(self):
        import torch
        self.b.decode_async(torch.cuda.current_stream().cuda_stream)
        self.status, self.length = self.b.results(torch.cuda.current_stream().cuda_stream)
        self.read_back()
        return self.status, self.length

    def read_back(self):
        d = self.D.download()
        self.out = [bytes(d[o:o + ln]) for o, ln in zip(self.do, self.length)]
        keep = np.ones(len(d), dtype=bool)
        for o, c in zip(self.do, self.chunks):
            keep[o:o + c.cap] = False
        assert (d[keep] == FILL).all(), "a byte outside the destinations was written"
        assert (self.P.download() == self.P.host).all(), "an external prefix or its slack changed"
        assert (self.S.download() == self.S.host).all(), "a source or its slack changed"

    def close(self):
        self.b.close()


def verify(chunks, st, ln, out, allowed=None):
    for i, c in enumerate(chunks):
        if allowed and i in allowed:
            assert st[i] in allowed[i] and ln[i] == 0, (i, st[i])
            continue
        assert st[i] == c.want, (i, st[i], c.want)
        if c.want == OK:
            assert ln[i] == len(c.record), i
            assert out[i] == c.record, i
        else:
            assert ln[i] == 0, i


def both(chunks, flags=0, levels=None, links=None, allowed=None):
    """The chunks through zd_batch_create_chain and zd_batch_create_device_chain,
    every chunk with its expected status and bytes, the two calls agreeing."""
    res = []
    for device in (False, True):
        r = Run(chunks, device, flags=flags)
        try:
            st, ln = r.decode()
            assert r.b.info.executors == 0
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
    return res[0]


# ---------------------------------------------------------------------------
# fixtures (built on the CPU; cached)
# ---------------------------------------------------------------------------
def line(base, n, seed, size_frac=100, dalign=(0, 0, 0), first=0, palign=0, checksum=False):
    """A line of n versions over the external prefix `base`: chunk `first` decodes against base, chunk first + k
    against chunk first + k - 1."""
    out, prev = [], base
    for k in range(n):
        rec = edit(prev, seed + k, size_frac)
        out.append(delta(rec, prev, parent=first + k - 1 if k else -1, external=k == 0, dalign=dalign[k % len(dalign)],
                         palign=palign, checksum=checksum))
        prev = rec
    return out


@functools.lru_cache(maxsize=None)
def case1(size):
    """Three lines of depth 3 over external bases of `size` bytes; the parents' destinations at alignments 1, 7, 15."""
    chunks = []
    for k, al in enumerate(((1, 7, 15), (7, 15, 1), (15, 1, 7))):
        base = gen.text(size + 64, seed=0xC1A0 + size + k)[:size] if size >= 64 else rnd(0xC1A0 + size + k, size)
        chunks += line(base, 3, 0xC1B0 + 16 * k + size, dalign=al, first=len(chunks), palign=3 * k + 1)
    return chunks


@functools.lru_cache(maxsize=None)
def case2():
    base = gen.text(PAGE, seed=0xC2A0)
    v = [edit(base, 0xC2A1)]
    v += [edit(v[0], 0xC2A2)]
    v += [edit(v[1], 0xC2A3)]
    # indices in reverse topological order: chunk 0 needs chunk 1 needs chunk 2 needs the external base
    chunks = [delta(v[2], v[1], parent=1, dalign=5), delta(v[1], v[0], parent=2, dalign=11),
              delta(v[0], base, external=True, dalign=9, palign=7)]
    chunks.append(plain(gen.text(3000, seed=0xC2B0)))                              # unrelated, no prefix
    hub = len(chunks)
    hub_rec = gen.text(PAGE, seed=0xC2C0)
    chunks.append(plain(hub_rec, dalign=13))                                       # a star: one parent ...
    chunks += [delta(edit(hub_rec, 0xC2D0 + k), hub_rec, parent=hub, dalign=k % 16) for k in range(64)]   # ... 64 children
    ext = gen.text(5000, seed=0xC2E0)
    chunks.append(delta(edit(ext, 0xC2E1), ext, external=True, palign=2))          # unrelated, an external prefix
    chunks.append(plain(rnd(0xC2F0, 700)))
    return chunks


@functools.lru_cache(maxsize=None)
def case3():
    n = 300 << 10
    old = gen.text(n, seed=0xC3A0)
    new = edit(old, 0xC3A1, 200)
    new = new[:5000] + rnd(0xC3A2, 3000) + new[5000:n - 3000]
    chunks = [plain(old, dalign=9), delta(new, old, parent=0, dalign=3)]            # 300 KiB against 300 KiB
    par = gen.text(200 << 10, seed=0xC3B0)
    head = rnd(0xC3B1, 128 << 10)                                                   # an incompressible first block
    chunks += [plain(par, dalign=1), delta(head + edit(par[:100 << 10], 0xC3B2), par, parent=2, dalign=7)]
    raw = rnd(0xC3C0, 200 << 10)                                                    # a parent of raw blocks only
    chunks += [plain(raw, dalign=15), delta(raw[5000:150000] + b"x" + raw[:3000], raw, parent=4, dalign=6)]
    return chunks


@functools.lru_cache(maxsize=None)
def case4(n=256):
    """A line of n chunks of 300 bytes, chunk k against chunk k - 1 (chunk 0: no prefix)."""
    rec = gen.text(300, seed=0xC4A0)
    chunks = [plain(rec, dalign=1)]
    for k in range(1, n):
        nxt = edit(rec, 0xC4B0 + k)
        chunks.append(delta(nxt, rec, parent=k - 1, dalign=k % 16))
        rec = nxt
    return chunks


def good_siblings(first, seed):
    base = gen.text(PAGE, seed=seed)
    return line(base, 3, seed + 1, dalign=(3, 8, 14), first=first, palign=5)


@functools.lru_cache(maxsize=None)
def corrupt_table(frame):
    """`frame` with the first one-bit flip that makes the oracle reject a table description."""
    for k in range(9, len(frame) - 4):
        for bit in range(8):
            bad = frame[:k] + bytes([frame[k] ^ (1 << bit)]) + frame[k + 1:]
            st = oracle.decompress_status(bad)[0]
            if st in (CORRUPTED_TABLE, LARGE_ACCURACY_LOG):
                return bad, st
    raise AssertionError("no flip gives a corrupted table in the oracle")


@functools.lru_cache(maxsize=None)
def case5(kind):
    """A good line, then parent / child / grandchild with a failing parent, then another good line."""
    checksum = kind == "checksum"
    chunks = good_siblings(0, 0xC5A0)
    p = len(chunks)
    rec = gen.text(PAGE, seed=0xC5B0)
    parent = plain(rec, checksum=checksum, dalign=7)
    if kind == "table":
        parent.frame, parent.want = corrupt_table(parent.frame)
        parent.against = None
    elif kind == "dst_cap":
        parent.cap, parent.want = len(rec) - 1, DST_TOO_SMALL
    else:
        f = bytearray(parent.frame)
        f[-1] ^= 0x10                                            # one bit of the stored Content_Checksum
        parent.frame, parent.want, parent.against = bytes(f), CHECKSUM_WRONG, None
    c1 = edit(rec, 0xC5B1)
    c2 = edit(c1, 0xC5B2)
    chunks += [parent, delta(c1, rec, parent=p, want=NOT_DECODED, checksum=checksum, dalign=2),
               delta(c2, c1, parent=p + 1, want=NOT_DECODED, checksum=checksum, dalign=12)]
    chunks += good_siblings(len(chunks), 0xC5C0)
    # a second child of the failing parent, behind everything else
    chunks.append(delta(edit(rec, 0xC5B3), rec, parent=p, want=NOT_DECODED, checksum=checksum))
    return chunks


@functools.lru_cache(maxsize=None)
def case6():
    rec = gen.text(PAGE, seed=0xC6A0)
    parent = plain(rec, content_size=False, dalign=4)
    child = delta(edit(rec, 0xC6A1), rec, parent=0, want=OUT_OF_DOMAIN)
    return [parent, child, plain(gen.text(2000, seed=0xC6A2))]


def skippable(payload):
    return b"\x50\x2a\x4d\x18" + payload.to_bytes(4, "little") + bytes((7 * i + 3) & 0xFF for i in range(payload))


@functools.lru_cache(maxsize=None)
def case7():
    a, b = gen.text(4000, seed=0xC7A0), gen.text(PAGE, seed=0xC7A1)
    return [Chunk(b"", b"", cap=0), plain(a, parent=0, dalign=3),                   # an empty parent chunk
            Chunk(skippable(40), b"", cap=0), plain(b, parent=2, dalign=9),         # a parent of one skippable frame
            delta(edit(b, 0xC7A2), b, parent=3)]                                    # and a child of that child


@functools.lru_cache(maxsize=None)
def case8():
    """Entries that the device call refuses chunk by chunk (the host call refuses the batch)."""
    rec = gen.text(PAGE, seed=0xC8A0)
    n = 10
    ext = gen.text(600, seed=0xC8A1)
    mk = lambda seed, **kw: delta(edit(rec, seed), rec, **kw)
    return [plain(rec, dalign=5),                                                   # 0: a good root
            mk(0xC8B1, parent=n, want=INVALID_ARG),                                 # 1: parent n
            mk(0xC8B2, parent=1, want=NOT_DECODED),                                 # 2: its child
            mk(0xC8B3, parent=-2, want=INVALID_ARG),                                # 3: parent -2
            mk(0xC8B4, parent=4, want=INVALID_ARG),                                 # 4: its own parent
            mk(0xC8B5, parent=6, want=INVALID_ARG),                                 # 5, 6: a 2-cycle
            mk(0xC8B6, parent=5, want=INVALID_ARG),
            Chunk(mk(0xC8B7).frame, edit(rec, 0xC8B7), parent=0, prefix=ext, want=INVALID_ARG, against=rec),   # 7: a prefix size on a chained chunk
            mk(0xC8B8, parent=0, dalign=11),                                        # 8: a good child of the root
            plain(gen.text(900, seed=0xC8B9))]                                      # 9: unrelated


@functools.lru_cache(maxsize=None)
def case9():
    """Prefix-batch chunks only (every parent -1): external prefixes and plain chunks."""
    chunks = []
    for k in range(24):
        base = gen.text(PAGE, seed=0xC9A0 + k)
        chunks.append(delta(edit(base, 0xC9B0 + k), base, external=True, palign=k % 16, dalign=(5 * k) % 16))
    chunks.append(plain(gen.text(3000, seed=0xC9C0)))
    return chunks


def test_fixtures_are_known_good():
    """No GPU: every fixture builds and every intact link decodes through libzstd with its parent's record."""
    sets = [case1(s) for s in (PAGE, 1, 15, 16, 17, 300)]
    sets += [case2(), case3(), case4(), case4(257), case6(), case7(), case9()]
    sets += [case5(k) for k in ("table", "dst_cap", "checksum")]
    for chunks in sets:
        check_links_on_the_cpu(chunks)
    # case 8's chunks carry entries no batch accepts; their frames are links of the root's record all the same
    c8 = case8()
    for c in c8[1:9]:
        assert zdict.prefix_decompress(c.frame, c8[0].record, PAGE) == c.record
    # what the cases are about
    from zstd_decompressor import batch
    c3 = case3()
    _, blocks, st, _ = batch.frames_index(c3[3].frame)
    assert st == 0 and blocks[0]["type"] == 0 and any(b["type"] == 2 for b in blocks)     # a raw first block, then compressed ones
    _, blocks, st, _ = batch.frames_index(c3[4].frame)
    assert st == 0 and len(blocks) >= 2 and all(b["type"] == 0 for b in blocks)           # a parent of raw blocks only
    _, blocks, st, _ = batch.frames_index(c3[1].frame)
    assert st == 0 and len(blocks) >= 3                                                   # 300 KiB: three blocks at least
    assert libzstd.frame_content_size(case6()[0].frame) == (1 << 64) - 1                  # ZSTD_CONTENTSIZE_UNKNOWN
    assert libzstd.frame_content_size(case6()[1].frame) == PAGE
    for kind in ("table", "dst_cap", "checksum"):
        c5 = case5(kind)
        assert [c.want for c in c5] == [0, 0, 0, c5[3].want, NOT_DECODED, NOT_DECODED, 0, 0, 0, NOT_DECODED]
        assert c5[3].want != 0
    # the flipped checksum is the frame's last byte and nothing else: libzstd refuses that frame alone
    bad = case5("checksum")[3]
    with pytest.raises(RuntimeError):
        libzstd.decompress_frame(bad.frame, PAGE)
    # the children need their parents: none of them decodes alone
    for c in case1(PAGE) + case2()[:3]:
        with pytest.raises(RuntimeError):
            libzstd.decompress_frame(c.frame, len(c.record))


# ---------------------------------------------------------------------------
# 1. lines of depth 3 over an external base
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("size", [PAGE, 1, 15, 16, 17, 300])
def test_lines_of_depth_3(size):
    both(case1(size), levels=3, links=6)


# ---------------------------------------------------------------------------
# 2. any order, a star, unrelated chunks beside the chains
# ---------------------------------------------------------------------------
@gpu
def test_reverse_order_star_and_unrelated_chunks():
    both(case2(), levels=3, links=2 + 64)


# ---------------------------------------------------------------------------
# 3. multi-block links
# ---------------------------------------------------------------------------
@gpu
def test_multi_block_links():
    both(case3(), levels=2, links=3)


# ---------------------------------------------------------------------------
# 4. the deepest line
# ---------------------------------------------------------------------------
@gpu
def test_a_line_of_256_decodes():
    both(case4(), levels=256, links=255)


@gpu
def test_the_257th_of_a_line_is_refused_by_the_device_call():
    from zstd_decompressor import _lib
    chunks = case4(257)
    r = Run(chunks, True)
    try:
        st, ln = r.decode()
        assert st[:256] == [0] * 256 and st[256] == INVALID_ARG and ln[256] == 0
        assert all(r.out[i] == chunks[i].record for i in range(256))
        assert r.b.chain_info == (256, 255)
    finally:
        r.close()
    with pytest.raises(_lib.ZdError) as e:
        Run(chunks, False)
    assert e.value.code == INVALID_ARG


# ---------------------------------------------------------------------------
# 5. failing parents: child and grandchild are not decoded, the siblings are bit-exact
# ---------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("kind", ["table", "dst_cap", "checksum"])
def test_failing_parent(kind):
    chunks = case5(kind)
    st, ln, out, _, _ = both(chunks, flags=F_VERIFY_CHECKSUM if kind == "checksum" else 0, levels=3)
    assert st[3] == chunks[3].want and st[4] == st[5] == st[9] == NOT_DECODED


@gpu
def test_without_verification_the_flipped_checksum_fails_nothing():
    chunks = case5("checksum")
    for device in (False, True):
        r = Run(chunks, device)
        try:
            st, ln = r.decode()
            assert st == [0] * len(chunks)
            assert all(o == c.record for o, c in zip(r.out, chunks))
        finally:
            r.close()


# ---------------------------------------------------------------------------
# 6. a parent without Frame_Content_Size
# ---------------------------------------------------------------------------
@gpu
def test_parent_without_content_size():
    both(case6(), levels=2, links=1)


# ---------------------------------------------------------------------------
# 7. parents that decode to nothing
# ---------------------------------------------------------------------------
@gpu
def test_empty_parents():
    both(case7(), levels=3, links=3)


# ---------------------------------------------------------------------------
# 8. the device call's per-chunk errors
# ---------------------------------------------------------------------------
@gpu
def test_device_per_chunk_errors():
    from zstd_decompressor import _lib
    chunks = case8()
    r = Run(chunks, True)
    try:
        st, ln = r.decode()
        verify(chunks, st, ln, r.out)
        assert r.b.info.prefix_bytes_total == 0          # the refused chunk's prefix is not kept
        # links: chunk 2 (behind a refused chunk, not refused itself) and chunk 8
        assert r.b.chain_info == (2, 2)
    finally:
        r.close()
    with pytest.raises(_lib.ZdError) as e:
        Run(chunks, False)
    assert e.value.code == INVALID_ARG


# ---------------------------------------------------------------------------
# 9. no parents at all: a prefix batch; relaunch; graph capture
# ---------------------------------------------------------------------------
@gpu
def test_without_parents_it_is_a_prefix_batch():
    chunks = case9()
    want = None
    for device in (False, True):
        for chain in (False, True):
            r = Run(chunks, device, chain=chain)
            try:
                got = []
                for _ in range(2 if chain else 1):                 # launching twice gives the same result
                    r.D.t.fill_(FILL)
                    st, ln = r.decode()
                    got.append((st, ln, r.out))
                assert got[0] == got[-1]
                if chain:
                    assert r.b.chain_info == (1, 0)
                verify(chunks, *got[0])
                want = want or got[0]
                assert got[0] == want, (device, chain)
            finally:
                r.close()


@gpu
@pytest.mark.parametrize("links", [False, True])
def test_graph_capture_replay(links):
    """One decode captured in a graph and replayed: a batch without parents, and one with chains (a launch a level)."""
    import torch
    if links:
        chunks = case1(PAGE) + case7()
        off = len(case1(PAGE))
        chunks = chunks[:off] + [Chunk(c.frame, c.record, parent=c.parent + off if c.parent >= 0 else -1,
                                       prefix=c.prefix, cap=c.cap, dalign=c.dalign, against=c.against)
                                 for c in chunks[off:]]
    else:
        chunks = case9()
    dev = torch.device("cuda", 0)
    for device in (False, True):
        r = Run(chunks, device)
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
                verify(chunks, r.status, r.length, r.out)
            del g
        finally:
            r.close()


# ---------------------------------------------------------------------------
# 10. decode_tensors(parents=...)
# ---------------------------------------------------------------------------
@gpu
def test_decode_tensors_with_parents():
    import torch
    from zstd_decompressor import decode_tensors
    dev = torch.device("cuda", 0)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    chunks = case1(PAGE)
    srcs = [up(c.frame) for c in chunks]
    dsts = [torch.zeros(c.cap, dtype=torch.uint8, device=dev) for c in chunks]
    pfx = [up(c.prefix) if c.prefix else None for c in chunks]
    st, ln = decode_tensors(srcs, dsts, prefixes=pfx, parents=[c.parent for c in chunks])
    assert st == [0] * len(chunks) and ln == [len(c.record) for c in chunks]
    assert all(bytes(d.cpu().numpy().tobytes()) == c.record for d, c in zip(dsts, chunks))
    assert all(bytes(p.cpu().numpy().tobytes()) == c.prefix for p, c in zip(pfx, chunks) if p is not None)
    with pytest.raises(ValueError):
        decode_tensors(srcs, dsts, prefixes=pfx, parents=[-1])
