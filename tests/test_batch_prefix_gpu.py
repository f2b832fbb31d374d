"""Prefix batches on the GPU (include/zd.h zd_batch_create_prefix /
zd_batch_create_device_prefix, Batch(prefixes=...), zd_k_execute_prefix): chunk
i decodes against its own caller-owned device buffer, read where it lies.

Expected bytes are always the original record AND corpus.zdict.prefix_decompress
(ZSTD_DCtx_refPrefix + ZSTD_decompressDCtx) of the same frame with the same
prefix; a chunk that must fail has one exact expected status.

Layout of every test (class Arena): the prefixes, the sources and the
destinations are carved out of the interior of three single device tensors
filled with 0xA5, with at least 64 bytes of slack on every side of every range,
each range at the 16-byte alignment the test names.  These tests check bytes,
not bounds, so nothing here can fault: after every decode the slack of all three
tensors, the prefixes and the sources are compared with what was uploaded.
Every case runs through both creation calls (host arrays / device arrays)."""
import functools
import os
import re

import numpy as np
import pytest

from corpus import gen, libzstd, zdict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
SLACK = 64
DICT_MAGIC = bytes.fromhex("37a430ec")


def rnd(seed, n):
    return np.random.default_rng(seed).integers(0, 256, n, dtype=np.uint8).tobytes()


# ---------------------------------------------------------------------------
# the harness
# ---------------------------------------------------------------------------
class Arena:
    """Ranges inside one uint8 tensor filled with FILL: place(data or size,
    align) gives the range's offset, with offset % 16 == (align + shift) % 16
    (the tensor's base is 256-byte aligned; shift moves every range of the
    arena by that many bytes) and SLACK bytes of FILL before and after it."""

    def __init__(self, shift=0):
        self.at = 256
        self.shift = shift
        self.items = []            # (offset, bytes or None, size)

    def place(self, data, align=0, size=None):
        n = len(data) if data is not None else size
        o = self.at + SLACK
        o += (align + self.shift - o) % 16
        self.items.append((o, data, n))
        self.at = o + n
        return o

    def upload(self):
        import torch
        total = self.at + SLACK + 256
        host = np.full(total, FILL, dtype=np.uint8)
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
    def __init__(self, frame, prefix=None, cap=None, record=None, palign=0, dalign=0, null_prefix_size=0):
        self.frame, self.prefix, self.cap, self.record = frame, prefix, cap, record
        self.palign, self.dalign, self.null_prefix_size = palign, dalign, null_prefix_size
        if cap is None:
            self.cap = len(record)


class Run:
    """The chunks laid out on the device and one batch over them."""

    def __init__(self, chunks, device, flags=0, with_prefixes=True, shift=0):
        import torch
        from zstd_decompressor import Batch
        self.chunks, n = chunks, len(chunks)
        self.P, self.S, self.D = Arena(shift), Arena(), Arena()
        po = [self.P.place(c.prefix, c.palign) if c.prefix else None for c in chunks]
        so = [self.S.place(c.frame, (3 * i) % 16) for i, c in enumerate(chunks)]
        # destinations in a shuffled order, so the lowest address is not chunk 0's
        order = np.random.default_rng(n).permutation(n)
        do = [None] * n
        for i in order:
            do[i] = self.D.place(None, chunks[i].dalign, size=chunks[i].cap)
        pb, sb, db = self.P.upload(), self.S.upload(), self.D.upload()
        self.do = do
        self.po = po
        sp = [sb + o for o in so]
        ss = [len(c.frame) for c in chunks]
        dp = [db + o for o in do]
        dc = [c.cap for c in chunks]
        pp = [pb + o if o is not None else 0 for o in po]
        ps = [len(c.prefix) if c.prefix else c.null_prefix_size for c in chunks]
        self.prefix_total = sum(len(c.prefix) for c in chunks if c.prefix)
        if device:
            dev = torch.device("cuda", 0)
            arr = [torch.tensor(v, dtype=torch.int64, device=dev) for v in (sp, ss, dp, dc, pp, ps)]
            torch.cuda.synchronize()
            self.b = Batch.from_device(*arr[:4], flags=flags, prefixes=(arr[4], arr[5]) if with_prefixes else None)
        else:
            self.b = Batch(sp, ss, dp, dc, flags=flags, prefixes=(pp, ps) if with_prefixes else None)
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
        # nothing written outside the destinations; prefixes and sources untouched
        keep = np.ones(len(d), dtype=bool)
        for o, c in zip(self.do, self.chunks):
            keep[o:o + c.cap] = False
        assert (d[keep] == FILL).all(), "a byte outside the destinations was written"
        assert (self.P.download() == self.P.host).all(), "a prefix or its slack changed"
        assert (self.S.download() == self.S.host).all(), "a source or its slack changed"

    def close(self):
        self.b.close()


def both(chunks, flags=0, shift=0):
    """The chunks through zd_batch_create_prefix and zd_batch_create_device_prefix:
    [(statuses, lengths, outputs, info)], the two agreeing on all of it."""
    res = []
    for device in (False, True):
        r = Run(chunks, device, flags=flags, shift=shift)
        try:
            st, ln = r.decode()
            assert r.b.info.executors == 0
            assert r.b.info.prefix_bytes_total == r.prefix_total
            res.append((st, ln, r.out))
        finally:
            r.close()
    assert res[0] == res[1], "the host-array and the device-array batch differ"
    return res[0]


def expect_all_ok(chunks, flags=0, shift=0):
    st, ln, out = both(chunks, flags, shift)
    assert st == [0] * len(chunks), [(i, s) for i, s in enumerate(st) if s]
    for i, c in enumerate(chunks):
        assert ln[i] == len(c.record), i
        assert out[i] == c.record, i


def delta(record, prefix, level=3, checksum=False, content_size=True, **kw):
    """A chunk: `record` compressed against `prefix`; libzstd with the prefix gives the record back."""
    frame = zdict.prefix_compress(record, prefix, level, checksum, content_size)
    assert zdict.prefix_decompress(frame, prefix, len(record)) == record
    return Chunk(frame, prefix, record=record, **kw)


def needs_its_prefix(frame, size):
    try:
        libzstd.decompress_frame(frame, size)
    except RuntimeError:
        return True
    return False


# ---------------------------------------------------------------------------
# 1. page deltas
# ---------------------------------------------------------------------------
PAGE = 16 << 10


@functools.lru_cache(maxsize=None)
def pages(n=256):
    """n seeded text pages of 16 KiB, each with 1 % of its bytes edited: (old, new, positions edited)."""
    text = gen.text(n * PAGE + PAGE, seed=0x9A6E)
    rng = np.random.default_rng(0x9A6F)
    out = []
    for i in range(n):
        old = text[i * PAGE:(i + 1) * PAGE]
        new = bytearray(old)
        at = np.sort(rng.choice(PAGE, PAGE // 100, replace=False))
        for p in at:
            new[p] ^= int(rng.integers(1, 256))
        out.append((old, bytes(new), at))
    return out


@functools.lru_cache(maxsize=None)
def page_chunks(checksum=False, n=256):
    return [delta(new, old, 3, checksum, palign=i % 16, dalign=(5 * i) % 16)
            for i, (old, new, _) in enumerate(pages()[:n])]


def test_page_deltas():
    chunks = page_chunks()
    assert sum(len(c.frame) for c in chunks) * 8 < 256 * PAGE          # deltas: far smaller than the pages
    expect_all_ok(chunks)
    # the same sources without their prefixes: no chunk decodes
    alone = [needs_its_prefix(c.frame, PAGE) for c in chunks]
    assert all(alone) and len(alone) == 256
    for device in (False, True):
        r = Run(chunks, device, with_prefixes=False)
        try:
            st, ln = r.decode()
            assert all(s != 0 for s in st) and ln == [0] * 256
        finally:
            r.close()


# ---------------------------------------------------------------------------
# 2. edges: prefix sizes around the 16-byte pieces, the window and far beyond it
# ---------------------------------------------------------------------------
EDGE_K = (15, 16, 17, 31, 32, 33, 63, 64, 100, 4095, 4096, 4097, 70000)


@functools.lru_cache(maxsize=None)
def edge_records():
    out = []
    for K in EDGE_K:
        P = rnd(0xED6E00 + K, K)
        tail = (P[-min(K, 100):] * (1500 // min(K, 100) + 1))[:1500]
        h = P[:min(K, 64)]
        head = h + rnd(0xED6F00 + K, 40) + h
        whole = P + b"xyz" + P if K != 70000 else P[1000:3000] + b"xyz" + P[-3000:]
        out += [(P, tail), (P, head), (P, whole)]
    return out


@pytest.mark.parametrize("shift", range(16))
def test_edges(shift):
    recs = edge_records()
    assert len(recs) == 39
    chunks = [delta(r, P, dalign=(7 * i) % 16) for i, (P, r) in enumerate(recs)]
    # (a precondition, not a skip: every one of these frames reaches into its prefix)
    assert all(needs_its_prefix(c.frame, len(c.record)) for c in chunks)
    expect_all_ok(chunks, shift=shift)


def test_periods_across_the_boundary():
    """64 frames whose records repeat their own 5000-byte prefix's last k bytes:
    pieces that begin before the boundary at every alignment, periods below 16."""
    chunks = []
    for i in range(64):
        k = (1, 7, 15, 16, 17, 33, 100)[i % 7]
        P = rnd(0x9E810D00 + i, 5000)
        chunks.append(delta((P[-k:] * (3200 // k + 1))[:200 + 47 * i], P, palign=i % 16, dalign=(3 * i) % 16))
    expect_all_ok(chunks)


# ---------------------------------------------------------------------------
# 3. tiny prefixes, 1..14 bytes
# ---------------------------------------------------------------------------
def test_tiny_prefixes_libzstd_frames():
    chunks = []
    for K in range(1, 15):
        P = rnd(0x7191 + K, K)
        rec = (P * 40)[:300] + rnd(0x7192 + K, 30) + P * 3
        chunks.append(delta(rec, P, palign=(K * 5) % 16, dalign=K))
    expect_all_ok(chunks)


LL_DIST = [4, 3, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 2, 1, 1, 1, 2, 2, 2, 2, 2, 2, 2, 2, 2, 3, 2, 1, 1, 1, 1, 1,
           -1, -1, -1, -1]
OF_DIST = [1, 1, 1, 1, 1, 1, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1]
ML_DIST = [1, 4, 3, 2, 2, 2, 2, 2, 2, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1,
           1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, -1, -1, -1, -1, -1, -1, -1]


def spread_symbols(al, dist):
    """The symbol of every state of an FSE table (RFC 8878 4.1.1; the serial
    construction of tests/test_fse_spread.py)."""
    T = 1 << al
    zero_pos, sym = T, [None] * T
    for s, c in enumerate(dist):
        if c == -1:
            zero_pos -= 1
            sym[zero_pos] = s
    pos, step, mask = 0, (T >> 1) + (T >> 3) + 3, T - 1
    for s, c in enumerate(dist):
        for _ in range(max(c, 0)):
            sym[pos] = s
            pos = (pos + step) & mask
            while pos >= zero_pos:
                pos = (pos + step) & mask
    return sym


def ml_code(ml):
    """(code, extra value, extra bits) of a match length (RFC 8878 3.1.1.3.2.1.1)."""
    if ml < 35:
        return ml - 3, 0, 0
    base = [(32, 35, 1), (33, 37, 1), (34, 39, 1), (35, 41, 1), (36, 43, 2), (37, 47, 2), (38, 51, 3), (39, 59, 3)]
    for code, b, bits in base:
        if b <= ml < b + (1 << bits):
            return code, ml - b, bits
    raise ValueError(ml)


def hand_frame(K, lits):
    """One frame of one compressed block: Raw literals `lits` (5 bytes), one
    sequence in Predefined mode -- literal length 5, offset 5 + K (prefix byte
    0), match length 3 K + 7: the copy runs through the K prefix bytes and the
    literals into the match's own bytes."""
    assert len(lits) == 5
    ml, off = 3 * K + 7, 5 + K
    ov = off + 3
    ofc = ov.bit_length() - 1
    mlc, mlx, mlb = ml_code(ml)
    st_ll = spread_symbols(6, LL_DIST).index(5)          # literal length 5: code 5, no extra bits
    st_of = spread_symbols(5, OF_DIST).index(ofc)
    st_ml = spread_symbols(6, ML_DIST).index(mlc)
    acc, nb = 0, 0
    # written in the reverse of the order they are read: the extra bits (read OF, ML, LL),
    # then the initial states (read LL, OF, ML), then the end mark
    for v, n in ((0, 0), (mlx, mlb), (ov - (1 << ofc), ofc), (st_ml, 6), (st_of, 5), (st_ll, 6), (1, 1)):
        acc |= v << nb
        nb += n
    bits = acc.to_bytes((nb + 7) // 8, "little")
    block = bytes([5 << 3]) + lits + bytes([1, 0]) + bits
    content = 5 + ml
    assert content < 256
    hdr = (1 | (2 << 1) | (len(block) << 3)).to_bytes(3, "little")
    return bytes.fromhex("28b52ffd") + bytes([0x20, content]) + hdr + block


@pytest.mark.parametrize("K", [1, 2, 8, 14])
def test_tiny_prefixes_hand_assembled(K):
    P = rnd(0x4A9D + K, K)
    lits = rnd(0x4A9E + K, 5)
    frame = hand_frame(K, lits)
    n = 5 + 3 * K + 7
    want = zdict.prefix_decompress(frame, P, n)          # libzstd accepts the frame: its output is the expectation
    hist = bytearray(P + lits)
    for j in range(3 * K + 7):
        hist.append(hist[j])                              # offset 5 + K from position K + 5: prefix byte 0 onwards
    assert want == bytes(hist[K:]) and len(want) == n
    assert needs_its_prefix(frame, n)
    chunks = [Chunk(frame, P, record=want, palign=a, dalign=(a + K) % 16) for a in range(16)]
    expect_all_ok(chunks)


# ---------------------------------------------------------------------------
# 4. sources far into the prefix (past K4's LDS window)
# ---------------------------------------------------------------------------
def test_far_sources():
    rng = np.random.default_rng(0xFA45)
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
    assert sum(len(c.frame) for c in chunks) * 10 < sum(len(c.record) for c in chunks)
    expect_all_ok(chunks)


# ---------------------------------------------------------------------------
# 5. multi-block frames, and a frame without Frame_Content_Size
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_pair():
    n = 300 << 10
    old = gen.text(n, seed=0xB16)
    new = bytearray(old)
    rng = np.random.default_rng(0xB17)
    for p in rng.choice(n, n // 200, replace=False):
        new[p] ^= 0x55
    return old, bytes(new[:5000] + rnd(0xB18, 3000) + new[5000:n - 3000])


@pytest.mark.parametrize("level", [1, 19])
def test_multi_block(level):
    old, new = big_pair()
    c = delta(new, old, level, palign=9, dalign=3)
    assert len(c.frame) * 4 < len(new)
    expect_all_ok([c, delta(new[:1000], old[:700], level)])


def test_frame_without_content_size_decodes_in_place():
    old, new = big_pair()
    c = delta(new, old, 3, content_size=False, palign=1, dalign=15)
    assert libzstd.frame_content_size(c.frame) == (1 << 64) - 1      # ZSTD_CONTENTSIZE_UNKNOWN
    expect_all_ok([c])


# ---------------------------------------------------------------------------
# 6. a prefix that starts with the dictionary magic is raw content
# ---------------------------------------------------------------------------
def test_prefix_starting_with_the_dictionary_magic():
    P = DICT_MAGIC + rnd(0x3A61C, 4000)
    with pytest.raises(RuntimeError):
        zdict.compress(b"x" * 100, P)                                 # "Dictionary is corrupted": not a prefix
    rec = P[:1500] + b"--" + P[2000:3500] + P[:4]
    c = delta(rec, P, palign=5, dalign=2)
    assert needs_its_prefix(c.frame, len(rec))
    expect_all_ok([c])


# ---------------------------------------------------------------------------
# 7. statuses: one batch, the neighbours ZD_OK with the right bytes
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def trained():
    text = gen.text(256 * 4096, seed=0x57A7)
    d = zdict.train([text[i:i + 4096] for i in range(0, len(text), 4096)], 16 << 10)
    assert zdict.dict_id(d) != 0
    return d


def test_statuses_one_batch():
    from zstd_decompressor import _lib
    P5 = rnd(0x57A0, 5000)
    good = lambda i: delta((P5[100 * i:100 * i + 900] + bytes([i]) * 7) * 2, P5, palign=i, dalign=2 * i)
    plain_rec = gen.text(3000, seed=0x57A1)
    plain = Chunk(libzstd.compress(plain_rec, 3), None, record=plain_rec)                  # no prefix, NULL address
    with_id = Chunk(zdict.compress(plain_rec, trained(), 3), P5, record=plain_rec)
    far_rec = P5[:1200] + b"+" + P5[200:900]
    far = delta(far_rec, P5)
    short = Chunk(far.frame, P5[-1000:], record=far_rec)                                  # only the last 1000 bytes
    g = good(9)
    truncated = Chunk(g.frame[:-3], P5, cap=len(g.record), record=g.record)
    g2 = good(10)
    one_short = Chunk(g2.frame, P5, cap=len(g2.record) - 1, record=g2.record)
    # (what the walk says of the truncated chunk: the same bytes as a chunk of a plain batch)
    chunks = [good(0), plain, good(1), with_id, good(2), short, good(3), truncated, good(4), one_short, good(5)]
    want = {1: 0, 3: _lib.DICT_MISMATCH, 5: _lib.IMPOSSIBLE_VALUE, 9: _lib.DST_TOO_SMALL}
    st, ln, out = both(chunks)
    for i, c in enumerate(chunks):
        if i == 7:
            assert st[i] != 0 and ln[i] == 0
            continue
        assert st[i] == want.get(i, 0), (i, st[i])
        if st[i] == 0:
            assert ln[i] == len(c.record) and out[i] == c.record, i
        else:
            assert ln[i] == 0, i
    # the truncated chunk's status is the walk's: what a plain batch gives the same bytes
    r = Run([truncated], False, with_prefixes=False)
    try:
        walk_status = r.decode()[0][0]
    finally:
        r.close()
    assert walk_status != 0 and st[7] == walk_status


def test_null_prefix_with_a_size_fails_its_chunk_in_the_device_call():
    from zstd_decompressor import _lib
    P = rnd(0x57B0, 3000)
    a, b = delta(P[:2000] + b"a", P), delta(P[500:2500] + b"b", P, palign=3)
    plain_rec = gen.text(2000, seed=0x57B1)
    bad = Chunk(libzstd.compress(plain_rec, 3), None, record=plain_rec, null_prefix_size=100)
    r = Run([a, bad, b], True)
    try:
        st, ln = r.decode()
        assert st == [0, _lib.INVALID_ARG, 0] and ln == [len(a.record), 0, len(b.record)]
        assert r.out[0] == a.record and r.out[2] == b.record
        assert r.b.info.prefix_bytes_total == 6000
    finally:
        r.close()
    # the host-array call refuses the whole batch for it
    with pytest.raises(_lib.ZdError) as e:
        Run([a, bad, b], False)
    assert e.value.code == _lib.INVALID_ARG


# ---------------------------------------------------------------------------
# 8. prefixes are read at decode time; verification inside the launch
# ---------------------------------------------------------------------------
def test_prefixes_are_read_by_the_launch_and_verified():
    from zstd_decompressor import _lib
    chunks = page_chunks(True, 64)
    old, new, edited = pages()[7]
    # a byte of prefix 7 inside a matched region: no edit within 32 bytes of it
    gaps = np.diff(edited)
    k = int(np.argmax(gaps))
    assert gaps[k] > 80
    pos = int(edited[k]) + int(gaps[k]) // 2
    for device in (False, True):
        r = Run(chunks, device, flags=_lib.F_VERIFY_CHECKSUM)
        try:
            st, ln = r.decode()
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


# ---------------------------------------------------------------------------
# 9. graph capture
# ---------------------------------------------------------------------------
def test_hip_graph_capture_replay():
    import torch
    chunks = page_chunks()[:64]
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
                assert r.status == [0] * 64
                assert all(o == c.record for o, c in zip(r.out, chunks))
            del g
        finally:
            r.close()


# ---------------------------------------------------------------------------
# 10. mutations
# ---------------------------------------------------------------------------
def test_mutated_sources_between_untouched_ones():
    header = open(os.path.join(ROOT, "include", "zd.h")).read()
    documented = {0} | {int(v) for v in re.findall(r"^#define\s+ZD_E_\w+\s+\((-\d+)\)", header, re.M)}
    base = page_chunks()
    rng = np.random.default_rng(0x3077)
    chunks = []
    for i in range(256):
        c = base[i]
        f = bytearray(c.frame)
        f[int(rng.integers(0, len(f)))] ^= int(rng.integers(1, 256))
        chunks.append(Chunk(bytes(f), c.prefix, cap=PAGE, record=None, palign=c.palign, dalign=c.dalign))
        chunks.append(c)
    st, ln, out = both(chunks)                 # (the run completes; nothing outside the destinations: Run.read_back)
    for i in range(0, 512, 2):
        assert st[i] in documented, (i, st[i])
        assert ln[i] <= PAGE and (st[i] == 0 or ln[i] == 0), i
        assert st[i + 1] == 0 and out[i + 1] == chunks[i + 1].record, i + 1


# ---------------------------------------------------------------------------
# 11. decode_tensors(prefixes=...) and the command line
# ---------------------------------------------------------------------------
def test_decode_tensors_with_a_none_entry():
    import torch
    from zstd_decompressor import decode_tensors
    dev = torch.device("cuda", 0)
    up = lambda b: torch.frombuffer(bytearray(b), dtype=torch.uint8).to(dev)
    old, new, _ = pages()[3]
    plain_rec = gen.text(5000, seed=0x11A)
    srcs = [up(zdict.prefix_compress(new, old)), up(libzstd.compress(plain_rec, 3))]
    dsts = [torch.zeros(len(new), dtype=torch.uint8, device=dev), torch.zeros(5000, dtype=torch.uint8, device=dev)]
    pfx = up(old)
    st, ln = decode_tensors(srcs, dsts, prefixes=[pfx, None])
    assert st == [0, 0] and ln == [len(new), 5000]
    assert bytes(dsts[0].cpu().numpy().tobytes()) == new and bytes(dsts[1].cpu().numpy().tobytes()) == plain_rec
    assert bytes(pfx.cpu().numpy().tobytes()) == old
    with pytest.raises(ValueError):
        decode_tensors(srcs, dsts, prefixes=[pfx])


def test_cli_patch_from(tmp_path, capsys):
    from zstd_decompressor.__main__ import main
    old, new, _ = pages()[5]
    (tmp_path / "new.zst").write_bytes(zdict.prefix_compress(new, old))
    (tmp_path / "old").write_bytes(old)
    (tmp_path / "wrong").write_bytes(old[:4000])
    out = tmp_path / "out"
    assert main([str(tmp_path / "new.zst"), "--patch-from", str(tmp_path / "old"), "-o", str(out)]) == 0
    assert out.read_bytes() == new
    assert main([str(tmp_path / "new.zst"), "--patch-from", str(tmp_path / "wrong"), "-o", str(out)]) != 0
    assert "ImpossibleValue" in capsys.readouterr().err
    assert main([str(tmp_path / "new.zst"), "--patch-from", str(tmp_path / "old"), "-D", str(tmp_path / "old")]) != 0
