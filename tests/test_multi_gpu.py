"""Multi-frame batches on the device (include/zd.h zd_multi_*; MultiFrameBatch,
decode_multi, chunk_sizes(multi_frame=True)): zd_k_multi_count, the scans,
zd_k_multi_fill, the inner device-built batch, zd_k_multi_join and
zd_k_multi_copy, and zd_k_multi_sizes.

Expected bytes are the source data's slices.  Expected statuses are those of
the CPU oracle on each sub-chunk alone -- the test assembled the parts, so it
knows where the rule of include/zd.h cuts (`split`) -- and a chunk's expected
status is the first that is not 0; every test first asserts that its good parts
are ZD_OK on the oracle with the source's bytes.  Two places where assembly
does not say where the rule cuts: a frame cut by three bytes in front of other
frames walks on into their bytes, so the host index (zd_frames_index) names the
frames that walk to their end there; and a frame of no bytes is one Raw block
of size 0, EmptySlice on the oracle as in the reference, so it stops the walk
and the chunk that ends with it is expected to fail with that status.  The counts a batch reports
(frames, staged frames, staged bytes, copy pieces) are computed here from the
parts by that rule: a sub-chunk is in place while every sub-chunk before it
carries a Frame_Content_Size, every one behind the first without it is staged
with its reserve rounded up to 16 (the reserve of a frame without the field:
128 KiB a compressed block + its raw and RLE blocks' sizes).

Layout of every test: each source at an odd device address, ending at its
tensor's last byte; the destinations at odd addresses inside one tensor filled
with 0xA5, 32 guard bytes between them; after every decode every byte outside
the delivered ranges (a failed chunk: outside its destination) is 0xA5.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from corpus import gen, libzstd, zdict
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dict")
FILL, GUARD, PIECE, K = 0xA5, 32, 32 << 10, 128 << 10
OK, NEB, NEBITS, EMPTY_SLICE, RBT, MAGIC = 0, -1, -2, -6, -50, -60
DST_TOO_SMALL, INVALID_ARG, OUT_OF_DOMAIN, CHECKSUM_WRONG = -92, -93, -91, -100


# --------------------------------------------------------------------------
# parts and the rule
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def expect(sub: bytes):
    """(status, bytes) of one sub-chunk alone on the CPU oracle; a failing one has no bytes."""
    st, out = oracle.decompress_status(sub)
    return st, (out if st == 0 else b"")


def header_len(frame: bytes) -> int:
    fhd = frame[4]
    single, fcs, did = (fhd >> 5) & 1, fhd >> 6, fhd & 3
    return 5 + (0 if single else 1) + (0, 1, 2, 4)[did] + ((1 if single else 0) if fcs == 0 else 1 << fcs)


def has_fcs(frame: bytes) -> bool:
    return bool((frame[4] >> 5) & 1) or (frame[4] >> 6) != 0


def fcs_value(frame: bytes) -> int:
    fhd = frame[4]
    single, fcs = (fhd >> 5) & 1, fhd >> 6
    size = (1 if single else 0) if fcs == 0 else 1 << fcs
    at = header_len(frame) - size
    return int.from_bytes(frame[at:at + size], "little") + (256 if size == 2 else 0)


def reserve(frame: bytes) -> int:
    """A frame's reserve: its Frame_Content_Size, else its bound."""
    return fcs_value(frame) if has_fcs(frame) else bound(frame)


def bound(frame: bytes) -> int:
    """128 KiB a compressed block + the sizes of the raw and RLE blocks."""
    at, total = header_len(frame), 0
    while True:
        x = int.from_bytes(frame[at:at + 3], "little")
        last, typ, size = x & 1, (x >> 1) & 3, x >> 3
        total += K if typ == 2 else size
        at += 3 + (1 if typ == 1 else size)
        if last:
            return total


class Part:
    """A piece of a chunk.  kind: "frame" (a zstd frame that walks to its end;
    data: its source), "skip" (a skippable frame) or "stop" (bytes at which the
    walk fails: everything from here on is the chunk's last sub-chunk)."""

    def __init__(self, kind, raw, data=b""):
        self.kind, self.raw, self.data = kind, raw, data
        self.good = True          # (False: a frame that walks to its end and does not decode)


@functools.lru_cache(maxsize=None)
def _frame(n, seed, level, fcs, checksum):
    data = gen.text(max(n, 1), seed=seed)[:n]
    return libzstd.compress(data, level, checksum=checksum, content_size=fcs), data


def frame(n, seed=1, level=3, fcs=True, checksum=False):
    """A frame of n bytes of seeded word text; one the oracle (like the reference) does not take at level 3 is
    written at level -1."""
    raw, data = _frame(n, seed, level, fcs, checksum)
    if n and expect(raw)[0] != 0:
        raw, data = _frame(n, seed, -1, fcs, checksum)
    assert has_fcs(raw) == fcs
    if n == 0:
        # a frame of no bytes is one Raw block of size 0, which the reference's parser refuses (a zero-length
        # slice) and the oracle and the walk with it: the walk stops there
        assert expect(raw)[0] == EMPTY_SLICE
        return Part("stop", raw)
    return Part("frame", raw, data)


def skip(n, magic=0x184D2A50):
    assert n > 0
    return Part("skip", magic.to_bytes(4, "little") + n.to_bytes(4, "little") + bytes((7 * i + 3) & 255 for i in range(n)))


def split(parts):
    """The chunk's sub-chunks by the rule: [(bytes, frame part or None)]."""
    subs, cur = [], b""
    for k, p in enumerate(parts):
        if p.kind == "stop":
            cur += b"".join(q.raw for q in parts[k:])
            break
        cur += p.raw
        if p.kind == "frame":
            subs.append((cur, p))
            cur = b""
    if cur or not subs:
        subs.append((cur, None))
    return subs


class Chunk:
    def __init__(self, parts, cap=None):
        self.parts = list(parts)
        self.raw = b"".join(p.raw for p in self.parts)
        self.subs = split(self.parts)
        self.sub_status = [expect(s)[0] for s, _ in self.subs]
        self.status = next((s for s in self.sub_status if s), 0)
        self.want = b"".join(expect(s)[1] for s, _ in self.subs) if self.status == 0 else b""
        self.cap = len(b"".join(p.data for p in self.parts if p.kind == "frame")) if cap is None else cap
        # placement
        self.place, in_place = [], True              # per sub-chunk: None (in place) or its reserve (staged)
        for s, p in self.subs:
            exact = p is not None and has_fcs(p.raw)
            self.place.append(None if in_place else (0 if p is None else reserve(p.raw)))
            in_place = in_place and exact

    def assert_good(self):
        for p in self.parts:
            if p.kind == "frame" and p.good:
                assert expect(p.raw) == (0, p.data)

    staged_frames = property(lambda self: sum(r is not None for r in self.place))
    staged_bytes = property(lambda self: sum((r + 15) & ~15 for r in self.place if r is not None))
    pieces = property(lambda self: sum(-(-r // PIECE) for r in self.place if r is not None))


def read_device(ptr, ctype, n):
    from zstd_decompressor.seekable import _read_device
    return _read_device(ptr, ctype, n)


def on_device_odd(blob: bytes):
    """blob at an odd device address, ending at its tensor's last byte: (address, base tensor)."""
    import torch
    host = np.empty(len(blob) + 1, dtype=np.uint8)
    host[0] = 0x5C
    host[1:] = np.frombuffer(blob, dtype=np.uint8)
    base = torch.from_numpy(host).to(torch.device("cuda", 0))
    assert base.data_ptr() % 2 == 0
    return (base.data_ptr() + 1 if blob else 0), base


class Layout:
    """The chunks' sources and destinations on the device.  residues: chunk
    i's destination address mod 16 (default: odd)."""

    def __init__(self, chunks, residues=None, null=()):
        import torch
        self.torch, self.chunks, self.n = torch, chunks, len(chunks)
        self.src = [on_device_odd(c.raw) for c in chunks]
        self.offs, at = [], 256
        for i, c in enumerate(chunks):
            at += GUARD
            r = 1 if residues is None else residues[i]
            at += (r - at) % 16 if residues is not None else (0 if at % 2 else 1)
            self.offs.append(at)
            at += c.cap
        self.t = torch.full((at + GUARD + 256,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
        assert self.t.data_ptr() % 256 == 0
        self.src_ptrs = [a for a, _ in self.src]
        self.src_sizes = [len(c.raw) for c in chunks]
        self.dst_ptrs = [0 if (i in null or not c.cap) else self.t.data_ptr() + o
                         for i, (c, o) in enumerate(zip(chunks, self.offs))]
        self.dst_caps = [c.cap for c in chunks]

    def batch(self, flags=0, dictionary=None):
        from zstd_decompressor import MultiFrameBatch
        return MultiFrameBatch(self.src_ptrs, self.src_sizes, self.dst_ptrs, self.dst_caps, flags=flags,
                               dictionary=dictionary)

    def refill(self):
        self.t.fill_(FILL)

    def check(self, st, ln, want_status=None, want_bytes=None):
        """Statuses, lengths, bytes; and every byte outside the delivered ranges is 0xA5."""
        host = self.t.cpu().numpy()
        mask = np.ones(host.size, dtype=bool)
        for i, c in enumerate(self.chunks):
            ws = c.status if want_status is None else want_status[i]
            wb = c.want if want_bytes is None else want_bytes[i]
            assert st[i] == ws, (i, st[i], ws)
            o = self.offs[i]
            if ws == 0:
                assert ln[i] == len(wb), (i, ln[i], len(wb))
                assert host[o:o + ln[i]].tobytes() == wb, i
                mask[o:o + ln[i]] = False
            else:
                assert ln[i] == 0, (i, ln[i])
                if self.dst_ptrs[i]:
                    mask[o:o + c.cap] = False        # (a failed chunk's destination bytes are unspecified)
        assert (host[mask] == FILL).all(), "a byte outside the delivered ranges was written"

    def run(self, flags=0, dictionary=None, want_status=None, want_bytes=None):
        b = self.batch(flags, dictionary)
        try:
            b.decode_async()
            st, ln = b.results()
            self.check(st, ln, want_status, want_bytes)
            d_st, d_ln = b.device_results()
            assert read_device(d_st, C.c_int32, self.n) == st and read_device(d_ln, C.c_uint64, self.n) == ln
            return b.info, b.frames(), (st, ln)
        finally:
            b.close()


def check_info(info, chunks):
    assert info.nchunks == len(chunks)
    assert info.frames == sum(len(c.subs) for c in chunks)
    assert info.staged_frames == sum(c.staged_frames for c in chunks)
    assert info.frames_in_place == info.frames - info.staged_frames
    assert info.staged_bytes == sum(c.staged_bytes for c in chunks)
    assert info.copy_pieces == sum(c.pieces for c in chunks)
    assert info.batch.nchunks == info.frames and info.batch.device_built == 1


def check_frames(frames, chunks):
    first, fst, fln = frames
    at = 0
    for i, c in enumerate(chunks):
        assert first[i] == at
        assert fst[at:at + len(c.subs)] == c.sub_status, (i, fst[at:at + len(c.subs)], c.sub_status)
        at += len(c.subs)
    assert first[len(chunks)] == at == len(fst) == len(fln)


# --------------------------------------------------------------------------
# 1. in place
# --------------------------------------------------------------------------
SIZES = (0, 1, 17, 300, 5000, 140000)


def in_place_chunk(i):
    nf = (1, 2, 3, 5)[i % 4]
    parts = []
    for j in range(nf):
        n = SIZES[1 + (i + 2 * j) % 4]
        if i % 16 == 3 and j == 1:
            n = 140000                           # (a 140,000-byte frame in one chunk of sixteen)
        if i % 8 == 5 and j == nf - 1:
            n = 0                                # (a frame of no bytes: the walk stops at it, so it comes last)
        if j and (i + j) % 2:
            parts.append(skip(1 + (i + j) % 40))
        parts.append(frame(n, seed=1 + (i * 7 + j) % 11, level=(3, 1, -1)[(i + j) % 3]))
    return Chunk(parts)


@pytest.mark.parametrize("nchunks", [1, 65, 257])
def test_in_place(nchunks):
    chunks = [in_place_chunk(i + (3 if nchunks == 1 else 0)) for i in range(nchunks)]
    for c in chunks[:16]:
        c.assert_good()
    # every part is ZD_OK on the oracle but the frames of no bytes, which are EmptySlice there
    assert all(c.status == (EMPTY_SLICE if c.parts[-1].kind == "stop" else 0) for c in chunks)
    assert all(c.staged_frames == 0 for c in chunks)
    if nchunks > 1:
        seen = {len(p.data) for c in chunks for p in c.parts if p.kind == "frame"}
        assert seen == set(SIZES[1:]) and any(c.status for c in chunks)
        assert {len(c.subs) for c in chunks} >= {1, 2, 3, 5}
    L = Layout(chunks)
    info, frames, _ = L.run()
    check_info(info, chunks)
    check_frames(frames, chunks)
    assert info.staged_bytes == 0 and info.copy_pieces == 0 and info.frames_in_place == info.frames


# --------------------------------------------------------------------------
# 2. staged
# --------------------------------------------------------------------------
STAGED_LENGTHS = (1, 15, 16, 17, 32767, 32768, 32769, 140000)


def test_staged_positions_lengths_and_alignments():
    chunks = []
    for k, n in enumerate(STAGED_LENGTHS):
        # the frame without a Frame_Content_Size first, in the middle, last; the frame of n bytes staged behind it
        nofcs = frame(300 + k, seed=2 + k, fcs=False)
        chunks.append(Chunk([nofcs, frame(n, seed=3 + k), frame(17, seed=5)]))
        chunks.append(Chunk([frame(300, seed=4), skip(9), frame(5000 + k, seed=6, fcs=False), frame(n, seed=7 + k),
                             skip(3)]))
        chunks.append(Chunk([frame(n, seed=8 + k), frame(17, seed=9), frame(n, seed=10 + k, fcs=False)]))
        chunks.append(Chunk([frame(n, seed=11 + k, fcs=False), frame(n, seed=12 + k, fcs=False), frame(n, seed=13 + k)]))
    for c in chunks:
        c.assert_good()
        assert c.status == 0
    assert sum(c.staged_frames for c in chunks) == 8 * (2 + 2 + 0 + 2)
    for base in (0, 5):
        # every residue mod 16 for the destinations; the staged frames land behind odd and even lengths
        L = Layout(chunks, residues=[(base + 3 * i) % 16 for i in range(len(chunks))])
        assert {p % 16 for p in L.dst_ptrs} == set(range(16))
        info, frames, _ = L.run()
        check_info(info, chunks)
        check_frames(frames, chunks)
        assert info.staged_bytes > 0 and info.copy_pieces > 0


# --------------------------------------------------------------------------
# 3. many frames
# --------------------------------------------------------------------------
def test_many_frames_beside_an_ordinary_chunk():
    parts = [frame(17 + (k * 37) % 284, seed=1 + k % 13, level=(3, 1, -1)[k % 3], fcs=k % 3 != 2) for k in range(300)]
    many = Chunk(parts)
    chunks = [Chunk([frame(5000, seed=3)]), many, Chunk([frame(300, seed=4)])]
    for c in chunks:
        c.assert_good()
        assert c.status == 0
    assert len(many.subs) == 300 and many.staged_frames == 297
    L = Layout(chunks)
    info, frames, _ = L.run()
    check_info(info, chunks)
    check_frames(frames, chunks)


# --------------------------------------------------------------------------
# 4. failures
# --------------------------------------------------------------------------
def reserved_block(p):
    b = bytearray(p.raw)
    b[header_len(p.raw)] |= 6
    return Part("stop", bytes(b))


def parts_from_index(blob):
    """A chunk's parts from the host index (zd_frames_index): the frames that walk to their end, then the stop."""
    from zstd_decompressor.batch import frames_index
    frames, _, _, consumed = frames_index(blob)
    out = []
    for f in frames:
        raw = blob[f["src_offset"]:f["src_offset"] + f["src_size"]]
        out.append(Part("skip", raw) if f["kind"] else Part("frame", raw, expect(raw)[1]))
        out[-1].good = expect(raw)[0] == 0
    assert sum(len(p.raw) for p in out) == consumed
    if consumed < len(blob):
        out.append(Part("stop", blob[consumed:]))
    return out


def corrupt(parts, pos, how):
    """parts with the frame at `pos` damaged."""
    out = list(parts)
    if how == "block type":
        out[pos] = reserved_block(parts[pos])
    elif how == "cut":
        out[pos] = Part("stop", parts[pos].raw[:-3])
        if pos < len(parts) - 1:
            # the walk of a cut frame runs on into the next frame's bytes, so where it stops is not known by
            # assembly: the host index says which frames walk to their end, and the rest is the stop
            out = parts_from_index(b"".join(q.raw for q in out))
    elif how == "3 trailing":
        out.insert(pos + 1, Part("stop", b"\x01\x02\x03"))
    elif how == "4 trailing":
        out.insert(pos + 1, Part("stop", b"\x01\x02\x03\x04"))
    return out


@pytest.mark.parametrize("how,status", [("block type", RBT), ("cut", NEB), ("3 trailing", NEB), ("4 trailing", MAGIC)])
def test_failures(how, status):
    good = [frame(300, seed=21), frame(5000, seed=22), frame(17, seed=23)]
    # the corruption alone, as the oracle sees it
    assert expect(b"".join(p.raw for p in corrupt([good[1]], 0, how)))[0] == status
    chunks = []
    for pos in range(3):
        for fcs in (True, False):
            parts = [frame(len(p.data), seed=21 + k, fcs=fcs or k != 0) for k, p in enumerate(good)]
            chunks += [Chunk([frame(140000 if pos == 1 else 300, seed=24)]),
                       Chunk(corrupt(parts, pos, how), cap=300 + 5000 + 17),
                       Chunk([frame(17, seed=25), frame(1, seed=26)])]
    for c in chunks:
        c.assert_good()
    bad = chunks[1::3]
    assert all(c.status != 0 for c in bad) and all(c.status == 0 for c in chunks[0::3] + chunks[2::3])
    # in the last position the chunk fails with the corruption's own status; in front of other frames three
    # trailing bytes read a magic number out of the next frame's, and a cut frame decodes into them
    assert bad[-1].status == status and bad[-2].status == status
    if how in ("block type", "4 trailing"):
        assert all(c.status == status for c in bad)
    L = Layout(chunks)
    info, frames, _ = L.run()
    check_info(info, chunks)
    check_frames(frames, chunks)
    first, fst, _ = frames
    for i, c in enumerate(chunks):
        if c.status:
            lead = c.sub_status.index(c.status)
            assert fst[first[i]:first[i] + lead] == [0] * lead       # the good leading frames


# --------------------------------------------------------------------------
# 5. too small
# --------------------------------------------------------------------------
def test_one_byte_short():
    def with_fcs():
        return [frame(300, seed=31), frame(5000, seed=32), frame(17, seed=33)]

    def without():
        return [frame(300, seed=31, fcs=False), frame(5000, seed=32), frame(17, seed=33, fcs=False)]
    total = 300 + 5000 + 17
    chunks = [Chunk(with_fcs()), Chunk(with_fcs(), cap=total - 1), Chunk(without()), Chunk(without(), cap=total - 1),
              Chunk([frame(17, seed=34)])]
    for c in chunks:
        c.assert_good()
    L = Layout(chunks)
    want = [0, DST_TOO_SMALL, 0, DST_TOO_SMALL, 0]
    b = L.batch()
    try:
        b.decode_async()
        st, ln = b.results()
        L.check(st, ln, want_status=want)
        first, fst, fln = b.frames()
        # with Frame_Content_Sizes the creation's capacity pass refuses the frame that does not fit ...
        assert fst[first[1]:first[2]] == [0, 0, DST_TOO_SMALL]
        # ... without them every frame decodes (two of them staged) and the join pass finds the sum too long
        assert fst[first[3]:first[4]] == [0, 0, 0] and fln[first[3]:first[4]] == [300, 5000, 17]
        check_info(b.info, chunks)
    finally:
        b.close()


# --------------------------------------------------------------------------
# 6. like a batch
# --------------------------------------------------------------------------
def test_one_frame_chunks_are_a_batch():
    import torch
    from zstd_decompressor import Batch
    chunks = [Chunk([frame(n, seed=41 + k, fcs=k % 3 != 1)], cap=n) for k, n in enumerate((300, 5000, 17, 140000, 1, 0))]
    chunks.insert(2, Chunk([]))                                          # an empty chunk
    chunks.insert(4, Chunk([frame(300, seed=47)]))                       # the bad entry: a NULL source with a size
    chunks.append(Chunk([skip(5), frame(17, seed=48), skip(7)]))
    for c in chunks:
        c.assert_good()
    L = Layout(chunks)
    L.src_ptrs[4] = 0
    want = [c.status for c in chunks]
    want[4] = INVALID_ARG
    _, frames, (st, ln) = L.run(want_status=want)
    mine = L.t.cpu().numpy().copy()
    L.refill()
    dev = torch.device("cuda", 0)
    arrs = [torch.tensor(v, dtype=torch.int64, device=dev) for v in (L.src_ptrs, L.src_sizes, L.dst_ptrs, L.dst_caps)]
    b = Batch.from_device(*arrs)
    try:
        b.decode_async()
        bst, bln = b.results()
    finally:
        b.close()
    assert (st, ln) == (bst, bln)
    assert (L.t.cpu().numpy() == mine).all()
    assert st[2] == 0 and ln[2] == 0


# --------------------------------------------------------------------------
# 7. flags
# --------------------------------------------------------------------------
def test_verify_checksum_in_a_middle_frame():
    from zstd_decompressor import _lib
    parts = [frame(300, seed=51, checksum=True), frame(5000, seed=52, checksum=True), frame(17, seed=53, checksum=True)]
    damaged = list(parts)
    raw = bytearray(parts[1].raw)
    raw[-1] ^= 0x40                                                      # the Content_Checksum's last byte
    damaged[1] = Part("frame", bytes(raw), parts[1].data)
    nofcs = [frame(300, seed=51, fcs=False, checksum=True), damaged[1], parts[2]]
    chunks = [Chunk(parts), Chunk(damaged), Chunk(nofcs), Chunk(parts[::-1])]
    for c in chunks:
        assert all(s == 0 for s in c.sub_status)                         # (the oracle does not verify checksums)
    L = Layout(chunks)
    want = [0, CHECKSUM_WRONG, CHECKSUM_WRONG, 0]
    info, frames, _ = L.run(flags=_lib.F_VERIFY_CHECKSUM, want_status=want)
    first, fst, _ = frames
    assert fst[first[1]:first[2]] == [0, CHECKSUM_WRONG, 0] and fst[first[2]:first[3]] == [0, CHECKSUM_WRONG, 0]
    L.refill()
    L.run(want_status=[0, 0, 0, 0], want_bytes=[c.want for c in chunks])  # without the flag the bytes decode


def big_chunks():
    chunks = [Chunk([frame(300, seed=61), frame(140000, seed=62), frame(140000, seed=63)]),
              Chunk([frame(140000, seed=64, fcs=False), frame(140000, seed=65), frame(17, seed=66)])]
    for c in chunks:
        c.assert_good()
        assert c.status == 0
    return chunks


def test_block_parallel_in_place_and_staged():
    from zstd_decompressor import _lib
    chunks = big_chunks()
    L = Layout(chunks)
    info, frames, _ = L.run(flags=_lib.F_BLOCK_PARALLEL)
    check_info(info, chunks)
    assert info.batch.executors & _lib.EXEC_K4J and info.batch.k4j_chunks >= 4
    assert info.staged_frames == 2


def test_one_round_is_decoded_again():
    from zstd_decompressor import _lib
    chunks = big_chunks()
    L = Layout(chunks)
    b = L.batch(_lib.F_BLOCK_PARALLEL | _lib.F_J_ONE_ROUND)
    try:
        b.decode_async()
        L.torch.cuda.synchronize()
        d_st, d_ln = b.device_results()
        before = read_device(d_st, C.c_int32, L.n)
        assert all(s != 0 for s in before), "one round of one hop converged: the test is not about the re-decode"
        assert read_device(d_ln, C.c_uint64, L.n) == [0, 0]
        st, ln = b.results()
        L.check(st, ln)
        assert read_device(d_st, C.c_int32, L.n) == st == [0, 0]
    finally:
        b.close()


def test_rfc_frame_in_a_middle_position():
    from zstd_decompressor import _lib
    letters = bytes(np.random.default_rng(1).integers(97, 123, 4096, dtype=np.uint8))
    f = libzstd.compress(letters, 3)
    assert libzstd.decompress_frame(f, 4096) == letters
    mid = Part("frame", f, letters)
    for fcs in (True, False):
        chunks = [Chunk([frame(300, seed=71, fcs=fcs), mid, frame(17, seed=72)]), Chunk([frame(5000, seed=73)])]
        want_bytes = [b"".join(p.data for p in c.parts) for c in chunks]
        L = Layout(chunks)
        b = L.batch()
        try:
            b.decode_async()
            st, _ = b.results()
            assert st[0] != 0 and st[1] == 0, "stale fixture: the letters decode without ZD_F_RFC"
        finally:
            b.close()
        L.refill()
        L.run(flags=_lib.F_RFC, want_status=[0, 0], want_bytes=want_bytes)


def test_two_dictionaries_in_one_chunk():
    from zstd_decompressor import Dictionary, DictionarySet
    d1 = open(os.path.join(GOLDEN, "dict.bin"), "rb").read()
    assert d1[:4] == bytes.fromhex("37a430ec")
    other = gen.xml(3000, seed=0xD1C2)
    d2 = d1[:4] + (zdict.dict_id(d1) + 1).to_bytes(4, "little") + d1[8:-3000] + other
    ids = (zdict.dict_id(d1), zdict.dict_id(d2))
    assert ids[0] != ids[1] and 0 not in ids
    recs = [gen.text(2000, seed=81), other[500:2500] + gen.xml(300, seed=82), gen.text(900, seed=83)]
    dicts = (d1, d2, d1)
    for fcs in (True, False):
        fr = [zdict.compress(r, d, 3, content_size=fcs or k != 0) for k, (r, d) in enumerate(zip(recs, dicts))]
        for f, r, d in zip(fr, recs, dicts):
            assert zdict.decompress(f, d, len(r)) == r
            at, size = 5 + (0 if (f[4] >> 5) & 1 else 1), (0, 1, 2, 4)[f[4] & 3]
            assert size and int.from_bytes(f[at:at + size], "little") == zdict.dict_id(d)
        parts = [Part("frame", f, r) for f, r in zip(fr, recs)]
        chunks = [Chunk.__new__(Chunk), Chunk.__new__(Chunk)]
        for c, ps in zip(chunks, (parts, parts[1:])):
            # (the oracle has no dictionaries: libzstd's decoder is the cross-check above)
            c.parts, c.raw = ps, b"".join(p.raw for p in ps)
            c.status, c.want = 0, b"".join(p.data for p in ps)
            c.cap = len(c.want)
        L = Layout(chunks)
        A, B = Dictionary(d1), Dictionary(d2)
        dset = DictionarySet([A, B])
        try:
            b = L.batch(dictionary=dset)
            try:
                b.decode_async()
                st, ln = b.results()
                L.check(st, ln)
                assert b.info.frames == 5 and b.info.staged_frames == (0 if fcs else 2)
            finally:
                b.close()
        finally:
            dset.close(); A.close(); B.close()


# --------------------------------------------------------------------------
# 8. repeat and size query
# --------------------------------------------------------------------------
def test_decoding_twice_gives_the_same():
    chunks = [Chunk([frame(300, seed=91, fcs=False), frame(32769, seed=92), frame(17, seed=93)]),
              Chunk([frame(5000, seed=94), frame(1, seed=95)]),
              Chunk([frame(300, seed=96), Part("stop", b"\x01\x02\x03\x04")], cap=300)]
    L = Layout(chunks)
    b = L.batch()
    try:
        b.decode_async()
        first = b.results()
        L.check(*first)
        L.refill()
        b.decode_async()
        L.torch.cuda.synchronize()
        d_st, d_ln = b.device_results()
        assert (read_device(d_st, C.c_int32, L.n), read_device(d_ln, C.c_uint64, L.n)) == first
        L.check(*first)
        L.refill()
        b.finish_async()                               # the join and copy passes alone deliver the staged frames again
        L.torch.cuda.synchronize()
        host = L.t.cpu().numpy()
        o = L.offs[0] + 300
        assert host[o:o + 32769 + 17].tobytes() == chunks[0].want[300:]
        assert (host[L.offs[0]:o] == FILL).all()       # (the frame in place is the decode's, not theirs)
    finally:
        b.close()


def test_size_query_sums_the_parts():
    import torch
    from zstd_decompressor import chunk_sizes, decode_multi
    chunks = [Chunk([frame(300, seed=101), skip(4), frame(5000, seed=102), frame(17, seed=103)]),
              Chunk([frame(300, seed=104, fcs=False), frame(140000, seed=105), frame(17, seed=106, fcs=False)]),
              Chunk([]), Chunk([skip(9)]),
              Chunk([frame(300, seed=107), Part("stop", b"\x01\x02\x03")]),
              Chunk([frame(17, seed=108), reserved_block(frame(300, seed=109)), frame(1, seed=110)]),
              Chunk([frame(5000, seed=111)])]
    for c in chunks:
        c.assert_good()
    L = Layout(chunks)
    sizes, statuses, exact = chunk_sizes(L.src_ptrs, L.src_sizes, multi_frame=True)
    torch.cuda.synchronize()
    reserves = [sum(0 if p is None else reserve(p.raw) for _, p in c.subs) for c in chunks]
    assert sizes.tolist() == reserves
    assert statuses.tolist() == [c.status for c in chunks] == [0, 0, 0, 0, NEB, RBT, 0]
    assert exact.tolist() == [1, 0, 0, 0, 0, 0, 1]
    # without the flag: a second frame is ZD_E_OUT_OF_DOMAIN, as ever
    _, plain, _ = chunk_sizes(L.src_ptrs, L.src_sizes)
    assert plain.tolist()[:2] == [OUT_OF_DOMAIN, OUT_OF_DOMAIN] and plain.tolist()[6] == 0
    # destinations of exactly those sizes decode
    dev = torch.device("cuda", 0)
    srcs = [torch.from_numpy(np.frombuffer(c.raw, dtype=np.uint8).copy()).to(dev) for c in chunks]
    dsts = [torch.full((r,), FILL, dtype=torch.uint8, device=dev) for r in reserves]
    st, ln = decode_multi(srcs, dsts)
    assert st == [c.status for c in chunks]
    for c, d, n in zip(chunks, dsts, ln):
        assert n == len(c.want) and d[:n].cpu().numpy().tobytes() == c.want


def test_hip_graph_capture_replay():
    """A launch allocates nothing and does not synchronise: captured once, replayed twice."""
    import torch
    chunks = [Chunk([frame(300, seed=121, fcs=False), frame(32769, seed=122), frame(17, seed=123)]),
              Chunk([frame(5000, seed=124), skip(6), frame(1, seed=125)]),
              Chunk([frame(300, seed=126), Part("stop", b"\x01\x02\x03\x04")], cap=300)]
    for c in chunks:
        c.assert_good()
    L = Layout(chunks)
    dev = torch.device("cuda", 0)
    b = L.batch()
    try:
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):                  # warm-up outside the capture
            b.decode_async(s.cuda_stream)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            b.decode_async(s.cuda_stream)
        d_st, d_ln = b.device_results()
        for _ in range(2):
            L.refill()
            torch.cuda.synchronize(dev)
            g.replay()
            torch.cuda.synchronize(dev)
            L.check(read_device(d_st, C.c_int32, L.n), read_device(d_ln, C.c_uint64, L.n))
        del g
    finally:
        b.close()
