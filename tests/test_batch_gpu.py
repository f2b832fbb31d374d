"""Batches of scattered device chunks (include/zd.h zd_batch, Batch in
zstd_decompressor/batch.py): N chunks at N device addresses, each decoded into
its own buffer with its own status -- zd_k_gather, zd_k_walk_chunks, the
planner's per-frame placement and zd_k_batch_results.

Expected bytes and statuses come from the CPU oracle on each chunk alone (the
dictionary test: from the source records), never from the batch.  Every test
first asserts that its good chunks are ZD_OK in the oracle, so it cannot pass
by everything failing alike.

Layout of every test: the sources packed into one uint8 tensor at odd offsets
with gaps of 1-5 bytes (one chunk in a tensor of exactly its own size); the
destinations carved from one tensor filled with 0xA5, in shuffled order (the
lowest address is not chunk 0), at odd offsets, 32 guard bytes between them.
After every decode every byte outside the chunks' [dst, dst + cap) is 0xA5.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from corpus import gen, libzstd
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dict")
FILL = 0xA5
GUARD = 32
SKIP5 = b"\x50\x2a\x4d\x18" + (5).to_bytes(4, "little") + b"hello"


@functools.lru_cache(maxsize=None)
def expect(chunk: bytes):
    """(status, bytes) of one chunk alone on the CPU oracle; a failing chunk has no bytes."""
    st, out = oracle.decompress_status(chunk)
    return st, (out if st == 0 else b"")


def blocks_of(frame: bytes):
    from zstd_decompressor.batch import frames_index
    frames, blocks, st, _ = frames_index(frame)
    assert st == 0 and len(frames) == 1
    return [b["type"] for b in blocks]


def rle_frame(n: int, byte: int) -> bytes:
    """A frame of one RLE block (libzstd writes runs as compressed blocks): single
    segment, a 2-byte Frame_Content_Size."""
    assert 256 <= n < 65536 + 256 and n < (1 << 21)
    return (b"\x28\xb5\x2f\xfd" + bytes([0x60]) + (n - 256).to_bytes(2, "little") +
            (1 | (1 << 1) | (n << 3)).to_bytes(3, "little") + bytes([byte]))


def read_device(ptr: int, nbytes: int) -> bytes:
    """nbytes at a raw device address, through the process's HIP runtime."""
    import torch
    rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = C.CDLL(rt if os.path.exists(rt) else "libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    buf = (C.c_uint8 * max(nbytes, 1))()
    assert hip.hipMemcpy(buf, C.c_void_p(ptr), nbytes, 2) == 0     # hipMemcpyDeviceToHost
    return bytes(buf)[:nbytes]


class Layout:
    """The common source / destination layout of a list of chunks."""

    def __init__(self, chunks, caps, seed, solo=None, order=None):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        rng = np.random.default_rng(seed)
        n = len(chunks)
        self.chunks, self.caps, self.n = chunks, list(caps), n
        solo = (max(range(n), key=lambda i: len(chunks[i])) if n else None) if solo is None else solo
        # sources: odd offsets, gaps of 1-5 bytes
        offs, at = [], 1
        for i, c in enumerate(chunks):
            at |= 1
            offs.append(at)
            if i != solo:
                at += len(c) + int(rng.integers(1, 6))
        host = np.full(at + 8, 0x5C, dtype=np.uint8)
        for i, c in enumerate(chunks):
            if i != solo:
                host[offs[i]:offs[i] + len(c)] = np.frombuffer(c, dtype=np.uint8)
        self.src = torch.from_numpy(host).to(self.dev)
        self.src_ptrs = [self.src.data_ptr() + o for o in offs]
        if solo is not None:
            self.solo = torch.from_numpy(np.frombuffer(chunks[solo], dtype=np.uint8).copy()).to(self.dev)
            assert self.solo.numel() == len(chunks[solo])
            self.src_ptrs[solo] = self.solo.data_ptr() if len(chunks[solo]) else 0
        self.src_sizes = [len(c) for c in chunks]
        # destinations: shuffled order, odd offsets, guard bytes between
        if order is None:
            order = [int(x) for x in rng.permutation(n)]
            if n > 1 and order[0] == 0:
                order[0], order[1] = order[1], order[0]
        self.dst_offs, at = [0] * n, GUARD + 1
        for j in order:
            at |= 1
            self.dst_offs[j] = at
            at += self.caps[j] + GUARD
        self.dst = torch.full((at + GUARD,), FILL, dtype=torch.uint8, device=self.dev)
        self.dst_ptrs = [self.dst.data_ptr() + o for o in self.dst_offs]
        if n > 1:
            assert min(range(n), key=lambda i: self.dst_offs[i]) != 0
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def batch(self, flags=0, dictionary=None):
        from zstd_decompressor.batch import Batch
        return Batch(self.src_ptrs, self.src_sizes, self.dst_ptrs, self.caps, flags=flags, dictionary=dictionary,
                     stream=self.stream)

    def refill(self):
        self.dst.fill_(FILL)
        self.torch.cuda.synchronize()

    def host(self):
        return self.dst.cpu().numpy()

    def check(self, h, statuses, lengths, want):
        """Guards untouched; chunk i's status, length and bytes are want[i]'s."""
        outside = np.ones(h.size, dtype=bool)
        for o, c in zip(self.dst_offs, self.caps):
            outside[o:o + c] = False
        assert (h[outside] == FILL).all(), "bytes outside the chunks' destinations were written"
        for i, (st, out) in enumerate(want):
            assert statuses[i] == st, (i, statuses[i], st)
            assert lengths[i] == len(out), (i, lengths[i], len(out))
            assert h[self.dst_offs[i]:self.dst_offs[i] + len(out)].tobytes() == out, i

    def run(self, want, flags=0, dictionary=None, after=None):
        """One batch: decode, device arrays == host arrays, the common checks; returns its info."""
        b = self.batch(flags, dictionary)
        try:
            b.decode_async(self.stream)
            st, ln = b.results(self.stream)
            d_st, d_ln = b.device_results()
            assert list(np.frombuffer(read_device(d_st, 4 * self.n), dtype=np.int32)) == st
            assert list(np.frombuffer(read_device(d_ln, 8 * self.n), dtype=np.uint64)) == ln
            self.check(self.host(), st, ln, want)
            if after:
                after(b, st, ln)
            return b.info
        finally:
            b.close()


# ---------------------------------------------------------------------------
# 1. mixed shapes in one batch
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed():
    rng = np.random.default_rng(0xBA7C)
    text2k = libzstd.compress(gen.text(2 << 10, seed=0xBA01), 3)
    named = [
        ("content of 0 bytes", libzstd.compress(b"")),
        ("content of 1 byte", libzstd.compress(b"x")),
        ("17-byte raw block", libzstd.compress(rng.integers(0, 256, 17, dtype=np.uint8).tobytes())),
        ("40 KiB of zeros", rle_frame(40 << 10, 0)),
        ("2 KiB text level 3", text2k),
        ("200 KiB text level 9", libzstd.compress(gen.text(200 << 10, seed=0xBA02), 9)),
        ("130 KiB incompressible", libzstd.compress(rng.integers(0, 256, 130 << 10, dtype=np.uint8).tobytes())),
        ("50 KiB without FCS", libzstd.compress(gen.text(50 << 10, seed=0xBA03), 3, content_size=False)),
        ("10 KiB with checksum", libzstd.compress(gen.text(10 << 10, seed=0xBA04), 3, checksum=True)),
        ("skippable then frame", SKIP5 + libzstd.compress(gen.text(3000, seed=0xBA05), 3) + SKIP5),
        ("zero-byte chunk", b""),
    ]
    return named


def test_mixed_shapes():
    named = mixed()
    names = [k for k, _ in named]
    chunks = [c for _, c in named]
    want = [expect(c) for c in chunks]
    # the shapes are what their names say, and the good ones are good on the CPU
    at = dict(zip(names, range(len(names))))
    for k in names:
        if k != "content of 0 bytes":      # (the reference's zero-length slice: whatever the oracle says)
            assert want[at[k]][0] == 0, k
    assert blocks_of(chunks[at["17-byte raw block"]]) == [0]
    assert blocks_of(chunks[at["40 KiB of zeros"]]) == [1]
    assert blocks_of(chunks[at["200 KiB text level 9"]]) == [2, 2]
    assert blocks_of(chunks[at["130 KiB incompressible"]]) == [0, 0]
    assert libzstd.frame_content_size(chunks[at["50 KiB without FCS"]]) != 50 << 10
    lens = [len(want[at[k]][1]) for k in ("content of 1 byte", "zero-byte chunk", "skippable then frame")]
    assert lens == [1, 0, 3000]
    # capacities: exact for most, larger for some (the frame without FCS among the exact ones)
    caps = [len(out) for _, out in want]
    for k, extra in (("2 KiB text level 3", 100), ("130 KiB incompressible", 4097), ("zero-byte chunk", 7),
                     ("content of 0 bytes", 16)):
        caps[at[k]] += extra
    L = Layout(chunks, caps, seed=0xBA10)

    def after(b, st, ln):
        ok, digest = b.checksums(L.stream)
        assert ok[at["10 KiB with checksum"]] == 1
        assert [ok[i] for i in range(len(names)) if i != at["10 KiB with checksum"]] == [-1] * (len(names) - 1)
        assert digest[at["zero-byte chunk"]] == 0xEF46DB3751D8E999     # XXH64 of no bytes

    info = L.run(want, after=after)
    assert info.nchunks == len(chunks) and info.gathered_bytes >= sum(len(c) for c in chunks)


# ---------------------------------------------------------------------------
# 2. failures among good chunks
# ---------------------------------------------------------------------------
def corrupt_table(frame: bytes) -> bytes:
    """`frame` with one bit of its first block's Huffman tree description
    flipped, the first flip the oracle rejects."""
    assert frame[:4] == b"\x28\xb5\x2f\xfd"
    fhd = frame[4]
    single = (fhd >> 5) & 1
    at = 5 + (0 if single else 1) + [0, 1, 2, 4][fhd & 3] + [1 if single else 0, 2, 4, 8][fhd >> 6]
    bh = frame[at] | frame[at + 1] << 8 | frame[at + 2] << 16
    assert (bh >> 1) & 3 == 2
    p = at + 3
    lt, sf = frame[p] & 3, (frame[p] >> 2) & 3
    assert lt == 2, "compressed literals with their own tree"
    desc = p + [3, 3, 4, 5][sf]
    for k in range(desc, desc + 6):
        for bit in range(8):
            bad = frame[:k] + bytes([frame[k] ^ (1 << bit)]) + frame[k + 1:]
            if oracle.decompress_status(bad)[0] != 0:
                return bad
    raise AssertionError("no flip in the tree description fails in the oracle")


def test_failures_among_good_chunks():
    good = [libzstd.compress(gen.text(1500 + 700 * i, seed=0xBB00 + i), 3) for i in range(8)]
    nofcs_src = gen.text(20 << 10, seed=0xBB20)
    nofcs = libzstd.compress(nofcs_src, 3, content_size=False)
    fcs_src = gen.text(6000, seed=0xBB21)
    fcs = libzstd.compress(fcs_src, 3)
    assert libzstd.frame_content_size(fcs) == 6000 and libzstd.frame_content_size(nofcs) != len(nofcs_src)
    from zstd_decompressor import _lib
    # (chunk, capacity or None for the oracle's length, expected or None for the oracle's)
    cases = [
        (good[0], None, None),
        (b"\x27" + good[1][1:], 4000, None),                                  # bad magic
        (good[1], None, None),
        (good[2][:len(good[2]) // 2], 4000, None),                              # a frame cut in half
        (good[2], None, None),
        (corrupt_table(good[3]), 8000, None),                                   # a flipped bit in a table description
        (good[3], None, None),
        (fcs, 5999, (_lib.DST_TOO_SMALL, b"")),                                # dst_cap = FCS - 1
        (good[4], None, None),
        (nofcs, len(nofcs_src) - 1, (_lib.DST_TOO_SMALL, b"")),                # no FCS, one byte short
        (good[5], None, None),
        (good[6] + good[7], 16000, (_lib.OUT_OF_DOMAIN, b"")),                 # two zstd frames in one chunk
        (good[6], None, None),
        (good[7] + b"\x01\x02\x03\x04\x05", 8000, None),                       # trailing garbage
        (good[7] + b"\x01", 8000, None),
        (good[7], None, None),
        (nofcs, len(nofcs_src), None),                                          # the same frames with room
        (fcs, 6000, None),
    ]
    chunks = [c for c, _, _ in cases]
    want = [w if w is not None else expect(c) for c, _, w in cases]
    failing = {1, 3, 5, 7, 9, 11, 13, 14}
    for i, (st, out) in enumerate(want):
        assert (st != 0) == (i in failing), (i, st)
        assert st == 0 or out == b""
    assert want[1][0] == _lib.UNRECOGNIZED_MAGIC and want[13][0] == _lib.UNRECOGNIZED_MAGIC
    assert want[3][0] == _lib.NOT_ENOUGH_BYTES and want[14][0] == _lib.NOT_ENOUGH_BYTES
    assert want[16][1] == nofcs_src and want[17][1] == fcs_src
    caps = [cap if cap is not None else len(want[i][1]) for i, (_, cap, _) in enumerate(cases)]
    L = Layout(chunks, caps, seed=0xBB30)
    L.run(want)


# ---------------------------------------------------------------------------
# 3. flags
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def multiblock():
    sizes = (130 << 10, 200 << 10, 260 << 10, 390 << 10, 300 << 10, 530 << 10)
    chunks = [libzstd.compress(gen.text(n, seed=0xBC00 + i), 3) for i, n in enumerate(sizes)]
    nblocks = []
    for c in chunks:
        t = blocks_of(c)
        assert set(t) == {2} and 2 <= len(t) <= 5
        nblocks.append(len(t))
    assert min(nblocks) == 2 and max(nblocks) == 5
    want = [expect(c) for c in chunks]
    assert all(st == 0 for st, _ in want)
    return chunks, want


def test_flags():
    from zstd_decompressor import _lib
    chunks, want = multiblock()
    L = Layout(chunks, [len(out) for _, out in want], seed=0xBC10)
    execs = {}
    for flags in (0, _lib.F_BLOCK_PARALLEL, _lib.F_FRAME_SERIAL, _lib.F_SEQ_ONE_LANE, _lib.F_SEQ_NO_LATENCY,
                  _lib.F_K1_LANES, _lib.F_K1_SPLIT):
        L.refill()
        execs[flags] = L.run(want, flags=flags).executors
    assert execs[_lib.F_BLOCK_PARALLEL] & _lib.EXEC_K4J
    assert not execs[_lib.F_FRAME_SERIAL] & _lib.EXEC_K4J


def test_one_round_is_decoded_again_on_the_streaming_executor():
    from zstd_decompressor import _lib
    chunks, want = multiblock()
    L = Layout(chunks, [len(out) for _, out in want], seed=0xBC11)
    b = L.batch(_lib.F_BLOCK_PARALLEL | _lib.F_J_ONE_ROUND)
    try:
        assert b.info.executors & _lib.EXEC_K4J
        b.decode_async(L.stream)
        L.torch.cuda.synchronize()
        d_st, d_ln = b.device_results()
        before = list(np.frombuffer(read_device(d_st, 4 * L.n), dtype=np.int32))
        assert _lib.OUT_OF_DOMAIN in before, "one round of one hop converged: the test is not about the re-decode"
        st, ln = b.results(L.stream)
        L.check(L.host(), st, ln, want)
        assert list(np.frombuffer(read_device(d_st, 4 * L.n), dtype=np.int32)) == st == [0] * L.n
        assert list(np.frombuffer(read_device(d_ln, 8 * L.n), dtype=np.uint64)) == ln
    finally:
        b.close()


# ---------------------------------------------------------------------------
# 4. few-frame routing
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small256():
    chunks = [libzstd.compress(gen.text(1024 + (i * 37) % 2048, seed=0xBD00 + i), 3) for i in range(256)]
    want = [expect(c) for c in chunks]
    assert all(st == 0 for st, _ in want) and all(blocks_of(c) == [2] for c in chunks[::17])
    return chunks, want


@pytest.mark.parametrize("no_fuse", [False, True])
def test_few_frame_routing(no_fuse):
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Plan
    chunks, want = small256()
    flags = _lib.F_NO_FUSE if no_fuse else 0
    plan = Plan(b"".join(chunks), False, flags)
    plan_exec = plan.info.executors
    plan.close()
    L = Layout(chunks, [len(out) for _, out in want], seed=0xBD10)
    info = L.run(want, flags=flags)
    assert info.executors == plan_exec
    assert info.nblocks == 256


# ---------------------------------------------------------------------------
# 5. dictionary
# ---------------------------------------------------------------------------
def test_dictionary_chunks():
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Dictionary
    from test_dict_gpu import header_layout
    idx = json.load(open(os.path.join(GOLDEN, "index.json")))
    dct = open(os.path.join(GOLDEN, "dict.bin"), "rb").read()
    blob = open(os.path.join(GOLDEN, "frames.bin"), "rb").read()
    records = open(os.path.join(GOLDEN, "records.bin"), "rb").read()
    frames, recs, fa, ra = [], [], 0, 0
    for fn, rn in zip(idx["frames"], idx["records"]):
        frames.append(blob[fa:fa + fn])
        recs.append(records[ra:ra + rn])
        fa, ra = fa + fn, ra + rn
    assert len(frames) == 8
    d = Dictionary(dct)
    try:
        order = list(range(7, -1, -1))
        L = Layout(frames, [len(r) for r in recs], seed=0xBE10, order=order)
        info = L.run([(0, r) for r in recs], dictionary=d)
        assert info.executors == 0
        # one chunk names another dictionary: only that chunk fails
        k = 3
        did_at, did_size, *_ = header_layout(frames[k])
        assert did_size == 4 and int.from_bytes(frames[k][did_at:did_at + 4], "little") == idx["dict_id"]
        other = (idx["dict_id"] ^ 0x5A5A).to_bytes(4, "little")
        patched = list(frames)
        patched[k] = frames[k][:did_at] + other + frames[k][did_at + 4:]
        want = [(0, r) for r in recs]
        want[k] = (_lib.DICT_MISMATCH, b"")
        L2 = Layout(patched, [len(r) for r in recs], seed=0xBE11, order=order)
        L2.run(want, dictionary=d)
    finally:
        d.close()


# ---------------------------------------------------------------------------
# 6. relaunch, and a batch of no chunks
# ---------------------------------------------------------------------------
def test_relaunch():
    named = mixed()
    chunks = [c for _, c in named]
    want = [expect(c) for c in chunks]
    L = Layout(chunks, [len(out) + (i % 3) for i, (_, out) in enumerate(want)], seed=0xBF10)
    b = L.batch()
    try:
        runs = []
        for _ in range(2):
            L.refill()
            b.decode_async(L.stream)
            st, ln = b.results(L.stream)
            h = L.host()
            L.check(h, st, ln, want)
            runs.append((st, ln, h))
        assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
        outside = np.ones(runs[0][2].size, dtype=bool)
        for o, c in zip(L.dst_offs, L.caps):
            outside[o:o + c] = False
        assert (runs[0][2][outside] == runs[1][2][outside]).all()
    finally:
        b.close()


def test_empty_batch():
    from zstd_decompressor.batch import Batch
    b = Batch([], [], [], [])
    try:
        assert b.info.nchunks == 0 and b.info.gathered_bytes == 0
        b.decode_async(0)
        assert b.results(0) == ([], [])
        assert b.checksums(0) == ([], [])
    finally:
        b.close()


def test_decode_tensors():
    import torch
    from zstd_decompressor import decode_tensors
    chunks, want = small256()
    dev = torch.device("cuda", 0)
    pick = (5, 0, 200)
    srcs = [torch.from_numpy(np.frombuffer(chunks[i], dtype=np.uint8).copy()).to(dev) for i in pick]
    dsts = [torch.full((len(want[i][1]) + 3,), FILL, dtype=torch.uint8, device=dev) for i in pick]
    st, ln = decode_tensors(srcs, dsts)
    assert st == [0, 0, 0] and ln == [len(want[i][1]) for i in pick]
    for i, t in zip(pick, dsts):
        h = t.cpu().numpy()
        assert h[:len(want[i][1])].tobytes() == want[i][1] and (h[len(want[i][1]):] == FILL).all()
