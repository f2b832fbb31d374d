"""Batches created from device-resident chunk arrays (include/zd.h
zd_batch_create_device / _dicts, Batch.from_device): the layout kernels
(zd_k_batch_layout, the scans, zd_k_batch_place), zd_k_gather_scan, the device
scan of the blocks' places, zd_k_batch_fit and the device planner with
placement and dictionaries.

Expected statuses and bytes come from the CPU oracle on each chunk alone (the
dictionary tests: from the source records), never from a batch; every test
first asserts that its good chunks are ZD_OK there.  Every chunk of every test
has one exact expected status.  Each device-created batch is also compared
with the host-created Batch over the same entries: statuses, lengths, the
zd_batch_info fields nchunks / gathered_bytes / nblocks / nsequences /
executors.  (zd_batch_create refuses a whole batch for a NULL address with a
non-zero count; the host batch of such a test gets that entry as the empty
chunk without a destination the device path turns it into, and the entry's
own status is compared with INVALID_ARG only.)

Layout of every test: the sources packed into one uint8 tensor at odd offsets
with gaps of 1-5 bytes; the destinations carved from one tensor filled with
0xA5, in shuffled order (the lowest address is not chunk 0), at odd offsets,
32 guard bytes between them.  After every decode every byte outside the
chunks' [dst, dst + cap) is 0xA5.
"""
import ctypes as C
import functools
import json
import os

import numpy as np
import pytest

from corpus import gen, libzstd, zdict
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dict")
FILL = 0xA5
GUARD = 32
INFO_FIELDS = ("nchunks", "gathered_bytes", "nblocks", "nsequences", "executors")


def skippable(payload: int) -> bytes:
    return b"\x50\x2a\x4d\x18" + payload.to_bytes(4, "little") + bytes((7 * i + 3) & 0xFF for i in range(payload))


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
    """A frame of one RLE block: single segment, a 2-byte Frame_Content_Size."""
    assert 256 <= n < 65536 + 256
    return (b"\x28\xb5\x2f\xfd" + bytes([0x60]) + (n - 256).to_bytes(2, "little") +
            (1 | (1 << 1) | (n << 3)).to_bytes(3, "little") + bytes([byte]))


def read_device(ptr: int, nbytes: int) -> bytes:
    import torch
    rt = os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so")
    hip = C.CDLL(rt if os.path.exists(rt) else "libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    buf = (C.c_uint8 * max(nbytes, 1))()
    assert hip.hipMemcpy(buf, C.c_void_p(ptr), nbytes, 2) == 0     # hipMemcpyDeviceToHost
    return bytes(buf)[:nbytes]


class Layout:
    """Sources and destinations of a list of chunks.  null_src / null_dst: the
    chunks whose source / destination address is NULL (their sizes and
    capacities stay as given: the entries zd_batch_create_device fails alone)."""

    def __init__(self, chunks, caps, seed, null_src=(), null_dst=()):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        rng = np.random.default_rng(seed)
        n = len(chunks)
        self.chunks, self.caps, self.n = chunks, list(caps), n
        self.null_src, self.null_dst = set(null_src), set(null_dst)
        offs, at = [], 1
        for c in chunks:
            at |= 1
            offs.append(at)
            at += len(c) + int(rng.integers(1, 6))
        host = np.full(at + 8, 0x5C, dtype=np.uint8)
        for o, c in zip(offs, chunks):
            host[o:o + len(c)] = np.frombuffer(c, dtype=np.uint8)
        self.src = torch.from_numpy(host).to(self.dev)
        self.src_ptrs = [0 if (i in self.null_src or not len(chunks[i])) else self.src.data_ptr() + o
                         for i, o in enumerate(offs)]
        self.src_sizes = [len(c) for c in chunks]
        order = [int(x) for x in rng.permutation(n)]
        if n > 1 and order[0] == 0:
            order[0], order[1] = order[1], order[0]
        self.dst_offs, at = [0] * n, GUARD + 1
        for j in order:
            at |= 1
            self.dst_offs[j] = at
            at += self.caps[j] + GUARD
        self.dst = torch.full((at + GUARD,), FILL, dtype=torch.uint8, device=self.dev)
        self.dst_ptrs = [0 if i in self.null_dst else self.dst.data_ptr() + o for i, o in enumerate(self.dst_offs)]
        if n > 1:
            assert min(range(n), key=lambda i: self.dst_offs[i]) != 0
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def tensors(self):
        t = self.torch
        return [t.tensor(v, dtype=t.int64, device=self.dev)
                for v in (self.src_ptrs, self.src_sizes, self.dst_ptrs, self.caps)]

    def device_batch(self, flags=0, dictionary=None):
        from zstd_decompressor.batch import Batch
        arrs = self.tensors()
        b = Batch.from_device(*arrs, flags=flags, dictionary=dictionary, stream=self.stream)
        assert b.info.device_built == 1 and b.nchunks == self.n
        return b

    def host_batch(self, flags=0, dictionary=None):
        """zd_batch_create over the same entries (a refused entry: the empty chunk it becomes)."""
        from zstd_decompressor.batch import Batch
        bad = self.null_src | self.null_dst
        z = lambda v: [0 if i in bad else x for i, x in enumerate(v)]
        b = Batch(z(self.src_ptrs), z(self.src_sizes), z(self.dst_ptrs), z(self.caps), flags=flags,
                  dictionary=dictionary, stream=self.stream)
        assert b.info.device_built == 0
        return b

    def refill(self):
        self.dst.fill_(FILL)
        self.torch.cuda.synchronize()

    def host(self):
        return self.dst.cpu().numpy()

    def check(self, h, statuses, lengths, want):
        outside = np.ones(h.size, dtype=bool)
        for i, (o, c) in enumerate(zip(self.dst_offs, self.caps)):
            if i not in self.null_dst:
                outside[o:o + c] = False
        assert (h[outside] == FILL).all(), "bytes outside the chunks' destinations were written"
        for i, (st, out) in enumerate(want):
            assert statuses[i] == st, (i, statuses[i], st)
            assert lengths[i] == len(out), (i, lengths[i], len(out))
            if i not in self.null_dst:
                assert h[self.dst_offs[i]:self.dst_offs[i] + len(out)].tobytes() == out, i

    def decode(self, b, want):
        """One decode of batch b: device arrays == host arrays, the common checks."""
        b.decode_async(self.stream)
        st, ln = b.results(self.stream)
        d_st, d_ln = b.device_results()
        assert list(np.frombuffer(read_device(d_st, 4 * self.n), dtype=np.int32)) == st
        assert list(np.frombuffer(read_device(d_ln, 8 * self.n), dtype=np.uint64)) == ln
        self.check(self.host(), st, ln, want)
        return st, ln

    def run(self, want, flags=0, dictionary=None, after=None):
        """The device-created batch against the oracle, then against the
        host-created one; returns (device info, host info)."""
        bad = self.null_src | self.null_dst
        d = self.device_batch(flags, dictionary)
        try:
            dst, dln = self.decode(d, want)
            dsum = d.checksums(self.stream)
            self.refill()
            h = self.host_batch(flags, dictionary)
            try:
                h.decode_async(self.stream)
                hst, hln = h.results(self.stream)
                keep = [i for i in range(self.n) if i not in bad]
                assert [dst[i] for i in keep] == [hst[i] for i in keep]
                assert [dln[i] for i in keep] == [hln[i] for i in keep]
                hsum = h.checksums(self.stream)
                assert [dsum[0][i] for i in keep] == [hsum[0][i] for i in keep]
                assert [dsum[1][i] for i in keep] == [hsum[1][i] for i in keep]
                for f in INFO_FIELDS:
                    assert getattr(d.info, f) == getattr(h.info, f), f
                if after:
                    after(d, h)
                return d.info, h.info
            finally:
                h.close()
        finally:
            d.close()
            self.refill()


# ---------------------------------------------------------------------------
# 1. mixed shapes, failing chunks among the good ones
# ---------------------------------------------------------------------------
def corrupt_table(frame: bytes) -> bytes:
    """`frame` with one bit flipped so that the oracle rejects a table
    description (ZD_E_CORRUPTED_TABLE / ZD_E_LARGE_ACCURACY_LOG): the first such flip."""
    from zstd_decompressor import _lib
    for k in range(9, len(frame) - 4):
        for bit in range(8):
            bad = frame[:k] + bytes([frame[k] ^ (1 << bit)]) + frame[k + 1:]
            if oracle.decompress_status(bad)[0] in (_lib.CORRUPTED_TABLE, _lib.LARGE_ACCURACY_LOG):
                return bad
    raise AssertionError("no flip gives a corrupted table in the oracle")


def padded_to(frame: bytes, size: int) -> bytes:
    """`frame` followed by one skippable frame, `size` bytes in all."""
    return frame + skippable(size - len(frame) - 8)


@functools.lru_cache(maxsize=None)
def mixed():
    """[(name, chunk, capacity or None for the oracle's length, expected or None
    for the oracle's, null: '' / 'src' / 'dst')]"""
    from zstd_decompressor import _lib
    rng = np.random.default_rng(0xDB7C)
    small = [libzstd.compress(gen.text(900 + 311 * i, seed=0xDB00 + i), 3) for i in range(32)]
    nofcs_src = gen.text(20 << 10, seed=0xDB20)
    nofcs = libzstd.compress(nofcs_src, 3, content_size=False)
    fcs = libzstd.compress(gen.text(6000, seed=0xDB21), 3)
    assert libzstd.frame_content_size(fcs) == 6000 and libzstd.frame_content_size(nofcs) != len(nofcs_src)
    t300 = libzstd.compress(gen.text(300 << 10, seed=0xDB22), 3)
    t4 = libzstd.compress(gen.text(4 << 10, seed=0xDB23), 3)
    t128 = libzstd.compress(gen.text(128 << 10, seed=0xDB24), 3)
    raw100 = libzstd.compress(rng.integers(0, 256, 100 << 10, dtype=np.uint8).tobytes())
    t90 = libzstd.compress(gen.text(60 << 10, seed=0xDB25), 3)
    assert len(blocks_of(t300)) == 3 and set(blocks_of(t300)) == {2}
    assert blocks_of(t4) == [2] and blocks_of(t128) == [2] and blocks_of(raw100) == [0]
    assert 3 * 32768 < len(raw100) <= 4 * 32768              # four gather pieces
    assert len(t90) < 32768 - 8
    bad_arg = (_lib.INVALID_ARG, b"")
    special = [
        ("300 KiB in three blocks", t300, None, None, ""),
        ("4 KiB single block", t4, None, None, ""),
        ("truncated", small[0][:len(small[0]) // 2], 4000, None, ""),
        ("128 KiB single block", t128, None, None, ""),
        ("100 KiB raw block", raw100, None, None, ""),
        ("trailing garbage", small[1] + b"\x01\x02\x03\x04\x05", 8000, None, ""),
        ("chunk of 32768 bytes", padded_to(t90, 32768), None, None, ""),
        ("chunk of 32769 bytes", padded_to(t90, 32769), None, None, ""),
        ("two zstd frames", small[2] + small[3], 16000, (_lib.OUT_OF_DOMAIN, b""), ""),
        ("RLE frame", rle_frame(40 << 10, 0x41), None, None, ""),
        ("FCS above capacity", fcs, 5999, (_lib.DST_TOO_SMALL, b""), ""),
        ("50 KiB without FCS", libzstd.compress(gen.text(50 << 10, seed=0xDB26), 3, content_size=False), None, None, ""),
        ("no FCS, one byte short", nofcs, len(nofcs_src) - 1, (_lib.DST_TOO_SMALL, b""), ""),
        ("10 KiB with checksum", libzstd.compress(gen.text(10 << 10, seed=0xDB27), 3, checksum=True), None, None, ""),
        ("corrupted table", corrupt_table(small[4]), 8000, None, ""),
        ("zero-byte chunk", b"", 7, None, ""),
        ("NULL source of 8 bytes", small[5][:8], 4000, bad_arg, "src"),
        ("skippable frames only", skippable(5) + skippable(3), 9, None, ""),
        ("NULL destination of 8 bytes", small[6], 8, bad_arg, "dst"),
        ("frame wrapped in skippable frames", skippable(5) + small[7] + skippable(11), None, None, ""),
        ("no FCS with room", nofcs, len(nofcs_src), None, ""),
    ]
    out, k = [], 8
    for s in special:                 # a good small chunk after every special one
        out.append(s)
        out.append(("small %d" % k, small[k], None, None, ""))
        k += 1
    assert len(out) >= 40
    return out


def mixed_layout(seed):
    from zstd_decompressor import _lib
    cases = mixed()
    names = [c[0] for c in cases]
    at = dict(zip(names, range(len(names))))
    chunks = [c[1] for c in cases]
    want = [c[3] if c[3] is not None else expect(c[1]) for c in cases]
    failing = {"truncated", "trailing garbage", "two zstd frames", "FCS above capacity", "no FCS, one byte short",
               "corrupted table", "NULL source of 8 bytes", "NULL destination of 8 bytes"}
    for k, (st, out) in zip(names, want):
        assert (st != 0) == (k in failing), (k, st)
        assert st == 0 or out == b""
    assert want[at["truncated"]][0] == _lib.NOT_ENOUGH_BYTES
    assert want[at["trailing garbage"]][0] == _lib.UNRECOGNIZED_MAGIC
    assert want[at["corrupted table"]][0] in (_lib.CORRUPTED_TABLE, _lib.LARGE_ACCURACY_LOG)
    assert [len(want[at[k]][1]) for k in ("zero-byte chunk", "skippable frames only")] == [0, 0]
    assert len(want[at["frame wrapped in skippable frames"]][1]) == 900 + 311 * 7
    assert [len(chunks[at[k]]) for k in ("chunk of 32768 bytes", "chunk of 32769 bytes")] == [32768, 32769]
    caps = [c[2] if c[2] is not None else len(want[i][1]) for i, c in enumerate(cases)]
    L = Layout(chunks, caps, seed, null_src=[i for i, c in enumerate(cases) if c[4] == "src"],
               null_dst=[i for i, c in enumerate(cases) if c[4] == "dst"])
    return L, want, at


def test_mixed_shapes_and_failures():
    L, want, at = mixed_layout(0xDB10)
    assert L.n >= 40

    def after(d, h):
        ok, digest = d.checksums(L.stream)
        assert ok[at["10 KiB with checksum"]] == 1
        assert [ok[i] for i in range(L.n) if i != at["10 KiB with checksum"]] == [-1] * (L.n - 1)
        assert digest[at["zero-byte chunk"]] == 0xEF46DB3751D8E999     # XXH64 of no bytes

    dinfo, hinfo = L.run(want, after=after)
    assert dinfo.nchunks == L.n and dinfo.nblocks > L.n - 10


# ---------------------------------------------------------------------------
# 2. tile edges: the 64-lane walk, the 256-entry scan tiles
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def small600():
    chunks = [libzstd.compress(gen.text(300 + (i * 37) % 700, seed=0xDC00 + i), 3) for i in range(600)]
    want = [expect(c) for c in chunks]
    assert all(st == 0 for st, _ in want) and all(blocks_of(c) == [2] for c in chunks[::41])
    return chunks, want


@pytest.mark.parametrize("no_fuse", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 600])
def test_tile_edges(n, no_fuse):
    from zstd_decompressor import _lib
    chunks, want = small600()
    flags = _lib.F_NO_FUSE if no_fuse else 0
    L = Layout(chunks[:n], [len(out) for _, out in want[:n]], seed=0xDC10 + n)
    dinfo, hinfo = L.run(want[:n], flags=flags)
    assert dinfo.executors == hinfo.executors and dinfo.nblocks == n
    if n in (257, 600) and not no_fuse:
        assert dinfo.executors & _lib.EXEC_FUSED
    if no_fuse:
        assert not dinfo.executors & _lib.EXEC_FUSED


# ---------------------------------------------------------------------------
# 3. executors
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def multiblock():
    sizes = (130 << 10, 200 << 10, 260 << 10, 390 << 10, 300 << 10)
    chunks = [libzstd.compress(gen.text(n, seed=0xDD00 + i), 3) for i, n in enumerate(sizes)]
    for c in chunks:
        t = blocks_of(c)
        assert set(t) == {2} and 2 <= len(t) <= 4
    want = [expect(c) for c in chunks]
    assert all(st == 0 for st, _ in want)
    return chunks, want


@pytest.mark.parametrize("flag", ["F_BLOCK_PARALLEL", "F_FRAME_SERIAL"])
def test_executors(flag):
    from zstd_decompressor import _lib
    chunks, want = multiblock()
    L = Layout(chunks, [len(out) for _, out in want], seed=0xDD10)
    dinfo, _ = L.run(want, flags=getattr(_lib, flag))
    assert bool(dinfo.executors & _lib.EXEC_K4J) == (flag == "F_BLOCK_PARALLEL")


def test_one_round_is_decoded_again_on_the_streaming_executor():
    from zstd_decompressor import _lib
    chunks, want = multiblock()
    L = Layout(chunks, [len(out) for _, out in want], seed=0xDD11)
    b = L.device_batch(_lib.F_BLOCK_PARALLEL | _lib.F_J_ONE_ROUND)
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
# 4. one dictionary
# ---------------------------------------------------------------------------
def test_one_dictionary():
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Dictionary
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
    # a record found wholly in the dictionary: one match, no literals
    inside = dct[-700:-100]
    fin = zdict.compress(inside, dct, 3)
    assert zdict.decompress(fin, dct, len(inside)) == inside and len(fin) < 40
    frames.append(fin)
    recs.append(inside)
    # a frame naming another dictionary: that chunk alone fails
    k = 3
    assert frames[k][4] & 3 == 3                                   # a 4-byte Dictionary_ID
    did_at = 5 + (0 if (frames[k][4] >> 5) & 1 else 1)
    assert int.from_bytes(frames[k][did_at:did_at + 4], "little") == idx["dict_id"]
    other = (idx["dict_id"] ^ 0x5A5A).to_bytes(4, "little")
    frames.append(frames[k][:did_at] + other + frames[k][did_at + 4:])
    recs.append(recs[k])
    want = [(0, r) for r in recs]
    want[-1] = (_lib.DICT_MISMATCH, b"")
    d = Dictionary(dct)
    try:
        L = Layout(frames, [len(r) for r in recs], seed=0xDE10)
        dinfo, _ = L.run(want, dictionary=d)
        assert dinfo.executors == 0
    finally:
        d.close()


# ---------------------------------------------------------------------------
# 5. a dictionary set
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("fallback", [0, -1])
def test_dictionary_set(fallback):
    from zstd_decompressor import _lib
    from test_dict_set_gpu import Dicts, derived, derived_frame, derived_record
    blobs = [derived(k) for k in range(3)]
    assert len({zdict.dict_id(b) for b in blobs}) == 3
    chunks, want = [], []
    for j in range(6):
        for k in (1, 2):                                           # round-robin over two of the three
            chunks.append(derived_frame(k, 0, j))
            want.append((0, derived_record(k, j)))
        # and records without an ID: the fallback (dictionary 0, else none) is theirs; a frame made
        # without a dictionary reads nothing before its own first byte, so it decodes alike with either
        plain = gen.text(800 + 97 * j, seed=0xDF00 + j)
        f = libzstd.compress(plain, 3)
        assert f[4] & 3 == 0                                       # no Dictionary_ID
        chunks.append(f)
        want.append((0, plain))
    assert all(c[4] & 3 != 0 for c in chunks[0:2])
    unknown = derived_frame(0, 9)                                   # names ID 9: the set lacks it
    chunks.insert(4, unknown)
    want.insert(4, (_lib.DICT_MISMATCH, b""))
    caps = [max(len(r), 1) + (i % 3) for i, (_, r) in enumerate(want)]
    caps[4] = len(derived_record(0))
    six = blobs + [derived(k) for k in (3, 4, 5)]
    with Dicts(blobs, fallback=fallback) as dset, Dicts(six, fallback=fallback) as dset6:
        L = Layout(chunks, caps, seed=0xDF10)
        dinfo, hinfo = L.run(want, dictionary=dset)
        assert dinfo.executors == 0
        # the plan's tables cover the dictionaries its chunks use, not the set's
        a, b = L.device_batch(0, dset), L.device_batch(0, dset6)
        try:
            assert a.info.workspace_bytes == b.info.workspace_bytes
            L.decode(b, want)
        finally:
            a.close()
            b.close()


# ---------------------------------------------------------------------------
# 6. relaunch
# ---------------------------------------------------------------------------
def test_relaunch():
    L, want, _ = mixed_layout(0xDB11)
    b = L.device_batch()
    try:
        runs = []
        for _ in range(2):
            L.refill()
            st, ln = L.decode(b, want)
            runs.append((st, ln, L.host()))
        assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1]
        assert (runs[0][2] == runs[1][2]).all()
    finally:
        b.close()


# ---------------------------------------------------------------------------
# 7. Batch.from_device: tensors, raw addresses; the batch owns its copies
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("raw", [False, True])
def test_from_device_owns_its_arrays(raw):
    import torch
    from zstd_decompressor.batch import Batch
    chunks, want = small600()
    chunks, want = chunks[:70], want[:70]
    L = Layout(chunks, [len(out) + (i % 4) for i, (_, out) in enumerate(want)], seed=0xE010)
    arrs = L.tensors()
    if raw:
        arrs[1] = arrs[1].view(torch.uint64) if hasattr(torch, "uint64") else arrs[1]
        b = Batch.from_device(*[a.data_ptr() for a in arrs], nchunks=L.n, stream=L.stream)
    else:
        b = Batch.from_device(*arrs, stream=L.stream)
    try:
        assert b.info.device_built == 1 and b.nchunks == L.n
        # the arrays (and the sources) go away before the decode
        del arrs
        L.src.fill_(0)
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        scribble = torch.full((4096,), -1, dtype=torch.int64, device=L.dev)   # (likely the arrays' old memory)
        torch.cuda.synchronize()
        L.decode(b, want)
        del scribble
    finally:
        b.close()


def test_from_device_argument_errors():
    import torch
    from zstd_decompressor.batch import Batch
    dev = torch.device("cuda", 0)
    a = torch.zeros(4, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError):
        Batch.from_device(a, a, a, a[:3])
    with pytest.raises(ValueError):
        Batch.from_device(a.to(torch.int32), a, a, a)
    with pytest.raises(ValueError):
        Batch.from_device(a.data_ptr(), a.data_ptr(), a.data_ptr(), a.data_ptr())
    with pytest.raises(ValueError):
        Batch.from_device(a.cpu(), a, a, a)
