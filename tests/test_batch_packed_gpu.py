"""The size query and the packed batches (include/zd.h zd_chunk_sizes_device,
zd_batch_create_device_packed / _dicts, zd_batch_output_layout,
zd_batch_bind_output; chunk_sizes, Batch.packed and decompress_tensors in
zstd_decompressor/batch.py): zd_k_chunk_sizes reading the chunks in place,
zd_k_batch_pack and the scan that lay a batch's outputs out, and the decode of
such a batch into a buffer bound afterwards.

Expected statuses and bytes come from the CPU oracle on each chunk alone (the
dictionary tests: from the source records), never from a batch; every test
first asserts that its good chunks are ZD_OK there.  Expected reserves are
computed here: a frame whose Frame_Content_Size libzstd reports expects that
size (the oracle's output length when it decodes) and exact 1; a frame made
with content_size=False expects exact 0 and 128 KiB for each compressed block
plus the sizes of its raw and RLE blocks, from the host index (frames_index).

Layout of every test: the sources packed into one uint8 tensor at odd offsets
with gaps of 1-5 bytes, the last chunk ending at the tensor's last byte; the
output buffer bound at an odd address inside a tensor filled with 0xA5, 32
guard bytes either side.  After every decode every byte outside the chunks'
[offset, offset + cap) is 0xA5.  Every packed batch is also compared with the
batch zd_batch_create_device makes from the same sources with dst = base +
offset and the same capacities: statuses, lengths, checksums and the
zd_batch_info fields nchunks / gathered_bytes / nblocks / nsequences / executors.
"""
import functools
import json
import os

import numpy as np
import pytest

from corpus import gen, libzstd, zdict
from test_batch_device_gpu import (FILL, GOLDEN, GUARD, INFO_FIELDS, expect, mixed, multiblock, read_device, small600)

pytestmark = pytest.mark.gpu

MAGIC_ZSTD = 0xFD2FB528
BLOCK_MAX = 128 << 10


def reserve_of(chunk: bytes):
    """(reserve, exact) of a chunk that holds one zstd frame, computed from
    libzstd's Frame_Content_Size and the host index, not from the code under test."""
    from zstd_decompressor.batch import frames_index
    frames, blocks, st, _ = frames_index(chunk)
    zf = [f for f in frames if f["magic"] == MAGIC_ZSTD]
    assert st == 0 and len(zf) == 1
    f = zf[0]
    bl = blocks[f["first_block"]:f["first_block"] + f["num_blocks"]]
    bound = sum(BLOCK_MAX if b["type"] == 2 else b["block_size"] for b in bl)
    frame = chunk[f["src_offset"]:f["src_offset"] + f["src_size"]]
    fcs = libzstd.frame_content_size(frame)
    if 0 <= fcs < 1 << 62:
        assert fcs <= bound
        return fcs, 1
    return bound, 0


class Sources:
    """Chunks in one device tensor at odd offsets, 1-5 byte gaps, the last chunk
    ending at the tensor's last byte.  null_src: chunks whose address is NULL."""

    def __init__(self, chunks, seed, null_src=()):
        import torch
        self.torch = torch
        self.dev = torch.device("cuda", 0)
        rng = np.random.default_rng(seed)
        self.chunks, self.n = list(chunks), len(chunks)
        offs, at = [], 1
        for c in chunks:
            at |= 1
            offs.append(at)
            at += len(c) + int(rng.integers(1, 6))
        end = max([o + len(c) for o, c in zip(offs, chunks)] + [1])
        host = np.full(end, 0x5C, dtype=np.uint8)
        for o, c in zip(offs, chunks):
            host[o:o + len(c)] = np.frombuffer(c, dtype=np.uint8)
        self.host_src = host
        self.src = torch.from_numpy(host.copy()).to(self.dev)
        if self.n and len(chunks[-1]):
            assert offs[-1] + len(chunks[-1]) == self.src.numel()
        self.ptrs = [0 if (i in set(null_src) or not len(chunks[i])) else self.src.data_ptr() + o
                     for i, o in enumerate(offs)]
        self.sizes = [len(c) for c in chunks]
        self.ptr_t = torch.tensor(self.ptrs, dtype=torch.int64, device=self.dev)
        self.size_t = torch.tensor(self.sizes, dtype=torch.int64, device=self.dev)
        self.stream = torch.cuda.current_stream(self.dev).cuda_stream

    def query(self, dictionary=False):
        from zstd_decompressor import chunk_sizes
        sz, st, ex = chunk_sizes(self.ptr_t, self.size_t, dictionary=dictionary)
        assert sz.dtype == self.torch.int64 and st.dtype == self.torch.int32 and ex.dtype == self.torch.uint8
        self.torch.cuda.synchronize()
        assert (self.src.cpu().numpy() == self.host_src).all(), "the size query wrote to the sources"
        return sz.tolist(), st.tolist(), ex.tolist()


def u64s(ptr, n):
    return [int(x) for x in np.frombuffer(read_device(ptr, 8 * n), dtype=np.uint64)]


def align_up(x, a):
    return (x + a - 1) // a * a


class Bound:
    """An output buffer for a packed batch: out_bytes at an odd address inside
    a tensor of 0xA5, GUARD bytes (and one more) before, GUARD after."""

    def __init__(self, S, out_bytes):
        t = S.torch
        self.lead = GUARD + 1
        self.buf = t.full((self.lead + out_bytes + GUARD,), FILL, dtype=t.uint8, device=S.dev)
        self.base = self.buf.data_ptr() + self.lead
        assert self.base & 1
        self.out_bytes = out_bytes

    def refill(self):
        self.buf.fill_(FILL)

    def host(self):
        return self.buf.cpu().numpy()

    def untouched(self):
        return bool((self.host() == FILL).all())


def check_layout(b, n, align, sizes=None):
    d_off, d_cap = b.output_layout()
    offs, caps = u64s(d_off, n), u64s(d_cap, n)
    if sizes is not None:
        assert caps == sizes
    assert all(o % align == 0 for o in offs)
    assert offs == sorted(offs) and (not n or offs[0] == 0)
    for i in range(n - 1):
        assert offs[i + 1] >= offs[i] + caps[i], i
        assert offs[i + 1] == offs[i] + align_up(caps[i], align), i
    assert b.out_bytes == sum(align_up(c, align) for c in caps)
    return offs, caps


def check_bytes(h, lead, offs, caps, statuses, lengths, want, slack=True):
    outside = np.ones(h.size, dtype=bool)
    for o, c in zip(offs, caps):
        outside[lead + o:lead + o + c] = False
    assert (h[outside] == FILL).all(), "bytes outside the chunks' places were written"
    for i, (st, out) in enumerate(want):
        assert statuses[i] == st, (i, statuses[i], st)
        assert lengths[i] == len(out), (i, lengths[i], len(out))
        assert len(out) <= caps[i]
        at = lead + offs[i]
        assert h[at:at + len(out)].tobytes() == out, i
        if slack and st == 0:
            assert (h[at + len(out):at + caps[i]] == FILL).all(), ("the slack after chunk %d was written" % i)


def decode_checked(S, b, O, offs, caps, want):
    """One decode of batch b into O: device arrays == host arrays, the common checks."""
    b.decode_async(S.stream)
    st, ln = b.results(S.stream)
    d_st, d_ln = b.device_results()
    assert list(np.frombuffer(read_device(d_st, 4 * S.n), dtype=np.int32)) == st
    assert u64s(d_ln, S.n) == ln
    check_bytes(O.host(), O.lead, offs, caps, st, ln, want)
    return st, ln


def run_packed(S, want, align, flags=0, dictionary=None, sizes=None, after=None):
    """The packed batch against the oracle, then against the batch
    zd_batch_create_device makes with the same places; returns the packed info."""
    from zstd_decompressor import Batch
    t = S.torch
    b = Batch.packed(S.ptr_t, S.size_t, align=align, flags=flags, dictionary=dictionary, stream=S.stream)
    try:
        assert b.info.device_built == 1 and b.nchunks == S.n
        offs, caps = check_layout(b, S.n, align, sizes)
        O = Bound(S, b.out_bytes)
        b.bind_output(O.base, b.out_bytes)
        pst, pln = decode_checked(S, b, O, offs, caps, want)
        psum = b.checksums(S.stream)
        if after:
            after(b, O, offs, caps)
        O.refill()
        dst_t = t.tensor([O.base + o for o in offs], dtype=t.int64, device=S.dev)
        cap_t = t.tensor(caps, dtype=t.int64, device=S.dev)
        d = Batch.from_device(S.ptr_t, S.size_t, dst_t, cap_t, flags=flags, dictionary=dictionary, stream=S.stream)
        try:
            d.decode_async(S.stream)
            dst, dln = d.results(S.stream)
            assert pst == dst and pln == dln
            assert psum == d.checksums(S.stream)
            for f in INFO_FIELDS:
                assert getattr(b.info, f) == getattr(d.info, f), f
            check_bytes(O.host(), O.lead, offs, caps, dst, dln, want)
        finally:
            d.close()
        return b.info
    finally:
        b.close()


# ---------------------------------------------------------------------------
# 1 / 3. mixed shapes, failing chunks among the good ones
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def mixed_sources():
    """(names, chunks, null sources, expected decode (status, bytes), expected
    (size, status, exact) of the size query): test_batch_device_gpu's mixed()
    list without its destinations and capacities."""
    from zstd_decompressor import _lib
    cases = mixed()
    names = [c[0] for c in cases]
    chunks = [c[1] for c in cases]
    null_src = [i for i, c in enumerate(cases) if c[4] == "src"]
    alone = [expect(c) for c in chunks]
    want, query = [], []
    failing = {"truncated": _lib.NOT_ENOUGH_BYTES, "trailing garbage": _lib.UNRECOGNIZED_MAGIC,
               "two zstd frames": _lib.OUT_OF_DOMAIN}
    for i, name in enumerate(names):
        st, out = alone[i]
        if i in null_src:
            want.append((_lib.INVALID_ARG, b""))
            query.append((0, _lib.INVALID_ARG, 0))
        elif name in failing:
            assert name == "two zstd frames" or st == failing[name], (name, st)
            want.append((failing[name], b""))
            query.append((0, failing[name], 0))
        elif name == "corrupted table":
            assert st in (_lib.CORRUPTED_TABLE, _lib.LARGE_ACCURACY_LOG)
            want.append((st, b""))
            r, ex = reserve_of(chunks[i])
            assert ex == 1 and r == 900 + 311 * 4
            query.append((r, 0, 1))
        elif name in ("zero-byte chunk", "skippable frames only"):
            assert (st, out) == (0, b"")
            want.append((0, b""))
            query.append((0, 0, 0))
        else:
            assert st == 0, (name, st)
            want.append((0, out))
            r, ex = reserve_of(chunks[i])
            assert r == len(out) if ex else r >= len(out)
            query.append((r, 0, ex))
    at = dict(zip(names, range(len(names))))
    assert all(k in at for k in failing) and len(null_src) == 1 and len(names) >= 40
    for k in ("50 KiB without FCS", "no FCS with room", "no FCS, one byte short"):
        assert query[at[k]] == (BLOCK_MAX, 0, 0)
    assert query[at["300 KiB in three blocks"]] == (300 << 10, 0, 1)
    return names, chunks, null_src, want, query


def test_sizes_mixed():
    names, chunks, null_src, want, query = mixed_sources()
    S = Sources(chunks, 0xE110, null_src=null_src)
    sz, st, ex = S.query()
    for i, name in enumerate(names):
        assert (sz[i], st[i], ex[i]) == query[i], (name, (sz[i], st[i], ex[i]), query[i])


@pytest.mark.parametrize("align", [1, 16, 256])
def test_packed_mixed(align):
    names, chunks, null_src, want, query = mixed_sources()
    S = Sources(chunks, 0xE120 + align, null_src=null_src)
    sz, _, _ = S.query()
    at = dict(zip(names, range(len(names))))

    def after(b, O, offs, caps):
        ok, digest = b.checksums(S.stream)
        assert ok[at["10 KiB with checksum"]] == 1
        assert digest[at["zero-byte chunk"]] == 0xEF46DB3751D8E999     # XXH64 of no bytes

    info = run_packed(S, want, align, sizes=sz, after=after)
    assert [q[0] for q in query] == sz
    assert info.nchunks == S.n and info.nblocks > S.n - 10


# ---------------------------------------------------------------------------
# 2 / 4. tile edges: the 64-lane walk, the 256-entry scan tiles
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,optional", [(n, o) for n in (1, 63, 64, 65, 257) for o in (True, False)] + [(600, True)])
def test_sizes_tile_edges(n, optional):
    import torch
    from zstd_decompressor import _lib
    chunks, want = small600()
    S = Sources(chunks[:n], 0xE200 + n)
    expected = [len(out) for _, out in want[:n]]
    if n == 1:
        assert reserve_of(chunks[0]) == (expected[0], 1)
    if optional:
        sz, st, ex = S.query()
        assert st == [0] * n and ex == [1] * n
    else:
        d_size = torch.full((n + 1,), -7, dtype=torch.int64, device=S.dev)
        r = _lib.lib().zd_chunk_sizes_device(S.ptr_t.data_ptr(), S.size_t.data_ptr(), n, 0, d_size.data_ptr(), None,
                                             None, S.stream)
        assert r == 0
        torch.cuda.synchronize()
        sz = d_size.tolist()
        assert sz[n] == -7
        sz = sz[:n]
    assert sz == expected


@pytest.mark.parametrize("no_fuse", [False, True])
@pytest.mark.parametrize("n", [1, 64, 65, 256, 257, 600])
def test_packed_tile_edges(n, no_fuse):
    from zstd_decompressor import _lib
    chunks, want = small600()
    flags = _lib.F_NO_FUSE if no_fuse else 0
    S = Sources(chunks[:n], 0xE300 + n)
    info = run_packed(S, want[:n], 16, flags=flags, sizes=[len(out) for _, out in want[:n]])
    assert info.nblocks == n
    if n in (257, 600) and not no_fuse:
        assert info.executors & _lib.EXEC_FUSED
    if no_fuse:
        assert not info.executors & _lib.EXEC_FUSED


# ---------------------------------------------------------------------------
# 5. executors
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["F_BLOCK_PARALLEL", "F_FRAME_SERIAL"])
def test_executors(flag):
    from zstd_decompressor import _lib
    chunks, want = multiblock()
    S = Sources(chunks, 0xE400)
    info = run_packed(S, want, 16, flags=getattr(_lib, flag), sizes=[len(out) for _, out in want])
    assert bool(info.executors & _lib.EXEC_K4J) == (flag == "F_BLOCK_PARALLEL")


def test_one_round_is_decoded_again_at_its_packed_place():
    from zstd_decompressor import Batch, _lib
    chunks, want = multiblock()
    S = Sources(chunks, 0xE401)
    b = Batch.packed(S.ptr_t, S.size_t, align=64, flags=_lib.F_BLOCK_PARALLEL | _lib.F_J_ONE_ROUND, stream=S.stream)
    try:
        assert b.info.executors & _lib.EXEC_K4J
        offs, caps = check_layout(b, S.n, 64, [len(out) for _, out in want])
        O = Bound(S, b.out_bytes)
        b.bind_output(O.base, b.out_bytes)
        b.decode_async(S.stream)
        S.torch.cuda.synchronize()
        d_st, d_ln = b.device_results()
        before = list(np.frombuffer(read_device(d_st, 4 * S.n), dtype=np.int32))
        assert _lib.OUT_OF_DOMAIN in before, "one round of one hop converged: the test is not about the re-decode"
        st, ln = b.results(S.stream)
        check_bytes(O.host(), O.lead, offs, caps, st, ln, want)
        assert list(np.frombuffer(read_device(d_st, 4 * S.n), dtype=np.int32)) == st == [0] * S.n
        assert u64s(d_ln, S.n) == ln
    finally:
        b.close()


# ---------------------------------------------------------------------------
# 6. frames without a usable Frame_Content_Size among frames with one
# ---------------------------------------------------------------------------
def test_no_usable_content_size():
    srcs = [gen.text(20 << 10, seed=0xE500), gen.text(50 << 10, seed=0xE501)]
    nofcs = [libzstd.compress(s, 3, content_size=False) for s in srcs]
    small, swant = small600()
    chunks = [small[0], nofcs[0], small[1], small[2], nofcs[1], small[3]]
    want = [expect(c) for c in chunks]
    assert all(st == 0 for st, _ in want) and [want[1][1], want[4][1]] == srcs
    expected = [reserve_of(c) for c in chunks]
    assert expected[1] == (BLOCK_MAX, 0) and expected[4] == (BLOCK_MAX, 0)
    assert [e[1] for e in expected] == [1, 0, 1, 1, 0, 1]
    S = Sources(chunks, 0xE510)
    sz, st, ex = S.query()
    assert list(zip(sz, ex)) == expected and st == [0] * 6
    # (run_packed's check_bytes: the oracle's lengths, and every byte of [offset + length, offset + cap) still 0xA5)
    run_packed(S, want, 16, sizes=sz)


# ---------------------------------------------------------------------------
# 7. dictionaries
# ---------------------------------------------------------------------------
def empty_raw_literals(frame: bytes) -> bool:
    """The frame's first block is compressed and opens with a Raw literals section of no bytes."""
    from zstd_decompressor.batch import frames_index
    frames, blocks, st, _ = frames_index(frame)
    if st != 0 or len(frames) != 1 or blocks[0]["type"] != 2:
        # (the host index refuses such a block without a dictionary: look at the bytes)
        fhd = frame[4]
        at = 5 + (0 if (fhd >> 5) & 1 else 1) + (0, 1, 2, 4)[fhd & 3] + ((1 if (fhd >> 5) & 1 else 0), 2, 4, 8)[fhd >> 6]
        bh = int.from_bytes(frame[at:at + 3], "little")
        return (bh >> 1) & 3 == 2 and frame[at + 3] == 0
    return frame[blocks[0]["src_offset"]] == 0


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
    assert zdict.decompress(fin, dct, len(inside)) == inside and len(fin) < 40 and empty_raw_literals(fin)
    frames.append(fin)
    recs.append(inside)
    k_empty = len(frames) - 1
    # a frame naming another dictionary: that chunk alone fails, when it is decoded
    k = 3
    assert frames[k][4] & 3 == 3
    did_at = 5 + (0 if (frames[k][4] >> 5) & 1 else 1)
    assert int.from_bytes(frames[k][did_at:did_at + 4], "little") == idx["dict_id"]
    other = (idx["dict_id"] ^ 0x5A5A).to_bytes(4, "little")
    frames.append(frames[k][:did_at] + other + frames[k][did_at + 4:])
    recs.append(recs[k])
    for f, r in zip(frames, recs):
        assert libzstd.frame_content_size(f) == len(r)
    want = [(0, r) for r in recs]
    want[-1] = (_lib.DICT_MISMATCH, b"")
    S = Sources(frames, 0xE600)
    sz, st, ex = S.query(dictionary=True)
    assert sz == [len(r) for r in recs] and st == [0] * S.n and ex == [1] * S.n
    sz0, st0, ex0 = S.query(dictionary=False)
    assert (sz0[k_empty], st0[k_empty], ex0[k_empty]) == (0, _lib.EMPTY_SLICE, 0)
    keep = [i for i in range(S.n) if i != k_empty and not empty_raw_literals(frames[i])]
    assert len(keep) >= 5 and all((sz0[i], st0[i], ex0[i]) == (sz[i], 0, 1) for i in keep)
    d = Dictionary(dct)
    try:
        info = run_packed(S, want, 16, dictionary=d, sizes=sz)
        assert info.executors == 0
    finally:
        d.close()


@pytest.mark.parametrize("fallback", [0, -1])
def test_dictionary_set(fallback):
    from zstd_decompressor import _lib
    from test_dict_set_gpu import Dicts, derived, derived_frame, derived_record
    blobs = [derived(k) for k in range(3)]
    chunks, want = [], []
    for j in range(6):
        for k in (1, 2):
            chunks.append(derived_frame(k, 0, j))
            want.append((0, derived_record(k, j)))
        plain = gen.text(800 + 97 * j, seed=0xDF00 + j)
        f = libzstd.compress(plain, 3)
        assert f[4] & 3 == 0                                       # no Dictionary_ID: the fallback, or none
        chunks.append(f)
        want.append((0, plain))
    unknown = derived_frame(0, 9)                                   # names ID 9: the set lacks it
    chunks.insert(4, unknown)
    want.insert(4, (_lib.DICT_MISMATCH, b""))
    expected = [len(r) for _, r in want]
    expected[4] = len(derived_record(0))
    for c, e in zip(chunks, expected):
        assert libzstd.frame_content_size(c) == e
    S = Sources(chunks, 0xE610)
    sz, st, ex = S.query(dictionary=True)
    assert sz == expected and st == [0] * S.n and ex == [1] * S.n
    with Dicts(blobs, fallback=fallback) as dset:
        info = run_packed(S, want, 16, dictionary=dset, sizes=sz)
        assert info.executors == 0


# ---------------------------------------------------------------------------
# 8. binding
# ---------------------------------------------------------------------------
def test_binding():
    import torch
    from zstd_decompressor import Batch, ZdError, _lib
    chunks, want = small600()
    chunks, want = chunks[:70], want[:70]
    S = Sources(chunks, 0xE700)
    b = Batch.packed(S.ptr_t, S.size_t, align=16, stream=S.stream)
    try:
        offs, caps = check_layout(b, S.n, 16, [len(out) for _, out in want])
        assert b.out_bytes > 0
        with pytest.raises(ZdError) as e:
            b.decode_async(S.stream)                               # no binding yet
        assert e.value.code == _lib.INVALID_ARG
        A, B = Bound(S, b.out_bytes), Bound(S, b.out_bytes)
        with pytest.raises(ZdError) as e:
            b.bind_output(A.base, b.out_bytes - 1)
        assert e.value.code == _lib.DST_TOO_SMALL
        with pytest.raises(ZdError) as e:
            b.decode_async(S.stream)                               # (a refused binding binds nothing)
        assert e.value.code == _lib.INVALID_ARG
        with pytest.raises(ZdError) as e:
            b.bind_output(0, b.out_bytes)
        assert e.value.code == _lib.INVALID_ARG
        b.bind_output(A.base, b.out_bytes)
        with pytest.raises(ZdError) as e:
            b.bind_output(B.base, b.out_bytes - 1)                 # one byte short: A stays bound
        assert e.value.code == _lib.DST_TOO_SMALL
        decode_checked(S, b, A, offs, caps, want)
        assert B.untouched()
        a_bytes = A.host().copy()
        b.bind_output(B.base, b.out_bytes + GUARD)                 # (a larger capacity is fine)
        decode_checked(S, b, B, offs, caps, want)
        assert (B.host() == a_bytes).all()
        A.refill()
        B.refill()
        decode_checked(S, b, B, offs, caps, want)
        assert A.untouched()
        # a tensor binds by itself
        t = torch.full((b.out_bytes,), FILL, dtype=torch.uint8, device=S.dev)
        b.bind_output(t)
        b.decode_async(S.stream)
        st, ln = b.results(S.stream)
        assert st == [0] * S.n
        h = t.cpu().numpy()
        assert all(h[o:o + len(out)].tobytes() == out for o, (_, out) in zip(offs, want))
    finally:
        b.close()
    # a batch that was not made packed refuses both calls
    O = Bound(S, sum(caps))
    dst_t = torch.tensor([O.base + sum(caps[:i]) for i in range(S.n)], dtype=torch.int64, device=S.dev)
    cap_t = torch.tensor(caps, dtype=torch.int64, device=S.dev)
    d = Batch.from_device(S.ptr_t, S.size_t, dst_t, cap_t, stream=S.stream)
    try:
        with pytest.raises(ZdError) as e:
            d.output_layout()
        assert e.value.code == _lib.INVALID_ARG
        with pytest.raises(ZdError) as e:
            d.bind_output(O.base, sum(caps))
        assert e.value.code == _lib.INVALID_ARG
    finally:
        d.close()


# ---------------------------------------------------------------------------
# 9. decompress_tensors / chunk_sizes on tensors
# ---------------------------------------------------------------------------
def test_decompress_tensors():
    import torch
    from zstd_decompressor import _lib, chunk_sizes, decompress_tensors
    chunks, want = small600()
    chunks, want = list(chunks[100:110]), list(want[100:110])
    chunks[6] = chunks[6][:len(chunks[6]) // 2]
    want[6] = expect(chunks[6])
    assert want[6] == (_lib.NOT_ENOUGH_BYTES, b"")
    dev = torch.device("cuda", 0)
    srcs = [torch.from_numpy(np.frombuffer(c, dtype=np.uint8).copy()).to(dev) for c in chunks]
    ptrs = torch.tensor([t.data_ptr() for t in srcs], dtype=torch.int64, device=dev)
    sizes = torch.tensor([t.numel() for t in srcs], dtype=torch.int64, device=dev)
    sz, st, ex = chunk_sizes(ptrs, sizes)
    assert sz.tolist() == [len(out) for _, out in want]
    assert st.tolist() == [s for s, _ in want] and ex.tolist() == [int(s == 0) for s, _ in want]
    # the same through raw addresses
    sz2, st2, ex2 = chunk_sizes(ptrs.data_ptr(), sizes.data_ptr(), nchunks=len(srcs))
    assert sz2.tolist() == sz.tolist() and st2.tolist() == st.tolist() and ex2.tolist() == ex.tolist()
    outs, statuses = decompress_tensors(srcs)
    assert statuses == [s for s, _ in want]
    for i, (_, out) in enumerate(want):
        assert outs[i].cpu().numpy().tobytes() == out, i
    assert outs[6].numel() == 0
    assert all(o.data_ptr() % 16 == 0 for i, o in enumerate(outs) if i != 6)
    assert decompress_tensors([]) == ([], [])


# ---------------------------------------------------------------------------
# 10. the size query in a HIP graph: no allocation, no copy, no synchronisation
# ---------------------------------------------------------------------------
def test_size_query_capture_replay():
    import torch
    from zstd_decompressor import _lib
    chunks, want = small600()
    n = 130
    S = Sources(chunks[:n], 0xE900)
    expected = [len(out) for _, out in want[:n]]
    d_size = torch.zeros(n, dtype=torch.int64, device=S.dev)
    d_status = torch.zeros(n, dtype=torch.int32, device=S.dev)
    d_exact = torch.zeros(n, dtype=torch.uint8, device=S.dev)
    s = torch.cuda.Stream(S.dev)

    def query():
        r = _lib.lib().zd_chunk_sizes_device(S.ptr_t.data_ptr(), S.size_t.data_ptr(), n, 0, d_size.data_ptr(),
                                             d_status.data_ptr(), d_exact.data_ptr(), s.cuda_stream)
        assert r == 0
    torch.cuda.synchronize(S.dev)
    with torch.cuda.stream(s):              # warm-up outside the capture
        query()
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        query()
    for _ in range(2):
        d_size.fill_(-1)
        d_status.fill_(-1)
        d_exact.fill_(9)
        torch.cuda.synchronize(S.dev)
        g.replay()
        torch.cuda.synchronize(S.dev)
        assert d_size.tolist() == expected and d_status.tolist() == [0] * n and d_exact.tolist() == [1] * n
