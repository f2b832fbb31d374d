"""Dictionary sets on the GPU path (include/zd.h zd_dict_set_create,
zd_plan_create_dicts, zd_batch_create_dicts; DictionarySet in
zstd_decompressor/batch.py): one plan or batch whose frames each choose their
dictionary by the Dictionary_ID in their header -- the planner's per-frame
dictionary table (zd_plan.h PlanCtx::dset), one prebuilt comp per dictionary a
plan uses, and the streaming K4 reading each frame's dictionary pointer
(zd_k_execute_dicts).

As in test_dict_gpu.py the expected bytes are the source records, which
libzstd reproduces from the same frames with the same dictionary
(corpus/zdict.py), and every test first asserts, from the frames' own bytes,
that they have the shape it is about.
"""
import ctypes as C
import functools

import numpy as np
import pytest

from corpus import gen, libzstd, zdict
from oracle import oracle

from test_dict_gpu import (decode_device, decode_host, entropy_layout, first_block_shape, header_layout, raw5000,
                           records_of, trained112, trained16, treeless_repeat, _flag)

pytestmark = pytest.mark.gpu

SIZES = (512, 1024, 4096, 8192)


# ---------------------------------------------------------------------------
# corpora (seeded; built once per session)
# ---------------------------------------------------------------------------
def _records64(blob: bytes):
    recs, at = [], 0
    for i in range(64):
        n = SIZES[i % 4]
        recs.append(blob[at:at + n])
        at += n
    return recs


@functools.lru_cache(maxsize=None)
def trained():
    """The four trained dictionaries: name -> (dictionary, 64 records of 512 B,
    1 KiB, 4 KiB and 8 KiB (16 of each), their frames at level 3)."""
    total = 16 * sum(SIZES)
    text16, trecs, tframes = trained16()
    xml16 = zdict.train(records_of(gen.xml(512 * 4096, seed=0xD5C0), 4096), 16 << 10)
    bin16 = zdict.train(records_of(gen.binary(512 * 4096, seed=0xD5C1), 4096), 16 << 10)
    text112 = trained112()
    out = {"text": (text16, list(trecs[:64]), list(tframes[:64]))}
    for name, d, blob in (("xml", xml16, gen.xml(total, seed=0xD5C2)),
                          ("text112", text112, gen.text(total, seed=0xD5C3)),
                          ("binary", bin16, gen.binary(total, seed=0xD5C4))):
        recs = _records64(blob)
        out[name] = (d, recs, [zdict.compress(r, d, 3) for r in recs])
    return out


NAMES = ("text", "xml", "text112", "binary")


def check_trained_shapes():
    T = trained()
    ids = [zdict.dict_id(T[n][0]) for n in NAMES]
    assert len(set(ids)) == 4 and 0 not in ids
    for n, did in zip(NAMES, ids):
        for f in T[n][2]:
            at, size = header_layout(f)[:2]
            assert size == 4 and int.from_bytes(f[at:at + 4], "little") == did
    assert sum(treeless_repeat(f) for f in T["text"][2]) >= 48
    assert sum(treeless_repeat(f) for f in T["xml"][2]) >= 48
    assert sum(treeless_repeat(f) for f in T["text112"][2]) == 64
    assert all(first_block_shape(f)[3] == (3, 3, 3) for f in T["binary"][2])


def interleaved(names=NAMES, count=64):
    """(frames, records) round-robin over the dictionaries: neighbouring frames never share one."""
    T = trained()
    frames, recs = [], []
    for i in range(count):
        for n in names:
            frames.append(T[n][2][i])
            recs.append(T[n][1][i])
    return frames, recs


@functools.lru_cache(maxsize=None)
def derived(k: int, did: int = 0) -> bytes:
    """A cheap formatted dictionary: trained16's entropy tables and repeat
    offsets (1, 4, 8), the ID `did` (default 1000 + k) and a content of its own,
    gen.text of 3000 + 997 k bytes."""
    base = trained16()[0]
    _, _, rep_at, content_at = entropy_layout(base)
    assert [int.from_bytes(base[rep_at + 4 * i:rep_at + 4 * i + 4], "little") for i in range(3)] == [1, 4, 8]
    body = gen.text(3000 + 997 * k, seed=0xD5E0 + k)
    return base[:4] + (did or 1000 + k).to_bytes(4, "little") + base[8:content_at] + body


@functools.lru_cache(maxsize=None)
def derived_record(k: int, j: int = 0) -> bytes:
    body = gen.text(3000 + 997 * k, seed=0xD5E0 + k)
    return gen.text(2048, seed=0xD5A0 + 64 * j + k) + body[-700:]


@functools.lru_cache(maxsize=None)
def derived_frame(k: int, did: int = 0, j: int = 0) -> bytes:
    f = zdict.compress(derived_record(k, j), derived(k, did), 3)
    assert j or treeless_repeat(f)          # (the first record of each: Treeless literals, Repeat tables)
    return f


def content_of(d: bytes) -> bytes:
    return d[entropy_layout(d)[3]:] if d[:4] == b"\x37\xa4\x30\xec" else d


# ---------------------------------------------------------------------------
# GPU helpers
# ---------------------------------------------------------------------------
class Dicts:
    """Dictionary objects and a DictionarySet over them, closed together."""

    def __init__(self, blobs, fallback=0):
        from zstd_decompressor import Dictionary, DictionarySet
        self.ds = [Dictionary(b) for b in blobs]
        self.set = DictionarySet(self.ds, fallback=fallback)

    def __enter__(self):
        return self.set

    def __exit__(self, *a):
        self.set.close()
        for d in self.ds:
            d.close()


def both_paths(frames, recs, dset, flags=0):
    """zd_decode_async + zd_plan_results and zd_plan_decompress: every frame's bytes are its record."""
    data = b"".join(frames)
    st, fst, parts, _, info = decode_device(data, dset, flags)
    assert st == 0 and fst == [0] * len(frames) and info.executors == 0 and info.nframes == len(frames)
    for i, (r, got) in enumerate(zip(recs, parts)):
        assert got == r, i
    st, out, hinfo = decode_host(data, dset, flags)
    assert st == 0 and out == b"".join(recs) and hinfo["executors"] == 0 and hinfo["replans"] == 0
    return info


# ---------------------------------------------------------------------------
# 1. four dictionaries interleaved frame by frame
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("flag", ["", "F_SEQ_NO_LATENCY", "F_SEQ_ONE_LANE", "F_K1_LANES", "F_K1_SPLIT"])
def test_interleaved_dictionaries(flag):
    check_trained_shapes()
    T = trained()
    # libzstd refuses a frame under another of the four dictionaries
    for n, other in zip(NAMES, NAMES[1:] + NAMES[:1]):
        with pytest.raises(RuntimeError):
            zdict.decompress(T[n][2][5], T[other][0], len(T[n][1][5]))
    frames, recs = interleaved()
    assert len(frames) == 256
    with Dicts([T[n][0] for n in NAMES], fallback=0) as dset:
        assert dset.dict_ids == tuple(zdict.dict_id(T[n][0]) for n in NAMES)
        info = both_paths(frames, recs, dset, _flag(flag))
        assert info.ncompressed == 256


# ---------------------------------------------------------------------------
# 2. dictionaries of different content sizes; sources that straddle the boundary
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def straddle_corpus():
    """Per dictionary: records that repeat its content's last k bytes (a
    match source that starts in the dictionary and runs into the frame, periods
    below, at and above 16), and records of pieces from all over its content."""
    T = trained()
    blobs = [raw5000(), T["text"][0], T["text112"][0], derived(0), derived(1)]
    rng = np.random.default_rng(0xD5F0)
    per = []
    for b in blobs:
        c = content_of(b)
        recs = []
        for i, k in enumerate((1, 7, 15, 16, 17, 33, 100)):
            recs.append((c[-k:] * (3200 // k + 1))[:200 + 47 * i + 13 * len(per)])
        for _ in range(3):
            parts = []
            for _ in range(12):
                n = int(rng.integers(40, 300))
                at = int(rng.integers(0, len(c) - n))
                parts.append(c[at:at + n])
                parts.append(rng.integers(0, 256, int(rng.integers(0, 6)), dtype=np.uint8).tobytes())
            recs.append(b"".join(parts))
        frames = [zdict.compress(r, b, 3) for r in recs]
        for r, f in zip(recs, frames):
            assert zdict.decompress(f, b, len(r)) == r
        per.append((recs, frames))
    return blobs, per


def test_content_sizes_and_straddle():
    blobs, per = straddle_corpus()
    assert [len(content_of(b)) for b in blobs[:1] + blobs[3:]] == [5000, 3000, 3997]
    assert len({len(content_of(b)) for b in blobs}) == 5
    for b, (recs, frames) in zip(blobs, per):
        did = zdict.dict_id(b)
        for f in frames:
            at, size = header_layout(f)[:2]
            # (the raw dictionary's frames carry no ID field: they take the fallback)
            assert (size == 0) if did == 0 else (size > 0 and int.from_bytes(f[at:at + size], "little") == did)
        # the repeats are matches from the very start of the frame (few sequences, a source in the
        # dictionary's tail), the pieces are found in the dictionary (frames far smaller than records)
        for r, f in list(zip(recs, frames))[:7]:
            assert first_block_shape(f)[0] == 2 and 1 <= first_block_shape(f)[2] <= 3 and len(f) < 64, len(f)
        assert 3 * sum(map(len, frames[7:])) < sum(map(len, recs[7:]))
    frames, recs = [], []
    for i in range(10):
        for rs, fs in per:
            frames.append(fs[i])
            recs.append(rs[i])
    with Dicts(blobs, fallback=0) as dset:
        both_paths(frames, recs, dset)


# ---------------------------------------------------------------------------
# 3. fallback = -1: frames without a dictionary among frames with one
# ---------------------------------------------------------------------------
def test_frames_without_a_dictionary():
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import frames_index
    T = trained()
    plain_recs = [gen.text(300, seed=0xD601), gen.text(4096, seed=0xD602), gen.text(300 << 10, seed=0xD603),
                  gen.text(4096, seed=0xD604)]
    plain = [libzstd.compress(r, 3) for r in plain_recs]
    assert all(header_layout(f)[1] == 0 for f in plain)                 # no Dictionary_ID
    assert frames_index(plain[2])[0][0]["num_blocks"] == 3
    t, x = T["text"], T["xml"]
    # a plain frame first, one between two frames of different dictionaries, one last
    frames = [plain[0], t[2][0], plain[1], x[2][0], x[2][1], plain[2], t[2][1], t[2][2], x[2][2], plain[3]]
    recs = [plain_recs[0], t[1][0], plain_recs[1], x[1][0], x[1][1], plain_recs[2], t[1][1], t[1][2], x[1][2],
            plain_recs[3]]
    where = [0, 2, 5, 9]
    # the plain frames alone in a plan made without a dictionary
    st0, fst0, parts0, _, info0 = decode_device(b"".join(plain), None)
    assert st0 == 0 and parts0 == plain_recs
    with Dicts([t[0], x[0]], fallback=-1) as dset:
        data = b"".join(frames)
        st, fst, parts, _, info = decode_device(data, dset)
        assert st == 0 and fst == [0] * 10 and info.executors == 0
        assert [parts[i] for i in where] == parts0 and [fst[i] for i in where] == fst0
        assert parts == recs
        st, out, _ = decode_host(data, dset)
        assert st == 0 and out == b"".join(recs)
        # a plan none of whose frames uses a dictionary of its set
        st, fst, parts, _, info = decode_device(b"".join(plain), dset)
        assert (st, fst, parts) == (st0, fst0, parts0) and info.executors == 0
        assert info.ncompressed == info0.ncompressed and info.nsequences == info0.nsequences
        # a frame without an ID that needs a dictionary (a raw-dictionary frame of
        # test 2: pieces from all over the dictionary, literals between them): a
        # match before the frame's start, what a plain plan gives it
        needy = straddle_corpus()[1][0][1][7]
        assert header_layout(needy)[1] == 0 and first_block_shape(needy)[2] > 1
        want_st, want_out = oracle.decompress_status(needy)
        pst, pfst, _, _, _ = decode_device(needy, None)
        assert pst == want_st == _lib.IMPOSSIBLE_VALUE and want_out == b"" and pfst == [pst]
        st, fst, parts, _, _ = decode_device(b"".join(frames[:4]) + needy + frames[4], dset)
        assert st == pst and fst == [0] * 4 + pfst + [_lib.NOT_DECODED]
        assert parts[:4] == recs[:4]
        # (the one difference from a plain plan, plan-wide in every dictionary
        # plan: a Raw literals section of 0 bytes -- a record found wholly in its
        # dictionary -- is an EmptySlice there, and is read on here)
        empty = straddle_corpus()[1][0][1][3]
        assert header_layout(empty)[1] == 0 and first_block_shape(empty)[1:3] == (0, 1)
        assert decode_device(empty, None)[0] == oracle.decompress_status(empty)[0] == _lib.EMPTY_SLICE
        assert decode_device(empty, dset)[0] == _lib.IMPOSSIBLE_VALUE


# ---------------------------------------------------------------------------
# 4. IDs the set does not hold; IDs swapped between members
# ---------------------------------------------------------------------------
def test_unknown_and_swapped_ids():
    from zstd_decompressor import _lib
    T = trained()
    ids = (5, 300, 70000)
    blobs = [derived(k, did) for k, did in enumerate(ids)]
    frames = [derived_frame(k, did) for k, did in enumerate(ids)]
    recs = [derived_record(k) for k in range(3)]
    assert [header_layout(f)[1] for f in frames] == [1, 2, 4]           # Dictionary_ID fields of 1, 2 and 4 bytes
    for f, did in zip(frames, ids):
        at, size = header_layout(f)[:2]
        assert int.from_bytes(f[at:at + size], "little") == did
    stranger = derived_frame(3, 9)                                      # ID 9: not in the set
    six = derived(4, 6)                                                 # ID 6: one bit from ID 5
    with Dicts(blobs + [six, T["text"][0], T["xml"][0]], fallback=-1) as dset:
        both_paths(frames * 2, recs * 2, dset)
        data = b"".join(frames) + stranger + b"".join(frames)
        st, fst, parts, _, _ = decode_device(data, dset)
        assert st == _lib.DICT_MISMATCH
        assert fst == [0] * 3 + [_lib.DICT_MISMATCH] + [_lib.NOT_DECODED] * 3
        assert parts[:3] == recs
        st, out, _ = decode_host(data, dset)
        assert st == _lib.DICT_MISMATCH and out == b"".join(recs)
        # a frame whose ID names another member decodes with THAT dictionary: never the record
        at, size = header_layout(frames[0])[:2]
        swapped = frames[0][:at] + (6).to_bytes(1, "little") + frames[0][at + 1:]
        try:
            assert zdict.decompress(swapped, six, len(recs[0])) != recs[0]
        except RuntimeError:
            pass
        st, fst, parts, _, _ = decode_device(frames[1] + swapped, dset)
        assert fst[0] == 0 and parts[0] == recs[1]
        assert not (fst[1] == 0 and parts[1] == recs[0])
        xf, xr = T["xml"][2][7], T["xml"][1][7]
        at, size = header_layout(xf)[:2]
        swapped = xf[:at] + zdict.dict_id(T["text"][0]).to_bytes(4, "little") + xf[at + 4:]
        with pytest.raises(RuntimeError):                               # libzstd: "Corrupted block detected"
            zdict.decompress(swapped, T["text"][0], len(xr))
        st, fst, parts, _, _ = decode_device(xf + swapped, dset)
        assert fst[0] == 0 and parts[0] == xr
        assert not (fst[1] == 0 and parts[1] == xr)


# ---------------------------------------------------------------------------
# 5. a plan pays for the dictionaries its frames use, not for the set's
# ---------------------------------------------------------------------------
def test_only_used_dictionaries_cost():
    from zstd_decompressor.batch import Plan
    blobs = [derived(k) for k in range(40)]
    assert len({zdict.dict_id(b) for b in blobs}) == 40
    used = (3, 17, 31)
    frames = [derived_frame(k, 0, j) for j in range(2) for k in used]
    recs = [derived_record(k, j) for j in range(2) for k in used]
    data = b"".join(frames)
    with Dicts(blobs, fallback=-1) as all40, Dicts([blobs[k] for k in used], fallback=-1) as only3:
        a, b = Plan(data, dictionary=all40), Plan(data, dictionary=only3)
        try:
            assert a.info.workspace_bytes == b.info.workspace_bytes
            assert a.info.ncompressed == b.info.ncompressed == 6
        finally:
            a.close()
            b.close()
        both_paths(frames, recs, all40)
        # every dictionary of the set used: one frame each, then six frames each
        both_paths([derived_frame(k) for k in range(40)], [derived_record(k) for k in range(40)], all40)
        info = both_paths([derived_frame(k, 0, j) for j in range(6) for k in range(40)],
                          [derived_record(k, j) for j in range(6) for k in range(40)], all40)
        assert info.ncompressed == 240


# ---------------------------------------------------------------------------
# 6. a plan past the small-plan thresholds (K3Q, several K4 rounds)
# ---------------------------------------------------------------------------
def test_large_plan_with_checksums():
    T = trained()
    blobs = [T["text"][0], T["text112"][0], derived(5)]
    recs = records_of(gen.text(2400 * 2048, seed=0xD610), 2048)
    assert len(recs) == 2400
    frames = [zdict.compress(r, blobs[i % 3], 3, checksum=True) for i, r in enumerate(recs)]
    ids = [zdict.dict_id(b) for b in blobs]
    for i in (0, 1, 2, 2399):
        at, size = header_layout(frames[i])[:2]
        assert int.from_bytes(frames[i][at:at + size], "little") == ids[i % 3]
    assert sum(treeless_repeat(f) for f in frames) >= 1200
    data, want = b"".join(frames), b"".join(recs)
    with Dicts(blobs, fallback=0) as dset:
        st, out, info = decode_host(data, dset)
        assert st == 0 and out == want and info["executors"] == 0 and info["replans"] == 0
        st, fst, parts, ok, _ = decode_device(data, dset, checksums=True)
        assert st == 0 and ok == [1] * 2400
        assert b"".join(parts) == want


# ---------------------------------------------------------------------------
# 7. frames of several blocks; frames without a Frame_Content_Size
# ---------------------------------------------------------------------------
def test_multi_block_and_no_content_size():
    from zstd_decompressor.batch import frames_index
    T = trained()
    blobs = [T["text112"][0], T["xml"][0], T["text"][0]]
    big = [gen.text(300 << 10, seed=0xD620), gen.xml(300 << 10, seed=0xD621), gen.text(300 << 10, seed=0xD622)]
    frames = [zdict.compress(r, b, 3) for r, b in zip(big, blobs)]
    for f in frames:
        fr, _, ist, _ = frames_index(f)
        assert ist == 0 and fr[0]["num_blocks"] == 3
        assert first_block_shape(f)[1] == 2               # the first block brings its own tree
    small, sframes = [], []
    for i in range(24):
        r = big[i % 3][8192 * i:8192 * (i + 1)]
        small.append(r)
        sframes.append(zdict.compress(r, blobs[i % 3], 3, content_size=False))
    assert all(header_layout(f)[3] == 0 for f in sframes)
    with Dicts(blobs, fallback=-1) as dset:
        both_paths(frames, big, dset)
        st, fst, parts, _, info = decode_device(b"".join(sframes), dset)
        assert st == 0 and info.out_exact == 0            # capacities are bounds: the output is compacted
        assert parts == small
        st, out, _ = decode_host(b"".join(sframes + frames[:1]), dset)
        assert st == 0 and out == b"".join(small) + big[0]


# ---------------------------------------------------------------------------
# 8. a frame that overruns its declared size is planned again, with its own dictionary
# ---------------------------------------------------------------------------
def test_capacity_replan_keeps_the_set():
    T = trained()
    dct, recs, frames = T["text"]
    i = next(i for i, r in enumerate(recs) if len(r) == 4096 and treeless_repeat(frames[i]))
    f = bytearray(frames[i])
    _, _, at, size, _ = header_layout(frames[i])
    assert size == 2 and int.from_bytes(f[at:at + 2], "little") + 256 == 4096
    f[at:at + 2] = (2048 - 256).to_bytes(2, "little")
    head = [T["xml"][2][0], T["text112"][2][0], T["xml"][2][1]]
    head_recs = [T["xml"][1][0], T["text112"][1][0], T["xml"][1][1]]
    tail, tail_recs = [T["text112"][2][1]], [T["text112"][1][1]]
    with Dicts([T["xml"][0], T["text112"][0], dct], fallback=-1) as dset:     # the frame's: the set's last
        st, out, info = decode_host(b"".join(head) + bytes(f) + b"".join(tail), dset)
        assert st == 0 and info["replans"] >= 1
        assert out == b"".join(head_recs) + recs[i] + b"".join(tail_recs)


# ---------------------------------------------------------------------------
# 9. zd_decode_async of a dictionary-set plan in a HIP graph
# ---------------------------------------------------------------------------
def test_hip_graph_capture_replay():
    import torch
    from zstd_decompressor.batch import Plan
    T = trained()
    frames, recs = interleaved()
    data, want = b"".join(frames), b"".join(recs)
    with Dicts([T[n][0] for n in NAMES], fallback=-1) as dset:
        plan = Plan(data, dictionary=dset)
        n = plan.info.out_bytes
        dev = torch.device("cuda", 0)
        d_src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
        d_src[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
        d_dst = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
        s = torch.cuda.Stream(dev)
        with torch.cuda.stream(s):          # warm-up outside the capture
            plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, s.cuda_stream)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, s.cuda_stream)
        for _ in range(2):
            d_dst.zero_()
            torch.cuda.synchronize(dev)
            g.replay()
            torch.cuda.synchronize(dev)
            st, total, _, _, _ = plan.results(d_dst.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            assert st == 0 and total == len(want)
            assert bytes(d_dst[:total].cpu().numpy().tobytes()) == want
        plan.close()


# ---------------------------------------------------------------------------
# 10. a batch of scattered chunks over a set
# ---------------------------------------------------------------------------
def test_batch_of_chunks():
    import torch
    from zstd_decompressor import _lib, decode_tensors
    from test_batch_gpu import Layout
    T = trained()
    frames, recs = interleaved()
    plain_recs = [gen.text(700 + 333 * i, seed=0xD630 + i) for i in range(8)]
    chunks = list(frames)
    want = [(0, r) for r in recs]
    for i, r in enumerate(plain_recs):                                  # plain chunks among them
        chunks.insert(31 * i + 5, libzstd.compress(r, 3))
        want.insert(31 * i + 5, (0, r))
    assert len(chunks) == 264
    assert sum(header_layout(c)[1] == 0 for c in chunks) == 8 and sum(header_layout(c)[1] == 4 for c in chunks) == 256
    caps = [len(r) + (i % 3) for i, (_, r) in enumerate(want)]
    with Dicts([T[n][0] for n in NAMES], fallback=-1) as dset:
        L = Layout(chunks, caps, seed=0xD631)
        info = L.run(want, dictionary=dset)
        assert info.executors == 0 and info.nchunks == 264
        # one chunk names an ID the set does not hold, one has a destination too small: each fails alone
        bad, short = 100, 201
        assert header_layout(chunks[bad])[1] == 4 and header_layout(chunks[short])[3] > 0
        chunks2, want2, caps2 = list(chunks), list(want), list(caps)
        chunks2[bad] = derived_frame(3, 9)
        want2[bad] = (_lib.DICT_MISMATCH, b"")
        caps2[bad] = len(derived_record(3))
        caps2[short] = len(want[short][1]) - 1
        want2[short] = (_lib.DST_TOO_SMALL, b"")
        L2 = Layout(chunks2, caps2, seed=0xD632)
        L2.run(want2, dictionary=dset)
        # torch tensors in, torch tensors out
        dev = torch.device("cuda", 0)
        pick = [0, 1, 2, 3, 5, 36]
        srcs = [torch.from_numpy(np.frombuffer(chunks[i], dtype=np.uint8).copy()).to(dev) for i in pick]
        dsts = [torch.zeros(len(want[i][1]), dtype=torch.uint8, device=dev) for i in pick]
        st, ln = decode_tensors(srcs, dsts, dictionary=dset)
        assert st == [0] * len(pick) and ln == [len(want[i][1]) for i in pick]
        for i, t in zip(pick, dsts):
            assert t.cpu().numpy().tobytes() == want[i][1], i


# ---------------------------------------------------------------------------
# 11. a set of one dictionary is the single-dictionary plan
# ---------------------------------------------------------------------------
def test_set_of_one_equals_the_dictionary_plan():
    from zstd_decompressor import Dictionary, DictionarySet, _lib
    dct, recs, frames = trained16()
    bad = bytearray(frames[5])
    at, size = header_layout(frames[5])[:2]
    assert size > 0 and int.from_bytes(bad[at:at + size], "little") == zdict.dict_id(dct)
    bad[at] ^= 1
    assert int.from_bytes(bad[at:at + size], "little") != 0
    mismatch = b"".join(frames[:5]) + bytes(bad) + b"".join(frames[6:8])
    d = Dictionary(dct)
    one = DictionarySet([d], fallback=0)
    try:
        for data in (b"".join(frames), mismatch):
            a = decode_device(data, d)
            b = decode_device(data, one)
            assert a[:3] == b[:3]                                       # status, frame statuses, frame bytes
            assert a[4].ncompressed == b[4].ncompressed and a[4].executors == b[4].executors == 0
            assert a[4].out_bytes == b[4].out_bytes and a[4].nsequences == b[4].nsequences
            assert decode_host(data, d) == decode_host(data, one)
        st, fst, parts, _, _ = decode_device(b"".join(frames), one)
        assert st == 0 and parts == list(recs)
        st, fst, _, _, _ = decode_device(mismatch, one)
        assert fst == [0] * 5 + [_lib.DICT_MISMATCH] + [_lib.NOT_DECODED] * 2
    finally:
        one.close()
        d.close()


# ---------------------------------------------------------------------------
# 12. plans and batches keep the set alive, the set its dictionaries
# ---------------------------------------------------------------------------
def test_lifetimes():
    from zstd_decompressor import Dictionary, DictionarySet, _lib
    from zstd_decompressor.batch import Plan, run_plan
    from test_batch_gpu import Layout
    T = trained()
    frames, recs = interleaved(("text", "xml"), 16)
    data = b"".join(frames)
    ds = [Dictionary(T["text"][0]), Dictionary(T["xml"][0])]
    dset = DictionarySet(ds)
    for d in ds:                                # a dictionary destroyed before the set is used
        d.close()
    plan = Plan(data, dictionary=dset)
    L = Layout(frames, [len(r) for r in recs], seed=0xD640)
    batch = L.batch(dictionary=dset)
    dset.close()                                # and the set before the plan and the batch decode
    with pytest.raises(ValueError):
        Plan(data, dictionary=dset)
    p, n, keep = _lib.buf(data)
    st, out = run_plan(plan, p, n)
    assert st == 0 and out == b"".join(recs)
    plan.close()
    batch.decode_async(L.stream)
    st, ln = batch.results(L.stream)
    L.check(L.host(), st, ln, [(0, r) for r in recs])
    batch.close()


# ---------------------------------------------------------------------------
# 13. argument errors
# ---------------------------------------------------------------------------
def test_argument_errors():
    from zstd_decompressor import Dictionary, DictionarySet, ZdError, _lib
    L = _lib.lib()
    T = trained()
    text, xml, raw = Dictionary(T["text"][0]), Dictionary(T["xml"][0]), Dictionary(raw5000())
    closed = Dictionary(derived(0))
    closed.close()

    def refused(ds, fallback):
        with pytest.raises(ZdError) as e:
            DictionarySet(ds, fallback=fallback)
        assert e.value.code == _lib.INVALID_ARG

    try:
        refused([], 0)                              # no dictionaries
        refused([text, closed], 0)                  # a destroyed entry
        refused([text, xml], 2)                     # fallback outside [-1, ndicts)
        refused([text, xml], -2)
        refused([text, xml, text], 0)               # two entries with one ID
        refused([text, raw], 0)                     # a raw-content dictionary that is not the fallback
        refused([text, raw], -1)
        refused([text] * (_lib.DICT_SET_MAX + 1), 0)
        s = DictionarySet([text, xml, raw], fallback=2)
        n, fb = C.c_size_t(), C.c_int()
        assert L.zd_dict_set_info(s._h, C.byref(n), C.byref(fb)) == 0 and (n.value, fb.value) == (3, 2)
        assert len(s) == 3 and s.dict_ids == (text.dict_id, xml.dict_id, 0)
        h = C.c_void_p()
        x = C.c_char_p(b"x")
        assert L.zd_plan_create_dicts(x, 1, 0, None, C.byref(h)) == _lib.INVALID_ARG and not h.value
        assert L.zd_plan_create_dicts(x, 1, 0, s._h, None) == _lib.INVALID_ARG
        s.close()
        s.close()
        with pytest.raises(ValueError):
            from zstd_decompressor.batch import Batch
            Batch([], [], [], [], dictionary=s)
        s = DictionarySet([raw, text], fallback=0)  # a raw-content dictionary at the fallback is fine
        s.close()
    finally:
        for d in (text, xml, raw):
            d.close()


# ---------------------------------------------------------------------------
# 14. the CLI: -D more than once
# ---------------------------------------------------------------------------
def test_cli_repeated_dictionary_option(tmp_path):
    from zstd_decompressor.__main__ import main
    T = trained()
    frames, recs = interleaved(("text", "xml"), 8)
    D = raw5000()
    tail_rec = D[-16:].hex().encode() * 40
    tail = zdict.compress(tail_rec, D.hex().encode(), 3)               # (the CLI's output is text)
    assert header_layout(tail)[1] == 0
    (tmp_path / "in.zst").write_bytes(b"".join(frames) + tail)
    (tmp_path / "text.dict").write_bytes(T["text"][0])
    (tmp_path / "xml.dict").write_bytes(T["xml"][0])
    (tmp_path / "raw.dict").write_bytes(D.hex().encode())
    out = tmp_path / "out.txt"
    args = [str(tmp_path / "in.zst"), "-D", str(tmp_path / "text.dict"), "-D", str(tmp_path / "raw.dict"),
            "-D", str(tmp_path / "xml.dict"), "-o", str(out)]
    assert main(args) == 0                                              # the raw-content file is the fallback
    assert out.read_bytes() == b"".join(recs) + tail_rec
    assert main(args[:3] + ["-o", str(out)]) == 1                       # one -D: as before, a mismatch
