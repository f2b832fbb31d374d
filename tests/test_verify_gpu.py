"""Content_Checksums verified inside the decode launch (ZD_F_VERIFY_CHECKSUM,
zd_k_verify; include/zd.h).  The yardsticks: the `xxhash` package for what the
digest of given bytes is, libzstd (corpus/libzstd.py, corpus/zdict.py) for
which frames a verifying decoder rejects ("Restored data doesn't match
checksum"), and the library's own statuses without the flag.  Frames come from
libzstd.compress / zdict.compress; a damaged frame is a clean one with one bit
flipped at a place where libzstd decodes it and then rejects its checksum.

A batch's destinations start at offsets 0 to 15 from a 16-byte boundary,
cycling, inside one tensor of 0xA5 with 32 guard bytes either side of each;
after every decode every byte outside the chunks' [dst, dst + cap) is 0xA5.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from corpus import gen, libzstd, zdict

xxhash = pytest.importorskip("xxhash")

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zstd-decompressor_amd")
GOLDEN = os.path.join(ROOT, "tests", "golden", "dict")
FILL, GUARD = 0xA5, 32
LENGTHS = [0, 1, 3, 4, 7, 8, 15, 31, 32, 33, 63, 64, 95, 96, 127, 128, 129, 4095, 4096, 4097, 100_000, 131_072,
           131_073]
EMPTY_XXH64 = 0xEF46DB3751D8E999
# The checksummed frame of no bytes that decodes: one RLE block of size 0.  (libzstd's own, a raw block of size
# 0, is EmptySliceError in this library as in the reference, with and without the flag: test below.)
EMPTY_FRAME = b"\x28\xb5\x2f\xfd\x24\x00\x03\x00\x00\x41" + (EMPTY_XXH64 & 0xFFFFFFFF).to_bytes(4, "little")


def xxh(b: bytes) -> int:
    return xxhash.xxh64(b, seed=0).intdigest()


def to_device(data: bytes):
    import torch
    t = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    if data:
        t[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


class _DeviceArray:
    def __init__(self, ptr, n, typestr):
        self.__cuda_array_interface__ = {"shape": (n,), "typestr": typestr, "data": (ptr, False), "version": 2}


def device_list(ptr: int, n: int, typestr: str):
    """n entries of a device array as Python ints, read with torch (no library call)."""
    import torch
    if not n:
        return []
    return torch.as_tensor(_DeviceArray(ptr, n, typestr), device="cuda:0").cpu().tolist()


def device_u64(ptr: int, n: int):
    return [v & (2 ** 64 - 1) for v in device_list(ptr, n, "<i8")]


def damaged(frame: bytes, size: int, decode=None, start=None):
    """`frame` with bit 0 of one payload byte flipped, at the first place from
    `start` where libzstd still decodes the frame and rejects only its checksum."""
    decode = decode or (lambda f: libzstd.decompress_frame(f, size))
    for p in range(start if start is not None else len(frame) // 2, len(frame) - 4):
        f = bytearray(frame)
        f[p] ^= 1
        try:
            decode(bytes(f))
        except RuntimeError as e:
            if "checksum" in str(e).lower():
                return bytes(f)
    raise AssertionError("no position where libzstd rejects the checksum alone")


class Layout:
    """Sources packed into one tensor 3 bytes apart; destination i at offset i % 16
    from a 16-byte boundary inside one tensor of 0xA5, GUARD bytes around each."""

    def __init__(self, chunks, caps):
        import torch
        self.torch = torch
        self.chunks, self.caps, self.n = list(chunks), list(caps), len(chunks)
        offs, at = [], 0
        for c in chunks:
            offs.append(at)
            at += len(c) + 3
        self.src = to_device(b"".join(c + b"\x5c\x5c\x5c" for c in chunks))
        self.src_ptrs = [self.src.data_ptr() + o for o in offs]
        self.sizes = [len(c) for c in chunks]
        self.dst_offs, at = [], GUARD
        for i, c in enumerate(self.caps):
            at = (at + 15) // 16 * 16 + i % 16
            self.dst_offs.append(at)
            at += c + GUARD
        self.dst = torch.full((at + GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
        assert self.dst.data_ptr() % 16 == 0
        self.dst_ptrs = [self.dst.data_ptr() + o for o in self.dst_offs]
        self.stream = torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream

    def host(self):
        return self.dst.cpu().numpy()

    def guards_untouched(self, host=None):
        host = self.host() if host is None else host
        mask = np.ones(host.shape, dtype=bool)
        for o, c in zip(self.dst_offs, self.caps):
            mask[o:o + c] = False
        return bool((host[mask] == FILL).all())

    def out(self, host, i, n):
        return host[self.dst_offs[i]: self.dst_offs[i] + n].tobytes()

    def batch(self, flags, dictionary=None, device=False):
        from zstd_decompressor.batch import Batch
        t = self.torch
        if device:
            arrs = [t.tensor(v, dtype=t.int64, device="cuda:0")
                    for v in (self.src_ptrs, self.sizes, self.dst_ptrs, self.caps)]
            b = Batch.from_device(*arrs, flags=flags, dictionary=dictionary, stream=self.stream)
            assert b.info.device_built == 1
            return b
        return Batch(self.src_ptrs, self.sizes, self.dst_ptrs, self.caps, flags=flags, dictionary=dictionary,
                     stream=self.stream)

    def run(self, flags, dictionary=None, device=False):
        """One decode: (statuses, lengths, digests, oks, host copy of the
        destinations); the device arrays are read before results() and agree with it."""
        from zstd_decompressor import _lib
        b = self.batch(flags, dictionary, device)
        try:
            self.dst.fill_(FILL)
            b.decode_async(self.stream)
            self.torch.cuda.synchronize()
            d_st, d_ln = b.device_results()
            st, ln = device_list(d_st, self.n, "<i4"), device_u64(d_ln, self.n)
            h = ok = None
            if flags & _lib.F_VERIFY_CHECKSUM:
                d_h, d_ok = b.device_checksums()
                h, ok = device_u64(d_h, self.n), device_list(d_ok, self.n, "|i1")
            assert (st, ln) == tuple(b.results(self.stream))
            host = self.host()
            assert self.guards_untouched(host)
            return st, ln, h, ok, host
        finally:
            b.close()


def run_plan(data: bytes, flags=0, dictionary=None, from_device=False):
    """(status, total, statuses, lengths, first error frame, output, info fields) of one plan."""
    import torch
    from zstd_decompressor.batch import Plan
    d_src = to_device(data)
    s = torch.cuda.current_stream(torch.device("cuda", 0)).cuda_stream
    plan = (Plan.from_device(d_src.data_ptr(), len(data), False, flags, s) if from_device
            else Plan(data, False, flags, dictionary=dictionary))
    try:
        n = plan.info.out_bytes
        d_dst = torch.zeros(n + 64, dtype=torch.uint8, device="cuda:0")
        plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, s)
        st, total, sts, lens, first = plan.results(d_dst.data_ptr(), s)
        info = {k: getattr(plan.info, k) for k in ("executors", "out_exact", "device_descriptors", "nframes",
                                                   "ncompressed", "nblocks")}
        return st, total, sts, lens, first, d_dst[:total].cpu().numpy().tobytes(), info
    finally:
        plan.close()


def check_plan_stops_at(data, sources, bad, flags=0, dictionary=None, from_device=False):
    """The verified plan fails at frame `bad` alone; the unverified one decodes everything."""
    from zstd_decompressor import _lib
    st, total, sts, lens, first, out, info = run_plan(data, flags | _lib.F_VERIFY_CHECKSUM, dictionary, from_device)
    n = len(sources)
    assert st == _lib.CHECKSUM_WRONG and first == bad
    assert sts == [0] * bad + [_lib.CHECKSUM_WRONG] + [_lib.NOT_DECODED] * (n - bad - 1)
    assert lens == [len(s) for s in sources[:bad]] + [0] * (n - bad)
    assert total == sum(len(s) for s in sources[:bad]) and out == b"".join(sources[:bad])
    st0, total0, sts0, _, first0, _, _ = run_plan(data, flags, dictionary, from_device)
    assert st0 == 0 and sts0 == [0] * n and first0 == -1 and total0 == sum(len(s) for s in sources)
    return info


def check_batch_fails_alone(chunks, sources, bad, flags=0, dictionary=None, device=False, caps=None):
    """Only chunk `bad` of the verified batch fails, with length 0; clean chunks are exact."""
    from zstd_decompressor import _lib
    L = Layout(chunks, caps or [len(s) for s in sources])
    st, ln, h, ok, host = L.run(flags | _lib.F_VERIFY_CHECKSUM, dictionary, device)
    for i, s in enumerate(sources):
        if i == bad:
            assert (st[i], ln[i], ok[i]) == (_lib.CHECKSUM_WRONG, 0, 0), i
        else:
            assert (st[i], ln[i], ok[i], h[i]) == (0, len(s), 1, xxh(s)), i
            assert L.out(host, i, len(s)) == s, i
    st0, ln0, _, _, _ = L.run(flags, dictionary, device)
    assert st0 == [0] * L.n and ln0[bad] == len(sources[bad])
    return L


# ---------------------------------------------------------------------------
# 1. lengths and grouping
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sized():
    """(frames, sources): for every length a checksummed frame of text and one of random bytes (raw blocks)."""
    rng = np.random.default_rng(0x5EED)
    sources = []
    for k, n in enumerate(LENGTHS):
        sources.append(gen.text(max(n, 1), seed=400 + k)[:n])
        sources.append(rng.bytes(n))
    frames = [libzstd.compress(s, 3, checksum=True) if s else EMPTY_FRAME for s in sources]
    for f, s in zip(frames, sources):
        assert libzstd.decompress_frame(f, len(s)) == s
    return frames, sources


def test_libzstd_empty_frame_keeps_its_own_status():
    """libzstd writes no bytes as a raw block of size 0, EmptySliceError here as in
    the reference: the same with the flag, and its bytes are never hashed."""
    from zstd_decompressor import _lib
    f = libzstd.compress(b"", 3, checksum=True)
    assert int.from_bytes(f[-4:], "little") == EMPTY_XXH64 & 0xFFFFFFFF
    L = Layout([EMPTY_FRAME, f], [0, 0])
    assert L.run(0)[0] == [0, _lib.EMPTY_SLICE]
    st, ln, h, ok, _ = L.run(_lib.F_VERIFY_CHECKSUM)
    assert st == [0, _lib.EMPTY_SLICE] and ln == [0, 0] and ok == [1, -1] and h == [EMPTY_XXH64, 0]


def test_lengths_as_one_plan(sized):
    from zstd_decompressor import _lib
    frames, sources = sized
    st, total, sts, lens, first, out, _ = run_plan(b"".join(frames), _lib.F_VERIFY_CHECKSUM)
    assert st == 0 and first == -1 and sts == [0] * len(frames)
    assert lens == [len(s) for s in sources] and out == b"".join(sources)


@pytest.mark.parametrize("nchunks", [1, 15, 16, 17, 33, len(LENGTHS) * 2])
def test_lengths_as_a_batch(sized, nchunks):
    from zstd_decompressor import _lib
    frames, sources = sized
    # (from the long end for the small counts, so that 1 chunk is not the empty frame)
    frames, sources = frames[::-1][:nchunks], sources[::-1][:nchunks]
    L = Layout(frames, [len(s) for s in sources])
    st, ln, h, ok, host = L.run(_lib.F_VERIFY_CHECKSUM)
    assert st == [0] * nchunks and ln == [len(s) for s in sources]
    assert h == [xxh(s) for s in sources] and ok == [1] * nchunks
    for i, s in enumerate(sources):
        assert L.out(host, i, len(s)) == s, i
    if nchunks == len(LENGTHS) * 2:
        assert xxh(b"") == EMPTY_XXH64 and EMPTY_XXH64 in h


# ---------------------------------------------------------------------------
# 2. a stored checksum flipped
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def six():
    """Six frames, 1 to 4 checksummed, the last byte of frame 2 xored with 0x5A."""
    src = bytes(b if b < 128 else 0x3F for b in gen.text(60_000, seed=21))      # (ASCII: the CLI prints it)
    sources = [src[i * 10_000:(i + 1) * 10_000] for i in range(6)]
    frames = [libzstd.compress(s, 3, checksum=1 <= i <= 4) for i, s in enumerate(sources)]
    f2 = bytearray(frames[2])
    f2[-1] ^= 0x5A
    frames[2] = bytes(f2)
    return frames, sources


def test_stored_checksum_flipped_plan(six):
    frames, sources = six
    check_plan_stops_at(b"".join(frames), sources, 2)


def test_stored_checksum_flipped_batch(six):
    from zstd_decompressor import _lib
    frames, sources = six
    L = Layout(frames, [len(s) for s in sources])
    st, ln, h, ok, host = L.run(_lib.F_VERIFY_CHECKSUM)
    assert st == [0, 0, _lib.CHECKSUM_WRONG, 0, 0, 0]
    assert ln == [len(s) if i != 2 else 0 for i, s in enumerate(sources)]
    assert ok == [-1, 1, 0, 1, 1, -1]
    assert [h[i] for i in (1, 3, 4)] == [xxh(sources[i]) for i in (1, 3, 4)]
    for i in (0, 1, 3, 4, 5):
        assert L.out(host, i, len(sources[i])) == sources[i]
    assert L.run(0)[0] == [0] * 6


def test_profiling_mode_1_times_the_pass(six):
    import torch
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Plan
    frames, _ = six
    data = b"".join(frames)
    d_src = to_device(data)
    for flags, modes in ((_lib.F_VERIFY_CHECKSUM, {1: True, 2: False}), (0, {1: False, 2: False})):
        plan = Plan(data, False, flags)
        try:
            n = plan.info.out_bytes
            d_dst = torch.zeros(n + 64, dtype=torch.uint8, device="cuda:0")
            for mode, want in modes.items():
                plan.set_profiling(mode)
                plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, 0)
                plan.results(d_dst.data_ptr(), 0)
                times = plan.kernel_times()
                assert ("zd_k_verify" in times) == want, (flags, mode, times)
                if want:
                    assert list(times)[-1] == "zd_k_verify" and times["zd_k_verify"] > 0
        finally:
            plan.close()


# ---------------------------------------------------------------------------
# 3. the payload sweep: the exact rule
# ---------------------------------------------------------------------------
def test_payload_sweep():
    from zstd_decompressor import _lib
    src = gen.text(20000, seed=3)
    f = libzstd.compress(src, 3, checksum=True)
    stored = int.from_bytes(f[-4:], "little")
    chunks = []
    for p in range(12, len(f) - 4, 5):
        c = bytearray(f)
        c[p] ^= 1
        chunks.append(bytes(c))
    n = len(chunks)
    lz_checksum = []
    for c in chunks:
        try:
            libzstd.decompress_frame(c, len(src))
            lz_checksum.append(False)
        except RuntimeError as e:
            lz_checksum.append("checksum" in str(e).lower())
    if 2 * sum(lz_checksum) < n:
        pytest.skip(f"this libzstd rejects only {sum(lz_checksum)} of {n} flips for the checksum alone")
    L = Layout(chunks, [len(src)] * n)
    s0, l0, _, _, host0 = L.run(0)
    s1, l1, h1, ok1, host1 = L.run(_lib.F_VERIFY_CHECKSUM)
    wrong = 0
    for i in range(n):
        if s0[i] != 0:
            assert s1[i] == s0[i] and l1[i] == 0 and ok1[i] == -1, i
            continue
        data = L.out(host0, i, l0[i])
        differs = (xxh(data) & 0xFFFFFFFF) != stored
        wrong += differs
        if differs:
            assert (s1[i], l1[i], ok1[i]) == (_lib.CHECKSUM_WRONG, 0, 0), i
        else:
            assert (s1[i], l1[i], ok1[i]) == (0, l0[i], 1) and L.out(host1, i, l1[i]) == data, i
        assert h1[i] == xxh(data), i
        if lz_checksum[i]:
            assert s1[i] == _lib.CHECKSUM_WRONG, i
    assert 2 * wrong >= n, (wrong, n)


# ---------------------------------------------------------------------------
# 4. every route
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small300():
    """300 single-block checksummed frames of 1-4 KiB of text; frame 137 damaged."""
    text = gen.text(300 * 4096, seed=97)
    sources, at = [], 0
    for i in range(300):
        n = 1024 + (i * 977) % 3073
        sources.append(text[at:at + n])
        at += n
    frames = [libzstd.compress(s, 3, checksum=True) for s in sources]
    frames[137] = damaged(frames[137], len(sources[137]))
    return frames, sources


@pytest.fixture(scope="module")
def big():
    """A 16-block 2 MiB checksummed frame: (clean, damaged, source)."""
    src = gen.text(2 << 20, seed=98)
    f = libzstd.compress(src, 3, checksum=True)
    return f, damaged(f, len(src)), src


@pytest.mark.parametrize("flag, executor", [(0, "EXEC_FUSED"), ("F_NO_FUSE", "EXEC_K4F")])
def test_route_small_frames(small300, flag, executor):
    from zstd_decompressor import _lib
    frames, sources = small300
    flags = getattr(_lib, flag) if flag else 0
    info = check_plan_stops_at(b"".join(frames), sources, 137, flags)
    assert info["executors"] & getattr(_lib, executor), info
    check_batch_fails_alone(frames, sources, 137, flags)


@pytest.mark.parametrize("side", ["below", "at"])
def test_many_frames_both_load_patterns(side):
    """zd_k_verify fetches whole lines in plans below 16 waves a CU and single words from there on
    (16 frames a wave): one wave below the threshold and exactly at it, a damaged frame in the middle."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 16 * (16 * cus - (1 if side == "below" else 0))
    rng = np.random.default_rng(0xC0DE)
    text = gen.text(1 << 16, seed=95)
    lengths = [33, 64, 96, 127, 128, 129, 200, 255, 256, 300, 511, 777, 1000, 31, 1, 160]
    uniq = [text[37 * k: 37 * k + m] if k % 2 else rng.bytes(m) for k, m in enumerate(lengths * 4)]
    frames = [libzstd.compress(s, 3, checksum=True) for s in uniq]
    bad = n // 2 // 64 * 64 + 6                          # (a 200-byte raw block)
    seq =[frames[i % 64] for i in range(n)]
    sources = [uniq[i % 64] for i in range(n)]
    seq[bad] = damaged(seq[bad], len(sources[bad]), start=12)
    info = check_plan_stops_at(b"".join(seq), sources, bad)
    assert info["nframes"] == n


def test_route_block_parallel(big):
    from zstd_decompressor import _lib
    clean, bad, src = big
    small = gen.text(5000, seed=99)
    frames = [clean, bad, libzstd.compress(small, 3, checksum=True)]
    info = check_plan_stops_at(b"".join(frames), [src, src, small], 1, _lib.F_BLOCK_PARALLEL)
    assert info["executors"] & _lib.EXEC_K4J and info["nblocks"] >= 33


def test_route_one_round_is_decoded_again(big):
    """K4J cut to one round: the streaming re-decode inside results() keeps the flag."""
    import torch
    from zstd_decompressor import _lib
    clean, bad, src = big
    L = Layout([bad, clean], [len(src)] * 2)
    b = L.batch(_lib.F_VERIFY_CHECKSUM | _lib.F_BLOCK_PARALLEL | _lib.F_J_ONE_ROUND)
    try:
        assert b.info.executors & _lib.EXEC_K4J
        b.decode_async(L.stream)
        torch.cuda.synchronize()
        d_st, _ = b.device_results()
        assert _lib.OUT_OF_DOMAIN in device_list(d_st, 2, "<i4"), "one round converged: not about the re-decode"
        st, ln = b.results(L.stream)
        assert st == [_lib.CHECKSUM_WRONG, 0] and ln == [0, len(src)]
        assert device_list(d_st, 2, "<i4") == st
        d_h, d_ok = b.device_checksums()
        assert device_list(d_ok, 2, "|i1") == [0, 1] and device_u64(d_h, 2)[1] == xxh(src)
        host = L.host()
        assert L.out(host, 1, len(src)) == src and L.guards_untouched(host)
    finally:
        b.close()


def raw_rle_frame(parts):
    """A checksummed frame of raw (bytes) and RLE ((byte, count)) blocks, single segment, 2-byte content size."""
    content = b"".join(p if isinstance(p, bytes) else bytes([p[0]]) * p[1] for p in parts)
    assert 256 <= len(content) < 65536 + 256
    out = bytearray(b"\x28\xb5\x2f\xfd" + bytes([0x64]) + (len(content) - 256).to_bytes(2, "little"))
    for k, p in enumerate(parts):
        last = int(k == len(parts) - 1)
        if isinstance(p, bytes):
            out += (last | (0 << 1) | (len(p) << 3)).to_bytes(3, "little") + p
        else:
            out += (last | (1 << 1) | (p[1] << 3)).to_bytes(3, "little") + bytes([p[0]])
    out += (xxh(content) & 0xFFFFFFFF).to_bytes(4, "little")
    return bytes(out), content


def test_route_raw_and_rle_blocks_only():
    rng = np.random.default_rng(7)
    parts = [rng.bytes(1000), (0x41, 500), rng.bytes(700)]
    f, content = raw_rle_frame(parts)
    assert libzstd.decompress_frame(f, len(content)) == content
    bad = damaged(f, len(content), start=20)            # inside the first raw block
    other, other_content = raw_rle_frame([(0x42, 300), rng.bytes(333)])
    frames, sources = [other, bad, f], [other_content, content, content]
    info = check_plan_stops_at(b"".join(frames), sources, 1)
    assert info["executors"] == 0 and info["ncompressed"] == 0
    check_batch_fails_alone(frames, sources, 1)


def test_route_streaming_with_fork(small300):
    """F_FRAME_SERIAL | F_NO_FUSE: two-block frames of 160 KiB run on the streaming
    executor beside the small frames, K2 forked beside K3."""
    import torch
    from zstd_decompressor import _lib
    frames, sources = small300
    text = gen.text(3 * (160 << 10), seed=96)
    two = [text[k * (160 << 10):(k + 1) * (160 << 10)] for k in range(3)]
    two_f = [libzstd.compress(s, 3, checksum=True) for s in two]
    two_f[1] = damaged(two_f[1], len(two[1]))
    clean = list(frames)
    clean[137] = libzstd.compress(sources[137], 3, checksum=True)
    fr, so = clean[:150] + two_f + clean[150:], sources[:150] + two + sources[150:]
    flags = _lib.F_FRAME_SERIAL | _lib.F_NO_FUSE
    info = check_plan_stops_at(b"".join(fr), so, 151, flags)
    assert not info["executors"] & (_lib.EXEC_FUSED | _lib.EXEC_K4J)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    r = C.c_uint32()
    nc = info["ncompressed"]
    assert _lib.lib().zd_route(cus, info["nframes"], nc, nc, nc, 0, flags, C.byref(r)) == 0
    if cus == 256:
        assert r.value & 8, "the plan was sized for the K2 | K3 fork on 256 CUs"
    check_batch_fails_alone(fr, so, 151, flags)


def test_route_no_content_size():
    """Frames without Frame_Content_Size: a plan (staging and compaction) and a packed batch (in place)."""
    import torch
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Batch
    srcs = [gen.text(n, seed=0xE500 + k) for k, n in enumerate((20 << 10, 3000, 50 << 10, 7000))]
    frames = [libzstd.compress(s, 3, checksum=True, content_size=(k == 1)) for k, s in enumerate(srcs)]
    frames[2] = damaged(frames[2], len(srcs[2]))
    info = check_plan_stops_at(b"".join(frames), srcs, 2)
    assert info["out_exact"] == 0
    L = Layout(frames, [0] * 4)                          # (the sources only: a packed batch places its outputs)
    t = lambda v: torch.tensor(v, dtype=torch.int64, device="cuda:0")
    for flags in (_lib.F_VERIFY_CHECKSUM, 0):
        b = Batch.packed(t(L.src_ptrs), t(L.sizes), align=16, flags=flags, stream=L.stream)
        try:
            d_off, _ = b.output_layout()
            offs = device_u64(d_off, 4)
            buf = torch.full((b.out_bytes + 2 * GUARD + 1,), FILL, dtype=torch.uint8, device="cuda:0")
            b.bind_output(buf.data_ptr() + GUARD + 1, b.out_bytes)
            b.decode_async(L.stream)
            st, ln = b.results(L.stream)
            host = buf.cpu().numpy()
            if flags:
                assert st == [0, 0, _lib.CHECKSUM_WRONG, 0] and ln == [len(srcs[0]), len(srcs[1]), 0, len(srcs[3])]
                d_h, d_ok = b.device_checksums()
                assert device_list(d_ok, 4, "|i1") == [1, 1, 0, 1]
                assert [device_u64(d_h, 4)[i] for i in (0, 1, 3)] == [xxh(srcs[i]) for i in (0, 1, 3)]
            else:
                assert st == [0] * 4 and ln == [len(s) for s in srcs]
            for i in (0, 1, 3):
                at = GUARD + 1 + offs[i]
                assert host[at:at + len(srcs[i])].tobytes() == srcs[i]
            assert (host[:GUARD + 1] == FILL).all() and (host[GUARD + 1 + b.out_bytes:] == FILL).all()
        finally:
            b.close()


def test_route_dictionaries():
    """A dictionary plan and a dictionary-set batch: 64 records of 4 KiB, record 40 damaged."""
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Dictionary, DictionarySet
    dct = open(os.path.join(GOLDEN, "dict.bin"), "rb").read()
    text = gen.text(64 * 4096, seed=0xD1C7)
    recs = [text[i * 4096:(i + 1) * 4096] for i in range(64)]
    frames = [zdict.compress(r, dct, 3, checksum=True) for r in recs]
    assert all(zdict.decompress(f, dct, 4096) == r for f, r in zip(frames, recs))
    frames[40] = damaged(frames[40], 4096, decode=lambda f: zdict.decompress(f, dct, 4096))
    d = Dictionary(dct)
    dset = DictionarySet([d], fallback=0)
    try:
        check_plan_stops_at(b"".join(frames), recs, 40, dictionary=d)
        check_batch_fails_alone(frames, recs, 40, dictionary=dset)
    finally:
        dset.close()
        d.close()


def test_route_built_on_the_device(small300):
    from zstd_decompressor import _lib
    frames, sources = small300
    info = check_plan_stops_at(b"".join(frames), sources, 137, from_device=True)
    assert info["device_descriptors"] == 1
    check_batch_fails_alone(frames[100:170], sources[100:170], 37, device=True)      # (Layout.batch: device_built)


# ---------------------------------------------------------------------------
# 5. a frame that fails for its own reason keeps its status
# ---------------------------------------------------------------------------
def test_own_failure_keeps_its_status():
    from oracle import oracle
    from zstd_decompressor import _lib
    srcs = [gen.text(9000, seed=0xF00 + k) for k in range(3)]
    frames = [libzstd.compress(s, 3, checksum=True) for s in srcs]
    trunc = frames[1][:-9]                               # the last block cut short (and no checksum left)
    # a corrupt literals section / tree description: the first byte of the block whose damage the CPU oracle refuses
    table = None
    for p in range(10, 60):
        c = bytearray(frames[1])
        c[p] ^= 0xFF
        if oracle.decompress_status(bytes(c))[0] != 0:
            table = bytes(c)
            break
    assert table is not None and oracle.decompress_status(trunc)[0] != 0
    for bad in (trunc, table):
        chunks = [frames[0], bad, frames[2]]
        L = Layout(chunks, [9000] * 3)
        s0 = L.run(0)[0]
        s1, l1, _, ok1, host = L.run(_lib.F_VERIFY_CHECKSUM)
        assert s0[1] != 0 and s1 == s0 and s1[1] != _lib.CHECKSUM_WRONG and (l1[1], ok1[1]) == (0, -1)
        assert ok1[0] == ok1[2] == 1 and L.out(host, 2, 9000) == srcs[2]
        p0, p1 = run_plan(b"".join(chunks), 0), run_plan(b"".join(chunks), _lib.F_VERIFY_CHECKSUM)
        # (in a plan the frame is followed by more input, so its own status may differ from the chunk's)
        assert p0[:6] == p1[:6] and p1[0] not in (0, _lib.CHECKSUM_WRONG) and p1[4] == 1


# ---------------------------------------------------------------------------
# 6. zd_plan_decompress: the re-plans keep the flag
# ---------------------------------------------------------------------------
def test_plan_decompress_replans_keep_the_flag():
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Plan, run_plan as host_run
    tile = gen.text(4096, seed=15)
    deep = b"".join(bytes([i & 255]) + tile for i in range(80))       # every tile copies the one before
    mid, tail = gen.text(7000, seed=17), gen.text(6000, seed=18)
    frames = [libzstd.compress(deep, 3, checksum=True, content_size=False), libzstd.compress(mid, 3, checksum=True),
              damaged(libzstd.compress(tail, 3, checksum=True), len(tail)), libzstd.compress(mid, 3)]
    data = b"".join(frames)
    for verify in (True, False):
        plan = Plan(data, False, _lib.F_BLOCK_PARALLEL | _lib.F_J_ONE_ROUND | (_lib.F_VERIFY_CHECKSUM if verify else 0))
        try:
            p, n, keep = _lib.buf(data)
            st, out = host_run(plan, p, n)
            assert plan.refresh_info().replans >= 1
            if verify:
                assert st == _lib.CHECKSUM_WRONG and out == deep + mid
                sts = (C.c_int32 * 4)()
                nf = C.c_size_t()
                _lib.check(_lib.lib().zd_plan_frame_outputs(plan._h, sts, None, None, 4, C.byref(nf)))
                assert nf.value == 4 and list(sts) == [0, 0, _lib.CHECKSUM_WRONG, _lib.NOT_DECODED]
            else:
                # (the damaged frame decodes, to other bytes than its source)
                assert st == 0 and len(out) == len(deep + mid + tail + mid)
                assert out[:len(deep + mid)] == deep + mid and out[-len(mid):] == mid
                assert out != deep + mid + tail + mid
        finally:
            plan.close()


# ---------------------------------------------------------------------------
# 7. a verified batch in a HIP graph
# ---------------------------------------------------------------------------
def test_capture_and_replay(six):
    import torch
    from zstd_decompressor import _lib
    frames, sources = six
    L = Layout(frames, [len(s) for s in sources])
    b = L.batch(_lib.F_VERIFY_CHECKSUM)
    try:
        s = torch.cuda.Stream(torch.device("cuda", 0))
        torch.cuda.synchronize()
        with torch.cuda.stream(s):                      # warm-up outside the capture
            b.decode_async(s.cuda_stream)
        s.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            b.decode_async(s.cuda_stream)
        d_st, d_ln = b.device_results()
        d_h, d_ok = b.device_checksums()
        for k in range(2):
            # garbage over one chunk's destination between the replays
            L.dst[L.dst_offs[3]: L.dst_offs[3] + L.caps[3]] = 0x3C + k
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert device_list(d_st, 6, "<i4") == [0, 0, _lib.CHECKSUM_WRONG, 0, 0, 0], k
            assert device_u64(d_ln, 6) == [len(x) if i != 2 else 0 for i, x in enumerate(sources)]
            assert device_list(d_ok, 6, "|i1") == [-1, 1, 0, 1, 1, -1]
            assert device_u64(d_h, 6)[3] == xxh(sources[3])
            host = L.host()
            assert L.out(host, 3, len(sources[3])) == sources[3] and L.guards_untouched(host)
    finally:
        b.close()


# ---------------------------------------------------------------------------
# 8. the command line
# ---------------------------------------------------------------------------
def test_cli_verify(six, tmp_path):
    frames, sources = six
    path = tmp_path / "six.zst"
    path.write_bytes(b"".join(frames))
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)

    def cli(*args):
        return subprocess.run([sys.executable, "-m", "zstd_decompressor", str(path), *args], cwd=ROOT, env=env,
                              capture_output=True, timeout=120)
    r = cli("--verify")
    assert r.returncode == 1 and r.stdout == b"" and b"Error: frame 2: ChecksumWrong" in r.stderr
    r = cli()
    assert r.returncode == 0 and r.stdout == b"".join(sources)


def test_python_decompress_verify(six):
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import decompress, decompress_status
    frames, sources = six
    data = b"".join(frames)
    assert decompress(data) == b"".join(sources)
    with pytest.raises(_lib.ZdError) as e:
        decompress(data, verify=True)
    assert e.value.code == _lib.CHECKSUM_WRONG and e.value.name == "ChecksumWrong"
    assert decompress_status(data, flags=_lib.F_VERIFY_CHECKSUM) == (_lib.CHECKSUM_WRONG, b"".join(sources[:2]))
