"""ZD_F_LONG_WINDOW: frames whose Window_Size is past the reference's 8 MiB
limit (frame.rs:44) and at most 2 GiB index and decode with the flag, and are
ZD_E_WINDOW_SIZE_TOO_BIG without it, as before.

The fixture is a libzstd frame written without a Frame_Content_Size (so that
it carries a Window_Descriptor, byte 5) whose descriptor is overwritten with
0x70: exponent 14, mantissa 0, 16 MiB.  libzstd still returns the record for
such a frame (checked here), since the descriptor only bounds how far back a
match may reach.  0xB0 is 4 GiB: refused with the flag too.

CPU: the walk without the flag through zd_frames_index (the host walk, as
tests/test_host_walk.py reaches it; that call takes no flags), with the flag
through tests/native/long_window.cpp, which calls the walk's per-frame
function (zd_walk.h index_frame, index_chunk, chunk_size_query) with the option
the flag sets.  GPU: plans, batches from host and device arrays and prefix
batches, in the arena layout of tests/test_batch_prefix_gpu.py."""
import os
import subprocess

import numpy as np
import pytest

from corpus import gen, libzstd, zdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WINDOW_SIZE_TOO_BIG = -66
WALK_LONG_WINDOW = 2
MIB16, GIB4 = 0x70, 0xB0


def patch_window(frame: bytes, descriptor: int) -> bytes:
    fhd = frame[4]
    # no Frame_Content_Size field, not Single_Segment, no Dictionary_ID: byte 5 is the Window_Descriptor
    assert frame[:4] == bytes.fromhex("28b52ffd") and fhd >> 6 == 0 and not fhd & 0x20 and not fhd & 3
    f = bytearray(frame)
    f[5] = descriptor
    return bytes(f)


def long_frame(record: bytes, prefix: bytes = None, descriptor: int = MIB16, level: int = 3) -> bytes:
    if prefix is None:
        frame = libzstd.compress(record, level, content_size=False)
    else:
        frame = zdict.prefix_compress(record, prefix, level, content_size=False)
    f = patch_window(frame, descriptor)
    if descriptor == MIB16:
        assert zdict.prefix_decompress(f, prefix or b"", len(record)) == record
    return f


RECORD = gen.text(5000, seed=0x10A6)


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_libzstd_still_decodes_the_patched_frame():
    f = long_frame(RECORD)
    assert f[5] == MIB16 and zdict.prefix_decompress(f, b"", len(RECORD)) == RECORD
    assert libzstd.decompress_frame(f, len(RECORD)) == RECORD


def test_without_the_flag_the_host_walk_refuses_the_window():
    from zstd_decompressor.batch import frames_index
    frames, blocks, st, consumed = frames_index(long_frame(RECORD))
    assert st == WINDOW_SIZE_TOO_BIG and frames == [] and consumed == 0
    # (and the unpatched frame indexes)
    assert frames_index(libzstd.compress(RECORD, 3, content_size=False))[2] == 0


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    d = tmp_path_factory.mktemp("long_window")
    exe = d / "long_window"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "long_window.cpp")])

    def run(frame, wopt):
        p = d / "frame.zst"
        p.write_bytes(frame)
        out = subprocess.run([str(exe), str(p), str(wopt)], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        return [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
    return run


def test_walk_with_and_without_the_option(walk):
    f = long_frame(RECORD)
    frame, chunk, query = walk(f, 0)
    assert frame[0] == chunk[0] == query[0] == WINDOW_SIZE_TOO_BIG and frame[1] == 0 and query[1] == 0
    frame, chunk, query = walk(f, WALK_LONG_WINDOW)
    assert frame == (0, 1, 16 << 20, 0) and chunk == frame                 # one block, 16 MiB, every byte consumed
    assert query == (0, 128 << 10, 0, 0)                                    # no Frame_Content_Size: 128 KiB a block
    # a window of exactly 2 GiB (exponent 21) is the last one accepted
    assert walk(patch_window(f, 21 << 3), WALK_LONG_WINDOW)[0][:3] == (0, 1, 1 << 31)
    assert walk(patch_window(f, (21 << 3) | 1), WALK_LONG_WINDOW)[0][0] == WINDOW_SIZE_TOO_BIG


def test_four_gib_is_refused_with_the_option_too(walk):
    f = long_frame(RECORD, descriptor=GIB4)
    for wopt in (0, WALK_LONG_WINDOW):
        frame, chunk, query = walk(f, wopt)
        assert frame[0] == chunk[0] == query[0] == WINDOW_SIZE_TOO_BIG, wopt


# ---------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------
def records():
    return [gen.text(700 + 977 * i, seed=0x10A7 + i) for i in range(7)] + [gen.text(300 << 10, seed=0x10AF)]


@pytest.mark.gpu
def test_plan_host_walk_and_device_walk():
    import torch
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Plan, decompress_status
    recs = records()
    data = b"".join(long_frame(r) for r in recs)
    assert decompress_status(data) == (WINDOW_SIZE_TOO_BIG, b"")
    st, out = decompress_status(data, flags=_lib.F_LONG_WINDOW)
    assert st == 0 and out == b"".join(recs)
    st, out = decompress_status(long_frame(RECORD, descriptor=GIB4), flags=_lib.F_LONG_WINDOW)
    assert st == WINDOW_SIZE_TOO_BIG and out == b""
    # zd_plan_create_device: the device walk (zd_k_walk)
    dev = torch.device("cuda", 0)
    d_src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    d_src[:len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    s = torch.cuda.current_stream(dev).cuda_stream
    for flags, want in ((0, WINDOW_SIZE_TOO_BIG), (_lib.F_LONG_WINDOW, 0)):
        plan = Plan.from_device(d_src.data_ptr(), len(data), flags=flags, stream=s)
        try:
            cap = max(int(plan.info.out_bytes), 1)
            d_dst = torch.empty(cap + 64, dtype=torch.uint8, device=dev)
            plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), cap, s)
            res = plan.results(d_dst.data_ptr(), s)
            assert res[0] == want, (flags, res)
            if want == 0:
                assert bytes(d_dst[:res[1]].cpu().numpy().tobytes()) == b"".join(recs)
        finally:
            plan.close()


@pytest.mark.gpu
def test_batches_from_host_and_device_arrays():
    from test_batch_prefix_gpu import Chunk, Run
    from zstd_decompressor import _lib
    recs = records()
    chunks = [Chunk(long_frame(r), None, record=r, dalign=(5 * i) % 16) for i, r in enumerate(recs)]
    plain = Chunk(libzstd.compress(RECORD, 3), None, record=RECORD)        # an ordinary window between them
    chunks.insert(3, plain)
    for device in (False, True):
        r = Run(chunks, device, flags=_lib.F_LONG_WINDOW, with_prefixes=False)
        try:
            st, ln = r.decode()
            assert st == [0] * len(chunks)
            assert all(o == c.record for o, c in zip(r.out, chunks))
        finally:
            r.close()
        r = Run(chunks, device, with_prefixes=False)
        try:
            st, ln = r.decode()
            assert st == [0 if c is plain else WINDOW_SIZE_TOO_BIG for c in chunks]
            assert ln == [len(RECORD) if c is plain else 0 for c in chunks] and r.out[3] == RECORD
        finally:
            r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("block_parallel", [False, True])
def test_prefix_batch(block_parallel):
    from test_batch_prefix_gpu import Chunk, Run, rnd
    from zstd_decompressor import _lib
    chunks = []
    for i, r in enumerate(records()):
        P = r[: len(r) // 2] + rnd(0x10B0 + i, 100) + r[len(r) // 2:]
        rec = bytearray(r)
        for p in range(50, len(rec), 997):
            rec[p] ^= 0x20
        rec = bytes(rec)
        chunks.append(Chunk(long_frame(rec, P), P, record=rec, palign=i % 16, dalign=(3 * i) % 16))
    extra = _lib.F_BLOCK_PARALLEL if block_parallel else 0
    for device in (False, True):
        r = Run(chunks, device, flags=_lib.F_LONG_WINDOW | extra)
        try:
            st, ln = r.decode()
            assert bool(r.b.info.executors & _lib.EXEC_K4J) == block_parallel
            assert st == [0] * len(chunks) and all(o == c.record for o, c in zip(r.out, chunks))
        finally:
            r.close()
        r = Run(chunks, device, flags=extra)
        try:
            st, ln = r.decode()
            assert st == [WINDOW_SIZE_TOO_BIG] * len(chunks) and ln == [0] * len(chunks)
        finally:
            r.close()


@pytest.mark.gpu
def test_chunk_sizes_agree_with_the_batch():
    import torch
    from zstd_decompressor.batch import chunk_sizes
    recs = records()
    frames = [long_frame(r) for r in recs] + [libzstd.compress(RECORD, 3)]
    dev = torch.device("cuda", 0)
    srcs = [torch.frombuffer(bytearray(f), dtype=torch.uint8).to(dev) for f in frames]
    ptrs, sizes = [t.data_ptr() for t in srcs], [len(f) for f in frames]
    from zstd_decompressor.batch import frames_index
    for long_window in (False, True):
        sz, st, ex = chunk_sizes(ptrs, sizes, long_window=long_window)
        torch.cuda.synchronize()
        sz, st, ex = sz.cpu().tolist(), st.cpu().tolist(), ex.cpu().tolist()
        assert st[-1] == 0 and sz[-1] == len(RECORD) and ex[-1] == 1
        for i, r in enumerate(recs):
            if long_window:
                # what a batch reserves for a frame without a Frame_Content_Size: 128 KiB a compressed block
                nb = len(frames_index(libzstd.compress(r, 3, content_size=False))[1])
                assert (st[i], ex[i]) == (0, 0) and sz[i] >= len(r) and sz[i] <= nb * (128 << 10), i
            else:
                assert (st[i], sz[i], ex[i]) == (WINDOW_SIZE_TOO_BIG, 0, 0), i


@pytest.mark.gpu
def test_cli_long(tmp_path, capsys):
    """--long for a plain decode and for --patch-from; a --patch-from frame of 2 MiB and more (decoded
    block-parallel) gives the same bytes as ever."""
    from test_batch_prefix_gpu import rnd
    from zstd_decompressor.__main__ import PATCH_BLOCK_PARALLEL_BYTES, main
    out = tmp_path / "out"
    (tmp_path / "plain.zst").write_bytes(long_frame(RECORD))
    assert main([str(tmp_path / "plain.zst"), "-o", str(out)]) != 0
    assert "WindowSizeTooBig" in capsys.readouterr().err
    assert main([str(tmp_path / "plain.zst"), "--long", "-o", str(out)]) == 0
    assert out.read_bytes() == RECORD
    old = RECORD[:2000] + rnd(0x10C0, 50) + RECORD[2000:]
    (tmp_path / "new.zst").write_bytes(long_frame(RECORD, old))
    (tmp_path / "old").write_bytes(old)
    assert main([str(tmp_path / "new.zst"), "--patch-from", str(tmp_path / "old"), "-o", str(out)]) != 0
    assert "WindowSizeTooBig" in capsys.readouterr().err
    assert main([str(tmp_path / "new.zst"), "--patch-from", str(tmp_path / "old"), "--long", "-o", str(out)]) == 0
    assert out.read_bytes() == RECORD
    # a delta past the block-parallel threshold, with and without --long
    big_old = gen.text(2560 << 10, seed=0x10C1)
    big_new = big_old[:1000] + rnd(0x10C2, 300) + big_old[1000:-300]
    assert len(big_new) >= PATCH_BLOCK_PARALLEL_BYTES == 2 << 20
    (tmp_path / "big.zst").write_bytes(zdict.prefix_compress(big_new, big_old))
    (tmp_path / "big_old").write_bytes(big_old)
    for extra in ([], ["--long"]):
        assert main([str(tmp_path / "big.zst"), "--patch-from", str(tmp_path / "big_old"), "-o", str(out)] + extra) == 0
        assert out.read_bytes() == big_new
