"""Every launch route a small plan can take (zd_route.h launch_route), decoded
bit-exact against the oracle with equal statuses: the fused kernel beside a
forked K2, K4F and the fork, K1 as two passes, the one-lane K3, and K1's
halves on two streams without a fork.  Each plan is launched under profiling
mode 0, 1, 2 and 0 again -- the route is resolved per launch, so the same plan
changes route between launches -- and once more as a Batch of its frames."""
import pytest

from corpus import gen, libzstd
from oracle import oracle

pytestmark = pytest.mark.gpu

N_SMALL = 300      # on 256 CUs: fused (1-4 frames per CU) and forked (K3's one round 0.02 full)


@pytest.fixture(scope="module")
def inputs():
    """name -> (frames, their oracle results): ~300 single-block frames of 1-4
    KiB of text, and eight frames of two blocks."""
    text = gen.text(N_SMALL * 4096 + 8 * (160 << 10), seed=97)
    small, at = [], 0
    for i in range(N_SMALL):
        n = 1024 + (i * 977) % 3073
        small.append(libzstd.compress(text[at:at + n], 3))
        at += n
    two = [libzstd.compress(text[at + k * (160 << 10):at + (k + 1) * (160 << 10)], 3) for k in range(8)]
    out = {}
    for name, frames in (("small", small), ("two-block", two)):
        res = [oracle.decompress_status(f) for f in frames]
        assert all(st == 0 for st, _ in res)
        out[name] = (frames, res)
    return out


def plans():
    from zstd_decompressor import _lib
    return [("small", 0, _lib.EXEC_FUSED), ("small", _lib.F_NO_FUSE, _lib.EXEC_K4F), ("small", _lib.F_K1_SPLIT, None),
            ("small", _lib.F_SEQ_ONE_LANE, None), ("two-block", 0, None)]


def to_device(data: bytes):
    import torch
    t = torch.zeros(len(data) + 64, dtype=torch.uint8, device="cuda:0")
    t[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    return t


@pytest.mark.parametrize("case", range(5))
def test_plan_under_every_profiling_mode(inputs, case):
    import torch
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Plan
    name, flags, executor = plans()[case]
    frames, res = inputs[name]
    data = b"".join(frames)
    want = b"".join(o for _, o in res)
    plan = Plan(data, False, flags)
    try:
        assert plan.info.nframes == len(frames)
        if name == "two-block":
            assert plan.info.nblocks == 2 * len(frames)
        else:
            assert plan.info.nblocks == len(frames) == plan.info.ncompressed
        if executor is not None:
            assert plan.info.executors & executor, plan.info.executors
        if flags & (_lib.F_NO_FUSE | _lib.F_SEQ_ONE_LANE) or name == "two-block":
            assert not plan.info.executors & _lib.EXEC_FUSED
        d_src = to_device(data)
        n = plan.info.out_bytes
        d_dst = torch.zeros(n + 64, dtype=torch.uint8, device="cuda:0")
        for mode in (0, 1, 2, 0):
            plan.set_profiling(mode)
            d_dst.zero_()
            torch.cuda.synchronize()
            plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, 0)
            st, total, statuses, lengths, _ = plan.results(d_dst.data_ptr(), 0)
            assert st == 0 and statuses == [s for s, _ in res], (mode, st)
            assert lengths == [len(o) for _, o in res] and total == len(want), mode
            assert d_dst[:total].cpu().numpy().tobytes() == want, f"profiling mode {mode}: output differs"
            if mode:
                assert plan.kernel_times()
    finally:
        plan.close()


@pytest.mark.parametrize("case", range(5))
def test_the_same_chunks_as_a_batch(inputs, case):
    import torch
    from zstd_decompressor.batch import Batch
    name, flags, _ = plans()[case]
    frames, res = inputs[name]
    d_src = to_device(b"".join(frames))
    caps = [len(o) for _, o in res]
    d_dst = torch.zeros(sum(caps) + 64, dtype=torch.uint8, device="cuda:0")
    src_ptrs, dst_ptrs, a, b = [], [], d_src.data_ptr(), d_dst.data_ptr()
    for f, c in zip(frames, caps):
        src_ptrs.append(a)
        dst_ptrs.append(b)
        a += len(f)
        b += c
    torch.cuda.synchronize()
    batch = Batch(src_ptrs, [len(f) for f in frames], dst_ptrs, caps, flags=flags)
    try:
        batch.decode_async(0)
        statuses, lengths = batch.results(0)
        assert statuses == [s for s, _ in res] and lengths == caps
        assert d_dst[: sum(caps)].cpu().numpy().tobytes() == b"".join(o for _, o in res)
    finally:
        batch.close()
