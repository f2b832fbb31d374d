"""The planner of a chain batch created with ZD_F_CHAIN_BLOCK_PARALLEL: K4J's
frames, blocks, scatter segments, state words and pieces numbered level-major
(zd_plan.h plan_frame with PlanCtx::j_at, plan_j_order, plan_j_levels; zd_route.h
k4j_mode_plan), driven on the host by tests/native/plan_chain_j.cpp over a
hand-made index of eight chunks on three levels (compiled with g++, no GPU).
The driver also runs built with ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "plan_chain_j.cpp")

# the driver's index (its header comment): level, blocks, segments and capacity of each chunk; None: no K4J frame
LEVEL = [1, 0, 2, 0, 2, 1, 0, 1]
NBLK = [2, 1, 1, 1, 3, 1, 2, 1]
RAW = [False, False, True, True, False, False, False, True]
SEGS = [2, 3, 1, 1, 3, 1, 2, 1]
CAP = [1000 + 37 * i for i in range(8)]


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    # (4: the counting and the filling pass disagree; 5: k4j_mode_plan; 6: chain_order)
    assert out.returncode == 0, (out.returncode, out.stderr)
    res = {}
    for line in out.stdout.splitlines():
        tag, *v = line.split()
        res.setdefault(tag, []).append(tuple(map(int, v)))
    return res


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_chain_j")
    exe = d / "plan_chain_j"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe), SRC])
    return _run(exe)


def _expected_order():
    """The J frames level-major: levels ascending, chunk order kept inside a level."""
    return [i for lvl in range(3) for i in range(8) if LEVEL[i] == lvl and not RAW[i]]


def test_the_flag_turns_k4j_on_for_a_chain_plan_only(plan):
    assert plan["M"] == [(1, 0)]


def test_j_frames_are_numbered_level_major(plan):
    order = _expected_order()
    assert order == [1, 6, 0, 5, 4]
    assert [j[1] for j in plan["J"]] == order
    assert [j[0] for j in plan["J"]] == list(range(5))
    base = piece = jblk = seg = 0
    for (k, frame, jbase, piece0, jb0, njb, seg0) in plan["J"]:
        assert (jbase, piece0, jb0, njb, seg0) == (base, piece, jblk, NBLK[frame], seg), (k, frame)
        base += (CAP[frame] + 16 + 15) // 16 * 16
        piece += (CAP[frame] + 15) // 16
        jblk += NBLK[frame]
        seg += SEGS[frame]
    assert plan["T"] == [(5, jblk, seg, base, piece)]
    assert (jblk, seg, base, piece) == (9, 11, 5712, 352)


def test_j_blocks_and_segments_follow_their_frames(plan):
    # block k of J frame j, in J order; the segments of a block one after another
    want_b, want_s, seg = [], [], 0
    for j, frame in enumerate(_expected_order()):
        per = [3] if frame == 1 else [1] * NBLK[frame]
        for b, ns in enumerate(per):
            want_b.append((len(want_b), j, b, seg))
            for g in range(ns):
                want_s.append((len(want_s), len(want_b) - 1, g))
            seg += ns
    assert plan["B"] == want_b
    assert plan["S"] == want_s


def test_each_level_owns_a_contiguous_range_and_the_ranges_tile_the_totals(plan):
    levels = plan["L"]
    assert [l[0] for l in levels] == [0, 1, 2]
    jf = seg = piece = 0
    for (lvl, jf0, njf, seg0, nseg, piece0, npieces) in levels:
        assert (jf0, seg0, piece0) == (jf, seg, piece), lvl
        mine = [f for f in _expected_order() if LEVEL[f] == lvl]
        assert njf == len(mine)
        assert nseg == sum(SEGS[f] for f in mine)
        assert npieces == sum((CAP[f] + 15) // 16 for f in mine)
        # the level's J frames are exactly [jf0, jf0 + njf)
        assert [j[1] for j in plan["J"][jf0:jf0 + njf]] == mine
        jf, seg, piece = jf + njf, seg + nseg, piece + npieces
    (jframes, _, jseg, _, jpieces), = plan["T"]
    assert (jf, seg, piece) == (jframes, jseg, jpieces)


def test_the_device_planners_scan_in_order_gives_the_same_numbers(plan):
    assert plan["D"] == [(1,)]


def test_an_unflagged_chain_plans_no_j_frame(plan):
    assert plan["U"] == [(0,)]


def test_the_driver_is_clean_under_asan_and_ubsan(plan, tmp_path):
    exe = tmp_path / "plan_chain_j_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", str(exe), SRC])
    assert _run(exe) == plan
