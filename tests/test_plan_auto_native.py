"""ZD_F_AUTO_EXECUTOR's routing in the planner (zd_plan.h plan_frame with
PlanCtx::auto_exec, plan_auto_j, plan_k4j_fields; zd_route.h auto_exec,
chain_j_layout), driven on the host by tests/native/plan_auto.cpp over
hand-made indexes (compiled with g++, no GPU): the counting pass and the
filling pass of every case agree (exit status 4 otherwise).  The four constants
come from include/zd.h.  The driver also runs built with ASan + UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "plan_auto.cpp")
HEADER = open(os.path.join(ROOT, "include", "zd.h")).read()


def const(name):
    return int(re.search(r"#define\s+%s\s+(\d+)u?\b" % name, HEADER).group(1))


MIN, FEW = const("ZD_AUTO_MIN_BLOCKS"), const("ZD_AUTO_MIN_BLOCKS_FEW")
FC, MC = const("ZD_AUTO_FEW_CHUNKS"), const("ZD_AUTO_MAX_CANDIDATES")
K4J, K0ONLY, OUT_OF_DOMAIN = 2, 3, -91     # FrameDesc::lds of a K4J frame / a frame K0 copies whole; ZD_E_OUT_OF_DOMAIN


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    # (4: the counting and the filling pass disagree; 6: chain_order; 7: lds and the J count disagree)
    assert out.returncode == 0, (out.returncode, out.stderr)
    res = {"C": {}, "A": {}, "S": {}, "J": [], "L": []}
    for line in out.stdout.splitlines():
        tag, *v = line.split()
        if tag == "C":
            frames = [tuple(map(int, x.split(":")))[1:] for x in v[2:]]      # (lds, status, nblocks)
            res["C"][v[0]] = (int(v[1]), frames)
        elif tag == "A":
            res["A"][v[0]] = (int(v[1]), int(v[2]))
        elif tag == "S":
            res["S"][v[0]] = int(v[1])
        elif tag in ("J", "L"):
            res[tag].append(tuple(map(int, v)))
        else:
            res[tag] = tuple(map(int, v))
    return res


@pytest.fixture(scope="module")
def plan(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_auto")
    exe = d / "plan_auto"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe), SRC])
    return _run(exe)


def on_j(case, plan):
    """The frames of a C case that went to K4J, by index (the first eight)."""
    n, frames = plan["C"][case]
    got = [i for i, f in enumerate(frames) if f[0] == K4J]
    assert n == len(got), case          # (the padding past the first eight is raw-only: never K4J's)
    return got


def test_the_constants_make_sense():
    assert 1 <= FEW <= MIN and FC >= 1 and MC >= 1


def test_the_block_minimum_at_a_width_above_the_few_limit(plan):
    # min - 1 blocks stays, min blocks goes
    assert on_j("a_min", plan) == [1]
    assert plan["C"]["a_min"][1][1][2] == MIN


def test_the_few_chunks_minimum_at_the_limit_and_one_past_it(plan):
    assert on_j("few_at", plan) == [1]                  # width == FC: FEW blocks are enough
    assert plan["C"]["few_at"][1][1][2] == FEW
    want = [2] if FEW < MIN else [1, 2]
    assert on_j("few_past", plan) == want               # width == FC + 1: the full minimum


def test_candidates_at_the_cap_and_one_past_it(plan):
    assert plan["A"]["cand_cap"][0] == MC               # MC frames of MIN blocks: all of them, not the one below
    assert plan["A"]["cand_past"][0] == 0               # MC + 1: (a) is off for the whole batch


def test_a_frame_the_streaming_executor_cannot_hold(plan):
    # prefix 0x70000000 + capacity 0x20000000: K4J under the flag, ZD_E_OUT_OF_DOMAIN without it
    assert plan["C"]["big_auto"] == (1, [(K4J, 0, 0x20000000 // (128 << 10))])
    assert plan["C"]["big_noflag"] == (0, [(0, OUT_OF_DOMAIN, 0)])
    # (b) alone: one block, far below the minimum, prefix just inside the limit
    assert on_j("edge_auto", plan) == [0]
    assert plan["C"]["edge_noflag"][0] == 0 and plan["C"]["edge_noflag"][1][0] == (0, OUT_OF_DOMAIN, 0)


def test_a_prefix_past_the_limit_is_refused_either_way(plan):
    assert plan["C"]["over_auto"] == plan["C"]["over_noflag"] == (0, [(0, OUT_OF_DOMAIN, 0)])


def test_raw_only_and_failed_frames_stay(plan):
    assert plan["C"]["rawonly"] == (1, [(K0ONLY, 0, 1), (K4J, 0, MIN)])
    assert plan["C"]["failed"] == (1, [(0, -50, 0), (K4J, 0, MIN)])


def test_precedence_in_a_prefix_batch(plan):
    auto = on_j("pfx_auto", plan)
    assert auto == ([1] if MIN > 1 else [0, 1])
    assert on_j("pfx_auto_bp", plan) == on_j("pfx_bp", plan) == [0, 1]      # every frame with a compressed block
    assert plan["C"]["pfx_auto_bp"] == plan["C"]["pfx_bp"]
    assert on_j("pfx_auto_fs", plan) == []
    assert plan["C"]["pfx_auto_bp_fs"] == plan["C"]["pfx_bp"]
    assert plan["C"]["pfx_auto_cbp"] == plan["C"]["pfx_auto"]               # (the chain flag means nothing here)
    # ZD_K4J in the environment means nothing behind a prefix, with the flag or without
    assert plan["C"]["pfx_auto_env1"] == plan["C"]["pfx_auto_env0"] == plan["C"]["pfx_auto"]
    assert on_j("pfx_env1", plan) == []


def test_precedence_in_a_chain_batch(plan):
    assert plan["C"]["chn_auto"] == plan["C"]["pfx_auto"]
    assert on_j("chn_auto_cbp", plan) == [0, 1] and plan["C"]["chn_auto_cbp"] == plan["C"]["chn_cbp"]
    assert plan["C"]["chn_auto_bp"] == plan["C"]["chn_auto_fs"] == plan["C"]["chn_auto"]


def test_a_chain_plan_reads_the_widest_level_and_numbers_level_major(plan):
    # levels 0, 1, 2 hold 3, 3, 2 chunks: the width is 3
    assert plan["W"] == (3, FEW if 3 <= FC else MIN)
    # chunks 6 (level 0) and 4 (level 2) have one block more than that minimum, the others one fewer or none compressed
    assert plan["J"] == [(0, 6), (1, 4)]
    (l0, l1, l2) = plan["L"]
    segs = plan["W"][1] + 1
    assert l0[:5] == (0, 0, 1, 0, segs)
    assert l1[:5] == (1, 1, 0, segs, 0) and l1[6] == 0          # a level without a K4J frame: an empty range in place
    assert l2[:5] == (2, 1, 1, segs, segs)
    assert l1[5] == l0[5] + l0[6] == l2[5]
    assert plan["D"] == (1,)


def test_the_flag_means_nothing_to_a_dictionary_plan_or_a_plain_plan(plan):
    assert plan["S"] == {"dict": 1, "plain": 1, "plain_many": 1, "plain_bp": 1}


def test_the_mode_functions(plan):
    assert plan["M"] == (1,)


def test_the_driver_is_clean_under_asan_and_ubsan(plan, tmp_path):
    exe = tmp_path / "plan_auto_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", str(exe), SRC])
    assert _run(exe) == plan
