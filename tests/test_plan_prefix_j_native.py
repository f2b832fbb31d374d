"""The planner's per-frame pass for prefix batches that ask for the
block-parallel executor (zd_plan.h plan_frame with PlanCtx::prefix_bytes and
k4j_mode 1; zd_route.h k4j_mode_behind, the mode plan_ctx hands it), driven on
the host by tests/native/plan_prefix_j.cpp (compiled with g++, no GPU): what
zd_batch_create_prefix and zd_batch_create_device_prefix plan with under
ZD_F_BLOCK_PARALLEL.  The driver also runs built with ASan + UBSan."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "plan_prefix_j.cpp")
OUT_OF_DOMAIN = -91
K4J, STREAMING, K0_ONLY = 2, 0, 3


def _lines(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    # (3: a frame count that is off; 4: the counting and the filling pass disagree; 5: k4j_mode_behind)
    assert out.returncode == 0, (out.returncode, out.stderr)
    res = {}
    for line in out.stdout.splitlines():
        name, *v = line.split()
        res[name] = dict(zip(("lds", "status", "nblocks", "jcap", "out_len0", "jframes"), map(int, v)))
    return res


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_prefix_j")
    exe = d / "plan_prefix_j"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe), SRC])
    return _lines(exe)


def test_every_case_ran(cases):
    assert len(cases) == 11


def test_a_large_prefix_and_capacity_go_to_k4j(cases):
    # prefix 0x70000000 + capacity 0x20000000 is past the streaming executor's 0x7FFF0000
    c = cases["big_j"]
    assert c == dict(lds=K4J, status=0, nblocks=4096, jcap=0x20000000, out_len0=0x70000000, jframes=1)


def test_the_same_frame_with_the_mode_off_is_out_of_domain_as_before(cases):
    c = cases["big_off"]
    assert c["status"] == OUT_OF_DOMAIN and c["nblocks"] == 0 and c["lds"] == STREAMING and c["jframes"] == 0


def test_a_prefix_above_the_limit_is_refused_in_both_modes(cases):
    for name in ("over_j", "over_off"):
        c = cases[name]
        assert c["status"] == OUT_OF_DOMAIN and c["nblocks"] == 0 and c["jframes"] == 0, name
        assert c["out_len0"] == 0, name          # (a size past the limit is not even kept)


def test_every_frame_with_a_compressed_block_goes_to_k4j(cases):
    assert cases["small_j"] == dict(lds=K4J, status=0, nblocks=1, jcap=200, out_len0=5000, jframes=1)
    assert cases["none_j"] == dict(lds=K4J, status=0, nblocks=1, jcap=200, out_len0=0, jframes=1)
    # a frame without one keeps today's rules: K0 copies it whole
    assert cases["rawonly_j"] == dict(lds=K0_ONLY, status=0, nblocks=1, jcap=0, out_len0=5000, jframes=0)


def test_chain_and_dictionary_plans_never_go_to_k4j(cases):
    for name in ("chain", "dict", "dict_forced", "unflagged"):
        c = cases[name]
        assert c["lds"] == STREAMING and c["jframes"] == 0 and c["status"] == 0 and c["nblocks"] == 1, name


def test_the_driver_is_clean_under_asan_and_ubsan(cases, tmp_path):
    exe = tmp_path / "plan_prefix_j_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", str(exe), SRC])
    assert _lines(exe) == cases
