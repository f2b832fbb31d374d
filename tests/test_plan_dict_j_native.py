"""The planner's per-frame pass for dictionary and dictionary-set plans created
with ZD_F_DICT_BLOCK_PARALLEL (zd_plan.h plan_frame with PlanCtx::dict_j, which
plan_k4j_fields sets from zd_route.h dict_j / dict_j_mode), driven on the host
by tests/native/plan_dict_j.cpp (compiled with g++, no GPU): what
zd_plan_create_dict / _dicts and the dictionary batches plan with under the
flag.  The driver also runs built with ASan + UBSan."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "plan_dict_j.cpp")
OUT_OF_DOMAIN, DICT_MISMATCH = -91, -99
K4J, STREAMING = 2, 0
GIB = 1 << 30
COLS = ("lds", "status", "nblocks", "jcap", "out_len0", "jframes", "jsrc", "rep0", "tab0")


def const(name):
    text = open(os.path.join(ROOT, "include", "zd.h")).read()
    return int(re.search(r"#define %s\s+(\d+)" % name, text).group(1))


def _lines(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    # (3: a frame count that is off; 4: the counting and the filling pass disagree; 5: an old route function
    # answers differently; 6: a set plan's JFrame names another entry than Sink::frame_dict)
    assert out.returncode == 0, (out.returncode, out.stderr)
    res = {}
    for line in out.stdout.splitlines():
        name, *v = line.split()
        res[name] = dict(zip(COLS, map(int, v)))
    return res


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_dict_j")
    exe = d / "plan_dict_j"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe), SRC])
    return _lines(exe)


def test_every_case_ran_and_the_passes_and_old_functions_agree(cases):
    # (exit status 0: the counting pass equals the filling pass in every case, and k4j_mode_of, k4j_mode_behind,
    # k4j_mode_plan, chain_j, auto_exec, plan_k4j_min, plan_k4j_counts and plan_k4j_fields answer as before)
    assert len(cases) == 18


def test_a_dictionary_frame_is_a_j_frame_only_under_the_field(cases):
    # the J frame keeps the dictionary's content size, first repeat offset and tables (prebuilt comp 0)
    assert cases["forced"] == dict(lds=K4J, status=0, nblocks=1, jcap=200, out_len0=5000, jframes=1, jsrc=0,
                                   rep0=11, tab0=0)
    streaming = dict(lds=STREAMING, status=0, jcap=0, out_len0=5000, jframes=0, jsrc=0, rep0=11, tab0=0)
    assert cases["noflag"] == dict(streaming, nblocks=1)
    for name in ("serial", "both", "old_fields"):
        assert cases[name] == dict(streaming, nblocks=3), name


def test_the_rule_without_a_forcing_flag(cases):
    few, many = const("ZD_AUTO_MIN_BLOCKS_FEW"), const("ZD_AUTO_MIN_BLOCKS")
    assert (few, many, const("ZD_AUTO_FEW_CHUNKS")) == (2, 4, 64)      # what the cases' block counts stand for
    assert cases["auto6_3"]["lds"] == K4J and cases["auto6_3"]["jcap"] == 300000
    assert cases["auto6_1"]["lds"] == STREAMING and cases["auto6_1"]["jframes"] == 0
    assert cases["auto65_3"]["lds"] == STREAMING and cases["auto65_3"]["jframes"] == 0
    assert cases["auto65_4"]["lds"] == K4J and cases["auto65_4"]["jcap"] == 400000
    # more candidates in the plan than the dictionary plans' cap: clause (a) holds for none of them
    assert const("ZD_AUTO_DICT_MAX_CANDIDATES") <= const("ZD_AUTO_MAX_CANDIDATES")
    assert cases["auto_at_cap"]["lds"] == K4J and cases["auto_at_cap"]["jframes"] == 1
    assert cases["auto_cap"]["lds"] == STREAMING and cases["auto_cap"]["jframes"] == 0
    for name in ("auto6_3", "auto6_1", "auto65_3", "auto65_4", "auto_at_cap", "auto_cap"):
        assert cases[name]["status"] == 0 and cases[name]["out_len0"] == 5000, name


def test_clause_b_content_plus_capacity_past_the_streaming_limit(cases):
    c = cases["b_auto"]
    assert c == dict(lds=K4J, status=0, nblocks=8192, jcap=GIB, out_len0=GIB, jframes=1, jsrc=0, rep0=11, tab0=0)
    for name in ("b_serial", "b_noflag"):
        c = cases[name]
        assert c["status"] == OUT_OF_DOMAIN and c["lds"] == STREAMING and c["jframes"] == 0, name


def test_a_set_frame_takes_its_own_entry(cases):
    # entry 2 of the table: ID 70000, 16384 bytes, repeat offsets 21 22 23, prebuilt comp 1
    assert cases["set_named"] == dict(lds=K4J, status=0, nblocks=1, jcap=200, out_len0=16384, jframes=1, jsrc=2,
                                      rep0=21, tab0=1)
    assert cases["set_noflag"] == dict(lds=STREAMING, status=0, nblocks=1, jcap=0, out_len0=16384, jframes=0, jsrc=0,
                                       rep0=21, tab0=1)
    # no ID and no fallback: no dictionary (0 bytes, 1 4 8, no previous tables: the Repeat_Mode block fails as it
    # does on the streaming executor), the source entry the set's address for such frames
    c = cases["set_none"]
    assert c["out_len0"] == 0 and c["rep0"] == 1 and c["tab0"] == -1 and c["status"] != 0
    assert c["lds"] == K4J and c["jsrc"] == 3 and c["jcap"] == 200
    c = cases["set_missing"]
    assert c["status"] == DICT_MISMATCH and c["nblocks"] == 0 and c["jframes"] == 0 and c["lds"] == STREAMING


def test_the_driver_is_clean_under_asan_and_ubsan(cases, tmp_path):
    exe = tmp_path / "plan_dict_j_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", str(exe), SRC])
    assert _lines(exe) == cases
