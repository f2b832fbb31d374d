"""The planner's per-frame pass with per-frame prefix sizes (zd_plan.h
plan_frame, PlanCtx::prefix_bytes), driven on the host by
tests/native/plan_prefix.cpp (compiled with g++, no GPU): what
zd_batch_create_prefix and zd_batch_create_device_prefix plan with."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HUFFMAN_DECODER_MISSING, OUT_OF_DOMAIN, DICT_MISMATCH = -20, -91, -99


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    d = tmp_path_factory.mktemp("plan_prefix")
    exe = d / "plan_prefix"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "plan_prefix.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    # (3: a frame count that is off; 4: the counting and the filling pass disagree)
    assert out.returncode == 0, (out.returncode, out.stderr)
    return [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]


def test_counting_and_filling_passes_agree(lines):
    assert len(lines) == 6


def test_every_frame_starts_at_its_own_prefix_size(lines):
    assert [l[0] for l in lines] == [0, 1, 15, 5000, 0x7FFF0000, 0]


def test_repeat_offsets_are_1_4_8_whatever_the_plan_wide_ones(lines):
    # (the driver sets the plan-wide offsets to 7 7 7 and out_len0 to 999)
    assert all(l[1:4] == (1, 4, 8) for l in lines)


def test_a_prefix_brings_no_previous_tables(lines):
    # frame 1: Treeless literals and Repeat tables with nothing before them,
    # though the plan-wide previous tables are comp 0
    assert lines[1][4:8] == (-1, -1, -1, -1) and lines[1][8] == HUFFMAN_DECODER_MISSING
    # the others use their own tables (comp i) and no Huffman table at all
    for i in (0, 3, 5):
        assert lines[i][4:8] == (-1, i, i, i) and lines[i][8] == 0 and lines[i][9] == 1, i


def test_a_frame_that_names_a_dictionary_id_is_a_mismatch(lines):
    assert lines[2][8] == DICT_MISMATCH and lines[2][9] == 0


def test_prefix_plus_capacity_past_the_limit_is_out_of_domain(lines):
    # frame 4 (5 sequences, 200 bytes): 0x7FFF0000 + 200 > K4_MAX_FRAME_OUT; none of its blocks runs
    assert lines[4][8] == OUT_OF_DOMAIN and lines[4][9] == 0
