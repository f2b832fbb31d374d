"""The carve of a batch's per-chunk arrays (zd_plan.h BatchCarve: the byte
offsets zd_batch_create* slices its one device allocation with), driven on
the host by tests/native/batch_arrays.cpp (compiled with g++, no GPU): every
offset and total against the layout's formulas, alignment, no overlap, and a
few totals as plain numbers."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    d = tmp_path_factory.mktemp("batch_arrays")
    exe = d / "batch_arrays"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "batch_arrays.cpp")])
    return subprocess.run([str(exe)], capture_output=True, text=True)


def test_every_offset_is_the_layouts(run):
    assert run.returncode == 0, run.stdout
    assert not [l for l in run.stdout.splitlines() if l.startswith("FAIL")]


def test_the_driver_ran_its_checks(run):
    # 8 sizes x (2 host + 2 device carves), each some dozens of checks, and the six spot totals
    last = run.stdout.splitlines()[-1].split()
    assert last[0] == "ok" and int(last[1]) > 8 * 4 * 50
