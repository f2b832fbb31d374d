"""The level rule of a chain batch (zd_chain.h chain_level / chain_order),
driven on the host by tests/native/chain_levels.cpp (compiled with g++, no
GPU): what zd_batch_create_chain checks its parent array with and groups its
chunks by, and what zd_k_chain_levels runs one lane per chunk."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cases(tmp_path_factory):
    d = tmp_path_factory.mktemp("chain_levels")
    exe = d / "chain_levels"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "chain_levels.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)
    rows = {}
    for line in out.stdout.splitlines():
        name, *nums = line.split()
        rows[name] = tuple(int(x) for x in nums)      # n, invalid, levels, level of the last chunk, props
    return rows


def test_every_case_ran(cases):
    assert set(cases) == {"root", "line256", "line257", "self", "cycle2", "cycle3", "tail_behind_cycle", "parent_n",
                          "parent_minus2", "child_of_bad_entry", "child_before_parent", "star1000", "forests",
                          "forests_agreeing"}


def test_order_is_a_permutation_grouped_by_level_and_counts_sum_to_n(cases):
    assert all(row[4] == 1 for row in cases.values()), {k: v for k, v in cases.items() if v[4] != 1}


def test_a_root_is_level_0(cases):
    assert cases["root"] == (1, 0, 1, 0, 1)


def test_a_line_of_256_is_valid_and_its_last_chunk_has_255_ancestors(cases):
    assert cases["line256"] == (256, 0, 256, 255, 1)


def test_the_257th_of_a_line_is_invalid_alone(cases):
    assert cases["line257"] == (257, 1, 256, -1, 1)


def test_a_self_parent_is_invalid(cases):
    assert cases["self"] == (2, 1, 1, -1, 1)


def test_every_chunk_of_a_cycle_is_invalid(cases):
    assert cases["cycle2"] == (3, 2, 1, -1, 1)
    assert cases["cycle3"] == (4, 3, 1, -1, 1)


def test_a_tail_behind_a_cycle_reaches_no_root(cases):
    assert cases["tail_behind_cycle"] == (5, 5, 1, -1, 1)


def test_out_of_range_parents_are_invalid(cases):
    assert cases["parent_n"] == (3, 1, 2, -1, 1)
    assert cases["parent_minus2"] == (3, 1, 2, -1, 1)


def test_chunks_behind_a_bad_entry_keep_their_levels(cases):
    # the chunk with the bad entry is refused alone; its child and grandchild
    # are levels 1 and 2 (they are not decoded because of its status)
    assert cases["child_of_bad_entry"] == (3, 1, 3, 2, 1)


def test_a_child_may_come_before_its_parent(cases):
    assert cases["child_before_parent"] == (3, 0, 3, 0, 1)


def test_a_star_of_1000_children_has_two_levels(cases):
    assert cases["star1000"] == (1001, 0, 2, 1, 1)


def test_200_random_forests_agree_with_the_recursive_reference(cases):
    assert cases["forests_agreeing"][0] == 200
