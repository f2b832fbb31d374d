"""The launch route (zstd-decompressor_amd/csrc/zd_route.h): what one
zd_decode_async launches and on which stream, as a pure function of the plan's
shape, its flags, its fused bit, the profiling mode, the CU count and the
experiment overrides.

tests/native/route_table.cpp (g++, no HIP, no GPU) prints launch_route,
plan_route and route_plan over a grid; this file holds the specification they
are compared with case for case: the rules as the launch path stated them
when the decision was spread over plan_ctx, plan_totals, decode_launch and
launch_pipeline, written out again here step by step in that order."""
import os
import subprocess
from collections import namedtuple
from types import SimpleNamespace as NS

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

F_BLOCK_PARALLEL, F_FRAME_SERIAL, F_SEQ_ONE_LANE, F_NO_FUSE, F_K1_LANES = 2, 4, 8, 32, 64
F_J_ONE_ROUND, F_SEQ_NO_LATENCY, F_K1_SPLIT = 128, 256, 512

ENV_FIELDS = ("fuse", "k4f", "fork", "k1fork", "k3l", "k1w_max", "k4j", "j_hops", "j_hops2")
Launch = namedtuple("Launch", "cus nf nt nh ns flags fused k4 prof env got plan_bits")
Plan = namedtuple("Plan", "cus nf flags single kind env got")


# ---------------------------------------------------------------------------
# the specification
# ---------------------------------------------------------------------------
def spec_route_plan(cus, nframes, n_tables, n_seq, n_huf, single, context, flags):
    """zd_route's rules: every bound in units of the CU count."""
    r = NS()
    r.fused = (not flags & (F_NO_FUSE | F_SEQ_ONE_LANE | F_BLOCK_PARALLEL) and not context and single
               and cus <= nframes <= 4 * cus)
    r.k4f = not r.fused and cus <= nframes <= 3 * cus
    r.k1_seq_waves = n_tables <= 64 * cus and not flags & F_K1_LANES
    r.k1_split = bool(flags & F_K1_SPLIT) or (n_tables > 64 * cus and not flags & F_K1_LANES)
    slots = 64 * cus
    rem = n_seq % slots
    r.fork = n_seq >= cus and rem != 0 and rem <= 0.65 * slots
    r.k1_fork = not r.fork and n_huf != 0 and n_seq != 0
    r.k3_lat = n_seq <= 8 * cus and not flags & (F_SEQ_ONE_LANE | F_SEQ_NO_LATENCY)
    return r


def spec_launch(c):
    """One launch: first what decode_launch put into the launch arguments,
    then what launch_pipeline made of them."""
    E = c.env
    profile = c.prof == 1
    # decode_launch: the shape rules without the plan-time inputs, then the overrides
    r = spec_route_plan(c.cus, c.nf, c.nt, c.ns, c.nh, False, False, c.flags)
    big_fused = c.fused and c.nf > 4 * c.cus
    want_fork = (E.fork == 1 if E.fork >= 0 else r.fork) and not big_fused
    aux = want_fork
    k1_fork = False
    if not want_fork and not profile and ((E.k1fork == 1 and c.nh and c.ns) if E.k1fork >= 0 else r.k1_fork):
        aux = k1_fork = True
    k1_seq_waves = (c.nt <= E.k1w_max and not c.flags & F_K1_LANES) if E.k1w_max >= 0 else r.k1_seq_waves
    k1_split = r.k1_split
    k3_lat = (E.k3l == 1 and not c.flags & (F_SEQ_ONE_LANE | F_SEQ_NO_LATENCY)) if E.k3l >= 0 else r.k3_lat
    k3_quad = not c.flags & F_SEQ_ONE_LANE
    arg_fused = c.fused and not profile
    events = profile
    one_round = bool(c.flags & F_J_ONE_ROUND)
    j_hops = 1 if one_round else max(1, E.j_hops) if E.j_hops >= 0 else 6
    j_hops2 = 1 if one_round else max(1, E.j_hops2) if E.j_hops2 >= 0 else 12
    # launch_pipeline
    fork = bool(aux and not k1_fork and not events and c.nh and c.ns)
    k1f = bool(aux and k1_fork and not events and c.nt)
    fz = arg_fused and not events
    if fz:
        k1 = "huf_split" if k1_split else "huf_lanes"
    elif k1_split:
        k1 = "split_two" if fork or k1f else "split_both"
    elif k1_seq_waves:
        k1 = "lanes_seqw"
    elif fork or k1f:
        k1 = "lanes_two"
    else:
        k1 = "lanes_both"
    k3 = "l" if k3_lat and k3_quad else "q" if k3_quad else "one_lane"
    return (int(fz), int(fork), int(k1f), int(events), int(c.prof == 2), k1, k3, c.k4, j_hops, j_hops2)


def spec_plan(c):
    """plan_ctx: what the plan is built for; kind 0 a plain plan, 1 a context
    plan, 2 a dictionary plan.  Then plan_totals' narrowing and K4J's mode."""
    E = c.env
    context = c.kind != 0
    r = spec_route_plan(c.cus, c.nf, 2 * c.nf, c.nf, c.nf, c.single, context, c.flags)
    fused = r.fused
    if E.fuse == 0:
        fused = False
    if E.fuse == 1:
        fused = (not c.flags & (F_NO_FUSE | F_SEQ_ONE_LANE | F_BLOCK_PARALLEL) and not context and bool(c.single)
                 and c.nf >= 1)
    k4f = E.k4f == 1 if E.k4f >= 0 else r.k4f
    if fused or c.kind == 2:
        k4f = False
    k4j = 1 if c.flags & F_BLOCK_PARALLEL else 0 if c.flags & F_FRAME_SERIAL else E.k4j
    # (a plan whose frames all stayed off K4J and K4F keeps the bit, any other loses it)
    return (int(fused), int(k4f), int(fused), 0, k4j)


# ---------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------
def _env(f):
    return NS(**{k: int(v) for k, v in zip(ENV_FIELDS, f)})


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    exe = tmp_path_factory.mktemp("route") / "route_table"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "route_table.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout
    launches, plans = [], []
    envs = {}
    for line in out.splitlines():
        head, *rest = line.split(" : ")
        f = head.split()
        key = tuple(f[-9:])
        env = envs.get(key) or envs.setdefault(key, _env(key))
        if f[0] == "L":
            g = rest[0].split()
            got = tuple(int(x) for x in g[:5]) + (g[5], g[6], g[7], int(g[8]), int(g[9]))
            cus, nf, nt, nh, ns, flags, fused = (int(x) for x in f[1:8])
            launches.append(Launch(cus, nf, nt, nh, ns, flags, fused, f[8], int(f[9]), env, got,
                                   tuple(int(x) for x in rest[1].split())))
        else:
            cus, nf, flags, single, kind = (int(x) for x in f[1:6])
            plans.append(Plan(cus, nf, flags, single, kind, env, tuple(int(x) for x in rest[0].split())))
    return NS(launches=launches, plans=plans, envs=list(envs.values()))


def _default(E):
    return all(getattr(E, k) == -1 for k in ENV_FIELDS)


def test_the_grid_is_the_one_asked_for(table):
    L = table.launches
    assert {c.cus for c in L} == {80, 256}
    for cus in (80, 256):
        assert {c.nf for c in L if c.cus == cus} == {1, cus - 1, cus, 3 * cus, 4 * cus, 4 * cus + 1, 40 * cus, 320 * cus}
    assert {(c.nt // c.nf, c.nh // c.nf, c.ns // c.nf) for c in L if _default(c.env)} == \
        {(t, h, s) for t in range(3) for h in range(3) for s in range(3)}
    assert {c.flags for c in L} >= {0, F_SEQ_ONE_LANE, F_SEQ_NO_LATENCY, F_NO_FUSE, F_K1_SPLIT, F_K1_LANES,
                                    F_BLOCK_PARALLEL}
    assert {c.fused for c in L} == {0, 1} and {c.prof for c in L} == {0, 1, 2}
    assert {c.k4 for c in L} == {"plain", "dict", "dicts"}
    seen = {tuple(getattr(E, k) for k in ENV_FIELDS) for E in table.envs}
    base = (-1,) * len(ENV_FIELDS)
    assert base in seen
    for i, k in enumerate(ENV_FIELDS):
        for v in ((0, 1 << 30) if k == "k1w_max" else (0, 1)):
            assert base[:i] + (v,) + base[i + 1:] in seen, (k, v)


def test_launch_route_equals_the_specification(table):
    bad = [(c, spec_launch(c)) for c in table.launches if c.got != spec_launch(c)]
    assert not bad, f"{len(bad)} of {len(table.launches)} cases differ, the first: {bad[0]}"


def test_plan_route_equals_the_specification(table):
    bad = [(c, spec_plan(c)) for c in table.plans if c.got != spec_plan(c)]
    assert not bad, f"{len(bad)} of {len(table.plans)} cases differ, the first: {bad[0]}"


def test_route_plan_equals_the_specification(table):
    for c in table.launches:
        r = spec_route_plan(c.cus, c.nf, c.nt, c.ns, c.nh, c.fused, False, c.flags)
        want = tuple(int(x) for x in (r.fused, r.k4f, r.k1_seq_waves, r.fork, r.k1_fork, r.k1_split, r.k3_lat))
        assert c.plan_bits == want, c


def test_launch_route_invariants(table):
    for c in table.launches:
        fused, fork, k1_fork, kev, gev, k1, k3, k4, j_hops, j_hops2 = c.got
        assert not (fork and k1_fork), c
        if c.prof == 1:
            assert not fork and not k1_fork and not fused and kev, c
        assert not fork or (c.nh and c.ns), c
        assert not k1_fork or c.nt, c
        assert (k1 in ("huf_lanes", "huf_split")) == bool(fused), c
        if c.fused and c.nf > 4 * c.cus:
            assert not fork, c
        if c.flags & F_SEQ_ONE_LANE:
            assert k3 == "one_lane", c
        assert k4 == c.k4 and j_hops >= 1 and j_hops2 >= 1, c
        assert gev == (c.prof == 2) and kev == (c.prof == 1), c


def test_launch_route_agrees_with_zd_route(table):
    """Default overrides, no profiling: the launch does what zd_route's bits
    say wherever the plan's counts leave the bit a meaning."""
    n = 0
    for c in table.launches:
        if not _default(c.env) or c.prof:
            continue
        n += 1
        p_fused, p_k4f, p_seqw, p_fork, p_k1fork, p_split, p_lat = c.plan_bits
        fused, fork, k1_fork, _, _, k1, k3, *_ = c.got
        assert fused == c.fused, c                               # the plan's bit, zd_route's FUSED when it fuses
        if c.nh and c.ns and not (c.fused and c.nf > 4 * c.cus):
            assert fork == p_fork, c
        if c.nt:
            assert k1_fork == p_k1fork, c
        assert (k1 in ("split_both", "split_two", "huf_split")) == bool(p_split), c
        if not fused and not p_split:
            assert (k1 == "lanes_seqw") == bool(p_seqw), c
        assert (k3 == "l") == bool(p_lat), c
    assert n > 1000
