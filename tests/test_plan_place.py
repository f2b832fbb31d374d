"""Host test of the planner's per-frame pass in the device planner's order with
per-frame placement and dictionaries (zd_plan.h plan_frame, as
zd_batch_create_device runs it through zd_k_plan_count, the scan seeded with
the dictionaries' prebuilt comps, and zd_k_plan_fill): ten hand-made frames
planned that way must give, field by field, what one serial running pass --
the host planner's order -- gives.  Compiled with g++ from
tests/native/plan_place.cpp (its own main); no GPU needed.  Built once more
with AddressSanitizer and UndefinedBehaviorSanitizer and run the same way."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "plan_place.cpp")
# mode -> (frames, comps with the prebuilt ones, blocks, K0 pieces, K4J frames)
MODES = {"single": (10, 10, 14, 5, 0), "set0": (10, 11, 14, 5, 0), "set-1": (10, 11, 14, 5, 0),
         "plain": (10, 9, 14, 4, 6), "fused": (10, 9, 14, 5, 0)}
# (the sanitizers' runtimes linked into the program itself: it needs nothing of its environment)
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]


@pytest.fixture(scope="module", params=["plain build", "sanitized build"])
def plan_place(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("plan_place") / "plan_place"
    extra = SAN if request.param == "sanitized build" else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", *extra, "-o", str(exe), SRC])

    def run(mode):
        env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
        out = subprocess.run([str(exe), mode], capture_output=True, text=True, env=env)
        assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
        assert out.stderr == ""
        words = out.stdout.split()
        assert words[0] == "equal"
        return tuple(int(x) for x in words[1:])
    return run


@pytest.mark.parametrize("mode", list(MODES))
def test_device_order_equals_host_order(plan_place, mode):
    assert plan_place(mode) == MODES[mode]
