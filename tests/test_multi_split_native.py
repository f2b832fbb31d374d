"""Host test of the multi-frame batch's rule (zd_multi.h: where a chunk of
several concatenated frames is cut into sub-chunks, which of them decode in
place and at what offset and capacity, which are staged and where, and the
sums zd_chunk_sizes_device reports with ZD_SIZES_MULTI_FRAME), the code
zd_k_multi_count, zd_k_multi_fill and zd_k_multi_sizes run one lane a chunk.
tests/native/multi_split.cpp (its own main) walks hand-assembled chunks, each
in a heap block of exactly its size, against literal sub-chunks.  Compiled
with g++, no GPU needed; built once more with AddressSanitizer and
UndefinedBehaviorSanitizer linked statically and run the same way, so a read
outside a chunk is a report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "multi_split.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("build", ["plain build", "sanitized build"])
def test_hand_made_chunks(build, tmp_path):
    exe = tmp_path / "multi_split"
    extra = SAN if build == "sanitized build" else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", *extra, "-o", str(exe), SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stderr == ""
    words = out.stdout.split()
    assert words[0] == "ok" and int(words[1]) >= 24 and int(words[2]) >= 50
