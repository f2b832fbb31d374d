"""Host test of a chunk's size query (zd_walk.h chunk_size_query: the shared
header walk over the bound-only sink, then the reserve), the code
zd_k_chunk_sizes runs one lane a chunk and zd_k_batch_pack / zd_k_batch_fit
share.  tests/native/chunk_sizes.cpp (its own main) walks some two dozen
hand-made chunks, each in a heap block of exactly its size, against literal
(status, reserve, exact) triples.  Compiled with g++, no GPU needed; built once
more with AddressSanitizer and UndefinedBehaviorSanitizer linked statically and
run the same way, so a read outside [src, src + size) is a report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "chunk_sizes.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("build", ["plain build", "sanitized build"])
def test_hand_made_chunks(build, tmp_path):
    exe = tmp_path / "chunk_sizes"
    extra = SAN if build == "sanitized build" else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", *extra, "-o", str(exe), SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stderr == ""
    words = out.stdout.split()
    assert words[0] == "ok" and int(words[1]) >= 24
