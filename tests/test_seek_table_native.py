"""Host test of the seek-table rules (zd_seek.h: footer and header checks, the
unaligned entry read, the sums, the clamp, the range-to-frames search, the
part of a frame a range wants), the code zd_seekable_open_device and the
zd_k_seek_* kernels run.  tests/native/seek_table.cpp (its own main) opens
hand-made tables, each in a heap block of exactly its size, against literal
verdicts and (f0, f1, clamped length) triples.  Compiled with g++, no GPU
needed; built once more with AddressSanitizer and UndefinedBehaviorSanitizer
linked statically and run the same way, so a read outside the table is a
report."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "seek_table.cpp")
SAN = ["-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer",
       "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("build", ["plain build", "sanitized build"])
def test_hand_made_tables(build, tmp_path):
    exe = tmp_path / "seek_table"
    extra = SAN if build == "sanitized build" else []
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", *extra, "-o", str(exe), SRC])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:halt_on_error=1", UBSAN_OPTIONS="halt_on_error=1")
    out = subprocess.run([str(exe)], capture_output=True, text=True, env=env)
    assert out.returncode == 0, (out.returncode, out.stdout, out.stderr)
    assert out.stderr == ""
    words = out.stdout.split()
    assert words[0] == "ok" and int(words[1]) >= 80
