"""The batch chunk walk on the CPU (zd_walk.h index_chunk, the code
zd_k_walk_chunks runs one lane per chunk; tests/native/chunk_walk.cpp drives
it with g++, no GPU needed): a chunk is any number of skippable frames around
exactly one zstd frame, walked within its own size.  Structural statuses are
checked against the oracle on each chunk alone."""
import os
import struct
import subprocess

import numpy as np
import pytest

from corpus import gen, libzstd
from oracle import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SKIP = b"\x50\x2a\x4d\x18" + (5).to_bytes(4, "little") + b"hello"
SKIP7 = b"\x57\x2a\x4d\x18" + (3).to_bytes(4, "little") + b"abc"
OUT_OF_DOMAIN = -91


@pytest.fixture(scope="module")
def walk(tmp_path_factory):
    d = tmp_path_factory.mktemp("chunk_walk")
    exe = d / "chunk_walk"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe),
                           os.path.join(ROOT, "tests", "native", "chunk_walk.cpp")])

    def run(chunks):
        path = d / "chunks.bin"
        with open(path, "wb") as f:
            for c in chunks:
                f.write(struct.pack("<I", len(c)) + c)
        out = subprocess.run([str(exe), str(path)], capture_output=True, text=True)
        assert out.returncode == 0, (out.returncode, out.stderr)
        rows = [tuple(int(x) for x in line.split()) for line in out.stdout.splitlines()]
        assert len(rows) == len(chunks)
        return rows
    return run


def test_chunk_walk(walk):
    f = libzstd.compress(gen.text(3000, seed=0xC0), 3)
    g = libzstd.compress(gen.text(300 << 10, seed=0xC1), 3)
    raw = libzstd.compress(np.random.default_rng(0xC2).integers(0, 256, 17, dtype=np.uint8).tobytes())
    good = [f, g, raw, SKIP + f, f + SKIP, SKIP + SKIP7 + f + SKIP7 + SKIP]
    empty = [b"", SKIP, SKIP + SKIP7]
    bad = [b"\x27" + f[1:], f[:len(f) // 2], f[:3], f + b"\x01\x02\x03\x04\x05", f + b"\x01", SKIP + b"\x00" * 4,
           SKIP[:-1], f + SKIP[:6], g[:len(g) - 1]]
    two = [f + f, f + SKIP + raw, SKIP + raw + f[:9]]
    rows = walk(good + empty + bad + two)
    at = 0
    for c in good:
        st, kind, nb, ncomp, fcs, left = rows[at]
        assert oracle.decompress_status(c)[0] == 0
        assert (st, kind, left) == (0, 0, 0) and nb >= 1 and fcs == len(oracle.decompress(c)), at
        at += 1
    assert rows[1][2] == 3 and rows[1][3] == 3          # 300 KiB: three compressed blocks
    assert rows[2][2:4] == (1, 0)                       # one raw block
    for c in empty:                                     # no zstd frame: a frame of no blocks, ZD_OK
        assert oracle.decompress_status(c) == (0, b"")
        assert rows[at][:4] == (0, 1, 0, 0) and rows[at][5] == 0, at
        at += 1
    for c in bad:                                       # the walk's own status, the oracle's on the chunk alone
        ost = oracle.decompress_status(c)[0]
        assert ost in (-1, -60) and rows[at][0] == ost, (at, rows[at], ost)
        at += 1
    for c in two:                                       # a second zstd frame
        assert rows[at][0] == OUT_OF_DOMAIN, at
        at += 1
