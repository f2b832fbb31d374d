"""Random access into seekable archives on the device (include/zd.h
zd_seekable_open_device, zd_seekable_read_create, zd_seek_read_*;
SeekableArchive): zd_k_seek_table, the read's layout kernels (zd_k_seek_cover,
zd_k_seek_mark, zd_k_seek_plan, the scans, zd_k_seek_chunks), the inner
device-built batch, zd_k_seek_finish and zd_k_seek_results.

Expected bytes are the source data's slices.  Expected per-entry statuses come
from the CPU oracle on that entry alone, never from the code under test; every
test first asserts that its good entries are ZD_OK there.  The counts a read
reports (frames decoded, in place, staged bytes, copy pieces) are computed
here from the entries' sizes by the rule include/zd.h states: a frame that
lies wholly inside exactly one range decodes in place, every other needed
frame is staged, rounded up to 16; a range whose destination is refused needs
no frame.

Layout of every test: the archive at an odd device address, ending at its
tensor's last byte; the destinations at odd addresses inside one tensor filled
with 0xA5, 32 guard bytes between them; after every decode every byte outside
the clamped ranges is 0xA5.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

from corpus import gen, libzstd, seekable
from oracle import oracle

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zstd-decompressor_amd")
FILL = 0xA5
GUARD = 32
PIECE = 32 << 10


@functools.lru_cache(maxsize=None)
def expect(entry: bytes):
    """(status, bytes) of one entry alone on the CPU oracle; a failing entry has no bytes."""
    st, out = oracle.decompress_status(entry)
    return st, (out if st == 0 else b"")


def on_device_odd(blob: bytes):
    """blob at an odd device address, ending at its tensor's last byte: (view, base tensor)."""
    import torch
    host = np.empty(len(blob) + 1, dtype=np.uint8)
    host[0] = 0x5C
    host[1:] = np.frombuffer(blob, dtype=np.uint8)
    base = torch.from_numpy(host).to(torch.device("cuda", 0))
    view = base[1:]
    assert view.data_ptr() % 2 == 1 and view.numel() == len(blob)
    return view, base


class Archive:
    """An archive of entries of the given content sizes (0: a skippable-only
    entry), its parts kept apart so that a test can damage one."""

    def __init__(self, data, sizes, checksums=False, frame_checksums=False, in_domain=False):
        self.data, self.sizes, self.checksums = data, list(sizes), checksums
        self.parts, self.rows = seekable.write_seekable_parts(data, self.sizes, 3, checksums, frame_checksums)
        self.d_off = [0]
        for z in self.sizes:
            self.d_off.append(self.d_off[-1] + z)
        if in_domain:
            # a few of the small level-3 frames libzstd writes lie outside the reference's domain (the oracle,
            # like the reference, ends them NoPreviousDecoder): those entries are written at level -1 instead
            for i, part in enumerate(self.parts):
                if expect(part)[0] != 0:
                    self.parts[i] = libzstd.compress(data[self.d_off[i]:self.d_off[i + 1]], -1)
                    self.rows[i] = (len(self.parts[i]), self.rows[i][1], self.rows[i][2])

    def assert_good(self):
        o = 0
        for part, z in zip(self.parts, self.sizes):
            assert expect(part) == (0, self.data[o:o + z])
            o += z

    def blob(self, parts=None, rows=None):
        return b"".join(parts or self.parts) + seekable.seek_table(rows or self.rows, self.checksums)

    def open(self, parts=None, rows=None):
        from zstd_decompressor import SeekableArchive
        view, base = on_device_odd(self.blob(parts, rows))
        a = SeekableArchive(view)
        a._base = base
        return a


def rule(d_off, ranges, null=()):
    """(needed frames, frames in place, staged bytes, copy pieces, clamped lengths, frames per range)"""
    F, total = len(d_off) - 1, d_off[-1]
    cover, partial = [0] * F, [0] * F
    clamped, touched = [], []
    pieces = 0
    starts = np.asarray(d_off, dtype=np.int64)
    for i, (o, n) in enumerate(ranges):
        l = 0 if (o >= total or i in null) else min(n, total - o)
        real = 0 if o >= total else min(n, total - o)
        clamped.append(real)
        fs = []
        if l:
            pieces += -(-l // PIECE)
            f = int(np.searchsorted(starts, o, side="right")) - 1
            while f < F and d_off[f] < o + l:
                lo, hi = max(d_off[f], o), min(d_off[f + 1], o + l)
                if hi > lo:
                    fs.append(f)
                    cover[f] += 1
                    partial[f] += not (lo == d_off[f] and hi == d_off[f + 1])
                f += 1
        touched.append(fs)
    needed = sum(1 for c in cover if c)
    in_place = sum(1 for c, p in zip(cover, partial) if c == 1 and p == 0)
    staged = sum((d_off[f + 1] - d_off[f] + 15) & ~15 for f in range(F)
                 if cover[f] and not (cover[f] == 1 and partial[f] == 0))
    return needed, in_place, staged, pieces, clamped, touched


class Dsts:
    """One destination a range, sized to its clamped length, at odd offsets of a 0xA5 tensor."""

    def __init__(self, clamped, null=(), seed=1):
        import torch
        self.torch = torch
        rng = np.random.default_rng(seed)
        order = [int(x) for x in rng.permutation(len(clamped))]
        self.offs, at = [0] * len(clamped), GUARD + 1
        for j in order:
            at |= 1
            self.offs[j] = at
            at += clamped[j] + GUARD
        self.clamped, self.null = clamped, set(null)
        self.t = torch.full((at + GUARD,), FILL, dtype=torch.uint8, device=torch.device("cuda", 0))
        self.ptrs = [0 if i in self.null else self.t.data_ptr() + o for i, o in enumerate(self.offs)]

    def refill(self):
        self.t.fill_(FILL)
        self.torch.cuda.synchronize()

    def check(self, data, ranges, statuses, lengths, want_status):
        """want_status[i]: the expected status; a failed range's bytes are unspecified."""
        h = self.t.cpu().numpy()
        exp = np.full(h.size, FILL, dtype=np.uint8)
        known = np.ones(h.size, dtype=bool)
        src = np.frombuffer(data, dtype=np.uint8)
        assert list(statuses) == list(want_status)
        for i, (o, n) in enumerate(ranges):
            l, at = self.clamped[i], self.offs[i]
            if i in self.null:
                assert lengths[i] == 0
                continue
            if want_status[i] == 0:
                assert lengths[i] == l, i
                exp[at:at + l] = src[o:o + l]
            else:
                assert lengths[i] == 0, i
                known[at:at + l] = False
        bad = np.nonzero((h != exp) & known)[0]
        assert bad.size == 0, "first differing byte of the destination tensor: %d" % int(bad[0])


def run_read(a, ranges, dsts, flags=0):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    r = a.reader(t([o for o, _ in ranges]), t([n for _, n in ranges]), t(dsts.ptrs), flags=flags)
    r.decode_async()
    st, ln = r.results()
    return r, st, ln


# ---------------------------------------------------------------------------
# Archive A: entries of 1, 40,000, 0 (skippable only), 131,077 (two blocks), 17
# and 300,000 content bytes, Content_Checksums on the odd entries
# ---------------------------------------------------------------------------
A_SIZES = [1, 40000, 0, 131077, 17, 300000]
A_TOTAL = sum(A_SIZES)


@functools.lru_cache(maxsize=None)
def archive_a(checksums: bool):
    a = Archive(gen.text(A_TOTAL + 64, seed=4242)[:A_TOTAL], A_SIZES, checksums, frame_checksums={1, 3, 5})
    a.assert_good()
    return a


def ranges_a(d_off):
    """(ranges, the index of the one with a NULL destination); d_off: the archive's own sums"""
    total = d_off[-1]
    b3, b4, b5 = d_off[3], d_off[4], d_off[5]
    return [
        (0, total),                   # 0 the whole content
        (100, 5000),                  # 1 inside one frame
        (d_off[2] - 1, 2),            # 2 one byte either side of a boundary (and of the entry of no bytes)
        (b4, 10),                     # 3 starting exactly at a boundary
        (b4 - 78, 78),                # 4 ending exactly at one
        (d_off[2] - 11, 100),         # 5 across the entry of no bytes
        (500, 0),                     # 6 len 0
        (total, 10),                  # 7 starting at the end
        (total - 50, 1000),           # 8 running past the end
        (b5 + 30000, 3000),           # 9, 10 identical
        (b5 + 30000, 3000),
        (b5 + 100000, 5000),          # 11, 12 overlapping in one frame
        (b5 + 102000, 5000),
        (b4 + 3, 100),                # 13 a NULL destination
        (b3, A_SIZES[3]),             # 14 exactly one entry
        (total + 5, 0),               # 15 past the end, len 0
    ], 13


@pytest.mark.parametrize("checksums", [False, True], ids=["8-byte entries", "12-byte entries"])
def test_archive_a_all_ranges(checksums):
    A = archive_a(checksums)
    a = A.open()
    try:
        assert (a.nframes, a.content_size, a.has_checksums) == (6, A_TOTAL, checksums)
        assert a.info.compressed_bytes == sum(len(p) for p in A.parts)
        assert a.info.table_bytes == 17 + 6 * (12 if checksums else 8) and a.info.max_frame_content == 300000
        c_off, d_off, cks = a.table()
        from zstd_decompressor.batch import _read_u64
        assert _read_u64(d_off, 7) == A.d_off
        assert _read_u64(c_off, 7) == [sum(len(p) for p in A.parts[:k]) for k in range(7)]
        assert bool(cks) == checksums
        ranges, null = ranges_a(A.d_off)
        needed, in_place, staged, pieces, clamped, _ = rule(A.d_off, ranges, {null})
        assert needed == 5 and clamped[8] == 50 and clamped[7] == 0
        dsts = Dsts(clamped, {null})
        r, st, ln = run_read(a, ranges, dsts)
        want = [0] * len(ranges)
        want[null] = -93
        dsts.check(A.data, ranges, st, ln, want)
        assert r.info.nranges == len(ranges)
        assert r.info.frames_decoded == needed and r.info.batch.nchunks == needed
        assert (r.info.frames_in_place, r.info.staged_bytes, r.info.copy_pieces) == (in_place, staged, pieces)
        # again on the same read: the same bytes
        dsts.refill()
        r.decode_async()
        st, ln = r.results()
        dsts.check(A.data, ranges, st, ln, want)
        r.close()
    finally:
        a.close()


def test_in_place_frames_and_a_closed_archive():
    """Disjoint ranges: whole frames decode in place, only the edges are
    staged; the read goes on working after its archive is closed."""
    A = archive_a(False)
    a = A.open()
    d = A.d_off
    ranges = [(d[1] + 5, d[4] - d[1] - 5 + 3), (d[5], 1000), (0, 1)]
    needed, in_place, staged, pieces, clamped, _ = rule(d, ranges)
    assert (needed, in_place) == (5, 2) and staged == 40000 + 32 + 300000
    dsts = Dsts(clamped, seed=3)
    r, st, ln = run_read(a, ranges, dsts)
    a.close()
    dsts.check(A.data, ranges, st, ln, [0, 0, 0])
    assert (r.info.frames_decoded, r.info.frames_in_place, r.info.staged_bytes, r.info.copy_pieces) == \
        (needed, in_place, staged, pieces)
    dsts.refill()
    r.decode_async()
    st, ln = r.results()
    dsts.check(A.data, ranges, st, ln, [0, 0, 0])
    r.close()


# ---------------------------------------------------------------------------
# Archive B: 3,000 entries of 50-650 content bytes
# ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def archive_b():
    rng = np.random.default_rng(77)
    sizes = [int(x) for x in rng.integers(50, 651, size=3000)]
    total = sum(sizes)
    b = Archive(gen.text(total + 64, seed=99)[:total], sizes, checksums=True, in_domain=True)
    b.assert_good()
    return b


def test_archive_b_random_ranges():
    B = archive_b()
    a = B.open()
    try:
        rng = np.random.default_rng(5)
        total = B.d_off[-1]
        ranges = [(int(rng.integers(0, total)), int(rng.integers(1, 2001))) for _ in range(2000)]
        needed, in_place, staged, pieces, clamped, _ = rule(B.d_off, ranges)
        dsts = Dsts(clamped, seed=9)
        r, st, ln = run_read(a, ranges, dsts)
        dsts.check(B.data, ranges, st, ln, [0] * len(ranges))
        assert (r.info.frames_decoded, r.info.frames_in_place, r.info.staged_bytes, r.info.copy_pieces) == \
            (needed, in_place, staged, pieces)
        r.close()
    finally:
        a.close()


def test_archive_b_one_range_over_everything():
    B = archive_b()
    a = B.open()
    try:
        ranges = [(0, B.d_off[-1] + 1000)]
        needed, in_place, staged, pieces, clamped, _ = rule(B.d_off, ranges)
        assert (needed, in_place, staged) == (3000, 3000, 0)
        dsts = Dsts(clamped)
        r, st, ln = run_read(a, ranges, dsts)
        dsts.check(B.data, ranges, st, ln, [0])
        assert (r.info.frames_decoded, r.info.frames_in_place, r.info.staged_bytes, r.info.copy_pieces) == \
            (needed, in_place, staged, pieces)
        r.close()
    finally:
        a.close()


# ---------------------------------------------------------------------------
# Failures
# ---------------------------------------------------------------------------
def failing_read(A, parts, rows, d_off, data, bad_entry, bad_status, flags=0):
    """Every range of ranges_a over the archive made of parts / rows: the ranges
    that touch bad_entry end bad_status with length 0, the others are intact."""
    a = A.open(parts, rows)
    try:
        ranges, null = ranges_a(d_off)
        _, _, _, _, clamped, touched = rule(d_off, ranges, {null})
        dsts = Dsts(clamped, {null}, seed=11)
        r, st, ln = run_read(a, ranges, dsts, flags)
        want = [bad_status if bad_entry in fs else 0 for fs in touched]
        want[null] = -93
        assert sum(1 for w in want if w == bad_status) >= 3 and sum(1 for w in want if w == 0) >= 6
        dsts.check(data, ranges, st, ln, want)
        r.close()
    finally:
        a.close()


def test_one_byte_flipped_in_an_entry():
    A = archive_a(True)
    entry = A.parts[3]
    for pos in range(len(entry) // 2, len(entry) // 2 + 64):
        damaged = entry[:pos] + bytes([entry[pos] ^ 0x40]) + entry[pos + 1:]
        st, _ = expect(damaged)
        if st != 0:
            break
    assert st != 0
    parts = list(A.parts)
    parts[3] = damaged
    failing_read(A, parts, None, A.d_off, A.data, 3, st)


@pytest.mark.parametrize("delta,status", [(1, -101), (-1, -92)], ids=["one too large", "one too small"])
def test_table_size_off_by_one(delta, status):
    """Decompressed_Size of entry 1 wrong by one: the content the table
    describes has one byte more (unspecified, never delivered) or one byte less
    (the entry's last) at that entry's end, and only the ranges over that entry fail."""
    A = archive_a(False)
    rows = list(A.rows)
    rows[1] = (rows[1][0], rows[1][1] + delta, rows[1][2])
    d_off = [0]
    for row in rows:
        d_off.append(d_off[-1] + row[1])
    end1 = A.d_off[2]
    data = A.data[:end1] + b"?" + A.data[end1:] if delta > 0 else A.data[:end1 - 1] + A.data[end1:]
    assert len(data) == d_off[-1]
    failing_read(A, None, rows, d_off, data, 1, status)


def test_damaged_content_checksum_with_verify():
    from zstd_decompressor import _lib
    A = archive_a(True)
    entry = A.parts[5]
    damaged = entry[:-1] + bytes([entry[-1] ^ 1])
    assert expect(damaged) == (0, A.data[A.d_off[5]:])        # (the reference hashes and never enforces)
    parts = list(A.parts)
    parts[5] = damaged
    failing_read(A, parts, None, A.d_off, A.data, 5, _lib.CHECKSUM_WRONG, flags=_lib.F_VERIFY_CHECKSUM)
    # without the flag every range is intact
    a = A.open(parts)
    try:
        ranges, null = ranges_a(A.d_off)
        clamped = rule(A.d_off, ranges, {null})[4]
        dsts = Dsts(clamped, {null})
        r, st, ln = run_read(a, ranges, dsts)
        want = [0] * len(ranges)
        want[null] = -93
        dsts.check(A.data, ranges, st, ln, want)
        r.close()
    finally:
        a.close()


def test_open_errors_on_the_device_path():
    from zstd_decompressor import SeekableArchive, ZdError, _lib
    A = archive_a(False)
    front = b"".join(A.parts)
    good = seekable.seek_table(A.rows, False)
    n = len(A.rows)

    def edit(table, at, value):
        return table[:at] + value + table[at + len(value):]

    cases = [
        (front[:3] + good[-14:], _lib.NOT_ENOUGH_BYTES),                       # a table larger than the archive
        (front + edit(good, len(good) - 4, b"\xb0"), _lib.UNRECOGNIZED_MAGIC),  # the footer's magic
        (front + edit(good, 0, b"\x50"), _lib.UNRECOGNIZED_MAGIC),              # the skippable header's
        (front + edit(good, len(good) - 5, b"\x10"), _lib.FRAME_RESERVED_SET),
        (front + edit(good, len(good) - 9, ((1 << 27) + 1).to_bytes(4, "little")), _lib.OUT_OF_DOMAIN),
        (front + edit(good, 4, (8 * n + 8).to_bytes(4, "little")), _lib.SEEK_TABLE),   # Frame_Size
        (front + b"\x00" + good, _lib.SEEK_TABLE),                              # one byte more than the sizes' sum
        (front[:-1] + good, _lib.SEEK_TABLE),                                   # one byte less
    ]
    for blob, status in cases:
        view, base = on_device_odd(blob)
        with pytest.raises(ZdError) as e:
            SeekableArchive(view)
        assert e.value.code == status, (status, e.value.code)
    view, base = on_device_odd(good[-16:])
    with pytest.raises(ZdError) as e:
        SeekableArchive(view)
    assert e.value.code == _lib.NOT_ENOUGH_BYTES
    # a table of no entries: every range is empty
    view, base = on_device_odd(seekable.seek_table([], True))
    a = SeekableArchive(view)
    try:
        assert (a.nframes, a.content_size) == (0, 0)
        r = a.reader([0, 5], [10, 0])
        r.decode_async()
        assert r.results() == ([0, 0], [0, 0]) and r.info.frames_decoded == 0
        r.close()
    finally:
        a.close()


# ---------------------------------------------------------------------------
# One K4J case: an entry of 2 MiB + 3 content bytes (17 blocks)
# ---------------------------------------------------------------------------
def test_block_parallel_entry():
    from zstd_decompressor import _lib
    size = (2 << 20) + 3
    K = Archive(gen.text(size + 64, seed=31)[:size], [size])
    K.assert_good()
    a = K.open()
    try:
        ranges = [(1000000, 5000), (0, size)]
        needed, in_place, staged, pieces, clamped, _ = rule(K.d_off, ranges)
        assert (needed, in_place, staged) == (1, 0, (size + 15) & ~15)
        dsts = Dsts(clamped)
        r, st, ln = run_read(a, ranges, dsts)
        dsts.check(K.data, ranges, st, ln, [0, 0])
        assert r.info.batch.executors & _lib.EXEC_K4J and r.info.batch.k4j_chunks == 1
        assert (r.info.frames_decoded, r.info.staged_bytes, r.info.copy_pieces) == (1, staged, pieces)
        r.close()
    finally:
        a.close()


# ---------------------------------------------------------------------------
# Python and the command line
# ---------------------------------------------------------------------------
def test_python_read_and_cli_range(tmp_path):
    from zstd_decompressor import SeekableArchive, ZdError
    A = archive_a(True)
    blob = A.blob()
    a = SeekableArchive(blob)                   # bytes are uploaded
    try:
        for off, n in ((0, 1), (39999, 3), (171000, 200000), (A_TOTAL - 7, 100), (A_TOTAL, 4), (12, 0)):
            t = a.read(off, n)
            assert t.is_cuda and bytes(t.cpu().numpy().tobytes()) == A.data[off:off + n]
        r = a.reader([5, 40000], [10, 20])      # lists; destinations allocated
        r.decode_async()
        assert r.results() == ([0, 0], [10, 20])
        assert [bytes(t.cpu().numpy().tobytes()) for t in r.outputs] == [A.data[5:15], A.data[40000:40020]]
        r.close()
    finally:
        a.close()
    path, out = tmp_path / "a.zst", tmp_path / "out.bin"
    path.write_bytes(blob)
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)

    def cli(*args):
        return subprocess.run([sys.executable, "-m", "zstd_decompressor", *args], cwd=ROOT, env=env,
                              capture_output=True, timeout=120)
    res = cli(str(path), "--range", "39990:131200", "-o", str(out))
    assert res.returncode == 0, res.stderr
    assert out.read_bytes() == A.data[39990:39990 + 131200]
    plain = tmp_path / "plain.zst"
    plain.write_bytes(b"".join(A.parts))       # the same frames without a seek table
    res = cli(str(plain), "--range", "0:10", "-o", str(out))
    assert res.returncode != 0 and b"not a seekable archive" in res.stderr
