"""Verified seekable reads (include/zd.h ZD_SEEK_VERIFY_TABLE,
zd_seekable_read_create_ex, zd_seek_read_device_verdicts; SeekableArchive.
reader(verify_table=True), verify_all): zd_k_seek_verify between the inner
batch's decode and zd_k_seek_finish, and the result pass that counts an entry
whose bytes do not hash to the table's Checksum as ZD_E_CHECKSUM_WRONG.

Expected bytes are the source data's slices.  Expected statuses of damaged
entries come from the CPU oracle on that entry alone.  Expected checksums are
the writer's rows (corpus/seekable.py: the low 32 bits libzstd itself stored
as the frame's Content_Checksum).  None of these come from the code under test.

Layout of every test, as tests/test_seekable_gpu.py (whose helpers these tests
use): the archive at an odd device address, the destinations at odd addresses
inside one tensor filled with 0xA5, 32 guard bytes between them; after every
decode every byte outside the clamped ranges is 0xA5.
"""
import ctypes as C
import functools
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

from corpus import gen, libzstd
from test_seekable_gpu import Archive, Dsts, archive_b, expect, rule

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "zstd-decompressor_amd")
CHECKSUM_WRONG, SEEK_TABLE, INVALID_ARG = -100, -101, -93


def run_read(a, ranges, dsts, flags=0, verify_table=True):
    import torch
    dev = torch.device("cuda", 0)
    t = lambda v: torch.tensor(v, dtype=torch.int64, device=dev)
    r = a.reader(t([o for o, _ in ranges]), t([n for _, n in ranges]), t(dsts.ptrs), flags=flags,
                 verify_table=verify_table)
    r.decode_async()
    st, ln = r.results()
    return r, st, ln


def needed_entries(touched):
    return sorted({f for fs in touched for f in fs})


def check_verdicts(r, rows, touched, wrong=(), uncompared=()):
    """The verdicts of read r over an archive whose true checksums are rows[f][2]:
    the entries are the needed ones in table order; an entry of `wrong` has
    verdict 0 and one of `uncompared` -1 with hash32 0; every compared entry's
    hash32 is the writer's checksum."""
    entries, ok, h32 = r.verdicts()
    need = needed_entries(touched)
    assert entries == need
    assert ok == [-1 if f in uncompared else 0 if f in wrong else 1 for f in need]
    assert h32 == [0 if f in uncompared else rows[f][2] for f in need]
    assert r.info.read_flags == 1 and r.info.verify_entries == r.info.frames_decoded == len(need)
    assert r.device_verdicts()[3] == len(need)


# ---------------------------------------------------------------------------
# Archive V: the sizes at which zd_k_seek_verify takes another path -- below 32
# bytes, one stripe, one line (128), one trip of 4 lines (512), two trips (1024:
# the loads issued ahead), leftover stripes plus a tail (1151), two blocks
# (131077), an entry of no bytes -- and 20 decoded entries: a second wave that
# is partly empty.  Content_Checksums on entries 4, 9, 18 and 20.
# ---------------------------------------------------------------------------
V_SIZES = [1, 31, 32, 33, 127, 128, 129, 0, 511, 512, 513, 1023, 1024, 1025, 1151, 1536, 2047, 4096, 40000, 131077,
           300000]
V_TOTAL = sum(V_SIZES)
V_OWN = {4, 9, 18, 20}


@functools.lru_cache(maxsize=None)
def archive_v():
    v = Archive(gen.text(V_TOTAL + 64, seed=515)[:V_TOTAL], V_SIZES, checksums=True, frame_checksums=V_OWN,
                in_domain=True)
    v.assert_good()
    for f in V_OWN:                                   # (Frame_Header_Descriptor bit 2: Content_Checksum_flag)
        assert v.parts[f][4] & 4 and struct.unpack("<I", v.parts[f][-4:])[0] == v.rows[f][2]
    return v


def ranges_whole(d):
    return [(0, d[-1])]                               # every entry in place


def ranges_mixed(d):
    """Entries 0-2, 4-6, 8, 10, 11, 13, 14 in place; 3, 9, 12, 15, 18, 19, 20
    staged; 16 and 17 not needed; 7 has no bytes."""
    return [
        (d[0], d[3] - d[0]),                          # 0 three whole entries
        (d[3] + 1, d[9] - d[3] + 4),                  # 1 partial edges (3 and 9), the entry of no bytes inside
        (d[10], d[12] - d[10]),                       # 2 exactly two entries
        (d[12] + 100, 200),                           # 3 inside one entry
        (d[12] + 1000, d[15] - d[12] - 1000 + 7),     # 4 shares entry 12 with range 3; 13, 14 whole; 7 bytes of 15
        (d[18] + 1000, 5000),                         # 5 inside entry 18
        (d[18] + 3000, 37000 + 70000),                # 6 shares 18 with range 5, runs into 19
        (d[19] + 131000, 77 + 1000),                  # 7 shares 19 with range 6, runs into 20
        (d[20] + 100000, 10 ** 6),                    # 8 shares 20, clamped at the end
        (d[16], 0),                                   # 9 of no bytes
    ]


def flipped(rows, which):
    rows = list(rows)
    for f in which:
        rows[f] = (rows[f][0], rows[f][1], rows[f][2] ^ (1 << (f % 32)))
    return rows


@pytest.mark.parametrize("flags", [0, 1024], ids=["flags 0", "F_VERIFY_CHECKSUM"])
@pytest.mark.parametrize("which", [ranges_whole, ranges_mixed], ids=["one range", "mixed ranges"])
def test_all_good(which, flags):
    V = archive_v()
    a = V.open()
    try:
        ranges = which(V.d_off)
        needed, in_place, staged, pieces, clamped, touched = rule(V.d_off, ranges)
        if which is ranges_whole:
            assert (needed, in_place, staged) == (20, 20, 0)
        else:
            assert (needed, in_place) == (18, 11) and staged > 0
        dsts = Dsts(clamped, seed=21)
        r, st, ln = run_read(a, ranges, dsts, flags)
        dsts.check(V.data, ranges, st, ln, [0] * len(ranges))
        check_verdicts(r, V.rows, touched)
        assert (r.info.frames_decoded, r.info.frames_in_place, r.info.staged_bytes, r.info.copy_pieces) == \
            (needed, in_place, staged, pieces)
        # again on the same read: the same
        dsts.refill()
        r.decode_async()
        st, ln = r.results()
        dsts.check(V.data, ranges, st, ln, [0] * len(ranges))
        check_verdicts(r, V.rows, touched)
        r.close()
        # a read without the option has no verdicts
        r, st, ln = run_read(a, ranges, dsts, flags, verify_table=False)
        assert r.verdicts() == ([], [], []) and r.device_verdicts() == (0, 0, 0, 0)
        assert (r.info.read_flags, r.info.verify_entries) == (0, 0) and r.info.frames_decoded == needed
        r.close()
    finally:
        a.close()


@pytest.mark.parametrize("wrong,flags", [((3, 13, 19), 0), ((3, 13, 19), 1024), ((18,), 1024), ((18,), 0)],
                         ids=["3-13-19", "3-13-19 F_VERIFY_CHECKSUM", "18 hashed by the batch", "18"])
def test_wrong_table_checksum(wrong, flags):
    """One bit of an entry's Checksum flipped in the table: entry 13 decodes in
    place, 3, 18 and 19 are staged; entry 18 carries its own, correct
    Content_Checksum, so under F_VERIFY_CHECKSUM its digest comes from the
    inner batch's pass."""
    V = archive_v()
    rows = flipped(V.rows, wrong)
    a = V.open(rows=rows)
    try:
        ranges = ranges_mixed(V.d_off)
        _, _, _, _, clamped, touched = rule(V.d_off, ranges)
        want = [CHECKSUM_WRONG if set(fs) & set(wrong) else 0 for fs in touched]
        assert 2 <= sum(1 for w in want if w) < len(want) - 3
        dsts = Dsts(clamped, seed=22)
        r, st, ln = run_read(a, ranges, dsts, flags)
        dsts.check(V.data, ranges, st, ln, want)
        check_verdicts(r, V.rows, touched, wrong=wrong)           # (hash32: the unflipped value)
        r.close()
        # the same archive without the option: every range intact
        dsts.refill()
        r, st, ln = run_read(a, ranges, dsts, flags, verify_table=False)
        dsts.check(V.data, ranges, st, ln, [0] * len(ranges))
        r.close()
        if 13 in wrong:                                           # all in place
            ranges = ranges_whole(V.d_off)
            _, _, _, _, clamped, touched = rule(V.d_off, ranges)
            dsts = Dsts(clamped, seed=23)
            r, st, ln = run_read(a, ranges, dsts, flags)
            dsts.check(V.data, ranges, st, ln, [CHECKSUM_WRONG])
            check_verdicts(r, V.rows, touched, wrong=wrong)
            r.close()
    finally:
        a.close()


def test_replaced_entry():
    """Entry 19's bytes swapped for a frame of other text of the same length:
    it decodes, to the table's Decompressed_Size, and only its checksum tells."""
    V = archive_v()
    other = gen.text(V_SIZES[19] + 64, seed=616)[:V_SIZES[19]]
    assert other != V.data[V.d_off[19]:V.d_off[20]]
    swapped = libzstd.compress(other, 3)
    assert expect(swapped) == (0, other)
    other_sum = struct.unpack("<I", libzstd.compress(other, 3, checksum=True)[-4:])[0]
    assert other_sum != V.rows[19][2]
    parts, rows = list(V.parts), list(V.rows)
    parts[19] = swapped
    rows[19] = (len(swapped), rows[19][1], rows[19][2])
    a = V.open(parts, rows)
    try:
        ranges = ranges_mixed(V.d_off)
        _, _, _, _, clamped, touched = rule(V.d_off, ranges)
        want = [CHECKSUM_WRONG if 19 in fs else 0 for fs in touched]
        assert sum(1 for w in want if w) == 2
        dsts = Dsts(clamped, seed=24)
        r, st, ln = run_read(a, ranges, dsts)
        dsts.check(V.data, ranges, st, ln, want)
        seen = list(V.rows)
        seen[19] = (0, 0, other_sum)
        check_verdicts(r, seen, touched, wrong=(19,))
        r.close()
        # without the option the other text comes back as ZD_OK
        data = V.data[:V.d_off[19]] + other + V.data[V.d_off[20]:]
        dsts.refill()
        r, st, ln = run_read(a, ranges, dsts, verify_table=False)
        dsts.check(data, ranges, st, ln, [0] * len(ranges))
        r.close()
    finally:
        a.close()


def test_precedence_of_a_failed_entry():
    """Entry 3 damaged so that it does not decode, entry 5 with a wrong
    checksum: a range over both gets entry 3's status (the lowest-numbered
    frame that did not end ZD_OK), a range over entry 5 alone CHECKSUM_WRONG."""
    V = archive_v()
    entry = V.parts[3]
    for pos in range(4, len(entry)):
        damaged = entry[:pos] + bytes([entry[pos] ^ 0x40]) + entry[pos + 1:]
        bad, _ = expect(damaged)
        if bad != 0:
            break
    assert bad != 0 and bad != CHECKSUM_WRONG
    parts = list(V.parts)
    parts[3] = damaged
    a = V.open(parts, flipped(V.rows, (5,)))
    try:
        d = V.d_off
        ranges = [(d[3], d[6] - d[3]), (d[5], V_SIZES[5]), (d[4], V_SIZES[4]), (d[5] + 3, d[9] - d[5]), (d[0], 60)]
        _, _, _, _, clamped, touched = rule(d, ranges)
        assert touched[0] == [3, 4, 5] and touched[1] == [5] and touched[4] == [0, 1, 2]
        dsts = Dsts(clamped, seed=25)
        r, st, ln = run_read(a, ranges, dsts)
        dsts.check(V.data, ranges, st, ln, [bad, CHECKSUM_WRONG, 0, CHECKSUM_WRONG, 0])
        check_verdicts(r, V.rows, touched, wrong=(5,), uncompared=(3,))
        r.close()
    finally:
        a.close()


def test_precedence_of_a_wrong_size():
    """Decompressed_Size of entry 12 one too large and its checksum wrong: the
    entry is not compared (verdict -1), its ranges get SEEK_TABLE."""
    V = archive_v()
    rows = flipped(V.rows, (12,))
    rows[12] = (rows[12][0], rows[12][1] + 1, rows[12][2])
    d_off = [0]
    for row in rows:
        d_off.append(d_off[-1] + row[1])
    end = V.d_off[13]
    data = V.data[:end] + b"?" + V.data[end:]
    assert len(data) == d_off[-1]
    a = V.open(rows=rows)
    try:
        ranges = [(d_off[11], d_off[14] - d_off[11]), (d_off[12] + 5, 10), (d_off[13], 1025), (0, 300)]
        _, _, _, _, clamped, touched = rule(d_off, ranges)
        assert touched[0] == [11, 12, 13] and touched[1] == [12] and touched[2] == [13]
        dsts = Dsts(clamped, seed=26)
        r, st, ln = run_read(a, ranges, dsts)
        dsts.check(data, ranges, st, ln, [SEEK_TABLE, SEEK_TABLE, 0, 0])
        check_verdicts(r, V.rows, touched, uncompared=(12,))
        r.close()
    finally:
        a.close()


def test_no_checksums_to_verify():
    from zstd_decompressor import ZdError, _lib
    N = Archive(gen.text(1000, seed=8)[:700], [300, 400], checksums=False)
    a = N.open()
    try:
        assert not a.has_checksums
        dsts = Dsts([700])
        import torch
        t = lambda v: torch.tensor(v, dtype=torch.int64, device=torch.device("cuda", 0))
        off, ln, dst = t([0]), t([700]), t(dsts.ptrs)
        h = C.c_void_p()
        args = [C.c_void_p(x.data_ptr()) for x in (off, ln, dst)]
        st = _lib.lib().zd_seekable_read_create_ex(a._h, *args, 1, 0, _lib.SEEK_VERIFY_TABLE, None, C.byref(h))
        assert st == INVALID_ARG and not h.value
        with pytest.raises(ZdError) as e:
            a.reader([0], [700], verify_table=True)
        assert e.value.code == INVALID_ARG
        with pytest.raises(ZdError) as e:
            a.read(0, 10, verify_table=True)
        assert e.value.code == INVALID_ARG
        with pytest.raises(ValueError):
            a.verify_all()
        r, st, ln = run_read(a, [(0, 700)], dsts, verify_table=False)     # and it reads as ever
        dsts.check(N.data, [(0, 700)], st, ln, [0])
        r.close()
    finally:
        a.close()


def test_block_parallel_entry():
    """One entry of 2 MiB + 3 bytes (17 blocks, K4J): in place and staged."""
    from zstd_decompressor import _lib
    size = (2 << 20) + 3
    K = Archive(gen.text(size + 64, seed=31)[:size], [size], checksums=True)
    K.assert_good()
    for rows, want in ((K.rows, 0), (flipped(K.rows, (0,)), CHECKSUM_WRONG)):
        a = K.open(rows=rows)
        try:
            for ranges in ([(0, size)], [(1000000, 5000), (0, size)]):
                _, in_place, _, _, clamped, touched = rule(K.d_off, ranges)
                assert in_place == (len(ranges) == 1)
                dsts = Dsts(clamped, seed=27)
                r, st, ln = run_read(a, ranges, dsts)
                dsts.check(K.data, ranges, st, ln, [want] * len(ranges))
                assert r.info.batch.executors & _lib.EXEC_K4J and r.info.batch.k4j_chunks == 1
                check_verdicts(r, K.rows, touched, wrong=(0,) if want else ())
                r.close()
        finally:
            a.close()


def test_many_entries():
    """Archive B of tests/test_seekable_gpu.py: 3,000 entries of 50-650 bytes,
    2,000 random ranges; then five rows' checksums flipped."""
    B = archive_b()
    rng = np.random.default_rng(5)
    total = B.d_off[-1]
    ranges = [(int(rng.integers(0, total)), int(rng.integers(1, 2001))) for _ in range(2000)]
    needed, in_place, staged, pieces, clamped, touched = rule(B.d_off, ranges)
    need = needed_entries(touched)
    wrong = tuple(need[i] for i in (0, 17, len(need) // 2, len(need) - 40, len(need) - 1))
    for rows, bad in ((B.rows, ()), (flipped(B.rows, wrong), wrong)):
        a = B.open(rows=rows)
        try:
            dsts = Dsts(clamped, seed=9)
            r, st, ln = run_read(a, ranges, dsts)
            want = [CHECKSUM_WRONG if set(fs) & set(bad) else 0 for fs in touched]
            assert sum(1 for w in want if w) >= len(bad)
            dsts.check(B.data, ranges, st, ln, want)
            check_verdicts(r, B.rows, touched, wrong=bad)
            assert (r.info.frames_decoded, r.info.frames_in_place, r.info.staged_bytes, r.info.copy_pieces) == \
                (needed, in_place, staged, pieces)
            r.close()
        finally:
            a.close()


def test_verify_all_and_the_command_line(tmp_path, capsys):
    from zstd_decompressor import SeekableArchive, ZdError
    V = archive_v()
    good, bad = V.blob(), V.blob(rows=flipped(V.rows, (13,)))
    for blob, want in ((good, ([], [])), (bad, ([13], [CHECKSUM_WRONG]))):
        a = SeekableArchive(blob)
        try:
            assert a.verify_all() == want
            assert a.verify_all(slab_bytes=100000) == want          # five slabs; entries 19 and 20 straddle them
        finally:
            a.close()
    a = SeekableArchive(bad)
    try:
        o = V.d_off[13]
        with pytest.raises(ZdError) as e:
            a.read(o - 10, 100, verify_table=True)
        assert e.value.code == CHECKSUM_WRONG and e.value.entries == [13]
        t = a.read(o + 1025, 100, verify_table=True)
        assert bytes(t.cpu().numpy().tobytes()) == V.data[o + 1025:o + 1125]
    finally:
        a.close()
    # the command line: one run as a process of its own (the exit status), the others through main() in this one
    env = dict(os.environ, PYTHONPATH=PKG + os.pathsep + ROOT)
    out = tmp_path / "out.bin"
    gp, bp = tmp_path / "good.zst", tmp_path / "bad.zst"
    gp.write_bytes(good)
    bp.write_bytes(bad)
    errors = lambda text: [l for l in text.splitlines() if l.startswith("Error")]
    res = subprocess.run([sys.executable, "-m", "zstd_decompressor", str(bp), "--verify-table"], cwd=ROOT, env=env,
                         capture_output=True, timeout=120)
    assert res.returncode == 1 and res.stdout == b"", res.stderr
    assert errors(res.stderr.decode()) == ["Error: entry 13: ChecksumWrong"], res.stderr
    from zstd_decompressor.__main__ import main
    span = "%d:%d" % (V.d_off[12], 3000)
    capsys.readouterr()
    assert main([str(gp), "--verify-table"]) == 0
    got = capsys.readouterr()
    assert got.out == "" and errors(got.err) == []
    assert main([str(bp), "--range", span, "--verify-table", "-o", str(out)]) == 1
    assert errors(capsys.readouterr().err) == ["Error: entry 13: ChecksumWrong"] and not out.exists()
    assert main([str(bp), "--range", span, "-o", str(out)]) == 0                # without the option: as ever
    assert out.read_bytes() == V.data[V.d_off[12]:V.d_off[12] + 3000]
    out.unlink()
    assert main([str(gp), "--range", span, "--verify-table", "-o", str(out)]) == 0
    assert out.read_bytes() == V.data[V.d_off[12]:V.d_off[12] + 3000]
