"""ZD_ROUTE_K1_SPLIT (zd_route, zd_host.cpp route_plan): K1 as a parse pass
and a build pass in plans past 64 tables per CU, in a plan of any size under
ZD_F_K1_SPLIT, never under ZD_F_K1_LANES alone; the other route bits are what
they are without it.  Host only."""
import ctypes as C

import pytest

from zstd_decompressor import _lib

SPLIT = 32
OLD_BITS = 1 | 2 | 4 | 8 | 16


def route(cus, nframes, n_tables, flags=0, single=True):
    r = C.c_uint32()
    assert _lib.lib().zd_route(cus, nframes, n_tables, nframes, nframes, int(single), flags, C.byref(r)) == 0
    return r.value


@pytest.mark.parametrize("cus", [80, 256, 304])
def test_split_route_bit(cus):
    assert _lib.F_K1_SPLIT == 512
    full = 320 * cus                                       # C4: 81,920 blocks on 256 CUs
    assert route(cus, full, full) & SPLIT
    assert route(cus, 32 * cus, 64 * cus + 1) & SPLIT
    assert not route(cus, 32 * cus, 64 * cus) & SPLIT
    assert not route(cus, full, full, _lib.F_K1_LANES) & SPLIT
    assert not route(cus, 32 * cus, 64 * cus + 1, _lib.F_K1_LANES) & SPLIT
    for nframes, n_tables in ((1, 1), (3 * cus, 3 * cus), (32 * cus, 64 * cus), (full, full)):
        assert route(cus, nframes, n_tables, _lib.F_K1_SPLIT) & SPLIT
        assert route(cus, nframes, n_tables, _lib.F_K1_SPLIT | _lib.F_NO_FUSE) & SPLIT


@pytest.mark.parametrize("cus", [80, 256, 304])
def test_other_route_bits_unchanged(cus):
    """Bits 1-16 do not depend on ZD_F_K1_SPLIT, and the shapes test_routing.py
    pins keep their values."""
    full = 320 * cus
    shapes = [(full, full, True), (32 * cus, 64 * cus + 1, True), (32 * cus, 64 * cus, True),
              (40 * cus, 40 * cus, True), (3 * cus, 6 * cus, True), (3 * cus, 6 * cus, False), (1, 1, True)]
    for nframes, n_tables, single in shapes:
        for flags in (0, _lib.F_K1_LANES, _lib.F_NO_FUSE):
            a = route(cus, nframes, n_tables, flags, single)
            b = route(cus, nframes, n_tables, flags | _lib.F_K1_SPLIT, single)
            assert a & OLD_BITS == b & OLD_BITS, (nframes, n_tables, single, flags)
    # (values from before the bit existed)
    assert route(cus, full, full) & OLD_BITS == 16                       # K1's halves on two streams
    assert route(cus, 40 * cus, 40 * cus) & OLD_BITS == 4 | 8            # wave-per-block tables, the fork
    assert route(cus, 3 * cus, 6 * cus) & OLD_BITS == 1 | 4 | 8          # fused
    assert route(cus, full, full, _lib.F_K1_LANES) & OLD_BITS == 16
