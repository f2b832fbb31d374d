"""ZD_F_RFC on the host side, driven by tests/native/rfc_mode.cpp (compiled with
g++, no GPU): the long-form Number_of_Sequences in parse_compressed (D1), an
empty Huffman stream (D8), plan_frame over a frame with a 0-sequence block
between two blocks (D2), and huf_close (zd_huf.h, the Huffman weight rule K1's
three builders share) for every total in 1..4096 against a plain restatement
of RFC 8878 4.2.1.1 and of the reference's rule (D3)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "rfc_mode.cpp")
REF_PANIC, CORRUPTED_TABLE, CORRUPTED_STREAMS_SIZE = -90, -13, -21
EMPTY_INPUT_DATA = -4
F_RFC = 16384


def _run(exe):
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0, (out.returncode, out.stderr)     # (4: counting and filling pass disagree)
    res = {"N": {}, "S": None, "P": {}, "H": []}
    for line in out.stdout.splitlines():
        tag, *v = line.split()
        if tag == "N":
            res["N"][int(v[0])] = (int(v[1]), int(v[2]))
        elif tag == "S":
            res["S"] = tuple(map(int, v))
        elif tag == "P":
            bar = v.index("|")
            res["P"][int(v[0])] = (list(map(int, v[1:bar])), list(map(int, v[bar + 1:])))
        elif tag == "H":
            res["H"].append(tuple(map(int, v)))
    return res


@pytest.fixture(scope="module")
def drv(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rfc_mode") / "rfc_mode"
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-o", str(exe), SRC])
    return _run(exe)


def test_the_flag_is_the_next_free_bit():
    header = open(os.path.join(ROOT, "include", "zd.h")).read()
    assert "#define ZD_F_RFC 16384u" in header and "#define ZD_SIZES_RFC 16384u" in header


@pytest.mark.parametrize("extra", [0, 88, 0xFFFF])
def test_long_form_number_of_sequences(drv, extra):
    # RFC 8878 3.1.1.3.2.1: byte1 + (byte2 << 8) + 0x7F00; the reference adds 0x7F (D1)
    assert drv["N"][extra] == (extra + 0x7F, extra + 0x7F00)


def test_an_empty_stream_among_four(drv):
    # the reference decodes the streams before the empty one; RFC mode refuses the section
    assert drv["S"] == (0, 2, CORRUPTED_STREAMS_SIZE)


def test_plan_frame_keys_a_zero_sequence_block_without_the_flag(drv):
    head, tail = drv["P"][0]
    # tab_prev is set by block A, so the reference's error is EmptyInputData, at block 1
    assert head[:2] == [EMPTY_INPUT_DATA, 1]
    assert tail[5] == 0                                         # CompBlock::rfc


def test_plan_frame_across_a_zero_sequence_block_with_the_flag(drv):
    head, tail = drv["P"][F_RFC]
    code, block, fses, nlisted, *listed = head
    assert (code, block) == (0, 0)                              # no key
    assert fses == 2                                            # A and C: B takes no FSE slot
    assert (nlisted, listed) == (2, [0, 2])                     # B is on no list_seq
    fse_slot_b, t0, t1, t2, huf_src_c, rfc_a, jseg = tail
    assert fse_slot_b == 0
    assert (t0, t1, t2) == (0, 0, 0)                            # C's Repeat_Mode tables are A's: tab_prev carried across B
    assert huf_src_c == 0                                       # and its Treeless literals take A's tree
    assert rfc_a == 1
    assert jseg == 3                                            # B still counts its scatter segment


def _rfc(total):
    """RFC 8878 4.2.1.1: Max_Number_of_Bits from the total, the last weight
    from what is left to the next power of two, which must be a power of two."""
    max_bits = total.bit_length()                               # highbit(total) + 1
    rest = (1 << max_bits) - total
    if rest & (rest - 1):
        return (CORRUPTED_TABLE, -1, 0)
    return (0, max_bits, rest.bit_length())                     # weight w: 2^(w - 1) == rest


def _reference(total, maxw):
    """HuffmanDecoder::from_weights (huffman.rs:177-203) as the decoder had it
    before the shared function: ceil(log2), `as u8`, the panics (D3)."""
    p = total.bit_length() - 1
    if (1 << p) < total:
        p += 1
    rest = ((1 << p) - total) & 0xFF
    if rest == 0:
        return (REF_PANIC, -1, 0)
    last = rest.bit_length()
    if maxw > p + 1 or last > p + 1:
        return (REF_PANIC, -1, 0)
    return (0, p, last)


def test_the_weight_rule_for_every_total(drv):
    assert len(drv["H"]) == 3 * 4096
    seen_pow2, seen_trunc = set(), 0
    for total, maxw, *got in drv["H"]:
        assert tuple(got[:3]) == _reference(total, maxw), (total, maxw)
        assert tuple(got[3:]) == _rfc(total), (total, maxw)
        if total & (total - 1) == 0 and maxw == 1:
            # D3: the reference panics, RFC 8878 gives one more bit and a last weight equal to the rest
            assert got[0] == REF_PANIC and got[3:] == [0, total.bit_length(), total.bit_length()]
            seen_pow2.add(total)
        if got[3] == 0 and got[0] == REF_PANIC and total & (total - 1) and maxw == 1:
            # D3's other half: what is left is 256 or more, and `as u8` made it 0 (768: 1024 - 768 = 256)
            assert (1 << total.bit_length()) - total >= 256
            seen_trunc += 1
    assert len(seen_pow2) == 13 and seen_trunc > 0                # 1, 2, 4 .. 4096


def test_the_driver_is_clean_under_asan_and_ubsan(drv, tmp_path):
    exe = tmp_path / "rfc_mode_san"
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-o", str(exe), SRC])
    assert _run(exe) == drv
