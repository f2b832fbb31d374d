"""K1 as two passes (ZD_F_K1_SPLIT: zd_k_tables_parse, one block per lane,
then zd_k_tables_build, one wave per block) against the oracle, through the
C ABI.

Every plan is made with ZD_F_K1_SPLIT | ZD_F_NO_FUSE, and again with
ZD_F_SEQ_NO_LATENCY added, so both K3 consumers (K3L and K3Q) read the tables.
Each case asks for the oracle's status and bytes, and for the number of
blocks the two passes left to the large-scratch lane kernels
(zd_plan_k1_fallbacks): none for what libzstd writes, one for each crafted
description outside the passes' domain.  A walk of the inputs' section
headers tells which table modes, accuracy logs and tree descriptions occur,
and the tests fail when the inputs miss what they are there for.
"""
import ctypes as C
import random

import pytest

from corpus import gen, libzstd
from oracle import oracle
from test_gpu_parity import _deep_tree_frame, _ncount, _table_frame

pytestmark = pytest.mark.gpu

OUT_OF_DOMAIN = -91
K1S_SYMS = 64                       # zd_kernels.hip: symbols of a table the two passes take
MODES = ("Predefined", "RLE", "FSE", "Repeat")


def split_flags():
    from zstd_decompressor import _lib
    base = _lib.F_K1_SPLIT | _lib.F_NO_FUSE
    return (base, base | _lib.F_SEQ_NO_LATENCY)


def decode(data, flags):
    """(status, output, (Huffman, sequence) fallback blocks) of one plan."""
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Plan, run_plan
    plan = Plan(data, False, flags)
    try:
        p, n, keep = _lib.buf(data)
        st, out = run_plan(plan, p, n)
        h, q = C.c_uint64(), C.c_uint64()
        _lib.check(_lib.lib().zd_plan_k1_fallbacks(plan._h, None, C.byref(h), C.byref(q)), "zd_plan_k1_fallbacks")
        return st, out, (h.value, q.value)
    finally:
        plan.close()


def assert_parity(data, what, flags=None, oracle_result=None):
    """The oracle's status and bytes (the output of the frames before a
    failure) under each flag set; returns (oracle status, the fallback
    counts, which must agree between the flag sets)."""
    ost, oout = oracle_result or oracle.decompress_status(data, False)
    fb = None
    for fl in (split_flags() if flags is None else flags):
        gst, gout, f = decode(data, fl)
        assert gst != OUT_OF_DOMAIN, f"{what} flags={fl}: out of the GPU path's domain (oracle status {ost})"
        assert gst == ost, f"{what} flags={fl}: oracle status {ost}, gpu status {gst}"
        assert gout == oout, f"{what} flags={fl}: output differs (len {len(gout)} vs {len(oout)})"
        assert fb is None or fb == f, f"{what}: fallback counts differ between flag sets ({fb} vs {f})"
        fb = f
    return ost, fb


def ncount_walk(data, o, end, max_sym=256):
    """parse_fse_table (fse.rs:16-69) at data[o:end]: ("ok", bytes, AL,
    symbols), ("big",) at the symbol past max_sym, or ("err",)."""
    pos, nbits = 0, 8 * (end - o)

    def peek(n):
        if nbits - pos < n:
            return None
        at = 8 * o + pos
        return (int.from_bytes(data[at >> 3:(at >> 3) + 5], "little") >> (at & 7)) & ((1 << n) - 1)

    v = peek(4)
    if v is None:
        return ("err",)
    pos += 4
    al = v + 5
    if al > 9:
        return ("err",)
    remaining, nsym = 1 << al, 0
    while remaining > 0 and nsym < 256:
        bits = (remaining + 1).bit_length()
        pk = peek(bits)
        if pk is None:
            return ("err",)
        low = (1 << (bits - 1)) - 1
        thr = (1 << bits) - 1 - (remaining + 1)
        if (pk & low) < thr:
            val, pos = pk & low, pos + bits - 1
        else:
            val, pos = (pk - thr if pk > low else pk), pos + bits
        remaining -= abs(val - 1)
        if nsym >= max_sym:
            return ("big",)
        nsym += 1
        if val == 1:
            while True:
                rep = peek(2)
                if rep is None:
                    return ("err",)
                pos += 2
                if nsym + rep > max_sym:
                    return ("big",)
                nsym += rep
                if rep != 3:
                    break
    if remaining != 0 or nsym >= 256:
        return ("err",)
    return ("ok", (pos + 7) >> 3, al, nsym)


def walk(data):
    """The compressed blocks of well-formed frames, in plan order: dicts of
    lit (0 raw, 1 RLE, 2 compressed, 3 treeless), desc (the Huffman tree
    description's bytes, compressed literals only), modes and als (LL, OF,
    ML; None without sequences)."""
    from zstd_decompressor.batch import frames_index
    _, blocks, st, _ = frames_index(data)
    assert st == 0
    out = []
    for b in blocks:
        if b["type"] != 2:
            continue
        o, end = b["src_offset"], b["src_offset"] + b["block_size"]
        b0 = data[o]
        kind, sf = b0 & 3, (b0 >> 2) & 3
        d = {"lit": kind, "desc": None, "modes": None, "als": None}
        if kind < 2:
            hl = (1, 2, 1, 3)[sf]
            v = int.from_bytes(data[o:o + hl], "little")
            o += hl + ((v >> (3 if hl == 1 else 4)) if kind == 0 else 1)
        else:
            hl, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
            v = int.from_bytes(data[o:o + hl], "little")
            comp = (v >> (4 + bits)) & ((1 << bits) - 1)
            if kind == 2:
                d["desc"] = data[o + hl:o + hl + comp]
            o += hl + comp
        s0 = data[o]
        if s0:
            o += 1 if s0 < 128 else (2 if s0 < 255 else 3)
            m = data[o]
            o += 1
            modes, als = (m >> 6, (m >> 4) & 3, (m >> 2) & 3), []
            for k, mode in enumerate(modes):
                if mode == 2:
                    r = ncount_walk(data, o, end)
                    assert r[0] == "ok", r
                    o += r[1]
                    als.append(r[2])
                else:
                    o += 1 if mode == 1 else 0
                    als.append((6, 5, 6)[k] if mode == 0 else None)
            assert o <= end
            d["modes"], d["als"] = modes, tuple(als)
        out.append(d)
    return out


def max_bits(desc):
    _, widths = oracle.huffman_widths(desc)
    return max(widths)


# ---------------------------------------------------------------------------
# libzstd's frames: parity, no fallback
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def text_plan():
    return gen.frames(gen.text(300 * 4096, seed=41), 4096, 3)


@pytest.fixture(scope="module")
def libzstd_plans(text_plan):
    plans = {"text 4 KiB L3": text_plan,
             "text 128 KiB L3": gen.frames(gen.text(8 * (128 << 10), seed=71), 128 << 10, 3),
             "binary 128 KiB L19": gen.frames(gen.binary(8 * (128 << 10), seed=42), 128 << 10, 19)}
    for kind in ("xml", "text", "binary"):
        for level in (1, 9, 19):
            src = getattr(gen, kind)(1 << 20, seed=72 + level)
            plans[f"{kind} 1 MiB L{level}"] = gen.frames(src, 1 << 20, level)
    # seeded extras for what the corpora above lack
    # RLE for all three tables: literal runs of 70-119 bytes (one LL code), 6-byte matches (one ML
    # code) at distinct offsets of 61-119 (one OF code, no repeat offset)
    r = random.Random(1)
    d = bytearray()
    offs = r.sample(range(61, 120), 40)
    for k in range(40):
        d += r.randbytes(r.randrange(70, 120))
        off = offs[k] if offs[k] <= len(d) else r.randrange(61, 70)
        d += d[-off:-off + 6]
    d += r.randbytes(5)
    plans["rle tables"] = libzstd.compress(bytes(d), 3) + gen.frames(gen.text(16 * 300, seed=73), 300, 3)
    # Repeat for LL and OF: a short second block after a full one
    for tail, level in ((1024, 9), (2048, 19)):
        src = gen.xml((128 << 10) + tail, seed=74)
        plans[f"xml 128 KiB + {tail} L{level}"] = gen.frames(src, len(src), level)
    # direct weights: literals evenly over the byte values 0..n-1 (equal weights do not compress)
    r = random.Random(2)
    parts = []
    # (a repeated piece at the end: the reference rejects a block without sequences)
    for n in (4, 8, 16):
        v = list(bytes(range(n)) * (4000 // n))
        r.shuffle(v)
        v = bytes(v)
        parts.append(libzstd.compress(v + v[100:140] + v[:50], 1))
    plans["direct weights"] = b"".join(parts)
    return plans


def test_libzstd_shapes(libzstd_plans):
    for name, data in libzstd_plans.items():
        ost, fb = assert_parity(data, name)
        assert ost == 0, name
        assert fb == (0, 0), f"{name}: {fb} blocks of libzstd's left to the lane kernels"


def test_input_coverage(libzstd_plans):
    """What the libzstd plans are there for: every mode of every table, the
    accuracy logs 9 / 8 / 9 in one block, both kinds of tree description, a
    tree of maxBits 11, Treeless literals."""
    seen = [set(), set(), set()]
    als, kinds, lits, deepest = set(), set(), set(), 0
    for data in libzstd_plans.values():
        for b in walk(data):
            lits.add(b["lit"])
            if b["modes"]:
                for k in range(3):
                    seen[k].add(b["modes"][k])
                als.add(b["als"])
            if b["desc"] is not None:
                kinds.add("direct" if b["desc"][0] >= 128 else "fse")
                deepest = max(deepest, max_bits(b["desc"]))
    for k, name in enumerate(("LL", "OF", "ML")):
        assert seen[k] == {0, 1, 2, 3}, f"{name} modes missing: {[MODES[m] for m in {0, 1, 2, 3} - seen[k]]}"
    assert (9, 8, 9) in als, sorted(a for a in als if None not in a)
    assert kinds == {"direct", "fse"}, kinds
    assert deepest == 11, deepest
    assert 3 in lits, "no Treeless literals"


# ---------------------------------------------------------------------------
# crafted descriptions
# ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def filler():
    return gen.frames(gen.text(299 * 2048, seed=51), 2048, 3)


def table_fallback(frame):
    """Whether the parse pass meets a 65th symbol in the crafted frame's
    sequence tables before an error ends its walk (_table_frame's layout: a
    6-byte frame header, 3-byte block header, raw literals "xyz")."""
    o, end = 9, len(frame)
    size = int.from_bytes(frame[6:9], "little") >> 3
    assert end == 9 + size
    o += 4                                                 # literals header + xyz
    if o + 2 > end:
        return False
    m = frame[o + 1]
    o += 2
    for mode in (m >> 6, (m >> 4) & 3, (m >> 2) & 3):
        if mode == 1:
            if o >= end:
                return False
            o += 1
        elif mode == 2:
            if o >= end:
                return False
            r = ncount_walk(frame, o, end, K1S_SYMS)
            if r[0] != "ok":
                return r[0] == "big"
            o += r[1]
    return False


def test_crafted_table_frames(filler):
    """test_fused_table_builds' crafted frames (predefined / RLE / FSE tables
    of AL 5-9 and up to 255 symbols, -1 probabilities, damaged descriptions),
    each the last frame of a 300-frame plan: a fallback exactly when a table
    has more than 64 symbols."""
    r = random.Random(4242)
    big = 0
    for i in range(40):
        f = _table_frame(r)
        _, fb = assert_parity(filler + f, f"table frame #{i}")
        want = table_fallback(f)
        big += want
        assert fb == (0, 1 if want else 0), f"table frame #{i}: fallbacks {fb}, more than 64 symbols: {want}"
    assert 5 <= big <= 35, big


def test_crafted_large_tables(filler):
    """test_k1_large_tables' descriptions of 65-255 symbols: each falls back."""
    r = random.Random(77)
    for nsym, al in ((70, 6), (65, 7), (100, 7), (255, 8)):
        probs = [1] * (nsym - 1) + [(1 << al) - (nsym - 1)]
        if probs[-1] <= 0:
            probs = [1] * ((1 << al) - 1) + [0] * (nsym - (1 << al)) + [1]
        table = _ncount(al, probs)
        for trial in range(2):
            bitstream = bytes(r.randrange(256) for _ in range(r.randrange(3, 12))) + bytes([r.randrange(1, 256)])
            seqs = bytes([r.choice([1, 2, 5]), 0x80]) + table + bitstream
            content = bytes([(3 << 3) | 0]) + b"xyz" + seqs
            hdr = ((len(content) << 3) | (2 << 1) | 1).to_bytes(3, "little")
            frame = b"\x28\xb5\x2f\xfd" + bytes([0x00, 0x00]) + hdr + content
            _, fb = assert_parity(filler + frame, f"nsym {nsym} al {al} trial {trial}")
            assert fb == (0, 1), (nsym, al, fb)


def _ok_tree_frame(r, weights, tries=200):
    """A _deep_tree_frame of these weights; one the oracle decodes when the
    random sequence allows it within `tries`, else the last one."""
    for _ in range(tries):
        f = _deep_tree_frame(r, r.randrange(20, 200), weights)
        if oracle.decompress_status(f, False)[0] == 0:
            break
    return f


CRAFTED_TREES = {
    # direct weights (the implied last one follows from them): name -> (weights, falls back)
    # sum 22, maxBits 5, rest 10: the implied weight 4 leaves the last two prefixes without a code
    "hole at the end": ([4, 4, 3, 1, 1], True),
    # sum 10, maxBits 4, rest 6 -> implied weight 3: the 4-bit codes end at prefix 2, the 2-bit
    # code starts at 4 (an alignment hole at 2..3)
    "hole between widths": ([1, 1, 4], True),
    "12 bits": (list(range(12, 0, -1)), True),
    # the most weights a direct description holds, 129 leaves: complete (sum 255, rest 1)
    "128 direct weights": ([1] * 127 + [8], False),
    "complete, 3 bits": ([2, 3], False),
    "complete, 4 bits": ([4, 3, 2, 1], False),
    "complete, 7 bits, 65 leaves": ([1] * 63 + [7], False),
    "complete, 11 bits": (list(range(11, 0, -1)), False),
}


def test_crafted_huffman_trees(text_plan):
    """Trees outside the build pass's domain -- a hole after the last code, a
    hole between two widths, 12 bits -- each counted as a fallback, alone
    after a plan of libzstd frames and all of them in between libzstd frames
    in one plan; complete trees of 3 to 11 bits beside them are not counted.

    Two of the shapes a reader may look for cannot be written down.  A
    description of direct weights holds at most 128 of them (header byte 255);
    that tree, 129 leaves, is here and is complete, so the two passes build
    it; weight streams past 255 weights are FSE-coded
    (test_fse_coded_weights_past_255).  And from_number_of_bits never fails to
    place a code of a tree from_weights made: the codes' sizes sum to at most
    2^maxBits and go in by ascending size, so the aligned position after each
    width is that sum rounded up to the width's size, never past the table;
    a tree that is not complete shows as holes, the cases above."""
    r = random.Random(88)
    frames = gen.frames(gen.text(24 * 4096, seed=89), 4096, 3)
    from zstd_decompressor.batch import frames_index
    spans = [(f["src_offset"], f["src_size"]) for f in frames_index(frames)[0]]
    names = list(CRAFTED_TREES)
    parts, want = [], 0
    for i, (o, n) in enumerate(spans):
        parts.append(frames[o:o + n])
        if i % 3 == 1:
            w, falls = CRAFTED_TREES[names[i // 3]]
            parts.append(_ok_tree_frame(r, w))
            want += falls
    assert len(parts) == 24 + len(names) and want == 3
    _, fb = assert_parity(b"".join(parts), "crafted trees in between libzstd frames")
    assert fb == (want, 0), fb
    for name, (w, falls) in CRAFTED_TREES.items():
        _, fb = assert_parity(text_plan + _ok_tree_frame(r, w), f"tree: {name}")
        assert fb == (1 if falls else 0, 0), (name, fb)


def test_fse_coded_weights_past_255(text_plan):
    """An FSE-coded weight stream of 7,709 weights (the huge-tree pass's
    input, test_k2_tree_past_the_lut_slot's description): the parse pass
    flags it, zd_k_tables<true> and zd_k_tables_huge build it."""
    from test_gpu_parity import _big_tree_frame, _tree_codes_7709
    r = random.Random(31)
    codes = _tree_codes_7709()
    for i in range(3):
        frame = _big_tree_frame(r, codes, r.randrange(100, 500))
        _, fb = assert_parity(text_plan + frame, f"7,709 weights #{i}")
        assert fb == (1, 0), fb


# ---------------------------------------------------------------------------
# corruptions, agreement between the routes, device plans, graph replay
# ---------------------------------------------------------------------------
def section_spans(data):
    """Byte ranges of the literals-section and sequences-section headers and
    table descriptions of every compressed block (not the streams)."""
    from zstd_decompressor.batch import frames_index
    _, blocks, st, _ = frames_index(data)
    assert st == 0
    spans = []
    for b in blocks:
        if b["type"] != 2:
            continue
        o, end = b["src_offset"], b["src_offset"] + b["block_size"]
        kind, sf = data[o] & 3, (data[o] >> 2) & 3
        if kind < 2:
            hl = (1, 2, 1, 3)[sf]
            v = int.from_bytes(data[o:o + hl], "little")
            spans.append((o, o + hl))
            o += hl + ((v >> (3 if hl == 1 else 4)) if kind == 0 else 1)
        else:
            hl, bits = ((3, 10), (3, 10), (4, 14), (5, 18))[sf]
            v = int.from_bytes(data[o:o + hl], "little")
            comp = (v >> (4 + bits)) & ((1 << bits) - 1)
            dl = 0
            if kind == 2:
                h = data[o + hl]
                dl = 1 + (h if h < 128 else (h - 127 + 1) // 2)
            spans.append((o, o + hl + dl))
            o += hl + comp
        s0, q = data[o], o
        if s0:
            o += 1 if s0 < 128 else (2 if s0 < 255 else 3)
            m = data[o]
            o += 1
            for mode in (m >> 6, (m >> 4) & 3, (m >> 2) & 3):
                if mode == 2:
                    o += ncount_walk(data, o, end)[1]
                elif mode == 1:
                    o += 1
        spans.append((q, max(o, q + 1)))
    return spans


def test_corruptions(text_plan):
    """Ten seeded 1-3 byte corruptions inside the section headers and table
    descriptions: the oracle's status (so the same first failing frame: the
    output is that of the frames before it) and partial output."""
    spans = section_spans(text_plan)
    r = random.Random(49)
    failed = 0
    for it in range(10):
        d = bytearray(text_plan)
        for _ in range(r.randrange(1, 4)):
            a, b = spans[r.randrange(len(spans))]
            d[r.randrange(a, b)] = r.randrange(256)
        ost, _ = assert_parity(bytes(d), f"corrupt #{it}")
        failed += ost != 0
    assert failed >= 3, failed


def test_routes_agree(text_plan, filler):
    """The same plans under ZD_F_K1_LANES, the default route and
    ZD_F_K1_SPLIT: byte-identical output and the same status."""
    from zstd_decompressor import _lib
    r = random.Random(4243)
    d = bytearray(text_plan)
    a, b = section_spans(text_plan)[301]
    d[a + (b - a) // 2] ^= 0x55
    plans = [text_plan, bytes(d)] + [filler + _table_frame(r) for _ in range(6)]
    for i, data in enumerate(plans):
        res = [decode(data, fl)[:2] for fl in (_lib.F_K1_LANES | _lib.F_NO_FUSE, _lib.F_NO_FUSE, 0,
                                               _lib.F_K1_SPLIT | _lib.F_NO_FUSE, _lib.F_K1_SPLIT)]
        assert all(x == res[0] for x in res), f"plan #{i}: statuses {[x[0] for x in res]}"


def test_device_plan(text_plan):
    """Plan.from_device with the flag: the host plan's sizes, and parity.
    The parsed records live in the blocks' own table slots, so the flag adds
    no workspace in either planner.  A plan whose descriptors the device
    built keeps the walk's frame index (96 bytes a frame, zd_walk.h HostFrame,
    rounded up to 256) after everything the host planner lays out, with or
    without the flag: workspace_bytes is compared with that tail taken off."""
    import torch
    from zstd_decompressor import _lib
    from zstd_decompressor.batch import Plan
    flags = split_flags()[0]
    data = text_plan
    ost, oout = oracle.decompress_status(data, False)
    assert ost == 0
    dev = torch.device("cuda", 0)
    d_src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    d_src[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    torch.cuda.synchronize(dev)
    host = Plan(data, False, flags)
    plan = Plan.from_device(d_src.data_ptr(), len(data), False, flags)
    try:
        for k in ("nframes", "nblocks", "nsequences", "out_bytes"):
            assert getattr(plan.info, k) == getattr(host.info, k), k
        tail = (96 * plan.info.nframes + 255) // 256 * 256 if plan.info.device_descriptors else 0
        assert plan.info.workspace_bytes - tail == host.info.workspace_bytes
        for other in (Plan(data, False, _lib.F_NO_FUSE), Plan.from_device(d_src.data_ptr(), len(data), False, _lib.F_NO_FUSE)):
            mine = plan if other.info.device_descriptors else host
            assert other.info.workspace_bytes == mine.info.workspace_bytes, "the flag changes the workspace"
            other.close()
        n = plan.info.out_bytes
        d_dst = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
        torch.cuda.synchronize(dev)
        plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, 0)
        st, total, _, _, _ = plan.results(d_dst.data_ptr(), 0)
        assert st == 0 and total == len(oout)
        assert d_dst[:total].cpu().numpy().tobytes() == oout
        h, q = C.c_uint64(), C.c_uint64()
        assert _lib.lib().zd_plan_k1_fallbacks(plan._h, None, C.byref(h), C.byref(q)) == 0
        assert (h.value, q.value) == (0, 0)
    finally:
        plan.close()
        host.close()


def test_graph_replay(text_plan):
    """One replay of a captured graph of a flagged plan: the new kernels
    allocate nothing and read no host memory."""
    import torch
    from zstd_decompressor.batch import Plan
    data = text_plan
    _, src = oracle.decompress_status(data, False)
    plan = Plan(data, False, split_flags()[0])
    n = plan.info.out_bytes
    dev = torch.device("cuda", 0)
    d_src = torch.zeros(len(data) + 64, dtype=torch.uint8, device=dev)
    d_src[: len(data)].copy_(torch.frombuffer(bytearray(data), dtype=torch.uint8))
    d_dst = torch.zeros(n + 64, dtype=torch.uint8, device=dev)
    s = torch.cuda.Stream(dev)
    with torch.cuda.stream(s):          # warm-up outside the capture
        plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, s.cuda_stream)
    s.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.decode_async(d_src.data_ptr(), d_dst.data_ptr(), n, s.cuda_stream)
    d_dst.zero_()
    torch.cuda.synchronize(dev)
    g.replay()
    torch.cuda.synchronize(dev)
    st, total, _, _, _ = plan.results(d_dst.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    assert st == 0 and total == len(src)
    assert bytes(d_dst[:total].cpu().numpy().tobytes()) == src
    plan.close()
