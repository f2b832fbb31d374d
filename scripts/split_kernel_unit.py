"""Makes the remaining cuts of csrc/zd_kernels.hip (DESIGN.md section 4's map): every section between two
banner comments becomes a part file that zd_kernels.hip includes in the text's order.  A pure move: no line
of code is edited or reordered, each part gets a three-line header, zd_kernels.hip keeps its head (includes,
namespace zd, the name tables), the include of zd_pipeline.hip where it stands, and its tail.  Check the
result with scripts/device_asm_diff.py: the device assembly must be the parent's, all kernels identical as
they stand.  The comments and docstrings that name zd_kernels.hip as a symbol's home are not touched.
usage: python scripts/split_kernel_unit.py [--dir zstd-decompressor_amd/csrc]"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = sys.argv[sys.argv.index("--dir") + 1] if "--dir" in sys.argv else os.path.join(ROOT, "zstd-decompressor_amd", "csrc")
TAIL = "Compiled only as part of zd_kernels.hip, which includes it inside namespace zd."
# (part, the line behind the banner line "// ----" that opens its section, what the header says it holds)
PARTS = [
    ("zd_k_bits.hip", "// constants (decoders/sequence.rs", "the constant tables, the backward and forward bit readers, "
     "parse_ncount, build_fse and the trace / profiling macros: what every decode kernel stands on."),
    ("zd_k1.hip", "// K1: tables, one compressed block per LANE", "K1 on lanes: zd_k_tables and zd_k_tables_huge."),
    ("zd_k2.hip", "// Per-lane backward bitstream windows (K2, K3)", "the bitstream windows K2 and K3 share, K2's pair "
     "tables (zd_k_huf_pairs), zd_k_dict_tables and zd_k_huffman."),
    ("zd_k3.hip", "// K3: sequences (sequences.rs", "K3, the FSE state chains: zd_k_sequences, zd_k_sequences_q, "
     "zd_k_sequences_l; rec_lane, K4's read of their records."),
    ("zd_k4.hip", "// K4: execute (decoding_context.rs:50-106 + block.rs:74-99), one frame per", "the streaming K4: K4W, "
     "k4_body and zd_k_execute, _dict, _dicts, _prefix, _chain (zd_fused.hip runs k4_body too)."),
    ("zd_fused.hip", "// zd_k_fused: K1's sequence half, K3 and K4 of FZ_FRAMES", "the wave-wide table builds (fz_*), "
     "zd_k_tables_seqw, K1's two passes (they use fz_build_fse) and zd_k_fused."),
    ("zd_k4f.hip", "// K4F: execute with the whole frame resident in LDS", "K4F, zd_k_execute_lds."),
    ("zd_k4j.hip", "// K4J: execute of frames of many blocks", "K4J: zd_k_jsum, zd_k_jsum_blocks, zd_k_jprefix, "
     "zd_k_jscatter, zd_k_jround (zd_pipeline.hip starts them)."),
    ("zd_post.hip", "// K0: raw / RLE blocks at the head of a frame", "zd_k_rawcopy, zd_k_xxh64 and zd_k_verify with "
     "their launchers, zd_k_compact (launch_compact is in zd_pipeline.hip)."),
    ("zd_devplan.hip", "// Device header walk (SURVEY", "the device walk (zd_k_walk*) and the device planner "
     "(zd_k_plan_*) with their launchers."),
    ("zd_batch.hip", "// Batches of scattered chunks (zd_batch_create).", "batches: gather, results, chain levels, "
     "layout, scans, pack, sizes, each with its launcher."),
]
PIPE = '#include "zd_pipeline.hip"'

L = open(os.path.join(CSRC, "zd_kernels.hip")).read().split("\n")
banner = lambda i: L[i].startswith("// ------")
starts = []
for name, key, _ in PARTS:
    hit = [i for i in range(1, len(L)) if L[i].startswith(key) and banner(i - 1)]
    assert len(hit) == 1, (name, hit)
    starts.append(hit[0] - 1)
assert starts == sorted(starts)
pipe = L.index(PIPE)
end = max(i for i, l in enumerate(L) if l == "}  // namespace zd")
assert starts[8] < pipe < starts[9] < end
# zd_post.hip ends before the comment that introduces the include of zd_pipeline.hip
pipe0 = pipe
while L[pipe0 - 1].startswith("//"):
    pipe0 -= 1
stops = starts[1:9] + [pipe0, starts[10], end]
out = L[:starts[0]]
for k, (name, _, holds) in enumerate(PARTS):
    body = L[starts[k]:stops[k]]
    while body and body[-1] == "":
        body.pop()
    words, lines, line = (name + " -- " + holds + "  " + TAIL).split(" "), [], "//"
    for w in words:
        if len(line) + 1 + len(w) > 100:
            lines.append(line)
            line = "//"
        line += " " + w
    open(os.path.join(CSRC, name), "w").write("\n".join(lines + [line] + body) + "\n")
    out.append('#include "%s"' % name)
    if k == 8:
        out += [""] + L[pipe0:pipe + 1] + [""]
out += [""] + L[end:]
open(os.path.join(CSRC, "zd_kernels.hip"), "w").write("\n".join(out))
print("zd_kernels.hip: %d lines, %d parts written" % (len(out) - 1, len(PARTS)))
