// Host driver of the planner's per-frame pass in the device planner's order
// (zd_plan.h plan_frame as zd_k_plan_count / the scan / zd_k_plan_fill run it
// for zd_batch_create_device), no GPU needed.  Ten hand-made frames -- single
// block, three blocks, raw only, failed to index, skippable, RLE then
// compressed, own tables, no Frame_Content_Size, a capacity below the
// Frame_Content_Size, one small raw block -- are planned twice with per-frame
// placement (PlanCtx::place_out / place_cap):
//   device order   plan_frame<false> per frame from zero (frames = the frame's
//                  own index while it runs), an exclusive scan whose comps /
//                  luts / fses start at the dictionaries' prebuilt comps, then
//                  plan_frame<true> per frame at its scanned counts
//   host order     one serial running pass (build_plan's)
// and every output must be equal, field by field: CompBlock, BlockRec,
// FrameDesc, FrameState, the work lists, K0's pieces, the K4J descriptors,
// frame_out / frame_cap, frame_dict and the totals.
// argv[1]: single   one formatted dictionary (prebuilt comp 0)
//          set0     a three-entry dictionary table, fallback entry 0
//          set-1    the same table, no fallback
//          plain    no dictionary, every frame with a compressed block on K4J
//          fused    no dictionary, the fused kernel's aligned slots
// Prints "equal <frames> <comps> <blocks> <copies> <jframes>" and exits 0, or
// names the first difference and exits 1.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_plan.h"

using namespace zd;

struct JMaxSeq {
  uint64_t m = 0;
  void note(uint64_t n) { if (n > m) m = n; }
};

static HostBlock block(uint64_t src, uint32_t size, uint8_t type) {
  HostBlock b;
  zero_bytes(&b, sizeof b);
  b.src = src;
  b.size = size;
  b.type = type;
  return b;
}
// a compressed block: own == true builds its own tables (LIT_COMPRESSED, FSE
// modes), else Treeless literals and Repeat tables (a dictionary's first block)
static HostBlock comp(uint64_t src, uint32_t size, uint32_t nseq, bool own, uint8_t stage = PS_ALL) {
  HostBlock b = block(src, size, 2);
  b.cb.src = src;
  b.cb.size = size;
  b.cb.lit_type = own ? LIT_COMPRESSED : LIT_TREELESS;
  b.cb.lit_regen = 100 + nseq;
  b.cb.nstreams = 1;
  b.cb.stream_size[0] = size / 2;
  b.cb.nseq = nseq;
  b.cb.modes[0] = b.cb.modes[1] = b.cb.modes[2] = own ? M_FSE : M_REPEAT;
  b.cb.host_stage = stage;
  return b;
}

struct Out {
  std::vector<CompBlock> comps;
  std::vector<BlockRec> blocks;
  std::vector<FrameDesc> fdesc;
  std::vector<FrameState> fstate;
  std::vector<uint32_t> lt, lh, ls, lk, fdict;
  std::vector<CopyDesc> copies;
  std::vector<JFrame> jframes;
  std::vector<JBlkDesc> jblkd;
  std::vector<JSegDesc> jsegd;
  std::vector<uint64_t> fout, fcap;
  Out() : comps(64), blocks(64), fdesc(16), fstate(16), lt(64, 77), lh(64, 77), ls(64, 77), lk(64, 77), fdict(16, 99),
          copies(64), jframes(16), jblkd(64), jsegd(64), fout(16), fcap(16) {
    // (whole objects zeroed: the comparison below is by field, this only keeps unwritten entries alike)
    memset(comps.data(), 0, comps.size() * sizeof(CompBlock));
    memset(blocks.data(), 0, blocks.size() * sizeof(BlockRec));
  }
  Sink sink(bool set) {
    Sink S{};
    S.comps = comps.data(); S.blocks = blocks.data(); S.fdesc = fdesc.data(); S.fstate0 = fstate.data();
    S.list_tables = lt.data(); S.list_huf = lh.data(); S.list_seq = ls.data(); S.list_k4f = lk.data();
    S.copies = copies.data(); S.jframes = jframes.data(); S.jblkd = jblkd.data(); S.jsegd = jsegd.data();
    S.frame_out = fout.data(); S.frame_cap = fcap.data();
    S.frame_dict = set ? fdict.data() : nullptr;
    return S;
  }
};

static int bad(const char* what, size_t i, const char* field) {
  printf("differs: %s[%zu].%s\n", what, i, field);
  return 1;
}
#define F(what, a, b, i, f) if ((a).f != (b).f) return bad(what, i, #f)

static int compare(const Out& A, const Out& B, const PlanCounts& T) {
  for (size_t i = 0; i < T.comps; i++) {
    const CompBlock &a = A.comps[i], &b = B.comps[i];
    F("comp", a, b, i, src); F("comp", a, b, i, lit_out); F("comp", a, b, i, seq_out); F("comp", a, b, i, seq_side);
    F("comp", a, b, i, size); F("comp", a, b, i, frame); F("comp", a, b, i, block_in_frame);
    F("comp", a, b, i, lit_regen); F("comp", a, b, i, lit_data); F("comp", a, b, i, huf_desc_size);
    F("comp", a, b, i, streams); F("comp", a, b, i, nseq); F("comp", a, b, i, seq_tables);
    F("comp", a, b, i, lut_slot); F("comp", a, b, i, fse_slot); F("comp", a, b, i, lit_extra);
    F("comp", a, b, i, huf_src); F("comp", a, b, i, lit_type); F("comp", a, b, i, nstreams);
    F("comp", a, b, i, lit_rle); F("comp", a, b, i, host_stage); F("comp", a, b, i, prebuilt);
    F("comp", a, b, i, seq_direct);
    for (int k = 0; k < 4; k++) if (a.stream_size[k] != b.stream_size[k]) return bad("comp", i, "stream_size");
    for (int k = 0; k < 3; k++)
      if (a.tab_src[k] != b.tab_src[k] || a.modes[k] != b.modes[k]) return bad("comp", i, "tab_src / modes");
  }
  for (size_t i = 0; i < T.blocks; i++) {
    const BlockRec &a = A.blocks[i], &b = B.blocks[i];
    F("block", a, b, i, src); F("block", a, b, i, size); F("block", a, b, i, comp); F("block", a, b, i, type);
    F("block", a, b, i, last); F("block", a, b, i, rle);
  }
  for (size_t i = 0; i < T.frames; i++) {
    const FrameDesc &a = A.fdesc[i], &b = B.fdesc[i];
    F("fdesc", a, b, i, out); F("fdesc", a, b, i, out_cap); F("fdesc", a, b, i, out_len0);
    F("fdesc", a, b, i, first_block); F("fdesc", a, b, i, nblocks); F("fdesc", a, b, i, lds);
    F("fdesc", a, b, i, skip); F("fdesc", a, b, i, skip_bytes);
    const FrameState &s = A.fstate[i], &t = B.fstate[i];
    F("fstate", s, t, i, key); F("fstate", s, t, i, out_len);
    for (int k = 0; k < 3; k++) if (s.rep[k] != t.rep[k]) return bad("fstate", i, "rep");
    if (A.fout[i] != B.fout[i]) return bad("frame_out", i, "");
    if (A.fcap[i] != B.fcap[i]) return bad("frame_cap", i, "");
    if (A.fdict[i] != B.fdict[i]) return bad("frame_dict", i, "");
  }
  for (size_t i = 0; i < T.tables; i++) if (A.lt[i] != B.lt[i]) return bad("list_tables", i, "");
  for (size_t i = 0; i < T.huf; i++) if (A.lh[i] != B.lh[i]) return bad("list_huf", i, "");
  for (size_t i = 0; i < T.seq; i++) if (A.ls[i] != B.ls[i]) return bad("list_seq", i, "");
  for (size_t i = 0; i < T.k4f; i++) if (A.lk[i] != B.lk[i]) return bad("list_k4f", i, "");
  for (size_t i = 0; i < T.copies; i++) {
    const CopyDesc &a = A.copies[i], &b = B.copies[i];
    F("copy", a, b, i, src); F("copy", a, b, i, dst); F("copy", a, b, i, size); F("copy", a, b, i, fill);
  }
  for (size_t i = 0; i < T.jframes; i++) {
    const JFrame &a = A.jframes[i], &b = B.jframes[i];
    F("jframe", a, b, i, base); F("jframe", a, b, i, cap); F("jframe", a, b, i, piece0); F("jframe", a, b, i, frame);
    F("jframe", a, b, i, jb0); F("jframe", a, b, i, njb);
  }
  for (size_t i = 0; i < T.jblk; i++) {
    const JBlkDesc &a = A.jblkd[i], &b = B.jblkd[i];
    F("jblkd", a, b, i, block); F("jblkd", a, b, i, jframe); F("jblkd", a, b, i, j); F("jblkd", a, b, i, seg0);
  }
  for (size_t i = 0; i < T.jseg; i++) {
    const JSegDesc &a = A.jsegd[i], &b = B.jsegd[i];
    F("jsegd", a, b, i, jblk); F("jsegd", a, b, i, k);
  }
  return 0;
}

int main(int argc, char** argv) {
  const char* mode = argc > 1 ? argv[1] : "single";
  const bool single = !strcmp(mode, "single"), set0 = !strcmp(mode, "set0"), set1 = !strcmp(mode, "set-1");
  const bool plain = !strcmp(mode, "plain"), fused = !strcmp(mode, "fused");
  if (!single && !set0 && !set1 && !plain && !fused) return 2;
  const bool set = set0 || set1, dict = single || set;

  // the dictionary table of the set modes: entry 1 and 2 formatted (prebuilt comps 0 and 1)
  const PlanDict tab[3] = {
      {0, -1, 5000, {1, 4, 8}},
      {300, 0, 3000, {11, 12, 13}},
      {70000, 1, 16384, {21, 22, 23}},
  };
  PlanCtx X{};
  X.prev_huf = single ? 0 : -1;
  X.prev_tab[0] = X.prev_tab[1] = X.prev_tab[2] = single ? 0 : -1;
  X.rep0[0] = single ? 5 : 1; X.rep0[1] = single ? 6 : 4; X.rep0[2] = single ? 7 : 8;
  X.out_len0 = single ? 3000 : 0;
  X.dict = dict;
  X.dict_id = single ? 300 : 0;
  X.k4j_mode = plain ? 1 : 0;
  X.k4j_min = K4J_MIN_BLOCKS_FEW;
  X.fused = fused;
  if (set) { X.dset = tab; X.ndset = 3; X.dset_fallback = set0 ? 0 : -1; }
  const uint32_t dict_comps = single ? 1 : set ? 2 : 0;

  // ---- the frames ----
  std::vector<HostBlock> blocks;
  std::vector<HostFrame> frames;
  auto frame = [&](uint64_t fcs, uint64_t did, uint32_t kind, uint32_t nb) {
    HostFrame f;
    zero_bytes(&f.d, sizeof f.d);
    f.d.src_offset = 4096 * frames.size();
    f.d.src_size = 4096;
    f.d.content_size = fcs;
    f.d.dict_id = did;
    f.d.kind = kind;
    f.b0 = (uint32_t)(blocks.size() - nb);
    f.nb = nb;
    f.ncomp = 0;
    for (uint32_t k = 0; k < nb; k++) f.ncomp += blocks[f.b0 + k].type == 2;
    frames.push_back(f);
  };
  const bool own = !dict;                      // without a dictionary the blocks build their own tables
  uint64_t at = 100;
  auto next = [&](uint32_t size) { const uint64_t r = at; at += size + 3; return r; };
  blocks.push_back(comp(next(500), 500, 40, own)); blocks.back().last = 1;
  frame(1000, 300, ZD_FRAME_ZSTD, 1);                                            // 0: one block
  blocks.push_back(comp(next(900), 900, 600, own));
  blocks.push_back(comp(next(800), 800, 0, true));                               //    (no sequences)
  blocks.push_back(comp(next(700), 700, 1300, true)); blocks.back().last = 1;
  frame(300000, 70000, ZD_FRAME_ZSTD, 3);                                        // 1: three blocks
  blocks.push_back(block(next(40000), 40000, 0));
  blocks.push_back(block(next(100), 100, 0)); blocks.back().last = 1;
  frame(40100, UINT64_MAX, ZD_FRAME_ZSTD, 2);                                    // 2: raw only
  blocks.push_back(comp(next(300), 300, 9, true, PS_HUF_DESC));
  frame(UINT64_MAX, UINT64_MAX, ZD_FRAME_ZSTD, 1);                               // 3: failed to index
  frames.back().status = ZD_E_NOT_ENOUGH_BYTES;
  frames.back().key = make_key(PH_PARSE, 0, PS_STRUCT, 0, ZD_E_NOT_ENOUGH_BYTES);
  blocks.push_back(block(next(64), 64, 4)); blocks.back().last = 1;
  frame(UINT64_MAX, UINT64_MAX, ZD_FRAME_SKIPPABLE, 1);                          // 4: skippable
  blocks.push_back(block(next(1), 5000, 1)); blocks.back().rle = 0x41;
  blocks.push_back(comp(next(600), 600, 70, true)); blocks.back().last = 1;
  frame(9000, 0, ZD_FRAME_ZSTD, 2);                                              // 5: RLE, then compressed
  blocks.push_back(comp(next(1200), 1200, 200, true)); blocks.back().last = 1;
  frame(20000, 5, ZD_FRAME_ZSTD, 1);                                             // 6: own tables, an unknown ID
  blocks.push_back(comp(next(400), 400, 30, own)); blocks.back().last = 1;
  frame(UINT64_MAX, 300, ZD_FRAME_ZSTD, 1);                                      // 7: no Frame_Content_Size
  blocks.push_back(comp(next(450), 450, 33, own)); blocks.back().last = 1;
  frame(50000, 70000, ZD_FRAME_ZSTD, 1);                                         // 8: capacity below the FCS
  blocks.push_back(block(next(17), 17, 0)); blocks.back().last = 1;
  frame(17, UINT64_MAX, ZD_FRAME_ZSTD, 1);                                       // 9: one small raw block
  const size_t nf = frames.size();
  if (nf != 10) return 3;
  // placement: shuffled offsets, capacities above, at and below what the frames need
  const uint64_t place_out[10] = {700000, 1000, 400000, 0, 650000, 500000, 520000, 900000, 600000, 450000};
  const uint64_t place_cap[10] = {1000, 300000, 50000, 10, 0, 9000, 30000, 1 << 20, 4096, 17};
  X.place_out = place_out;
  X.place_cap = place_cap;

  // ---- device order ----
  Out D;
  const Sink none{};
  std::vector<PlanCounts> cnt(nf), start(nf);
  JMaxSeq jm_dev, jm_host;
  for (size_t f = 0; f < nf; f++) {
    PlanCounts c{};
    c.frames = f;
    plan_frame<false, JMaxSeq>(X, frames[f], blocks.data(), c, none, &jm_dev);
    c.frames -= f;
    cnt[f] = c;
  }
  PlanCounts acc{};
  acc.comps = acc.luts = acc.fses = dict_comps;
  for (size_t f = 0; f < nf; f++) { start[f] = acc; acc.add(cnt[f]); }
  {
    const Sink S = D.sink(set);
    for (size_t f = 0; f < nf; f++) {
      PlanCounts c = start[f];
      plan_frame<true, JMaxSeq>(X, frames[f], blocks.data(), c, S, nullptr);
    }
  }
  // ---- host order ----
  Out H;
  PlanCounts run{};
  run.comps = run.luts = run.fses = dict_comps;
  {
    const Sink S = H.sink(set);
    for (size_t f = 0; f < nf; f++) plan_frame<true, JMaxSeq>(X, frames[f], blocks.data(), run, S, &jm_host);
  }
  const uint64_t *a = (const uint64_t*)&acc, *b = (const uint64_t*)&run;
  // (inexact is a flag: the running pass sets it, the scan adds the frames' flags up)
  const int w_inexact = (int)(offsetof(PlanCounts, inexact) / 8);
  if (acc.exact() != run.exact()) { printf("differs: exact\n"); return 1; }
  for (int w = 0; w < PLAN_FIELDS; w++)
    if (w != w_inexact && a[w] != b[w]) { printf("differs: totals word %d: %llu %llu\n", w, (unsigned long long)a[w], (unsigned long long)b[w]); return 1; }
  if (jm_dev.m != jm_host.m) { printf("differs: largest K4J frame\n"); return 1; }
  if (run.frames != nf || run.comps > 60 || run.blocks > 60 || run.copies > 60 || run.jseg > 60) return 3;
  if (int r = compare(D, H, run)) return r;
  // the shapes the frames were made for
  if (run.copies < 3 || (plain && run.jframes < 4) || (!plain && run.jframes) || run.inexact == 0) return 4;
  if (dict && D.comps[D.blocks[D.fdesc[0].first_block].comp].huf_src != 0) return 4;
  printf("equal %llu %llu %llu %llu %llu\n", (unsigned long long)run.frames, (unsigned long long)run.comps,
         (unsigned long long)run.blocks, (unsigned long long)run.copies, (unsigned long long)run.jframes);
  return 0;
}
