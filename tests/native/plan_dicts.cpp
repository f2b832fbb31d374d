// Host driver of the planner's per-frame pass with a dictionary table
// (zd_plan.h plan_frame, PlanCtx::dset: what zd_plan_create_dicts plans with),
// no GPU needed.  Hand-made frames of one compressed block each -- Treeless
// literals and three Repeat sequence tables, the first block of a frame
// compressed with a trained dictionary -- go through the filling pass with the
// table
//   entry 0: ID 0   (raw content), 5000 bytes, no tables, repeat offsets 1 4 8
//   entry 1: ID 300, 3000 bytes, prebuilt comp 0, repeat offsets 11 12 13
//   entry 2: ID 70000, 16384 bytes, prebuilt comp 1, repeat offsets 21 22 23
// and the fallback given on the command line (an entry index, or -1).  The
// frames: IDs 300, absent, 70000, 0, 5 (unknown), a skippable frame, 300.
// One line per frame:
//   out_len0  rep0 rep1 rep2  huf_src  tab_src0 tab_src1 tab_src2  status of the key (0: none)  dictionary index
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_plan.h"

using namespace zd;

struct NoJ {
  void note(uint64_t) {}
};

int main(int argc, char** argv) {
  const int fallback = argc > 1 ? atoi(argv[1]) : -1;
  const PlanDict tab[3] = {
      {0, -1, 5000, {1, 4, 8}},
      {300, 0, 3000, {11, 12, 13}},
      {70000, 1, 16384, {21, 22, 23}},
  };
  PlanCtx X{};
  X.prev_huf = -1;
  X.prev_tab[0] = X.prev_tab[1] = X.prev_tab[2] = -1;
  X.rep0[0] = 1; X.rep0[1] = 4; X.rep0[2] = 8;
  X.dict = true;
  X.k4j_mode = 0;
  X.dset = tab;
  X.ndset = 3;
  X.dset_fallback = fallback;

  const uint64_t ids[] = {300, UINT64_MAX, 70000, 0, 5, UINT64_MAX, 300};
  const size_t nf = sizeof ids / sizeof ids[0];
  std::vector<HostFrame> frames(nf);
  std::vector<HostBlock> blocks(nf);
  for (size_t i = 0; i < nf; i++) {
    HostBlock& b = blocks[i];
    zero_bytes(&b, sizeof b);
    b.src = 64 * i + 16;
    b.size = 40;
    b.type = 2;
    b.last = 1;
    b.cb.src = b.src;
    b.cb.size = b.size;
    b.cb.lit_type = LIT_TREELESS;
    b.cb.lit_regen = 100;
    b.cb.nstreams = 1;
    b.cb.stream_size[0] = 20;
    b.cb.nseq = 5;
    b.cb.modes[0] = b.cb.modes[1] = b.cb.modes[2] = M_REPEAT;
    b.cb.host_stage = PS_ALL;
    HostFrame& f = frames[i];
    zero_bytes(&f.d, sizeof f.d);
    f.d.src_offset = 64 * i;
    f.d.src_size = 64;
    f.d.content_size = 200;
    f.d.dict_id = ids[i];
    f.d.kind = i == 5 ? ZD_FRAME_SKIPPABLE : ZD_FRAME_ZSTD;
    f.b0 = (uint32_t)i;
    f.nb = 1;
    f.ncomp = 1;
  }
  // (the skippable frame: one payload block, never output without ZD_F_SKIPPABLE)
  blocks[5].type = 4;
  frames[5].ncomp = 0;

  // two prebuilt comps before the frames', as build_plan counts them
  PlanCounts c;
  c.comps = c.luts = c.fses = 2;
  std::vector<CompBlock> comps(2 + nf);
  std::vector<BlockRec> brec(nf);
  std::vector<FrameDesc> fdesc(nf);
  std::vector<FrameState> fstate(nf);
  std::vector<uint32_t> lt(nf), lh(nf), ls(nf), lk(nf), fdict(nf, 99);
  std::vector<CopyDesc> copies(nf);
  std::vector<uint64_t> fout(nf), fcap(nf);
  Sink S{};
  S.comps = comps.data(); S.blocks = brec.data(); S.fdesc = fdesc.data(); S.fstate0 = fstate.data();
  S.list_tables = lt.data(); S.list_huf = lh.data(); S.list_seq = ls.data(); S.list_k4f = lk.data();
  S.copies = copies.data();
  S.frame_out = fout.data(); S.frame_cap = fcap.data();
  S.frame_dict = fdict.data();
  for (size_t i = 0; i < nf; i++) plan_frame<true, NoJ>(X, frames[i], blocks.data(), c, S, nullptr);
  if (c.frames != nf) return 3;
  for (size_t i = 0; i < nf; i++) {
    const FrameDesc& fd = fdesc[i];
    const FrameState& fs = fstate[i];
    const BlockRec& br = brec[fd.first_block];
    int huf = -9, t0 = -9, t1 = -9, t2 = -9;
    if (br.comp >= 0) {
      const CompBlock& cb = comps[(size_t)br.comp];
      huf = cb.huf_src; t0 = cb.tab_src[0]; t1 = cb.tab_src[1]; t2 = cb.tab_src[2];
    }
    printf("%llu %llu %llu %llu %d %d %d %d %d %u\n", (unsigned long long)fd.out_len0, (unsigned long long)fs.rep[0],
           (unsigned long long)fs.rep[1], (unsigned long long)fs.rep[2], huf, t0, t1, t2,
           fs.key == KEY_NONE ? 0 : key_code(fs.key), fdict[i]);
  }
  return 0;
}
