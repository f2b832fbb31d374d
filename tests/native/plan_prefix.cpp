// Host driver of the planner's per-frame pass with per-frame prefix sizes
// (zd_plan.h plan_frame, PlanCtx::prefix_bytes: what zd_batch_create_prefix
// plans with), no GPU needed.  Six hand-made frames of one compressed block
// each against prefix sizes {0, 1, 15, 5000, 0x7FFF0000, 0}:
//   frame 0  Raw literals, three FSE tables of its own
//   frame 1  Treeless literals, three Repeat tables (nothing to repeat: a
//            prefix brings no tables)
//   frame 2  as frame 0, names Dictionary_ID 300
//   frame 3  as frame 0
//   frame 4  as frame 0 (5 sequences): prefix + capacity passes K4_MAX_FRAME_OUT
//   frame 5  as frame 0
// The plan-wide fields are set to what a formatted dictionary would give
// (out_len0 999, repeat offsets 7 7 7, previous tables comp 0), so every value
// printed is the prefix branch's own.  The counting pass runs first; exit
// status 4 when its counts differ from the filling pass's.  One line per frame:
//   out_len0  rep0 rep1 rep2  huf_src  tab_src0 tab_src1 tab_src2  status of the key (0: none)  nblocks
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_plan.h"

using namespace zd;

struct NoJ {
  void note(uint64_t) {}
};

int main() {
  const uint64_t prefix[] = {0, 1, 15, 5000, 0x7FFF0000ull, 0};
  const size_t nf = sizeof prefix / sizeof prefix[0];
  PlanCtx X{};
  X.prev_huf = 0;
  X.prev_tab[0] = X.prev_tab[1] = X.prev_tab[2] = 0;
  X.rep0[0] = X.rep0[1] = X.rep0[2] = 7;
  X.out_len0 = 999;
  X.dict = true;
  X.k4j_mode = 0;
  X.prefix_bytes = prefix;

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
    b.cb.lit_type = i == 1 ? LIT_TREELESS : LIT_RAW;
    b.cb.lit_regen = 100;
    b.cb.nstreams = i == 1 ? 1 : 0;
    b.cb.stream_size[0] = i == 1 ? 20 : 0;
    b.cb.nseq = 5;
    b.cb.modes[0] = b.cb.modes[1] = b.cb.modes[2] = i == 1 ? M_REPEAT : M_FSE;
    b.cb.host_stage = PS_ALL;
    HostFrame& f = frames[i];
    zero_bytes(&f.d, sizeof f.d);
    f.d.src_offset = 64 * i;
    f.d.src_size = 64;
    f.d.content_size = 200;
    f.d.dict_id = i == 2 ? 300 : UINT64_MAX;
    f.d.kind = ZD_FRAME_ZSTD;
    f.b0 = (uint32_t)i;
    f.nb = 1;
    f.ncomp = 1;
  }

  PlanCounts cc;
  const Sink none{};
  for (size_t i = 0; i < nf; i++) plan_frame<false, NoJ>(X, frames[i], blocks.data(), cc, none, nullptr);

  PlanCounts c;
  std::vector<CompBlock> comps(nf);
  std::vector<BlockRec> brec(nf);
  std::vector<FrameDesc> fdesc(nf);
  std::vector<FrameState> fstate(nf);
  std::vector<uint32_t> lt(nf), lh(nf), ls(nf), lk(nf);
  std::vector<CopyDesc> copies(nf);
  std::vector<uint64_t> fout(nf), fcap(nf);
  Sink S{};
  S.comps = comps.data(); S.blocks = brec.data(); S.fdesc = fdesc.data(); S.fstate0 = fstate.data();
  S.list_tables = lt.data(); S.list_huf = lh.data(); S.list_seq = ls.data(); S.list_k4f = lk.data();
  S.copies = copies.data();
  S.frame_out = fout.data(); S.frame_cap = fcap.data();
  for (size_t i = 0; i < nf; i++) plan_frame<true, NoJ>(X, frames[i], blocks.data(), c, S, nullptr);
  if (c.frames != nf) return 3;
  if (memcmp(&c, &cc, sizeof c) != 0) return 4;
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
           fs.key == KEY_NONE ? 0 : key_code(fs.key), fd.nblocks);
  }
  return 0;
}
