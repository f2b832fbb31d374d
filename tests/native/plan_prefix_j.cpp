// Host driver of the planner's per-frame pass for prefix batches that ask for
// the block-parallel executor (zd_plan.h plan_frame with PlanCtx::prefix_bytes
// and k4j_mode, zd_route.h k4j_mode_behind: what zd_batch_create_prefix plans
// with under ZD_F_BLOCK_PARALLEL), no GPU needed.  One line per case:
//   name  lds  status of the key (0: none)  nblocks  JFrame.cap (0: no JFrame)  out_len0  jframes
// Cases:
//   big_j      prefix 0x70000000, capacity 0x20000000 (4096 compressed blocks), k4j_mode 1
//   big_off    the same frame, k4j_mode 0
//   over_j     prefix K4_MAX_FRAME_OUT + 1, small frame, k4j_mode 1
//   over_off   the same, k4j_mode 0
//   small_j    prefix 5000, one block, k4j_mode 1
//   none_j     no prefix (size 0) in a prefix plan, k4j_mode 1
//   rawonly_j  prefix 5000, one raw block, k4j_mode 1 (no compressed block: not K4J's)
//   chain      prefix 5000 in a chain plan: the mode k4j_mode_behind gives it under ZD_F_BLOCK_PARALLEL
//   dict       a dictionary plan (content 5000), likewise
//   dict_forced  a dictionary plan's frame with k4j_mode 1 handed to plan_frame all the same
//   unflagged  a prefix plan without the flag, ZD_K4J=1 in the environment (mode 1 coming in)
// The counting pass runs first for every case; exit status 4 when its counts
// differ from the filling pass's.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_plan.h"
#include "../../zstd-decompressor_amd/csrc/zd_route.h"

using namespace zd;

struct NoJ {
  void note(uint64_t) {}
};

static int run_case(const char* name, PlanCtx X, uint64_t prefix, uint32_t nblocks, uint64_t content, bool raw) {
  const uint64_t pfx[1] = {prefix};
  if (X.prefix_bytes) X.prefix_bytes = pfx;
  std::vector<HostBlock> blocks(nblocks);
  for (uint32_t i = 0; i < nblocks; i++) {
    HostBlock& b = blocks[i];
    zero_bytes(&b, sizeof b);
    b.src = 64ull * i + 16;
    b.size = 40;
    b.type = raw ? 0 : 2;
    b.last = i + 1 == nblocks;
    if (!raw) {
      b.cb.src = b.src;
      b.cb.size = b.size;
      b.cb.lit_type = LIT_RAW;
      b.cb.lit_regen = 100;
      b.cb.nseq = 5;
      b.cb.modes[0] = b.cb.modes[1] = b.cb.modes[2] = M_FSE;
      b.cb.host_stage = PS_ALL;
    }
  }
  HostFrame f;
  zero_bytes(&f, sizeof f);
  f.d.src_size = 64ull * nblocks;
  f.d.content_size = content;
  f.d.dict_id = UINT64_MAX;
  f.d.kind = ZD_FRAME_ZSTD;
  f.b0 = 0;
  f.nb = nblocks;
  f.ncomp = raw ? 0 : nblocks;
  f.key = KEY_NONE;

  PlanCounts cc;
  const Sink none{};
  plan_frame<false, NoJ>(X, f, blocks.data(), cc, none, nullptr);

  const size_t n = nblocks + 1;
  PlanCounts c;
  std::vector<CompBlock> comps(n);
  std::vector<BlockRec> brec(n);
  std::vector<FrameDesc> fdesc(1);
  std::vector<FrameState> fstate(1);
  std::vector<uint32_t> lt(n), lh(n), ls(n), lk(n);
  std::vector<CopyDesc> copies(n);
  std::vector<JFrame> jf(1);
  std::vector<JBlkDesc> jb(n);
  std::vector<JSegDesc> js(n);
  std::vector<uint64_t> fout(1), fcap(1);
  Sink S{};
  S.comps = comps.data(); S.blocks = brec.data(); S.fdesc = fdesc.data(); S.fstate0 = fstate.data();
  S.list_tables = lt.data(); S.list_huf = lh.data(); S.list_seq = ls.data(); S.list_k4f = lk.data();
  S.copies = copies.data();
  S.jframes = jf.data(); S.jblkd = jb.data(); S.jsegd = js.data();
  S.frame_out = fout.data(); S.frame_cap = fcap.data();
  plan_frame<true, NoJ>(X, f, blocks.data(), c, S, nullptr);
  if (c.frames != 1) return 3;
  if (memcmp(&c, &cc, sizeof c) != 0) return 4;
  const FrameDesc& fd = fdesc[0];
  const FrameState& fs = fstate[0];
  printf("%s %u %d %u %llu %llu %llu\n", name, fd.lds, fs.key == KEY_NONE ? 0 : key_code(fs.key), fd.nblocks,
         (unsigned long long)(c.jframes ? jf[0].cap : 0), (unsigned long long)fd.out_len0,
         (unsigned long long)c.jframes);
  return 0;
}

int main() {
  // a prefix plan: the plan-wide fields set to what a formatted dictionary
  // would give, so every value printed is the prefix branch's own
  const uint64_t some[1] = {0};
  PlanCtx X{};
  X.prev_huf = X.prev_tab[0] = X.prev_tab[1] = X.prev_tab[2] = -1;
  X.rep0[0] = 1; X.rep0[1] = 4; X.rep0[2] = 8;
  X.dict = true;
  X.prefix_bytes = some;
  const uint64_t BIG_P = 0x70000000ull, BIG_C = 0x20000000ull;
  const uint32_t BIG_B = (uint32_t)(BIG_C / MAX_BLOCK_OUT);
  int r = 0;
  PlanCtx J = X, OFF = X;
  J.k4j_mode = 1;
  OFF.k4j_mode = 0;
  if ((r = run_case("big_j", J, BIG_P, BIG_B, BIG_C, false))) return r;
  if ((r = run_case("big_off", OFF, BIG_P, BIG_B, BIG_C, false))) return r;
  if ((r = run_case("over_j", J, K4_MAX_FRAME_OUT + 1, 1, 200, false))) return r;
  if ((r = run_case("over_off", OFF, K4_MAX_FRAME_OUT + 1, 1, 200, false))) return r;
  if ((r = run_case("small_j", J, 5000, 1, 200, false))) return r;
  if ((r = run_case("none_j", J, 0, 1, 200, false))) return r;
  if ((r = run_case("rawonly_j", J, 5000, 1, 40, true))) return r;
  // what plan_ctx makes of the mode (k4j_mode_of gives 1 under ZD_F_BLOCK_PARALLEL)
  RouteEnv E;
  const int m = k4j_mode_of(ZD_F_BLOCK_PARALLEL, E);
  PlanCtx CH = X;
  CH.k4j_mode = k4j_mode_behind(m, ZD_F_BLOCK_PARALLEL, true, true, true);
  if ((r = run_case("chain", CH, 5000, 1, 200, false))) return r;
  PlanCtx D = X;
  D.prefix_bytes = nullptr;
  D.out_len0 = 5000;
  D.k4j_mode = k4j_mode_behind(m, ZD_F_BLOCK_PARALLEL, true, false, false);
  if ((r = run_case("dict", D, 0, 1, 200, false))) return r;
  D.k4j_mode = 1;
  if ((r = run_case("dict_forced", D, 0, 1, 200, false))) return r;
  PlanCtx U = X;
  E.k4j = 1;
  U.k4j_mode = k4j_mode_behind(k4j_mode_of(0, E), 0, true, true, false);
  if ((r = run_case("unflagged", U, 5000, 1, 200, false))) return r;
  // (and the flagged prefix plan keeps its mode)
  if (k4j_mode_behind(m, ZD_F_BLOCK_PARALLEL, true, true, false) != 1) return 5;
  if (k4j_mode_behind(-1, 0, false, false, false) != -1) return 5;
  return 0;
}
