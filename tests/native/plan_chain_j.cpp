// Host driver of the planner for a chain batch created with
// ZD_F_CHAIN_BLOCK_PARALLEL (zd_plan.h plan_frame with PlanCtx::j_at, plan_j_order,
// plan_j_levels; zd_route.h k4j_mode_plan), no GPU needed: the K4J frames of such
// a plan are numbered level-major, so that every level of the chain owns one
// contiguous range of J frames, J blocks, scatter segments, state words and
// pieces.  The index is hand-made: eight chunks on three levels, their order
// interleaved, frames with compressed blocks (K4J's) and raw-only ones mixed:
//   chunk   0  1  2  3  4  5  6  7
//   parent  1 -1  0 -1  5  6 -1  3
//   level   1  0  2  0  2  1  0  1
//   blocks  2c 1c 1r 1r 3c 1c 2c 1r      (c: compressed, r: raw; chunk 1's block has 3 segments)
// Output, one line each:
//   M <mode of a flagged chain plan> <mode of an unflagged one under ZD_F_BLOCK_PARALLEL>
//   J <jframe> <frame> <base> <piece0> <jb0> <njb> <first segment>      per J frame, in J order
//   B <jblk> <jframe> <block in frame> <seg0>                           per J block
//   S <segment> <jblk> <segment in block>                               per scatter segment
//   L <level> <jf0> <njf> <seg0> <nseg> <piece0> <npieces>              per level
//   T <jframes> <jblk> <jseg> <jwords> <jpieces>                        the totals
//   D <1: the device planner's form (gather in order[] order, exclusive scans, scatter back) agrees>
//   U <jframes of the same index planned with the unflagged mode>
// Exit status 4: the counting and the filling pass disagree.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_chain.h"
#include "../../zstd-decompressor_amd/csrc/zd_plan.h"
#include "../../zstd-decompressor_amd/csrc/zd_route.h"

using namespace zd;

struct NoJ {
  void note(uint64_t) {}
};

constexpr size_t N = 8;
static const int64_t PARENT[N] = {1, -1, 0, -1, 5, 6, -1, 3};
static const uint32_t NBLK[N] = {2, 1, 1, 1, 3, 1, 2, 1};
static const bool RAW[N] = {false, false, true, true, false, false, false, true};

struct Index {
  std::vector<HostBlock> blocks;
  std::vector<HostFrame> frames;
};

static Index make_index() {
  Index I;
  for (size_t i = 0; i < N; i++) {
    HostFrame f;
    zero_bytes(&f, sizeof f);
    f.b0 = (uint32_t)I.blocks.size();
    f.nb = NBLK[i];
    f.ncomp = RAW[i] ? 0 : NBLK[i];
    f.key = KEY_NONE;
    f.d.kind = ZD_FRAME_ZSTD;
    f.d.dict_id = UINT64_MAX;
    f.d.src_size = 64ull * NBLK[i];
    f.d.content_size = RAW[i] ? 40ull * NBLK[i] : 1000 + 37 * i;   // (odd sizes: pieces that do not end a frame's line)
    for (uint32_t k = 0; k < NBLK[i]; k++) {
      HostBlock b;
      zero_bytes(&b, sizeof b);
      b.src = 64ull * I.blocks.size() + 16;
      b.size = 40;
      b.type = RAW[i] ? 0 : 2;
      b.last = k + 1 == NBLK[i];
      if (!RAW[i]) {
        b.cb.src = b.src;
        b.cb.size = b.size;
        b.cb.lit_type = LIT_RAW;
        b.cb.lit_regen = 100;
        b.cb.nseq = i == 1 ? 2 * J_SEG + 1 : 5;      // chunk 1: three scatter segments
        b.cb.modes[0] = b.cb.modes[1] = b.cb.modes[2] = M_FSE;
        b.cb.host_stage = PS_ALL;
      }
      I.blocks.push_back(b);
    }
    I.frames.push_back(f);
  }
  return I;
}

struct Plan {
  PlanCounts T;
  std::vector<JFrame> jf;
  std::vector<JBlkDesc> jb;
  std::vector<JSegDesc> js;
  std::vector<FrameDesc> fd;
  std::vector<uint64_t> jcnt;
};

// build_plan's two passes over one part, the frames in chunk order; j_at as PlanCtx::j_at
static int plan(const Index& I, PlanCtx X, const uint64_t* j_at, Plan& P) {
  std::vector<uint64_t> out(N), cap(N, 1ull << 20);
  for (size_t i = 0; i < N; i++) out[i] = (N - i) << 20;    // (placed, as every batch's frames)
  X.place_out = out.data();
  X.place_cap = cap.data();
  const Sink none{};
  PlanCounts cc;
  P.jcnt.assign(PLAN_J_COLS * N, 0);
  for (size_t i = 0; i < N; i++) {
    uint64_t a[PLAN_J_COLS], b[PLAN_J_COLS];
    plan_j_get(cc, a);
    plan_frame<false, NoJ>(X, I.frames[i], I.blocks.data(), cc, none, nullptr);
    plan_j_get(cc, b);
    for (int w = 0; w < PLAN_J_COLS; w++) P.jcnt[PLAN_J_COLS * i + w] = b[w] - a[w];
  }
  const size_t nb = I.blocks.size() + 1;
  std::vector<CompBlock> comps(nb);
  std::vector<BlockRec> brec(nb);
  std::vector<FrameState> fstate(N);
  std::vector<uint32_t> lt(nb), lh(nb), ls(nb), lk(N + 1);
  std::vector<CopyDesc> copies(nb);
  std::vector<uint64_t> fout(N), fcap(N);
  P.fd.assign(N, FrameDesc{});
  P.jf.assign(cc.jframes + 1, JFrame{});
  P.jb.assign(cc.jblk + 1, JBlkDesc{});
  P.js.assign(cc.jseg + 1, JSegDesc{});
  Sink S{};
  S.comps = comps.data(); S.blocks = brec.data(); S.fdesc = P.fd.data(); S.fstate0 = fstate.data();
  S.list_tables = lt.data(); S.list_huf = lh.data(); S.list_seq = ls.data(); S.list_k4f = lk.data();
  S.copies = copies.data();
  S.jframes = P.jf.data(); S.jblkd = P.jb.data(); S.jsegd = P.js.data();
  S.frame_out = fout.data(); S.frame_cap = fcap.data();
  X.j_at = j_at;
  PlanCounts c;
  for (size_t i = 0; i < N; i++) plan_frame<true, NoJ>(X, I.frames[i], I.blocks.data(), c, S, nullptr);
  if (memcmp(&c, &cc, sizeof c) != 0) return 4;
  P.T = c;
  return 0;
}

int main() {
  const Index I = make_index();
  const uint64_t pfx[N] = {0, 5000, 0, 0, 0, 0, 777, 0};   // (external prefixes on two roots; the rest: the parents' sizes)
  uint64_t pb[N];
  for (size_t i = 0; i < N; i++) pb[i] = PARENT[i] >= 0 ? I.frames[PARENT[i]].d.content_size : pfx[i];
  PlanCtx X{};
  X.prev_huf = X.prev_tab[0] = X.prev_tab[1] = X.prev_tab[2] = -1;
  X.rep0[0] = 1; X.rep0[1] = 4; X.rep0[2] = 8;
  X.dict = true;
  X.prefix_bytes = pb;
  RouteEnv E;
  const int m = k4j_mode_of(ZD_F_BLOCK_PARALLEL, E);
  const int flagged = k4j_mode_plan(k4j_mode_of(ZD_F_CHAIN_BLOCK_PARALLEL, E), ZD_F_CHAIN_BLOCK_PARALLEL, true, true, true);
  const int unflagged = k4j_mode_plan(m, ZD_F_BLOCK_PARALLEL, true, true, true);
  // (the flag means nothing outside a chain: a prefix batch, a dictionary plan, a plain plan)
  if (k4j_mode_plan(-1, ZD_F_CHAIN_BLOCK_PARALLEL, true, true, false) != 0 ||
      k4j_mode_plan(-1, ZD_F_CHAIN_BLOCK_PARALLEL, true, false, false) != 0 ||
      k4j_mode_plan(-1, ZD_F_CHAIN_BLOCK_PARALLEL, false, false, false) != -1)
    return 5;
  printf("M %d %d\n", flagged, unflagged);

  int32_t level[N];
  uint32_t order[N], count[CHAIN_LEVELS];
  if (chain_order(PARENT, N, level, order, count)) return 6;
  uint32_t levels = 0;
  for (uint32_t l = 0; l < CHAIN_LEVELS; l++) if (count[l]) levels = l + 1;

  // the counts (no j_at yet), the level-major places, the fill
  PlanCtx XJ = X;
  XJ.k4j_mode = flagged;
  Plan C;
  if (int r = plan(I, XJ, nullptr, C)) return r;
  std::vector<uint64_t> j_at(PLAN_J_COLS * N);
  std::vector<JLevel> lev(levels);
  uint64_t tot[PLAN_J_COLS];
  plan_j_order(C.jcnt.data(), order, count, levels, j_at.data(), lev.data(), tot);
  Plan P;
  if (int r = plan(I, XJ, j_at.data(), P)) return r;
  for (uint64_t k = 0; k < P.T.jframes; k++)
    printf("J %llu %u %llu %llu %u %u %u\n", (unsigned long long)k, P.jf[k].frame, (unsigned long long)P.jf[k].base,
           (unsigned long long)P.jf[k].piece0, P.jf[k].jb0, P.jf[k].njb, P.jb[P.jf[k].jb0].seg0);
  for (uint64_t k = 0; k < P.T.jblk; k++) printf("B %llu %u %u %u\n", (unsigned long long)k, P.jb[k].jframe, P.jb[k].j, P.jb[k].seg0);
  for (uint64_t k = 0; k < P.T.jseg; k++) printf("S %llu %u %u\n", (unsigned long long)k, P.js[k].jblk, P.js[k].k);
  for (uint32_t l = 0; l < levels; l++)
    printf("L %u %llu %llu %llu %llu %llu %llu\n", l, (unsigned long long)lev[l].jf0, (unsigned long long)lev[l].njf,
           (unsigned long long)lev[l].seg0, (unsigned long long)lev[l].nseg, (unsigned long long)lev[l].piece0,
           (unsigned long long)lev[l].npieces);
  printf("T %llu %llu %llu %llu %llu\n", (unsigned long long)P.T.jframes, (unsigned long long)P.T.jblk,
         (unsigned long long)P.T.jseg, (unsigned long long)P.T.jwords, (unsigned long long)P.T.jpieces);
  bool totals = tot[PJ_FRAMES] == P.T.jframes && tot[PJ_BLK] == P.T.jblk && tot[PJ_SEG] == P.T.jseg &&
                tot[PJ_WORDS] == P.T.jwords && tot[PJ_PIECES] == P.T.jpieces;

  // the device planner's form: the columns gathered in order[] order, an
  // exclusive scan of each, the starts scattered back to the frames; the
  // levels' first entries read at the levels' first places (the cursors after
  // the bucket pass are the levels' ends) and turned into ranges by plan_j_levels
  std::vector<uint64_t> col(PLAN_J_COLS * N), j_at2(PLAN_J_COLS * N), start(3 * CHAIN_LEVELS, 0);
  for (size_t q = 0; q < N; q++)
    for (int w = 0; w < PLAN_J_COLS; w++) col[w * N + q] = C.jcnt[PLAN_J_COLS * order[q] + w];
  for (int w = 0; w < PLAN_J_COLS; w++) {
    uint64_t acc = 0;
    for (size_t q = 0; q < N; q++) { const uint64_t v = col[w * N + q]; col[w * N + q] = acc; acc += v; }
  }
  uint32_t end = 0;
  for (uint32_t l = 0; l < levels; l++) {
    end += count[l];
    if (!count[l]) continue;
    const size_t b = end - count[l];
    start[3 * l + 0] = col[PJ_FRAMES * N + b]; start[3 * l + 1] = col[PJ_SEG * N + b]; start[3 * l + 2] = col[PJ_PIECES * N + b];
  }
  for (size_t q = 0; q < N; q++)
    for (int w = 0; w < PLAN_J_COLS; w++) j_at2[PLAN_J_COLS * order[q] + w] = col[w * N + q];
  std::vector<JLevel> lev2(levels);
  plan_j_levels(start.data(), count, levels, P.T.jframes, P.T.jseg, P.T.jpieces, lev2.data());
  const bool same = totals && j_at2 == j_at && memcmp(lev2.data(), lev.data(), levels * sizeof(JLevel)) == 0;
  printf("D %d\n", same ? 1 : 0);

  PlanCtx XU = X;
  XU.k4j_mode = unflagged;
  Plan U;
  if (int r = plan(I, XU, nullptr, U)) return r;
  printf("U %llu\n", (unsigned long long)U.T.jframes);
  return 0;
}
