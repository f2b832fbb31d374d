// Host driver of ZD_F_AUTO_EXECUTOR's routing (zd_plan.h plan_frame with
// PlanCtx::auto_exec, plan_auto_j, plan_k4j_fields; zd_route.h auto_exec,
// chain_j_layout, auto_min_blocks), no GPU needed.  Every case is a small
// hand-made index planned as build_plan plans it: the candidates counted with
// plan_k4j_min, the PlanCtx fields from plan_k4j_fields, then the counting pass
// and the filling pass (exit status 4 when the two disagree).
// Output, one line a case:
//   C <case> <jframes> <frame:lds:status:nblocks ...>     frames with more than 8 entries: the first 8
//   A <case> <number of frames on K4J> <number of frames>  the big cases (candidate cap)
// and for the chain plan
//   W <width> <minimum at that width>
//   J <jframe> <frame>                                      per J frame, in J order
//   L <level> <jf0> <njf> <seg0> <nseg> <piece0> <npieces>  per level
//   D <1: the device planner's form of the level-major numbering agrees>
//   S <case> <1: the plan with the flag equals the plan without it, byte for byte>
//   M <mode functions hold: 1>
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

// One frame of a case: nblocks blocks, compressed or raw; `failed`: the walk
// found an error; prefix: its entry of prefix_bytes; content: Frame_Content_Size
struct Spec {
  uint32_t nblocks;
  bool raw;
  bool failed;
  uint64_t prefix;
  uint64_t content;
};
static Spec comp(uint32_t nblocks, uint64_t prefix = 5000) {
  // (no compressed block asked for: a raw-only frame in its place)
  if (!nblocks) return Spec{1, true, false, prefix, 40};
  return Spec{nblocks, false, false, prefix, 1000ull * nblocks + 37};
}
static Spec raw_only() { return Spec{1, true, false, 5000, 40}; }

struct Index {
  std::vector<HostBlock> blocks;
  std::vector<HostFrame> frames;
  std::vector<uint64_t> prefix;
};
static Index make_index(const std::vector<Spec>& specs) {
  Index I;
  for (const Spec& sp : specs) {
    HostFrame f;
    zero_bytes(&f, sizeof f);
    f.b0 = (uint32_t)I.blocks.size();
    f.nb = sp.nblocks;
    f.ncomp = sp.raw ? 0 : sp.nblocks;
    f.key = sp.failed ? make_key(PH_PARSE, 0, PS_STRUCT, 0, ZD_E_RESERVED_BLOCK_TYPE) : KEY_NONE;
    f.d.kind = ZD_FRAME_ZSTD;
    f.d.dict_id = UINT64_MAX;
    f.d.src_size = 64ull * sp.nblocks;
    f.d.content_size = sp.content;
    for (uint32_t k = 0; k < sp.nblocks; k++) {
      HostBlock b;
      zero_bytes(&b, sizeof b);
      b.src = 64ull * I.blocks.size() + 16;
      b.size = 40;
      b.type = sp.raw ? 0 : 2;
      b.last = k + 1 == sp.nblocks;
      if (!sp.raw) {
        b.cb.src = b.src;
        b.cb.size = b.size;
        b.cb.lit_type = LIT_RAW;
        b.cb.lit_regen = 100;
        b.cb.nseq = 5;
        b.cb.modes[0] = b.cb.modes[1] = b.cb.modes[2] = M_FSE;
        b.cb.host_stage = PS_ALL;
      }
      I.blocks.push_back(b);
    }
    I.frames.push_back(f);
    I.prefix.push_back(sp.prefix);
  }
  return I;
}

enum Kind { PLAIN, DICT, PREFIX, CHAIN };

struct Plan {
  PlanCounts T;
  std::vector<FrameDesc> fd;
  std::vector<FrameState> fs;
  std::vector<JFrame> jf;
  std::vector<JBlkDesc> jb;
  std::vector<JSegDesc> js;
  std::vector<uint64_t> jcnt;
};

// plan_ctx's fields for a plan of `kind` (a batch: placed frames)
static PlanCtx make_ctx(Kind kind, uint32_t flags, const RouteEnv& E, const Index& I, uint64_t width) {
  PlanCtx X{};
  X.prev_huf = X.prev_tab[0] = X.prev_tab[1] = X.prev_tab[2] = -1;
  X.rep0[0] = 1; X.rep0[1] = 4; X.rep0[2] = 8;
  X.flags = flags;
  X.dict = kind != PLAIN;
  if (kind == DICT) X.out_len0 = 5000;
  const bool prefix = kind == PREFIX || kind == CHAIN, chain = kind == CHAIN;
  if (prefix) X.prefix_bytes = I.prefix.data();
  const uint64_t n = I.frames.size();
  uint64_t cand = 0;
  if (plan_k4j_counts(flags, E, prefix, chain, 0)) {
    const uint32_t m = plan_k4j_min(flags, prefix, chain, n, width);
    for (const HostFrame& hf : I.frames) cand += hf.key == KEY_NONE && hf.ncomp >= m;
  }
  plan_k4j_fields(X, flags, E, X.dict, prefix, chain, 0, n, width, cand);
  return X;
}

// build_plan's two passes over one part; j_at as PlanCtx::j_at
static int plan(const Index& I, PlanCtx X, const uint64_t* j_at, Plan& P) {
  const size_t N = I.frames.size();
  std::vector<uint64_t> out(N), cap(N, 1ull << 40);
  for (size_t i = 0; i < N; i++) out[i] = (uint64_t)i << 20;
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
  std::vector<uint32_t> lt(nb), lh(nb), ls(nb), lk(N + 1);
  std::vector<CopyDesc> copies(cc.copies + 1);
  std::vector<uint64_t> fout(N), fcap(N);
  P.fd.assign(N, FrameDesc{});
  P.fs.assign(N, FrameState{});
  P.jf.assign(cc.jframes + 1, JFrame{});
  P.jb.assign(cc.jblk + 1, JBlkDesc{});
  P.js.assign(cc.jseg + 1, JSegDesc{});
  Sink S{};
  S.comps = comps.data(); S.blocks = brec.data(); S.fdesc = P.fd.data(); S.fstate0 = P.fs.data();
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

static int status_of(const FrameState& fs) { return fs.key == KEY_NONE ? 0 : key_code(fs.key); }

// A prefix batch (or a plan of another kind) of `specs`: one C line
static int run_case(const char* name, Kind kind, uint32_t flags, const std::vector<Spec>& specs, bool big = false,
                    const RouteEnv& E = RouteEnv()) {
  const Index I = make_index(specs);
  const PlanCtx X = make_ctx(kind, flags, E, I, specs.size());
  Plan P;
  if (int r = plan(I, X, nullptr, P)) return r;
  if (big) {
    uint64_t on_j = 0;
    for (const FrameDesc& fd : P.fd) on_j += fd.lds == 2;
    if (on_j != P.T.jframes) return 7;
    printf("A %s %llu %zu\n", name, (unsigned long long)on_j, specs.size());
    return 0;
  }
  printf("C %s %llu", name, (unsigned long long)P.T.jframes);
  for (size_t i = 0; i < specs.size() && i < 8; i++)
    printf(" %zu:%u:%d:%u", i, P.fd[i].lds, status_of(P.fs[i]), P.fd[i].nblocks);
  printf("\n");
  return 0;
}

// The same index planned with and without the flag: every descriptor equal
static int same_case(const char* name, Kind kind, uint32_t flags, const std::vector<Spec>& specs) {
  const Index I = make_index(specs);
  RouteEnv E;
  Plan A, B;
  if (int r = plan(I, make_ctx(kind, flags, E, I, specs.size()), nullptr, A)) return r;
  if (int r = plan(I, make_ctx(kind, flags | ZD_F_AUTO_EXECUTOR, E, I, specs.size()), nullptr, B)) return r;
  bool same = memcmp(&A.T, &B.T, sizeof A.T) == 0 && A.jcnt == B.jcnt;
  for (size_t i = 0; same && i < specs.size(); i++)
    same = memcmp(&A.fd[i], &B.fd[i], sizeof(FrameDesc)) == 0 && memcmp(&A.fs[i], &B.fs[i], sizeof(FrameState)) == 0;
  for (size_t k = 0; same && k < A.T.jframes; k++) same = memcmp(&A.jf[k], &B.jf[k], sizeof(JFrame)) == 0;
  printf("S %s %d\n", name, same ? 1 : 0);
  return 0;
}

static std::vector<Spec> padded(std::vector<Spec> v, size_t width) {
  while (v.size() < width) v.push_back(raw_only());
  return v;
}

// Eight chunks on three levels, as tests/native/plan_chain_j.cpp:
//   chunk   0  1  2  3  4  5  6  7
//   parent  1 -1  0 -1  5  6 -1  3
//   level   1  0  2  0  2  1  0  1
// blocks: chunks 4 and 6 have `big` compressed blocks, chunks 0, 1 and 5 have
// `small`, chunks 2, 3 and 7 one raw block: level 1 has no K4J frame when only
// the `big` ones meet the minimum
static int chain_case(uint32_t big, uint32_t small) {
  constexpr size_t N = 8;
  const int64_t PARENT[N] = {1, -1, 0, -1, 5, 6, -1, 3};
  std::vector<Spec> specs = {comp(small, 0), comp(small), raw_only(), raw_only(),
                             comp(big, 0),   comp(small, 0), comp(big, 777), raw_only()};
  specs[2].prefix = specs[7].prefix = specs[3].prefix = 0;
  Index I = make_index(specs);
  for (size_t i = 0; i < N; i++)
    if (PARENT[i] >= 0) I.prefix[i] = I.frames[PARENT[i]].d.content_size;
  int32_t level[N];
  uint32_t order[N], count[CHAIN_LEVELS];
  if (chain_order(PARENT, N, level, order, count)) return 6;
  uint32_t levels = 0, width = 0;
  for (uint32_t l = 0; l < CHAIN_LEVELS; l++)
    if (count[l]) { levels = l + 1; if (count[l] > width) width = count[l]; }
  RouteEnv E;
  const PlanCtx X = make_ctx(CHAIN, ZD_F_AUTO_EXECUTOR, E, I, width);
  printf("W %u %u\n", width, X.k4j_min);
  Plan C;
  if (int r = plan(I, X, nullptr, C)) return r;
  std::vector<uint64_t> j_at(PLAN_J_COLS * N);
  std::vector<JLevel> lev(levels);
  uint64_t tot[PLAN_J_COLS];
  plan_j_order(C.jcnt.data(), order, count, levels, j_at.data(), lev.data(), tot);
  Plan P;
  if (int r = plan(I, X, j_at.data(), P)) return r;
  for (uint64_t k = 0; k < P.T.jframes; k++) printf("J %llu %u\n", (unsigned long long)k, P.jf[k].frame);
  for (uint32_t l = 0; l < levels; l++)
    printf("L %u %llu %llu %llu %llu %llu %llu\n", l, (unsigned long long)lev[l].jf0, (unsigned long long)lev[l].njf,
           (unsigned long long)lev[l].seg0, (unsigned long long)lev[l].nseg, (unsigned long long)lev[l].piece0,
           (unsigned long long)lev[l].npieces);
  bool same = tot[PJ_FRAMES] == P.T.jframes && tot[PJ_SEG] == P.T.jseg && tot[PJ_PIECES] == P.T.jpieces;
  // the device planner's form (plan_chain_j.cpp): gather in order[] order, scan, the levels' first entries
  std::vector<uint64_t> col(PLAN_J_COLS * N), start(3 * CHAIN_LEVELS, 0);
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
  std::vector<JLevel> lev2(levels);
  plan_j_levels(start.data(), count, levels, P.T.jframes, P.T.jseg, P.T.jpieces, lev2.data());
  same = same && memcmp(lev2.data(), lev.data(), levels * sizeof(JLevel)) == 0;
  for (size_t q = 0; same && q < N; q++)
    for (int w = 0; w < PLAN_J_COLS; w++) same = same && j_at[PLAN_J_COLS * order[q] + w] == col[w * N + q];
  printf("D %d\n", same ? 1 : 0);
  return 0;
}

int main() {
  const uint32_t MIN = ZD_AUTO_MIN_BLOCKS, FEW = ZD_AUTO_MIN_BLOCKS_FEW;
  const size_t FC = ZD_AUTO_FEW_CHUNKS, MC = ZD_AUTO_MAX_CANDIDATES;
  const uint32_t A = ZD_F_AUTO_EXECUTOR;
  int r = 0;
  // (a) the minimum at a width above the few limit
  if ((r = run_case("a_min", PREFIX, A, padded({comp(MIN - 1), comp(MIN)}, FC + 1)))) return r;
  // (a) the few-chunks minimum at the limit and one past it
  if ((r = run_case("few_at", PREFIX, A, padded({comp(FEW - 1), comp(FEW)}, FC)))) return r;
  if ((r = run_case("few_past", PREFIX, A, padded({comp(FEW - 1), comp(FEW), comp(MIN)}, FC + 1)))) return r;
  // (a) candidates at the cap and one past it (and a frame below the minimum beside them)
  {
    std::vector<Spec> v(MC, comp(MIN));
    v.push_back(comp(MIN - 1));
    if ((r = run_case("cand_cap", PREFIX, A, padded(v, FC + 1), true))) return r;
    v.push_back(comp(MIN));
    if ((r = run_case("cand_past", PREFIX, A, padded(v, FC + 1), true))) return r;
  }
  // (b) the streaming executor cannot hold the frame
  const uint64_t BIG_P = 0x70000000ull, BIG_C = 0x20000000ull;
  const Spec bigf{(uint32_t)(BIG_C / MAX_BLOCK_OUT), false, false, BIG_P, BIG_C};
  if ((r = run_case("big_auto", PREFIX, A, {bigf}))) return r;
  if ((r = run_case("big_noflag", PREFIX, 0, {bigf}))) return r;
  // ((b) alone: one block, below every minimum at this width, its prefix just inside the limit)
  const Spec edge{1, false, false, K4_MAX_FRAME_OUT - 100, 200};
  if ((r = run_case("edge_auto", PREFIX, A, padded({edge}, FC + 1)))) return r;
  if ((r = run_case("edge_noflag", PREFIX, 0, padded({edge}, FC + 1)))) return r;
  const Spec over{MIN, false, false, K4_MAX_FRAME_OUT + 1, 200};
  if ((r = run_case("over_auto", PREFIX, A, {over}))) return r;
  if ((r = run_case("over_noflag", PREFIX, 0, {over}))) return r;
  // raw blocks only; a frame the walk failed
  Spec failed = comp(MIN);
  failed.failed = true;
  if ((r = run_case("rawonly", PREFIX, A, {raw_only(), comp(MIN)}))) return r;
  if ((r = run_case("failed", PREFIX, A, {failed, comp(MIN)}))) return r;
  // precedence: frames of 1 and of MIN blocks and a raw-only one, in a batch above the few limit
  const std::vector<Spec> mix = padded({comp(1), comp(MIN), raw_only()}, FC + 1);
  if ((r = run_case("pfx_auto", PREFIX, A, mix))) return r;
  if ((r = run_case("pfx_auto_bp", PREFIX, A | ZD_F_BLOCK_PARALLEL, mix))) return r;
  if ((r = run_case("pfx_bp", PREFIX, ZD_F_BLOCK_PARALLEL, mix))) return r;
  if ((r = run_case("pfx_auto_fs", PREFIX, A | ZD_F_FRAME_SERIAL, mix))) return r;
  if ((r = run_case("pfx_auto_bp_fs", PREFIX, A | ZD_F_BLOCK_PARALLEL | ZD_F_FRAME_SERIAL, mix))) return r;
  if ((r = run_case("pfx_auto_cbp", PREFIX, A | ZD_F_CHAIN_BLOCK_PARALLEL, mix))) return r;
  if ((r = run_case("chn_auto", CHAIN, A, mix))) return r;
  if ((r = run_case("chn_auto_cbp", CHAIN, A | ZD_F_CHAIN_BLOCK_PARALLEL, mix))) return r;
  if ((r = run_case("chn_cbp", CHAIN, ZD_F_CHAIN_BLOCK_PARALLEL, mix))) return r;
  if ((r = run_case("chn_auto_bp", CHAIN, A | ZD_F_BLOCK_PARALLEL, mix))) return r;
  if ((r = run_case("chn_auto_fs", CHAIN, A | ZD_F_FRAME_SERIAL, mix))) return r;
  RouteEnv K1;
  K1.k4j = 1;
  if ((r = run_case("pfx_auto_env1", PREFIX, A, mix, false, K1))) return r;
  if ((r = run_case("pfx_env1", PREFIX, 0, mix, false, K1))) return r;
  RouteEnv K0;
  K0.k4j = 0;
  if ((r = run_case("pfx_auto_env0", PREFIX, A, mix, false, K0))) return r;
  // the chain plan: the widest level's width, level-major places, a level without a K4J frame
  if ((r = chain_case(auto_min_blocks(3) + 1, auto_min_blocks(3) - 1))) return r;   // (levels of 3, 3 and 2 chunks)
  // the flag means nothing to a dictionary plan or a plain plan
  const std::vector<Spec> plainmix = {comp(1, 0), comp(MIN, 0), comp(K4J_MIN_BLOCKS, 0), raw_only()};
  if ((r = same_case("dict", DICT, 0, plainmix))) return r;
  if ((r = same_case("plain", PLAIN, 0, plainmix))) return r;
  if ((r = same_case("plain_many", PLAIN, 0, padded(plainmix, K4J_FEW_FRAMES + 1)))) return r;
  if ((r = same_case("plain_bp", PLAIN, ZD_F_BLOCK_PARALLEL, plainmix))) return r;
  // the mode functions
  RouteEnv E;
  bool m = auto_exec(A, true, false) && auto_exec(A, true, true) && !auto_exec(A, false, false) &&
           !auto_exec(0, true, false) && !auto_exec(A | ZD_F_BLOCK_PARALLEL, true, false) &&
           !auto_exec(A | ZD_F_FRAME_SERIAL, true, false) && auto_exec(A | ZD_F_CHAIN_BLOCK_PARALLEL, true, false) &&
           !auto_exec(A | ZD_F_CHAIN_BLOCK_PARALLEL, true, true) && auto_exec(A | ZD_F_BLOCK_PARALLEL, true, true) &&
           auto_exec(A | ZD_F_FRAME_SERIAL, true, true);
  m = m && chain_j_layout(A, true) && chain_j_layout(ZD_F_CHAIN_BLOCK_PARALLEL, true) && !chain_j_layout(A, false) &&
      !chain_j_layout(0, true) && !chain_j(A, true);
  m = m && k4j_mode_plan(k4j_mode_of(A, E), A, true, true, false) == 0 && k4j_mode_plan(k4j_mode_of(A, E), A, true, true, true) == 0 &&
      k4j_mode_plan(k4j_mode_of(A, E), A, false, false, false) == -1 &&
      k4j_mode_plan(k4j_mode_of(A | ZD_F_BLOCK_PARALLEL, E), A | ZD_F_BLOCK_PARALLEL, true, true, false) == 1;
  m = m && auto_min_blocks(FC) == FEW && auto_min_blocks(FC + 1) == MIN && auto_candidates_ok(MC) &&
      !auto_candidates_ok(MC + 1) && !auto_candidates_ok(0);
  m = m && plan_auto_j(MIN, MIN, true, 0, 100) && !plan_auto_j(MIN - 1, MIN, true, 0, 100) && !plan_auto_j(MIN, MIN, false, 0, 100) &&
      plan_auto_j(1, MIN, false, BIG_P, BIG_C) && !plan_auto_j(1, MIN, false, K4_MAX_FRAME_OUT + 1, 100) &&
      plan_auto_j(1, MIN, false, 0, K4_MAX_FRAME_OUT + 1) && !plan_auto_j(1, MIN, false, K4_MAX_FRAME_OUT - 100, 100);
  printf("M %d\n", m ? 1 : 0);
  return 0;
}
