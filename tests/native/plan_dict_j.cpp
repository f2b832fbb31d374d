// Host driver of the planner's per-frame pass for dictionary and dictionary-set
// plans created with ZD_F_DICT_BLOCK_PARALLEL (zd_plan.h plan_frame with
// PlanCtx::dict_j, set by plan_k4j_fields from zd_route.h dict_j / dict_j_mode),
// no GPU needed.  One line per case:
//   name  lds  status of the key (0: none)  nblocks  JFrame.cap (0: no JFrame)  out_len0  jframes
//         JFrame.src  first repeat offset  tab_src[0] of the frame's first block (Repeat_Mode)
// The frame of every case has `blocks` compressed blocks whose first uses
// Repeat_Mode tables.  Cases (content 5000, repeat offsets 11 12 13, tables in
// the prebuilt comp 0, unless said otherwise):
//   forced       flag | ZD_F_BLOCK_PARALLEL, one block
//   noflag       ZD_F_BLOCK_PARALLEL | ZD_F_AUTO_EXECUTOR without the flag, one block
//   serial       flag | ZD_F_FRAME_SERIAL, three blocks
//   both         flag | ZD_F_BLOCK_PARALLEL | ZD_F_FRAME_SERIAL: ZD_F_FRAME_SERIAL wins
//   auto6_3      flag alone, 6 frames in the plan, 1 candidate, three blocks
//   auto6_1      ... one block (below ZD_AUTO_MIN_BLOCKS_FEW)
//   auto65_3     flag alone, 65 frames, three blocks (below ZD_AUTO_MIN_BLOCKS)
//   auto65_4     ... four blocks
//   auto_at_cap  flag alone, 6 frames, ZD_AUTO_DICT_MAX_CANDIDATES candidates, three blocks
//   auto_cap     flag alone, 6 frames, ZD_AUTO_DICT_MAX_CANDIDATES + 1 candidates, three blocks
//   b_auto       flag alone, content 1 GiB and capacity 1 GiB, no candidate counted: clause (b)
//   b_serial     the same frame with ZD_F_FRAME_SERIAL: out of the streaming executor's domain
//   b_noflag     the same frame without the flag: likewise, as ever
//   set_named    a set plan (the table of plan_dicts.cpp), forced, the frame names ID 70000
//   set_none     ... a frame without an ID, no fallback: no dictionary, source entry ndset
//   set_missing  ... a frame that names an ID the set lacks
//   set_noflag   set_named without the flag
// The counting pass runs first for every case; exit status 4 when its counts
// differ from the filling pass's, 5 when a route function of zd_route.h /
// zd_plan.h that existed before the flag answers differently for it.
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

static int run_case(const char* name, const PlanCtx& X, uint32_t nblocks, uint64_t content, uint64_t dict_id) {
  std::vector<HostBlock> blocks(nblocks);
  for (uint32_t i = 0; i < nblocks; i++) {
    HostBlock& b = blocks[i];
    zero_bytes(&b, sizeof b);
    b.src = 64ull * i + 16;
    b.size = 40;
    b.type = 2;
    b.last = i + 1 == nblocks;
    b.cb.src = b.src;
    b.cb.size = b.size;
    b.cb.lit_type = LIT_RAW;
    b.cb.lit_regen = 100;
    b.cb.nseq = 5;
    b.cb.modes[0] = b.cb.modes[1] = b.cb.modes[2] = i == 0 ? M_REPEAT : M_FSE;
    b.cb.host_stage = PS_ALL;
  }
  HostFrame f;
  zero_bytes(&f, sizeof f);
  f.d.src_size = 64ull * nblocks;
  f.d.content_size = content;
  f.d.dict_id = dict_id;
  f.d.kind = ZD_FRAME_ZSTD;
  f.b0 = 0;
  f.nb = nblocks;
  f.ncomp = nblocks;
  f.key = KEY_NONE;

  // (the plan's prebuilt comps come first, as build_plan counts them)
  PlanCounts cc;
  cc.comps = cc.luts = cc.fses = 2;
  const Sink none{};
  plan_frame<false, NoJ>(X, f, blocks.data(), cc, none, nullptr);

  const size_t n = nblocks + 3;
  PlanCounts c;
  c.comps = c.luts = c.fses = 2;
  std::vector<CompBlock> comps(n);
  std::vector<BlockRec> brec(n);
  std::vector<FrameDesc> fdesc(1);
  std::vector<FrameState> fstate(1);
  std::vector<uint32_t> lt(n), lh(n), ls(n), lk(n), fdict(1, 0xFFFFFFFFu);
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
  S.frame_dict = fdict.data();
  plan_frame<true, NoJ>(X, f, blocks.data(), c, S, nullptr);
  if (c.frames != 1) return 3;
  if (memcmp(&c, &cc, sizeof c) != 0) return 4;
  const FrameDesc& fd = fdesc[0];
  const FrameState& fs = fstate[0];
  // a set plan's J frame names the entry the streaming kernel reads for the frame
  if (X.dset && c.jframes && jf[0].src != fdict[0]) return 6;
  printf("%s %u %d %u %llu %llu %llu %u %llu %d\n", name, fd.lds, fs.key == KEY_NONE ? 0 : key_code(fs.key),
         fd.nblocks, (unsigned long long)(c.jframes ? jf[0].cap : 0), (unsigned long long)fd.out_len0,
         (unsigned long long)c.jframes, c.jframes ? jf[0].src : 0u, (unsigned long long)fs.rep[0],
         (int)comps[2].tab_src[0]);
  return 0;
}

// A dictionary plan's PlanCtx as plan_ctx (zd_host.cpp) makes it
static PlanCtx dict_ctx(uint32_t flags, uint64_t content, uint64_t nframes, uint64_t candidates, bool flag_seen) {
  PlanCtx X{};
  X.prev_huf = X.prev_tab[0] = X.prev_tab[1] = X.prev_tab[2] = 0;
  X.rep0[0] = 11; X.rep0[1] = 12; X.rep0[2] = 13;
  X.out_len0 = content;
  X.flags = flags;
  X.dict = true;
  RouteEnv E;
  if (flag_seen)
    plan_k4j_fields(X, flags, E, true, false, false, content, nframes, nframes, candidates, dict_j(flags, true));
  else
    plan_k4j_fields(X, flags, E, true, false, false, content, nframes, nframes, candidates);
  return X;
}

int main() {
  const uint32_t DJ = ZD_F_DICT_BLOCK_PARALLEL, BP = ZD_F_BLOCK_PARALLEL, FS = ZD_F_FRAME_SERIAL;
  const uint64_t NONE = UINT64_MAX;
  int r = 0;
  if ((r = run_case("forced", dict_ctx(DJ | BP, 5000, 1, 0, true), 1, 200, NONE))) return r;
  if ((r = run_case("noflag", dict_ctx(BP | ZD_F_AUTO_EXECUTOR, 5000, 1, 1, true), 1, 200, NONE))) return r;
  if ((r = run_case("serial", dict_ctx(DJ | FS, 5000, 1, 0, true), 3, 300000, NONE))) return r;
  if ((r = run_case("both", dict_ctx(DJ | BP | FS, 5000, 1, 0, true), 3, 300000, NONE))) return r;
  if ((r = run_case("auto6_3", dict_ctx(DJ, 5000, 6, 1, true), 3, 300000, NONE))) return r;
  if ((r = run_case("auto6_1", dict_ctx(DJ, 5000, 6, 1, true), 1, 200, NONE))) return r;
  if ((r = run_case("auto65_3", dict_ctx(DJ, 5000, 65, 1, true), 3, 300000, NONE))) return r;
  if ((r = run_case("auto65_4", dict_ctx(DJ, 5000, 65, 1, true), 4, 400000, NONE))) return r;
  if ((r = run_case("auto_at_cap", dict_ctx(DJ, 5000, 6, ZD_AUTO_DICT_MAX_CANDIDATES, true), 3, 300000, NONE)))
    return r;
  if ((r = run_case("auto_cap", dict_ctx(DJ, 5000, 6, ZD_AUTO_DICT_MAX_CANDIDATES + 1, true), 3, 300000, NONE)))
    return r;
  static_assert(ZD_AUTO_DICT_MAX_CANDIDATES <= ZD_AUTO_MAX_CANDIDATES, "the dictionary plans' cap is the tighter one");
  const uint64_t GIB = 1ull << 30;
  const uint32_t GIB_B = (uint32_t)(GIB / MAX_BLOCK_OUT);
  if ((r = run_case("b_auto", dict_ctx(DJ, GIB, 1, 0, true), GIB_B, GIB, NONE))) return r;
  if ((r = run_case("b_serial", dict_ctx(DJ | FS, GIB, 1, 0, true), GIB_B, GIB, NONE))) return r;
  if ((r = run_case("b_noflag", dict_ctx(0, GIB, 1, 0, true), GIB_B, GIB, NONE))) return r;
  // a set plan: the plan-wide fields are another dictionary's, so every value printed is the entry's own
  const PlanDict tab[3] = {
      {0, -1, 3000, {1, 4, 8}},
      {7, 0, 9000, {5, 6, 7}},
      {70000, 1, 16384, {21, 22, 23}},
  };
  PlanCtx SX = dict_ctx(DJ | BP, 5000, 1, 0, true);
  SX.dset = tab;
  SX.ndset = 3;
  SX.dset_fallback = -1;
  if ((r = run_case("set_named", SX, 1, 200, 70000))) return r;
  if ((r = run_case("set_none", SX, 1, 200, NONE))) return r;
  if ((r = run_case("set_missing", SX, 1, 200, 8))) return r;
  PlanCtx SN = dict_ctx(BP, 5000, 1, 0, true);
  SN.dset = tab;
  SN.ndset = 3;
  SN.dset_fallback = -1;
  if ((r = run_case("set_noflag", SN, 1, 200, 70000))) return r;

  // the route functions that were there before the flag answer as they did, with the bit set too
  RouteEnv E;
  const uint32_t ALL = DJ | BP | ZD_F_AUTO_EXECUTOR;
  if (k4j_mode_of(DJ, E) != -1 || k4j_mode_of(ALL, E) != 1) return 5;
  if (k4j_mode_behind(1, ALL, true, false, false) != 0 || k4j_mode_behind(1, ALL, true, true, false) != 1) return 5;
  if (k4j_mode_plan(1, ALL, true, false, false) != 0 || chain_j(DJ, true)) return 5;
  if (auto_exec(ALL, false, false) || auto_exec(DJ, true, false) || !auto_exec(DJ | ZD_F_AUTO_EXECUTOR, true, false))
    return 5;
  if (plan_k4j_min(DJ, false, false, 6, 6) != K4J_MIN_BLOCKS_FEW || plan_k4j_min(DJ, false, false, 65, 65) != K4J_MIN_BLOCKS)
    return 5;
  if (plan_k4j_counts(DJ, E, false, false, 5000) || !plan_k4j_counts(DJ, E, false, false, 0)) return 5;
  // (a prefix or chain batch is no dictionary plan for the flag, and neither is a plain plan)
  if (dict_j(DJ, false) || !dict_j(DJ, true) || dict_j(BP, true)) return 5;
  if (dict_j_mode(DJ) != -1 || dict_j_mode(DJ | BP) != 1 || dict_j_mode(DJ | BP | FS) != 0) return 5;
  // a dictionary plan's fields by the old signature, whatever its flags: streaming only
  const PlanCtx OLD = dict_ctx(ALL, 5000, 6, 1, false);
  if (OLD.dict_j || OLD.k4j_mode != 0 || OLD.auto_exec || OLD.k4j_auto) return 5;
  if ((r = run_case("old_fields", OLD, 3, 300000, NONE))) return r;
  return 0;
}
