// zd_route.h — which kernels a plan launches and on which stream: pure host
// functions (no HIP, no global state) of the plan's shape and flags, the CU
// count and the overrides.  route_plan: the shape rules (zd_route); plan_route:
// what a plan is built for; launch_route: all that launch_pipeline branches on.
#pragma once
#include <stdint.h>
#include <stdlib.h>

#include <algorithm>

#include "../../include/zd.h"

namespace zd {

// Executor routing (zd_route, a pure function of the plan's shape and the
// device's CU count; every bound below is in units of the CU count, measured
// on the 256-CU MI355X):
// * K4F takes one workgroup per CU: rounds of one frame per CU at ~0.21 ms
//   each against the streaming K4's one round (~0.75 ms) of up to 16 frames
//   per CU, so it pays for up to three rounds (scripts/exp_thresholds.sh:
//   8192 frames 12.1 vs 7.7 ms per step): plans of 1-3 frames per CU.
// * zd_k_fused holds four frames per workgroup and at most one workgroup per
//   CU beside K2 (which its K4 waves wait for): plans of 1-4 single-block
//   frames per CU (C3: 763 frames).
// * K1's sequence half one wave per block (zd_k_tables_seqw) while the plan
//   fits one round of 64 tables per CU (scripts/r3_k1wmax.sh: one rank's C4
//   share at 8 GPUs, 10,240 blocks, +1 %; full C4, 81,920 blocks, -1 %).
// * K2 beside K3 (the fork) where K3's last round of chains (64 per CU)
//   leaves LDS for K2: the round's fill f = (blocks mod 64 CUs) / (64 CUs),
//   measured with K3Q on C4-shaped plans (value, no fork -> fork): 10,240
//   blocks (f 0.63) 194 -> 221 GB/s, 20,480 (0.25) 211 -> 234, 40,960 (0.5)
//   247 -> 253; 12,288 (0.75) 221 -> 210, 16,384 (0) 251 -> 214, 32,768 (0)
//   266 -> 250, 81,920 (0) 273 -> 268; 763 (C3) and 8,192 (0.5) fork.  So
//   fork when 0 < f <= 0.65 (and at least one block per CU).
// * Without the fork, K1's two halves on the two streams (C4 273.3 -> 274.0).
struct RouteIn {
  uint32_t cus;
  uint64_t nframes, n_tables, n_seq, n_huf;
  bool single_block_frames;      // every frame a zstd frame of one compressed block, no host-found error
  bool context;                  // a DecodingContext plan (existing output or prebuilt tables)
  uint32_t flags;                // ZD_F_*
};
struct Route {
  bool fused = false, k4f = false, k1_seq_waves = false, fork = false, k1_fork = false, k3_lat = false;
  bool k1_split = false;
};
constexpr uint32_t K4F_MIN_PER_CU = 1, K4F_MAX_PER_CU = 3;
constexpr uint32_t FUSE_MIN_PER_CU = 1, FUSE_MAX_PER_CU = 4;
constexpr uint32_t K1W_MAX_PER_CU = 64;
constexpr uint32_t K3_CHAINS_PER_CU = 64;
// K3L (one chain per wave, latency-first) while its waves fit two a SIMD:
// beyond that K3Q's 16 chains a wave win on issue
constexpr uint32_t K3L_MAX_PER_CU = 8;
constexpr double FORK_MAX_FILL = 0.65;
// What the fused kernel needs of a plan, whatever its size
inline bool fusable(const RouteIn& in) {
  return !(in.flags & (ZD_F_NO_FUSE | ZD_F_SEQ_ONE_LANE | ZD_F_BLOCK_PARALLEL)) && !in.context &&
         in.single_block_frames;
}
inline Route route_plan(const RouteIn& in) {
  Route r;
  const uint64_t cus = std::max<uint32_t>(in.cus, 1);
  r.fused = fusable(in) && in.nframes >= FUSE_MIN_PER_CU * cus && in.nframes <= FUSE_MAX_PER_CU * cus;
  r.k4f = !r.fused && in.nframes >= K4F_MIN_PER_CU * cus && in.nframes <= K4F_MAX_PER_CU * cus;
  r.k1_seq_waves = in.n_tables <= K1W_MAX_PER_CU * cus && !(in.flags & ZD_F_K1_LANES);
  r.k1_split = (in.flags & ZD_F_K1_SPLIT) || (in.n_tables > K1W_MAX_PER_CU * cus && !(in.flags & ZD_F_K1_LANES));
  const uint64_t slots = K3_CHAINS_PER_CU * cus, rem = in.n_seq % slots;
  r.fork = in.n_seq >= cus && rem != 0 && (double)rem <= FORK_MAX_FILL * (double)slots;
  r.k1_fork = !r.fork && in.n_huf && in.n_seq;
  r.k3_lat = in.n_seq <= K3L_MAX_PER_CU * cus && !(in.flags & (ZD_F_SEQ_ONE_LANE | ZD_F_SEQ_NO_LATENCY));
  return r;
}

// The environment overrides (experiments only; -1: not set; 1 / 0 forces a route
// on / off, ZD_FUSE=1 on any plan of single-block frames).  The library reads
// them once per process (route_env, zd_host.cpp); nothing else in csrc/ reads one.
struct RouteEnv {
  int fuse = -1, k4f = -1, fork = -1, k1fork = -1, k3l = -1, k4j = -1, j_hops = -1, j_hops2 = -1;
  int64_t k1w_max = -1;
  static RouteEnv from_process() {
    auto get = [](const char* n) { const char* e = getenv(n); return e ? atoi(e) : -1; };
    auto hops = [](const char* n) { const char* e = getenv(n); return e ? std::max(1, atoi(e)) : -1; };
    RouteEnv E;
    E.fuse = get("ZD_FUSE"); E.k4f = get("ZD_K4F"); E.fork = get("ZD_FORK"); E.k1fork = get("ZD_K1FORK");
    E.k3l = get("ZD_K3L"); E.k4j = get("ZD_K4J"); E.j_hops = hops("ZD_J_HOPS"); E.j_hops2 = hops("ZD_J_HOPS2");
    if (const char* e = getenv("ZD_K1W_MAX")) E.k1w_max = atoll(e);
    return E;
  }
};
// K4J's mode from the plan flags, else ZD_K4J: 1 every frame, 0 none, < 0 automatic
inline int k4j_mode_of(uint32_t flags, const RouteEnv& E) {
  return (flags & ZD_F_BLOCK_PARALLEL) ? 1 : (flags & ZD_F_FRAME_SERIAL) ? 0 : E.k4j;
}
// The mode of a plan whose frames decode behind a dictionary, a dictionary set
// or prefixes (`dict`): the streaming executor only, but for a prefix batch
// (`prefix`) that is no chain and was created with ZD_F_BLOCK_PARALLEL
inline int k4j_mode_behind(int mode, uint32_t flags, bool dict, bool prefix, bool chain) {
  return !dict ? mode : (prefix && !chain && (flags & ZD_F_BLOCK_PARALLEL) && mode == 1) ? 1 : 0;
}
// A chain batch created with ZD_F_CHAIN_BLOCK_PARALLEL: K4J for every frame
// with a compressed block, level by level (the flag means nothing anywhere else)
inline bool chain_j(uint32_t flags, bool chain) { return chain && (flags & ZD_F_CHAIN_BLOCK_PARALLEL) != 0; }
// The mode of any plan: k4j_mode_behind, with the chain case beside it
inline int k4j_mode_plan(int mode, uint32_t flags, bool dict, bool prefix, bool chain) {
  return chain_j(flags, chain) ? 1 : k4j_mode_behind(mode, flags, dict, prefix, chain);
}
// ZD_F_AUTO_EXECUTOR holds: a prefix or chain batch (`prefix`: both) without the
// forcing flags of its kind -- each frame is routed by plan_auto_j (zd_plan.h),
// the plan's mode stays 0.  The flag means nothing anywhere else.
inline bool auto_exec(uint32_t flags, bool prefix, bool chain) {
  return prefix && (flags & ZD_F_AUTO_EXECUTOR) &&
         !(flags & (chain ? ZD_F_CHAIN_BLOCK_PARALLEL : ZD_F_BLOCK_PARALLEL | ZD_F_FRAME_SERIAL));
}
// ZD_F_DICT_BLOCK_PARALLEL holds: a dictionary or dictionary-set plan or batch
// (`dictionary`: not a prefix or chain batch) created with it.  The functions
// above keep their answers for such a plan (its k4j_mode_behind stays 0): what
// it sends to K4J is dict_j_mode's -- 0 no frame (ZD_F_FRAME_SERIAL), 1 every
// frame with a compressed block (ZD_F_BLOCK_PARALLEL), < 0 each frame by
// plan_auto_j (zd_plan.h).  ZD_K4J is not read for it.
inline bool dict_j(uint32_t flags, bool dictionary) { return dictionary && (flags & ZD_F_DICT_BLOCK_PARALLEL) != 0; }
inline int dict_j_mode(uint32_t flags) {
  return (flags & ZD_F_FRAME_SERIAL) ? 0 : (flags & ZD_F_BLOCK_PARALLEL) ? 1 : -1;
}
// (the rule's candidate cap behind a dictionary: auto_candidates_ok with the dictionary plans' own constant)
inline bool auto_dict_candidates_ok(uint64_t candidates) {
  return candidates > 0 && candidates <= ZD_AUTO_DICT_MAX_CANDIDATES;
}
// A chain batch laid out for K4J level by level (J frames numbered level-major,
// launches and pend words per level): forced or automatic
inline bool chain_j_layout(uint32_t flags, bool chain) { return chain_j(flags, chain) || (chain && auto_exec(flags, true, true)); }
// The automatic rule's block minimum at a width (the chunks that execute
// together: a prefix batch's count, a chain batch's widest level)
inline uint32_t auto_min_blocks(uint64_t width) {
  return width <= ZD_AUTO_FEW_CHUNKS ? ZD_AUTO_MIN_BLOCKS_FEW : ZD_AUTO_MIN_BLOCKS;
}
inline bool auto_candidates_ok(uint64_t candidates) { return candidates > 0 && candidates <= ZD_AUTO_MAX_CANDIDATES; }

// What a plan is built for (plan_ctx).  `in` as route_plan's, its `context` set
// for a dictionary or dictionary-set plan too (`dict`): the streaming executor only.
struct PlanRoute { bool fused, k4f; };
inline PlanRoute plan_route(const RouteIn& in, bool dict, const RouteEnv& E) {
  const Route r = route_plan(in);
  PlanRoute p;
  p.fused = E.fuse == 0 ? false : E.fuse == 1 ? fusable(in) && in.nframes >= 1 : r.fused;
  p.k4f = (E.k4f >= 0 ? E.k4f == 1 : r.k4f) && !p.fused && !dict;
  return p;
}
// The plan's final `fused` bit (plan_totals): not when some frame went to K4J or K4F
inline bool plan_fused(bool routed, uint64_t n_jframes, uint64_t n_k4f) { return routed && !n_jframes && !n_k4f; }

// K1: both halves in one launch of zd_k_tables<.., 3> / the halves as <.., 1>
// and <.., 2> / <.., 1> and zd_k_tables_seqw (the sequence half one wave per
// block) / the same two as zd_k_tables_parse + _build / a fused launch (its
// sequence half runs in zd_k_fused): the Huffman half alone, lanes or split
enum K1Kind : uint8_t {
  K1_LANES_BOTH, K1_LANES_TWO, K1_LANES_SEQW, K1_SPLIT_BOTH, K1_SPLIT_TWO, K1_HUF_LANES, K1_HUF_SPLIT
};
// K3: zd_k_sequences (one lane per block) / _q (four lanes) / _l (one block per wave, few-block plans)
enum K3Kind : uint8_t { K3_ONE_LANE, K3_Q, K3_L };
// K4: zd_k_execute / _dict (LaunchArgs::dict) / _dicts (each frame's own, from the workspace's table) /
// _prefix (each frame's own caller-owned prefix, read in place with exact bounds) / _chain (a chain batch: the
// prefix kernel's body, one launch per level of the chain over that level's frames, LaunchArgs::chain_*)
enum K4Kind : uint8_t { K4_PLAIN, K4_DICT, K4_DICT_SET, K4_PREFIX, K4_CHAIN };
// Everything launch_pipeline branches on
struct LaunchRoute {
  bool fused = false;        // K1's sequence half + K3 + K4 as zd_k_fused, then the redo pass
  bool fork = false;         // K1's Huffman half and K2 on the aux stream beside K1's sequence half and K3
  bool k1_fork = false;      // no such fork: K1's halves on the two streams, joined before K2
  uint8_t profiling = 0;     // 1: an event after every kernel (LaunchArgs::events); 2: around the launch groups
  K1Kind k1 = K1_LANES_BOTH; K3Kind k3 = K3_Q; K4Kind k4 = K4_PLAIN;
  uint32_t j_hops = 6, j_hops2 = 12;   // K4J: hops per pending word in round 1 / in the sweeps after it
};
// The DecodingContext's launches (ctx_run, zd_execute_sequences): everything on one stream
inline LaunchRoute context_route() { LaunchRoute R; R.k1 = K1_LANES_BOTH; R.k3 = K3_Q; R.k4 = K4_PLAIN; return R; }

struct LaunchIn {
  uint32_t cus;                  // of the plan's device
  uint64_t n_frames, n_tables, n_huf, n_seq;
  uint32_t flags;                // ZD_F_*
  bool fused; K4Kind k4;         // plan_fused(); a dictionary / dictionary-set plan
  int profiling;                 // zd_plan_set_profiling: 0, 1 (kernels one by one: no fork, no fusion), 2
};
inline LaunchRoute launch_route(const LaunchIn& in, const RouteEnv& E) {
  const Route r = route_plan(RouteIn{in.cus, in.n_frames, in.n_tables, in.n_seq, in.n_huf, false, false, in.flags});
  const bool serial = in.profiling == 1, both = in.n_huf && in.n_seq;
  LaunchRoute R;
  R.profiling = (uint8_t)in.profiling;
  R.k4 = in.k4;
  R.fused = in.fused && !serial;
  // (a forced fused plan past FUSE_MAX_PER_CU frames per CU: K2 before it, its
  // workgroups could not find room beside the fused ones)
  const bool big_fused = in.fused && in.n_frames > FUSE_MAX_PER_CU * (uint64_t)in.cus;
  const bool fork = (E.fork >= 0 ? E.fork == 1 : r.fork) && !big_fused;
  R.fork = fork && !serial && both;
  R.k1_fork = !fork && !serial && (E.k1fork >= 0 ? E.k1fork == 1 && both : r.k1_fork) && in.n_tables;
  const bool seqw = E.k1w_max >= 0 ? in.n_tables <= (uint64_t)E.k1w_max && !(in.flags & ZD_F_K1_LANES) : r.k1_seq_waves;
  const bool two = R.fork || R.k1_fork;
  R.k1 = R.fused ? (r.k1_split ? K1_HUF_SPLIT : K1_HUF_LANES) : r.k1_split ? (two ? K1_SPLIT_TWO : K1_SPLIT_BOTH)
         : seqw  ? K1_LANES_SEQW : two ? K1_LANES_TWO : K1_LANES_BOTH;
  // K3 as four lanes per block (K3Q, default): C3 (763 blocks) 2.89 -> 2.31
  // ms, a forked 8,192-block plan 4.24 -> 2.48, full C4 13.88 -> 13.80; the
  // plan flag ZD_F_SEQ_ONE_LANE keeps the one-lane chain (same records)
  const bool lat = E.k3l >= 0 ? E.k3l == 1 && !(in.flags & (ZD_F_SEQ_ONE_LANE | ZD_F_SEQ_NO_LATENCY)) : r.k3_lat;
  R.k3 = (in.flags & ZD_F_SEQ_ONE_LANE) ? K3_ONE_LANE : lat ? K3_L : K3_Q;
  // hops per pending word and K4J round (c3s, scripts/exp_jhops.sh, K4J ms
  // with the word-per-lane rounds, round 5: 4 hops 1.91, 5 1.85, 6 1.75-1.77,
  // 7 1.76, 8 1.78-1.79, 12 1.85, 16 1.90); in the sweeps after round 1 (c3s,
  // round 6: 4 / 6 / 8 / 12 hops 3.19 / 3.09 / 3.08 / 3.06 ms a step,
  // profiles/r6_graph_replay_ab.txt).  ZD_F_J_ONE_ROUND (a test switch): one hop
  const bool one_round = (in.flags & ZD_F_J_ONE_ROUND) != 0;
  R.j_hops = one_round ? 1u : E.j_hops >= 0 ? (uint32_t)std::max(1, E.j_hops) : 6u;
  R.j_hops2 = one_round ? 1u : E.j_hops2 >= 0 ? (uint32_t)std::max(1, E.j_hops2) : 12u;
  return R;
}

}  // namespace zd
