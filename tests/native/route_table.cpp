// Prints the routing resolvers of zstd-decompressor_amd/csrc/zd_route.h over a
// grid of plan shapes, flags, profiling modes and overrides, one line a case
// (tests/test_launch_route.py holds the expected table).  Host only: the
// header compiles without HIP.
//   L <inputs> <env> : <launch_route> : <route_plan bits>
//   P <inputs> <env> : <plan_route> <plan_fused> <k4j_mode_of>
#include <cstdio>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_route.h"
using namespace zd;

static const char* k1_name(K1Kind k) {
  switch (k) {
    case K1_LANES_BOTH: return "lanes_both";
    case K1_LANES_TWO: return "lanes_two";
    case K1_LANES_SEQW: return "lanes_seqw";
    case K1_SPLIT_BOTH: return "split_both";
    case K1_SPLIT_TWO: return "split_two";
    case K1_HUF_LANES: return "huf_lanes";
    case K1_HUF_SPLIT: return "huf_split";
  }
  return "?";
}
static const char* k3_name(K3Kind k) { return k == K3_ONE_LANE ? "one_lane" : k == K3_Q ? "q" : k == K3_L ? "l" : "?"; }
static const char* k4_name(K4Kind k) { return k == K4_PLAIN ? "plain" : k == K4_DICT ? "dict" : k == K4_DICT_SET ? "dicts" : "?"; }

static void print_env(const RouteEnv& E) {
  printf(" %d %d %d %d %d %lld %d %d %d", E.fuse, E.k4f, E.fork, E.k1fork, E.k3l, (long long)E.k1w_max, E.k4j, E.j_hops,
         E.j_hops2);
}

int main() {
  // the default, each variable forced to 0 and to 1 in turn, ZD_K1W_MAX at -1 (as not set), 0 and 1 << 30
  std::vector<RouteEnv> envs(1);
  int RouteEnv::* const vars[] = {&RouteEnv::fuse, &RouteEnv::k4f,    &RouteEnv::fork,   &RouteEnv::k1fork,
                                  &RouteEnv::k3l,  &RouteEnv::k4j,    &RouteEnv::j_hops, &RouteEnv::j_hops2};
  for (auto v : vars)
    for (int x = 0; x < 2; x++) { RouteEnv E; E.*v = x; envs.push_back(E); }
  for (long long x : {-1ll, 0ll, 1ll << 30}) { RouteEnv E; E.k1w_max = x; envs.push_back(E); }
  const uint32_t flag_set[] = {0, ZD_F_SEQ_ONE_LANE, ZD_F_SEQ_NO_LATENCY, ZD_F_NO_FUSE, ZD_F_K1_SPLIT, ZD_F_K1_LANES,
                               ZD_F_BLOCK_PARALLEL, ZD_F_FRAME_SERIAL, ZD_F_J_ONE_ROUND};
  for (uint32_t cus : {80u, 256u}) {
    const uint64_t nfs[] = {1, cus - 1, cus, 3ull * cus, 4ull * cus, 4ull * cus + 1, 40ull * cus, 320ull * cus};
    for (uint64_t nf : nfs)
      for (uint32_t flags : flag_set)
        for (size_t e = 0; e < envs.size(); e++) {
          const RouteEnv& E = envs[e];
          // the launch: every count from {0, n, 2n} under the default overrides; under an override it
          // reads, three mixes and the flags that meet an override; under any other, one shape
          const bool plan_env = E.fuse >= 0 || E.k4f >= 0 || E.k4j >= 0;
          const bool few_flags = flags == 0 || flags == ZD_F_SEQ_ONE_LANE || flags == ZD_F_SEQ_NO_LATENCY ||
                                 flags == ZD_F_K1_LANES || flags == ZD_F_J_ONE_ROUND;
          for (int c = 0; c < 27; c++) {
            const uint64_t nt = nf * (c % 3), nh = nf * (c / 3 % 3), ns = nf * (c / 9);
            if (e && !(c == 14 || ((c == 11 || c == 0) && !plan_env))) continue;
            if (e && (plan_env ? flags != 0 : !few_flags)) continue;
            for (int fused = 0; fused < 2; fused++)
              for (int prof = 0; prof < (plan_env ? 1 : e ? 2 : 3); prof++)
                for (int k4 = 0; k4 < ((e || flags || prof) ? 1 : 3); k4++) {
                  LaunchIn in{};
                  in.cus = cus; in.n_frames = nf; in.n_tables = nt; in.n_huf = nh; in.n_seq = ns;
                  in.flags = flags; in.fused = fused != 0; in.k4 = (K4Kind)k4; in.profiling = prof;
                  const LaunchRoute R = launch_route(in, E);
                  RouteIn ri{};
                  ri.cus = cus; ri.nframes = nf; ri.n_tables = nt; ri.n_seq = ns; ri.n_huf = nh;
                  ri.single_block_frames = fused != 0; ri.flags = flags;
                  const Route r = route_plan(ri);
                  printf("L %u %llu %llu %llu %llu %u %d %s %d", cus, (unsigned long long)nf, (unsigned long long)nt,
                         (unsigned long long)nh, (unsigned long long)ns, flags, fused, k4_name(in.k4), prof);
                  print_env(E);
                  printf(" : %d %d %d %d %d %s %s %s %u %u : %d %d %d %d %d %d %d\n", R.fused, R.fork, R.k1_fork,
                         R.profiling == 1, R.profiling == 2, k1_name(R.k1), k3_name(R.k3), k4_name(R.k4), R.j_hops,
                         R.j_hops2, r.fused, r.k4f, r.k1_seq_waves, r.fork, r.k1_fork, r.k1_split, r.k3_lat);
                }
          }
          // the plan (under the overrides it reads): single-block frames or not; a plain plan, a context
          // plan, a dictionary plan
          if (e && !plan_env) continue;
          for (int single = 0; single < 2; single++)
            for (int kind = 0; kind < 3; kind++) {
              RouteIn ri{};
              ri.cus = cus; ri.nframes = nf; ri.n_tables = 2 * nf; ri.n_seq = nf; ri.n_huf = nf;
              ri.single_block_frames = single != 0; ri.context = kind != 0; ri.flags = flags;
              const PlanRoute p = plan_route(ri, kind == 2, E);
              printf("P %u %llu %u %d %d", cus, (unsigned long long)nf, flags, single, kind);
              print_env(E);
              printf(" : %d %d %d %d %d\n", p.fused, p.k4f, plan_fused(p.fused, 0, 0),
                     plan_fused(p.fused, 1, 0) || plan_fused(p.fused, 0, 1), k4j_mode_of(flags, E));
            }
        }
  }
  return 0;
}
