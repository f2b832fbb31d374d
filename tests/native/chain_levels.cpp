// Host driver of the chain batch's level rule (zd_chain.h chain_level /
// chain_order: what zd_batch_create_chain checks and groups with, and what
// zd_k_chain_levels runs one lane per chunk), no GPU needed.  Builds with g++,
// also as a stand-alone program under -fsanitize=address,undefined.
// One line per case:
//   name  n  invalid chunks  levels in use  level of the last chunk (-1: invalid)  props
// props = 1 when order[] is a permutation of 0..n-1 grouped by ascending level
// (an invalid chunk counts as level 0), count[] sums to n and matches the
// levels.  The random forests are checked against a naive recursive reference
// here; their line carries the number of forests that agreed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_chain.h"

using namespace zd;

struct Out {
  std::vector<int32_t> level;
  std::vector<uint32_t> order;
  uint32_t count[CHAIN_LEVELS];
  uint64_t bad;
  bool props;
  uint32_t levels;
};

static Out run(const std::vector<int64_t>& parent) {
  const size_t n = parent.size();
  // exact-size heap copies, so that a sanitizer sees any index outside [0, n)
  int64_t* p = (int64_t*)malloc(n ? n * sizeof(int64_t) : 1);
  for (size_t i = 0; i < n; i++) p[i] = parent[i];
  Out o;
  o.level.assign(n, -7);
  o.order.assign(n, 0xFFFFFFFFu);
  o.bad = chain_order(p, n, o.level.data(), o.order.data(), o.count);
  free(p);
  uint64_t sum = 0;
  o.levels = 1;
  for (uint32_t l = 0; l < CHAIN_LEVELS; l++) {
    sum += o.count[l];
    if (o.count[l]) o.levels = l + 1;
  }
  bool ok = sum == n;
  std::vector<uint8_t> seen(n, 0);
  std::vector<uint32_t> per(CHAIN_LEVELS, 0);
  int32_t last = 0;
  uint64_t bad = 0;
  for (size_t k = 0; k < n && ok; k++) {
    const uint32_t i = o.order[k];
    if (i >= n || seen[i]) { ok = false; break; }
    seen[i] = 1;
    const int32_t l = o.level[i] == CHAIN_INVALID ? 0 : o.level[i];
    if (l < last || l < 0 || l >= (int32_t)CHAIN_LEVELS) ok = false;
    last = l;
    per[l]++;
  }
  for (size_t i = 0; i < n; i++) bad += o.level[i] == CHAIN_INVALID;
  for (uint32_t l = 0; l < CHAIN_LEVELS && ok; l++) ok = per[l] == o.count[l];
  o.props = ok && bad == o.bad;
  return o;
}

static void line(const char* name, const std::vector<int64_t>& parent) {
  const Out o = run(parent);
  printf("%s %zu %llu %u %d %d\n", name, parent.size(), (unsigned long long)o.bad, o.levels,
         parent.empty() ? 0 : o.level.back(), o.props ? 1 : 0);
}

// the naive reference: levels by recursion over valid entries, -1 where the
// recursion meets a chunk again (a cycle, or a tail behind one) or passes the depth limit
static int32_t ref_level(const std::vector<int64_t>& parent, size_t i, std::vector<uint8_t>& on_path, uint32_t depth) {
  const int64_t n = (int64_t)parent.size(), p = parent[i];
  const bool bad = p < -1 || p >= n || p == (int64_t)i;
  if ((depth == 0 && bad) || depth > CHAIN_MAX_DEPTH) return -1;
  if (p == -1 || bad) return 0;
  if (on_path[i]) return -1;
  on_path[i] = 1;
  const int32_t up = ref_level(parent, (size_t)p, on_path, depth + 1);
  on_path[i] = 0;
  return up < 0 ? -1 : up + 1;
}

int main() {
  line("root", {-1});
  {
    std::vector<int64_t> p(256);
    for (size_t i = 0; i < p.size(); i++) p[i] = (int64_t)i - 1;
    line("line256", p);
    p.push_back(255);
    line("line257", p);
  }
  line("self", {-1, 1});
  line("cycle2", {-1, 2, 1});
  line("cycle3", {-1, 3, 1, 2});
  line("tail_behind_cycle", {2, 0, 1, 2, 3});        // 0 -> 2 -> 1 -> 0, then 3 -> 2, 4 -> 3
  line("parent_n", {-1, 0, 3});
  line("parent_minus2", {-1, 0, -2});
  line("child_of_bad_entry", {7, 0, 1});             // chunk 0 names no chunk; 1 and 2 hang off it
  line("child_before_parent", {1, 2, -1});
  {
    std::vector<int64_t> p(1001, 0);
    p[0] = -1;
    line("star1000", p);
  }
  // 200 random forests (xorshift, fixed seed), some with bad entries and cycles
  uint64_t x = 0x9E3779B97F4A7C15ull;
  auto rnd = [&x]() { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  uint32_t agree = 0;
  for (int t = 0; t < 200; t++) {
    const size_t n = 1 + (size_t)(rnd() % 600);
    std::vector<int64_t> p(n);
    for (size_t i = 0; i < n; i++) {
      const uint64_t r = rnd() % 100;
      if (r < 25) p[i] = -1;
      else if (t % 4 == 3 && r < 28) p[i] = (int64_t)(rnd() % (n + 3)) - 2;     // anything, bad entries and cycles included
      else if (t % 2) p[i] = i ? (int64_t)(rnd() % i) : -1;                     // an earlier chunk: deep lines
      else p[i] = (int64_t)(rnd() % n) == (int64_t)i ? -1 : (int64_t)(rnd() % n);
    }
    const Out o = run(p);
    bool ok = o.props;
    std::vector<uint8_t> on_path(n, 0);
    for (size_t i = 0; i < n && ok; i++) ok = o.level[i] == ref_level(p, i, on_path, 0);
    agree += ok;
  }
  printf("forests 200 0 0 0 %d\n", agree == 200 ? 1 : 0);
  printf("forests_agreeing %u 0 0 0 1\n", agree);
  return 0;
}
