// Host driver of the multi-frame batch's rule (zd_multi.h: MultiWalk cuts a
// chunk into sub-chunks, MultiPlace puts each in place or into the staging
// buffer, multi_size_query sums the reserves), the code zd_k_multi_count,
// zd_k_multi_fill and zd_k_multi_sizes run one lane a chunk; no GPU needed.
// Hand-made chunks, each copied into a heap block of exactly its size so that
// a read past either end is a sanitizer report, with the expected sub-chunks
// written down here as literals.
// Prints "ok <chunks> <sub-chunks>" and exits 0, or names the first difference
// and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_multi.h"

using namespace zd;
typedef std::vector<uint8_t> V;

static V cat(std::initializer_list<V> parts) {
  V r;
  for (const V& p : parts) r.insert(r.end(), p.begin(), p.end());
  return r;
}
static const V MAGIC = {0x28, 0xB5, 0x2F, 0xFD};
// single segment, a one-byte Frame_Content_Size
static V hdr_fcs(uint8_t fcs) { return cat({MAGIC, {0x20, fcs}}); }
// a window descriptor (1 KiB), no Frame_Content_Size
static V hdr_nofcs() { return cat({MAGIC, {0x00, 0x00}}); }
static V bhdr(uint32_t size, int type, bool last) {
  const uint32_t x = (last ? 1u : 0u) | ((uint32_t)type << 1) | (size << 3);
  return {(uint8_t)x, (uint8_t)(x >> 8), (uint8_t)(x >> 16)};
}
static V raw(uint32_t n, bool last) {
  V r = bhdr(n, 0, last);
  for (uint32_t i = 0; i < n; i++) r.push_back((uint8_t)(0x30 + i));
  return r;
}
// a compressed block: a Raw literals section of k bytes (k < 32), no sequences
static V comp(uint32_t k, bool last) {
  V r = bhdr(k + 2, 2, last);
  r.push_back((uint8_t)(k << 3));
  for (uint32_t i = 0; i < k; i++) r.push_back((uint8_t)(0x61 + i));
  r.push_back(0);
  return r;
}
static V skippable(uint32_t n) {
  V r = {0x53, 0x2A, 0x4D, 0x18, (uint8_t)n, (uint8_t)(n >> 8), 0, 0};
  for (uint32_t i = 0; i < n; i++) r.push_back((uint8_t)(7 * i + 3));
  return r;
}
static V cut(V v, size_t n) { v.resize(n); return v; }

constexpr uint64_t NONE = ~0ull;
struct Sub {
  uint64_t begin, end;
  int status;
  uint64_t reserve;
  int exact;
  uint64_t offset;   // in place: its offset in the destination; NONE: staged
  uint64_t stage;    // staged: its staging offset in the chunk; NONE: in place
  uint64_t cap;
  uint64_t pieces;
};
struct Case {
  const char* name;
  V chunk;
  uint64_t dst_cap;
  std::vector<Sub> subs;
  // the size query
  int status;
  uint64_t reserve;
  int exact;
  // the chunk's staging bytes
  uint64_t staged_bytes;
};

int main() {
  const V A = cat({hdr_fcs(5), raw(5, true)});          // 14 bytes, Frame_Content_Size 5
  const V B = cat({hdr_fcs(9), raw(9, true)});          // 18 bytes, Frame_Content_Size 9
  const V N = cat({hdr_nofcs(), raw(7, true)});         // 16 bytes, none: its bound is 7
  const V C = cat({hdr_nofcs(), comp(3, true)});        // 14 bytes, none: its bound is 131,072
  const V S = skippable(4);                             // 12 bytes
  const V bad3 = cat({hdr_fcs(5), bhdr(5, 3, true), {1, 2, 3, 4, 5}});   // 14 bytes, a reserved block type
  const int NEB = ZD_E_NOT_ENOUGH_BYTES, MAG = ZD_E_UNRECOGNIZED_MAGIC, RBT = ZD_E_RESERVED_BLOCK_TYPE;
  const std::vector<Case> cases = {
      {"no bytes", V{}, 100, {{0, 0, 0, 0, 0, 0, NONE, 100, 0}}, 0, 0, 0, 0},
      {"skippable frames only", cat({S, S}), 100, {{0, 24, 0, 0, 0, 0, NONE, 100, 0}}, 0, 0, 0, 0},
      {"one frame, FCS", A, 100, {{0, 14, 0, 5, 1, 0, NONE, 5, 0}}, 0, 5, 1, 0},
      {"one frame, no FCS", N, 100, {{0, 16, 0, 7, 0, 0, NONE, 100, 0}}, 0, 7, 0, 0},
      {"two frames, FCS", cat({A, B}), 100, {{0, 14, 0, 5, 1, 0, NONE, 5, 0}, {14, 32, 0, 9, 1, 5, NONE, 9, 0}}, 0, 14, 1, 0},
      {"two frames, the first without FCS", cat({N, A}), 100,
       {{0, 16, 0, 7, 0, 0, NONE, 100, 0}, {16, 30, 0, 5, 1, NONE, 0, 5, 1}}, 0, 12, 0, 16},
      {"two frames, the last without FCS", cat({A, N}), 100,
       {{0, 14, 0, 5, 1, 0, NONE, 5, 0}, {14, 30, 0, 7, 0, 5, NONE, 95, 0}}, 0, 12, 0, 0},
      {"five frames, FCS", cat({A, B, A, B, A}), 100,
       {{0, 14, 0, 5, 1, 0, NONE, 5, 0}, {14, 32, 0, 9, 1, 5, NONE, 9, 0}, {32, 46, 0, 5, 1, 14, NONE, 5, 0},
        {46, 64, 0, 9, 1, 19, NONE, 9, 0}, {64, 78, 0, 5, 1, 28, NONE, 5, 0}}, 0, 33, 1, 0},
      {"five frames, the first without FCS", cat({N, A, B, A, B}), 100,
       {{0, 16, 0, 7, 0, 0, NONE, 100, 0}, {16, 30, 0, 5, 1, NONE, 0, 5, 1}, {30, 48, 0, 9, 1, NONE, 16, 9, 1},
        {48, 62, 0, 5, 1, NONE, 32, 5, 1}, {62, 80, 0, 9, 1, NONE, 48, 9, 1}}, 0, 35, 0, 64},
      {"five frames, the middle one without FCS", cat({A, B, N, A, B}), 100,
       {{0, 14, 0, 5, 1, 0, NONE, 5, 0}, {14, 32, 0, 9, 1, 5, NONE, 9, 0}, {32, 48, 0, 7, 0, 14, NONE, 86, 0},
        {48, 62, 0, 5, 1, NONE, 0, 5, 1}, {62, 80, 0, 9, 1, NONE, 16, 9, 1}}, 0, 35, 0, 32},
      {"five frames, the last without FCS", cat({A, B, A, B, N}), 100,
       {{0, 14, 0, 5, 1, 0, NONE, 5, 0}, {14, 32, 0, 9, 1, 5, NONE, 9, 0}, {32, 46, 0, 5, 1, 14, NONE, 5, 0},
        {46, 64, 0, 9, 1, 19, NONE, 9, 0}, {64, 80, 0, 7, 0, 28, NONE, 72, 0}}, 0, 35, 0, 0},
      {"a compressed block without FCS in front: 128 KiB staged behind it", cat({C, C, A}), 1 << 20,
       {{0, 14, 0, 131072, 0, 0, NONE, 1 << 20, 0}, {14, 28, 0, 131072, 0, NONE, 0, 131072, 4},
        {28, 42, 0, 5, 1, NONE, 131072, 5, 1}}, 0, 262149, 0, 131088},
      {"skippable frames between and behind", cat({S, A, S, B, S}), 100,
       {{0, 26, 0, 5, 1, 0, NONE, 5, 0}, {26, 56, 0, 9, 1, 5, NONE, 9, 0}, {56, 68, 0, 0, 0, 14, NONE, 86, 0}}, 0, 14,
       0, 0},
      {"skippable frames behind a frame without FCS: staged, of no bytes", cat({N, S}), 100,
       {{0, 16, 0, 7, 0, 0, NONE, 100, 0}, {16, 28, 0, 0, 0, NONE, 0, 0, 0}}, 0, 7, 0, 0},
      {"three trailing bytes", cat({A, B, {1, 2, 3}}), 100,
       {{0, 14, 0, 5, 1, 0, NONE, 5, 0}, {14, 32, 0, 9, 1, 5, NONE, 9, 0}, {32, 35, NEB, 0, 0, 14, NONE, 86, 0}}, NEB,
       14, 0, 0},
      {"four trailing bytes", cat({A, B, {1, 2, 3, 4}}), 100,
       {{0, 14, 0, 5, 1, 0, NONE, 5, 0}, {14, 32, 0, 9, 1, 5, NONE, 9, 0}, {32, 36, MAG, 0, 0, 14, NONE, 86, 0}}, MAG,
       14, 0, 0},
      {"four garbage bytes and nothing else", V{1, 2, 3, 4}, 100, {{0, 4, MAG, 0, 0, 0, NONE, 100, 0}}, MAG, 0, 0, 0},
      {"the last frame cut by three bytes", cat({A, cut(B, 15)}), 100,
       {{0, 14, 0, 5, 1, 0, NONE, 5, 0}, {14, 29, NEB, 0, 0, 5, NONE, 95, 0}}, NEB, 5, 0, 0},
      {"the only frame cut by three bytes", cut(A, 11), 100, {{0, 11, NEB, 0, 0, 0, NONE, 100, 0}}, NEB, 0, 0, 0},
      {"a reserved block type in the middle frame: it and everything behind it", cat({A, bad3, B}), 100,
       {{0, 14, 0, 5, 1, 0, NONE, 5, 0}, {14, 46, RBT, 0, 0, 5, NONE, 95, 0}}, RBT, 5, 0, 0},
      {"a reserved block type behind a frame without FCS: staged", cat({N, S, bad3, B}), 100,
       {{0, 16, 0, 7, 0, 0, NONE, 100, 0}, {16, 60, RBT, 0, 0, NONE, 0, 0, 0}}, RBT, 7, 0, 0},
      {"an offset past dst_cap", cat({A, B, A, N}), 8,
       {{0, 14, 0, 5, 1, 0, NONE, 5, 0}, {14, 32, 0, 9, 1, 5, NONE, 3, 0}, {32, 46, 0, 5, 1, 14, NONE, 0, 0},
        {46, 62, 0, 7, 0, 19, NONE, 0, 0}}, 0, 26, 0, 0},
      {"an offset at dst_cap", cat({A, B}), 5, {{0, 14, 0, 5, 1, 0, NONE, 5, 0}, {14, 32, 0, 9, 1, 5, NONE, 0, 0}}, 0,
       14, 1, 0},
      {"no destination", cat({A, N, A}), 0,
       {{0, 14, 0, 5, 1, 0, NONE, 0, 0}, {14, 30, 0, 7, 0, 5, NONE, 0, 0}, {30, 44, 0, 5, 1, NONE, 0, 5, 1}}, 0, 17, 0,
       16},
  };
  size_t n = 0, nsub = 0;
  for (const Case& c : cases) {
    // exactly the chunk's bytes on the heap: redzones either side under AddressSanitizer
    uint8_t* p = new uint8_t[c.chunk.size()];
    if (!c.chunk.empty()) memcpy(p, c.chunk.data(), c.chunk.size());
    MultiWalk w(p, c.chunk.size(), 0);
    MultiPlace place(c.dst_cap);
    MultiSub s;
    size_t k = 0;
    bool ok = true;
    while (w.next(&s)) {
      const MultiSlot o = place.place(s);
      if (k >= c.subs.size()) { ok = false; break; }
      const Sub& e = c.subs[k];
      const uint64_t offset = o.staged() ? NONE : o.offset, stage = o.staged() ? o.stage : NONE;
      const bool past = !o.staged() && o.offset > c.dst_cap;
      if (s.begin != e.begin || s.end != e.end || s.status != e.status || s.reserve != e.reserve ||
          s.exact != e.exact || offset != e.offset || stage != e.stage || o.cap != e.cap || o.pieces != e.pieces ||
          o.past != past) {
        printf("differs: %s: sub-chunk %zu: [%llu, %llu) status %d reserve %llu exact %d offset %lld stage %lld cap "
               "%llu pieces %llu past %d\n", c.name, k, (unsigned long long)s.begin, (unsigned long long)s.end,
               s.status, (unsigned long long)s.reserve, (int)s.exact, (long long)offset, (long long)stage,
               (unsigned long long)o.cap, (unsigned long long)o.pieces, (int)o.past);
        ok = false;
        break;
      }
      k++;
    }
    if (ok && (k != c.subs.size() || w.k != k || place.stage_bytes != c.staged_bytes)) {
      printf("differs: %s: %zu sub-chunks (want %zu), %llu staging bytes (want %llu)\n", c.name, k, c.subs.size(),
             (unsigned long long)place.stage_bytes, (unsigned long long)c.staged_bytes);
      ok = false;
    }
    uint64_t reserve = 77;
    uint8_t exact = 77;
    const int st = multi_size_query(p, c.chunk.size(), 0, &reserve, &exact);
    delete[] p;
    if (!ok) return 1;
    if (st != c.status || reserve != c.reserve || exact != c.exact) {
      printf("differs: %s: size query: status %d (want %d), reserve %llu (want %llu), exact %d (want %d)\n", c.name,
             st, c.status, (unsigned long long)reserve, (unsigned long long)c.reserve, (int)exact, c.exact);
      return 1;
    }
    n++;
    nsub += k;
  }
  // a chunk of one frame: the size query is chunk_size_query's
  for (const V& one : {A, N, C, cat({S, A, S})}) {
    uint64_t r0 = 1, r1 = 2;
    uint8_t e0 = 3, e1 = 4;
    const int s0 = chunk_size_query(one.data(), one.size(), 0, &r0, &e0);
    const int s1 = multi_size_query(one.data(), one.size(), 0, &r1, &e1);
    // (skippable frames behind the frame are a sub-chunk of their own, which is not exact)
    const bool trailing = one.size() == S.size() + A.size() + S.size();
    if (s0 != s1 || r0 != r1 || (e0 != e1 && !trailing)) {
      printf("differs: a chunk of one frame against chunk_size_query\n");
      return 1;
    }
  }
  // the entries zd_k_batch_layout refuses
  if (!multi_entry_refused(0, 1, 16, 1) || !multi_entry_refused(16, 1, 0, 1) || !multi_entry_refused(~0ull, 2, 16, 1) ||
      !multi_entry_refused(16, 1, ~0ull, 2) || !multi_entry_refused(16, 1ull << 32, 16, 1) ||
      multi_entry_refused(0, 0, 0, 0) || multi_entry_refused(16, 1, 0, 0) || multi_entry_refused(16, 0xFFFFFFFFull, 16, 1)) {
    printf("differs: multi_entry_refused\n");
    return 1;
  }
  printf("ok %zu %zu\n", n, nsub);
  return 0;
}
