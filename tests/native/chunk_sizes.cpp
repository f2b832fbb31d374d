// Host driver of a chunk's size query (zd_walk.h chunk_size_query: index_chunk
// over the WalkBound sink, then chunk_reserve), the code zd_k_chunk_sizes runs
// one lane a chunk and zd_k_batch_pack shares; no GPU needed.  Hand-made chunks,
// each copied into a heap block of exactly its size so that a read past either
// end is a sanitizer report, with the expected (status, reserve, exact) written
// down here as literals.
// Prints "ok <chunks>" and exits 0, or names the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <string>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_walk.h"

using namespace zd;
typedef std::vector<uint8_t> V;

static V cat(std::initializer_list<V> parts) {
  V r;
  for (const V& p : parts) r.insert(r.end(), p.begin(), p.end());
  return r;
}
static const V MAGIC = {0x28, 0xB5, 0x2F, 0xFD};
// single segment, a one-byte Frame_Content_Size (checksum: the Content_Checksum flag)
static V hdr_fcs(uint8_t fcs, bool checksum = false) { return cat({MAGIC, {(uint8_t)(0x20 | (checksum ? 4 : 0)), fcs}}); }
// a window descriptor (1 KiB), no Frame_Content_Size
static V hdr_nofcs() { return cat({MAGIC, {0x00, 0x00}}); }
// a window descriptor, a two-byte Frame_Content_Size (256 + the field)
static V hdr_fcs2(uint32_t fcs) { return cat({MAGIC, {0x40, 0x00, (uint8_t)(fcs - 256), (uint8_t)((fcs - 256) >> 8)}}); }
static V bhdr(uint32_t size, int type, bool last) {
  const uint32_t x = (last ? 1u : 0u) | ((uint32_t)type << 1) | (size << 3);
  return {(uint8_t)x, (uint8_t)(x >> 8), (uint8_t)(x >> 16)};
}
static V raw(uint32_t n, bool last) {
  V r = bhdr(n, 0, last);
  for (uint32_t i = 0; i < n; i++) r.push_back((uint8_t)(0x30 + i));
  return r;
}
static V rle(uint32_t n, bool last) { return cat({bhdr(n, 1, last), {0x41}}); }
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

struct Case {
  const char* name;
  V chunk;
  bool dict;
  int status;
  uint64_t reserve;
  int exact;
};

int main() {
  const V f5 = cat({hdr_fcs(5), raw(5, true)});                       // 4 + 2 + 3 + 5 = 14 bytes
  const V c3 = cat({hdr_nofcs(), comp(3, true)});
  const V mixed3 = cat({raw(4, false), rle(1000, false), comp(2, true)});
  const V f5sum = cat({hdr_fcs(5, true), raw(5, true)});
  const V empty_lits = cat({hdr_nofcs(), comp(0, true)});
  const std::vector<Case> cases = {
      {"FCS present", f5, false, ZD_OK, 5, 1},
      {"FCS absent", c3, false, ZD_OK, 131072, 0},
      {"FCS above the bound", cat({hdr_fcs(200), raw(5, true)}), false, ZD_OK, 5, 0},
      {"raw + RLE + compressed, no FCS", cat({hdr_nofcs(), mixed3}), false, ZD_OK, 132076, 0},
      {"raw + RLE + compressed, FCS 1006", cat({hdr_fcs2(1006), mixed3}), false, ZD_OK, 1006, 1},
      {"two compressed blocks, no FCS", cat({hdr_nofcs(), comp(1, false), comp(31, true)}), false, ZD_OK, 262144, 0},
      {"skippable frames before and after", cat({skippable(5), skippable(1), f5, skippable(11)}), false, ZD_OK, 5, 1},
      // (a skippable frame of no bytes: the reference's zero-length slice, as everywhere else)
      {"empty skippable frame after the frame", cat({f5, skippable(0)}), false, ZD_E_EMPTY_SLICE, 0, 0},
      {"skippable frames only", cat({skippable(5), skippable(3)}), false, ZD_OK, 0, 0},
      {"empty", V{}, false, ZD_OK, 0, 0},
      {"three bytes", V{0x28, 0xB5, 0x2F}, false, ZD_E_NOT_ENOUGH_BYTES, 0, 0},
      {"truncated after the magic number", cut(f5, 4), false, ZD_E_NOT_ENOUGH_BYTES, 0, 0},
      {"truncated inside the frame header", cut(f5, 5), false, ZD_E_NOT_ENOUGH_BYTES, 0, 0},
      {"truncated inside a block header", cut(f5, 8), false, ZD_E_NOT_ENOUGH_BYTES, 0, 0},
      {"truncated inside a block", cut(f5, 13), false, ZD_E_NOT_ENOUGH_BYTES, 0, 0},
      {"truncated inside a compressed block's literals", cut(c3, c3.size() - 2), false, ZD_E_NOT_ENOUGH_BYTES, 0, 0},
      {"truncated before the checksum", f5sum, false, ZD_E_MISSING_CHECKSUM, 0, 0},
      {"truncated inside the checksum", cat({f5sum, {1, 2, 3}}), false, ZD_E_MISSING_CHECKSUM, 0, 0},
      {"with its checksum", cat({f5sum, {1, 2, 3, 4}}), false, ZD_OK, 5, 1},
      {"five trailing bytes", cat({f5, {1, 2, 3, 4, 5}}), false, ZD_E_UNRECOGNIZED_MAGIC, 0, 0},
      {"three trailing bytes", cat({f5, {1, 2, 3}}), false, ZD_E_NOT_ENOUGH_BYTES, 0, 0},
      {"truncated skippable frame after the frame", cat({f5, cut(skippable(9), 12)}), false, ZD_E_NOT_ENOUGH_BYTES, 0, 0},
      {"two zstd frames", cat({f5, c3}), false, ZD_E_OUT_OF_DOMAIN, 0, 0},
      {"reserved block type", cat({hdr_fcs(5), bhdr(5, 3, true), {1, 2, 3, 4, 5}}), false, ZD_E_RESERVED_BLOCK_TYPE, 0, 0},
      {"empty Raw literals section", empty_lits, false, ZD_E_EMPTY_SLICE, 0, 0},
      {"empty Raw literals section, ZD_SIZES_DICT", empty_lits, true, ZD_OK, 131072, 0},
      {"FCS present, ZD_SIZES_DICT", f5, true, ZD_OK, 5, 1},
  };
  size_t n = 0;
  for (const Case& c : cases) {
    // exactly the chunk's bytes on the heap: redzones either side under AddressSanitizer
    uint8_t* p = new uint8_t[c.chunk.size()];
    if (!c.chunk.empty()) memcpy(p, c.chunk.data(), c.chunk.size());
    uint64_t reserve = 77;
    uint8_t exact = 77;
    const int st = chunk_size_query(p, c.chunk.size(), c.dict, &reserve, &exact);
    delete[] p;
    if (st != c.status || reserve != c.reserve || exact != c.exact) {
      printf("differs: %s: status %d (want %d), reserve %llu (want %llu), exact %d (want %d)\n", c.name, st, c.status,
             (unsigned long long)reserve, (unsigned long long)c.reserve, (int)exact, c.exact);
      return 1;
    }
    n++;
  }
  // frame_bound over an index (zd_k_batch_pack, zd_k_batch_fit) agrees with the sink
  {
    HostBlock b[3];
    zero_bytes(b, sizeof b);
    b[0].type = 0; b[0].size = 4;
    b[1].type = 1; b[1].size = 1000;
    b[2].type = 2; b[2].size = 4;
    HostFrame hf;
    zero_bytes(&hf.d, sizeof hf.d);
    hf.d.kind = ZD_FRAME_ZSTD;
    hf.d.content_size = UINT64_MAX;
    hf.b0 = 0; hf.nb = 3;
    uint8_t exact = 77;
    if (frame_bound(hf, b) != 132076 || chunk_reserve(hf, 132076, &exact) != 132076 || exact != 0) {
      printf("differs: frame_bound\n");
      return 1;
    }
    hf.key = make_key(PH_PARSE, 0, PS_STRUCT, 0, ZD_E_NOT_ENOUGH_BYTES);
    if (chunk_reserve(hf, 132076, &exact) != 0 || exact != 0) {
      printf("differs: a failed frame reserves\n");
      return 1;
    }
  }
  printf("ok %zu\n", n);
  return 0;
}
