// Host driver of the seek-table rules (zd_seek.h): the footer and header
// checks, the unaligned entry read, the sums, the clamp, the range-to-frames
// search and the part of a frame a range wants -- the code zd_seekable_open_device
// and zd_seek.hip's kernels run; no GPU needed.  Hand-made tables, each archive
// copied into a heap block of exactly its size so that a read past either end
// is a sanitizer report, with the expected verdicts and (f0, f1, clamped
// length) triples written down here as literals.
// Prints "ok <checks>" and exits 0, or names the first difference and exits 1.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_seek.h"

using namespace zd;
typedef std::vector<uint8_t> V;

static int checks = 0;
#define EXPECT(cond, ...) do { checks++; if (!(cond)) { printf("line %d: ", __LINE__); printf(__VA_ARGS__); \
  printf("\n"); exit(1); } } while (0)

static void le32(V& v, uint32_t x) { for (int k = 0; k < 4; k++) v.push_back((uint8_t)(x >> (8 * k))); }

struct Entry { uint32_t c, d, k; };

// a seek table: header, entries, footer (each field can be overridden)
static V table(const std::vector<Entry>& es, bool sums, uint32_t skip_magic = 0x184D2A5Eu, int64_t frame_size = -1,
               int64_t nframes = -1, int desc = -1, uint32_t magic = 0x8F92EAB1u) {
  V t;
  le32(t, skip_magic);
  le32(t, frame_size >= 0 ? (uint32_t)frame_size : (uint32_t)(es.size() * (sums ? 12 : 8) + 9));
  for (const Entry& e : es) { le32(t, e.c); le32(t, e.d); if (sums) le32(t, e.k); }
  le32(t, nframes >= 0 ? (uint32_t)nframes : (uint32_t)es.size());
  t.push_back(desc >= 0 ? (uint8_t)desc : (uint8_t)(sums ? 0x80 : 0));
  le32(t, magic);
  return t;
}
// `front` bytes of entries, then the table
static V archive(size_t front, const V& t) {
  V a(front, 0xEE);
  a.insert(a.end(), t.begin(), t.end());
  return a;
}

struct Opened {
  int status = 0;
  SeekFooter ft;
  std::vector<uint64_t> c_off, d_off;
  std::vector<uint32_t> sum;
};
// what zd_seekable_open_device does, on a heap block of exactly the archive's size
static Opened open_host(const V& a) {
  Opened o;
  uint8_t* p = (uint8_t*)malloc(a.size() ? a.size() : 1);
  if (!a.empty()) memcpy(p, a.data(), a.size());
  const uint64_t n = a.size();
  do {
    if (n < SEEK_MIN_BYTES) { o.status = ZD_E_NOT_ENOUGH_BYTES; break; }
    if ((o.status = seek_footer(p + n - SEEK_FOOTER_BYTES, n, &o.ft))) break;
    const uint8_t* t = p + n - o.ft.table_bytes;
    if ((o.status = seek_header(t, o.ft))) break;
    uint64_t c = 0, d = 0;
    for (uint32_t i = 0; i < o.ft.nframes; i++) {
      uint32_t cs, ds, k;
      seek_entry(t, o.ft, i, &cs, &ds, &k);
      o.c_off.push_back(c); o.d_off.push_back(d); o.sum.push_back(k);
      c += cs; d += ds;
    }
    o.c_off.push_back(c); o.d_off.push_back(d);
    o.status = seek_sums(c, n, o.ft);
  } while (0);
  free(p);
  return o;
}

struct Want { uint64_t off, len; uint32_t f0, f1; uint64_t clamped; };

static void search(const std::vector<uint64_t>& d_off, const Want& w) {
  const uint32_t F = (uint32_t)d_off.size() - 1;
  // (the sums in a heap block of exactly their size)
  uint64_t* h = (uint64_t*)malloc(8 * d_off.size());
  memcpy(h, d_off.data(), 8 * d_off.size());
  const uint64_t l = seek_clamp(w.off, w.len, h[F]);
  EXPECT(l == w.clamped, "range (%llu, %llu): clamped %llu, expected %llu", (unsigned long long)w.off,
         (unsigned long long)w.len, (unsigned long long)l, (unsigned long long)w.clamped);
  if (l) {
    uint32_t f0 = ~0u, f1 = ~0u;
    seek_frames(h, F, w.off, l, &f0, &f1);
    EXPECT(f0 == w.f0 && f1 == w.f1, "range (%llu, %llu): frames %u..%u, expected %u..%u", (unsigned long long)w.off,
           (unsigned long long)w.len, f0, f1, w.f0, w.f1);
    EXPECT(h[f0] <= w.off && w.off < h[f0 + 1] && h[f1] < w.off + l && w.off + l <= h[f1 + 1], "the search's contract");
  }
  free(h);
}

int main() {
  const std::vector<Entry> three = {{10, 100, 0xAABBCCDDu}, {7, 0, 0x51D8E999u}, {33, 50000, 0x01020304u}};
  // ---- footer and header verdicts ----
  for (int sums = 0; sums < 2; sums++)
    for (size_t odd = 0; odd < 2; odd++) {
      // (the table starts at byte 50 or, with one more skippable byte in the middle entry, at the odd byte 51)
      std::vector<Entry> es = three;
      es[1].c += (uint32_t)odd;
      const Opened o = open_host(archive(50 + odd, table(es, sums)));
      EXPECT(o.status == ZD_OK, "a good table (sums %d, odd %zu): %d", sums, odd, o.status);
      EXPECT(o.ft.nframes == 3 && o.ft.entry_bytes == (sums ? 12u : 8u) && o.ft.checksums == (uint32_t)sums &&
             o.ft.table_bytes == 17 + 3 * (sums ? 12u : 8u), "the footer's fields");
      EXPECT(o.c_off == (std::vector<uint64_t>{0, 10, 17 + odd, 50 + odd}), "c_off");
      EXPECT(o.d_off == (std::vector<uint64_t>{0, 100, 100, 50100}), "d_off");
      EXPECT(o.sum == (sums ? std::vector<uint32_t>{0xAABBCCDDu, 0x51D8E999u, 0x01020304u}
                            : std::vector<uint32_t>{0, 0, 0}), "checksums");
    }
  EXPECT(open_host(archive(50, table(three, false, 0x184D2A5Eu, -1, -1, 0x03))).status == ZD_OK,
         "descriptor bits 1-0 are ignored");
  EXPECT(open_host(V(16, 0)).status == ZD_E_NOT_ENOUGH_BYTES, "16 bytes");
  EXPECT(open_host(V()).status == ZD_E_NOT_ENOUGH_BYTES, "no bytes");
  {
    // five entries named, one present: the table is larger than the archive
    const Opened o = open_host(table({{1, 1, 0}}, false, 0x184D2A5Eu, -1, 5));
    EXPECT(o.status == ZD_E_NOT_ENOUGH_BYTES, "a table larger than the archive: %d", o.status);
  }
  EXPECT(open_host(archive(50, table(three, false, 0x184D2A5Eu, -1, -1, -1, 0x8F92EAB0u))).status ==
         ZD_E_UNRECOGNIZED_MAGIC, "the footer's magic");
  EXPECT(open_host(archive(50, table(three, true, 0x184D2A50u))).status == ZD_E_UNRECOGNIZED_MAGIC,
         "the skippable header's magic");
  for (int bit = 2; bit < 7; bit++)
    EXPECT(open_host(archive(50, table(three, false, 0x184D2A5Eu, -1, -1, 1 << bit))).status ==
           ZD_E_FRAME_RESERVED_SET, "reserved bit %d", bit);
  {
    // more than 2^27 entries: known from the footer alone, whatever the archive's size
    V t = table({}, false, 0x184D2A5Eu, -1, (1 << 27) + 1);
    SeekFooter ft;
    uint8_t* last = (uint8_t*)malloc(9);
    memcpy(last, t.data() + t.size() - 9, 9);
    EXPECT(seek_footer(last, 1ull << 40, &ft) == ZD_E_OUT_OF_DOMAIN, "2^27 + 1 entries");
    t = table({}, true, 0x184D2A5Eu, -1, 1 << 27);
    memcpy(last, t.data() + t.size() - 9, 9);
    EXPECT(seek_footer(last, 1ull << 40, &ft) == ZD_OK && ft.table_bytes == 12ull * (1 << 27) + 17, "2^27 entries");
    EXPECT(seek_footer(last, 12ull * (1 << 27) + 16, &ft) == ZD_E_NOT_ENOUGH_BYTES, "2^27 entries, one byte short");
    free(last);
  }
  EXPECT(open_host(archive(50, table(three, false, 0x184D2A5Eu, 3 * 8 + 8))).status == ZD_E_SEEK_TABLE, "Frame_Size");
  EXPECT(open_host(archive(50, table(three, true, 0x184D2A5Eu, 3 * 8 + 9))).status == ZD_E_SEEK_TABLE,
         "Frame_Size of the other entry size");
  EXPECT(open_host(archive(51, table(three, false))).status == ZD_E_SEEK_TABLE, "one byte more than the sizes' sum");
  EXPECT(open_host(archive(49, table(three, true))).status == ZD_E_SEEK_TABLE, "one byte less than the sizes' sum");
  {
    const Opened o = open_host(table({}, false));
    EXPECT(o.status == ZD_OK && o.ft.nframes == 0 && o.ft.table_bytes == 17 && o.d_off == std::vector<uint64_t>{0},
           "a table of no entries: %d", o.status);
    EXPECT(open_host(archive(1, table({}, true))).status == ZD_E_SEEK_TABLE, "no entries, one byte in front");
    EXPECT(seek_clamp(0, 10, 0) == 0 && seek_clamp(5, 0, 0) == 0, "no content: every range is empty");
  }

  // ---- the search: sizes 10, 0, 0, 5, 20, 0, 7 ----
  const std::vector<uint64_t> d_off = {0, 10, 10, 10, 15, 35, 35, 42};
  const uint64_t MAX = ~0ull;
  const Want wants[] = {
      {3, 4, 0, 0, 4},            // inside a frame
      {0, 1, 0, 0, 1},            // the first byte
      {41, 1, 6, 6, 1},           // the last byte
      {10, 5, 3, 3, 5},           // starts exactly at a boundary (behind two entries of no bytes), ends at one
      {5, 5, 0, 0, 5},            // ends exactly at a boundary
      {10, 1, 3, 3, 1},
      {9, 1, 0, 0, 1},            // one byte either side of a boundary
      {9, 2, 0, 3, 2},            // across the entries of no bytes
      {14, 22, 3, 6, 22},         // across another one
      {34, 2, 4, 6, 2},
      {15, 20, 4, 4, 20},         // exactly one frame
      {0, 42, 0, 6, 42},          // everything
      {42, 5, 0, 0, 0},           // starts at the content's end
      {100, 5, 0, 0, 0},          // starts past it
      {40, 100, 6, 6, 2},         // ends past it
      {0, MAX, 0, 6, 42},
      {41, MAX, 6, 6, 1},
      {MAX, MAX, 0, 0, 0},        // (off + len would wrap)
      {3, 0, 0, 0, 0},            // len 0
      {42, 0, 0, 0, 0},
  };
  for (const Want& w : wants) search(d_off, w);

  // ---- the part of a frame a range wants; in place or staged ----
  {
    uint64_t from, bytes, at;
    EXPECT(!seek_part(10, 15, 9, 2, &from, &bytes, &at) && from == 0 && bytes == 1 && at == 1, "a frame's first byte");
    EXPECT(!seek_part(0, 10, 9, 2, &from, &bytes, &at) && from == 9 && bytes == 1 && at == 0, "a frame's last byte");
    EXPECT(seek_part(10, 15, 10, 5, &from, &bytes, &at) && from == 0 && bytes == 5 && at == 0, "a whole frame");
    EXPECT(seek_part(15, 35, 14, 22, &from, &bytes, &at) && from == 0 && bytes == 20 && at == 1, "a frame inside");
    EXPECT(!seek_part(15, 35, 16, 5, &from, &bytes, &at) && from == 1 && bytes == 5 && at == 0, "a range inside");
    EXPECT(!seek_part(10, 10, 9, 2, &from, &bytes, &at) && bytes == 0, "a frame of no bytes");
    EXPECT(!seek_part(35, 42, 9, 2, &from, &bytes, &at) && bytes == 0, "a frame elsewhere");
    EXPECT(seek_in_place(1, 0) && !seek_in_place(2, 0) && !seek_in_place(1, 1) && !seek_in_place(0, 0), "in place");
    EXPECT(!seek_staged(0, 0) && !seek_staged(1, 0) && seek_staged(1, 1) && seek_staged(2, 0) && seek_staged(3, 2),
           "staged");
    EXPECT(seek_stage_bytes(0) == 0 && seek_stage_bytes(1) == 16 && seek_stage_bytes(16) == 16 &&
           seek_stage_bytes(0xFFFFFFFFull) == 0x100000000ull, "staging sizes");
    EXPECT(seek_dst_ok(0, 0) && !seek_dst_ok(0, 5) && seek_dst_ok(4096, 5) && !seek_dst_ok(MAX - 2, 5) &&
           seek_dst_ok(MAX - 5, 5), "destinations");
  }

  // ---- sums past 2^32 ----
  {
    const uint32_t big = 0xFFFFFFFFu;
    const V t = table({{big, big, 1}, {big, big, 2}, {big, big, 3}}, true);
    uint8_t* p = (uint8_t*)malloc(t.size());
    memcpy(p, t.data(), t.size());
    const uint64_t front = 3ull * big, n = front + t.size();
    SeekFooter ft;
    EXPECT(seek_footer(p + t.size() - 9, n, &ft) == ZD_OK && seek_header(p, ft) == ZD_OK, "a table of large entries");
    std::vector<uint64_t> c{0}, d{0};
    for (uint32_t i = 0; i < 3; i++) {
      uint32_t cs, ds, k;
      seek_entry(p, ft, i, &cs, &ds, &k);
      EXPECT(k == i + 1, "entry %u's checksum", i);
      c.push_back(c.back() + cs); d.push_back(d.back() + ds);
    }
    free(p);
    EXPECT(c.back() == 12884901885ull && d.back() == 12884901885ull, "the sums: %llu", (unsigned long long)c.back());
    EXPECT(seek_sums(c.back(), n, ft) == ZD_OK && seek_sums(c.back() & 0xFFFFFFFFull, n, ft) == ZD_E_SEEK_TABLE,
           "the compressed sizes against the archive");
    search(d, {4294967301ull, 1ull << 33, 1, 2, 8589934584ull});      // from 2^32 + 5 to the end (clamped)
    search(d, {4294967294ull, 2, 0, 1, 2});                           // one byte either side of 2^32 - 1
    search(d, {8589934590ull, 4294967295ull, 2, 2, 4294967295ull});   // exactly the last frame
    search(d, {12884901884ull, MAX, 2, 2, 1});
  }
  printf("ok %d\n", checks);
  return 0;
}
