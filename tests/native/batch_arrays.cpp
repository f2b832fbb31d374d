// Host driver of the carve of a batch's per-chunk arrays (zd_plan.h
// BatchCarve: what zd_batch_create* slices zd_batch::d_arr with), no GPU
// needed.  For n in {1, 7, 8, 9, 255, 256, 257, 65536}, host arrays with
// npieces in {n, n + 3} and device arrays with and without prefixes:
//   - every offset and the total against the layout's formulas, written out
//     here and not taken from the carve
//   - u64 arrays 8-aligned, u32 arrays 4-aligned
//   - no two arrays overlap, the last one ends at or before the total
//   - piece0 == off + n (BatchArrays: the layout scans them as two columns)
// and a few totals as plain numbers.  Prints one line per failed check and
// exits with status 1 if there was one; "ok <checks>" otherwise.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_plan.h"

using namespace zd;

static int failures = 0;
static long checks = 0;

static void expect(bool ok, const char* what, const char* kind, uint64_t n, uint64_t got, uint64_t want) {
  checks++;
  if (ok) return;
  failures++;
  printf("FAIL %s (%s, n = %llu): %llu, expected %llu\n", what, kind, (unsigned long long)n, (unsigned long long)got,
         (unsigned long long)want);
}

static uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

struct Arr {
  const char* name;
  uint64_t at, bytes, align;
};

// alignment, no overlap, the end inside the total
static void check_arrays(const std::vector<Arr>& arrs, uint64_t total, const char* kind, uint64_t n) {
  for (size_t i = 0; i < arrs.size(); i++) {
    const Arr& a = arrs[i];
    expect(a.at != BatchCarve::ABSENT, a.name, kind, n, a.at, 0);
    expect(a.at % a.align == 0, a.name, kind, n, a.at % a.align, 0);
    expect(a.at + a.bytes <= total, a.name, kind, n, a.at + a.bytes, total);
    for (size_t j = 0; j < i; j++) {
      const Arr& b = arrs[j];
      const bool apart = a.at + a.bytes <= b.at || b.at + b.bytes <= a.at;
      expect(apart, a.name, b.name, n, a.at, b.at);
    }
  }
}

static void host_arrays(uint64_t n, uint64_t npieces) {
  const char* kind = "host";
  BatchCarve C;
  C.carve(n, false, npieces, false);
  const uint64_t head_words = 4 * n + npieces;
  const uint64_t total = 8 * (head_words + 3 * n) + 4 * n + 4 * n + align_up(n, 8);
  expect(C.src == 0, "src", kind, n, C.src, 0);
  expect(C.size == 8 * n, "size", kind, n, C.size, 8 * n);
  expect(C.off == 16 * n, "off", kind, n, C.off, 16 * n);
  expect(C.out == 24 * n, "out", kind, n, C.out, 24 * n);
  expect(C.pieces == 32 * n, "pieces", kind, n, C.pieces, 32 * n);
  expect(C.head_bytes == 8 * head_words, "head_bytes", kind, n, C.head_bytes, 8 * head_words);
  expect(C.boff == 8 * head_words, "boff", kind, n, C.boff, 8 * head_words);
  expect(C.len == 8 * head_words + 8 * n, "len", kind, n, C.len, 8 * head_words + 8 * n);
  expect(C.hash == 8 * head_words + 16 * n, "hash", kind, n, C.hash, 8 * head_words + 16 * n);
  expect(C.status == 8 * (head_words + 3 * n), "status", kind, n, C.status, 8 * (head_words + 3 * n));
  expect(C.nblk == 8 * (head_words + 3 * n) + 4 * n, "nblk", kind, n, C.nblk, 8 * (head_words + 3 * n) + 4 * n);
  expect(C.bind == 8 * (head_words + 3 * n) + 8 * n, "bind", kind, n, C.bind, 8 * (head_words + 3 * n) + 8 * n);
  expect(C.total == total, "total", kind, n, C.total, total);
  // the arrays a batch made from device arrays has are absent
  const uint64_t absent[] = {C.piece0, C.cap, C.flag, C.scratch, C.res, C.pfx, C.pfx_bytes};
  for (uint64_t a : absent) expect(a == BatchCarve::ABSENT, "absent", kind, n, a, BatchCarve::ABSENT);
  check_arrays({{"src", C.src, 8 * n, 8}, {"size", C.size, 8 * n, 8}, {"off", C.off, 8 * n, 8},
                {"out", C.out, 8 * n, 8}, {"pieces", C.pieces, 8 * npieces, 8}, {"boff", C.boff, 8 * n, 8},
                {"len", C.len, 8 * n, 8}, {"hash", C.hash, 8 * n, 8}, {"status", C.status, 4 * n, 4},
                {"nblk", C.nblk, 4 * n, 4}, {"bind", C.bind, n, 1}},
               C.total, kind, n);
}

static void device_arrays(uint64_t n, bool prefixes) {
  const char* kind = prefixes ? "device, prefixes" : "device";
  BatchCarve C;
  C.carve(n, true, 0, prefixes);
  const uint64_t nt = (n + 255) / 256;
  const uint64_t scratch_words = 2 * (nt + 1) + 1, res_words = 4;
  const uint64_t bytes_at = 9 * 8 * n + 2 * 4 * n, words_at = align_up(bytes_at + 2 * n, 8);
  const uint64_t pfx_at = words_at + 8 * (scratch_words + res_words);
  const uint64_t total = pfx_at + (prefixes ? 2 * 8 * n : 0);
  expect(C.src == 0, "src", kind, n, C.src, 0);
  expect(C.size == 8 * n, "size", kind, n, C.size, 8 * n);
  expect(C.off == 16 * n, "off", kind, n, C.off, 16 * n);
  expect(C.piece0 == 24 * n, "piece0", kind, n, C.piece0, 24 * n);
  expect(C.piece0 == C.off + 8 * n, "piece0 == off + n", kind, n, C.piece0, C.off + 8 * n);
  expect(C.out == 32 * n, "out", kind, n, C.out, 32 * n);
  expect(C.cap == 40 * n, "cap", kind, n, C.cap, 40 * n);
  expect(C.boff == 48 * n, "boff", kind, n, C.boff, 48 * n);
  expect(C.len == 56 * n, "len", kind, n, C.len, 56 * n);
  expect(C.hash == 64 * n, "hash", kind, n, C.hash, 64 * n);
  expect(C.status == 72 * n, "status", kind, n, C.status, 72 * n);
  expect(C.nblk == 76 * n, "nblk", kind, n, C.nblk, 76 * n);
  expect(C.bind == bytes_at, "bind", kind, n, C.bind, bytes_at);
  expect(C.bind == 80 * n, "bind", kind, n, C.bind, 80 * n);
  expect(C.flag == 81 * n, "flag", kind, n, C.flag, 81 * n);
  expect(C.scratch_words == scratch_words, "scratch_words", kind, n, C.scratch_words, scratch_words);
  expect(C.scratch == words_at, "scratch", kind, n, C.scratch, words_at);
  expect(C.res == words_at + 8 * scratch_words, "res", kind, n, C.res, words_at + 8 * scratch_words);
  expect(C.total == total, "total", kind, n, C.total, total);
  expect(C.pieces == BatchCarve::ABSENT, "absent", kind, n, C.pieces, BatchCarve::ABSENT);
  std::vector<Arr> arrs = {{"src", C.src, 8 * n, 8}, {"size", C.size, 8 * n, 8}, {"off", C.off, 8 * n, 8},
                           {"piece0", C.piece0, 8 * n, 8}, {"out", C.out, 8 * n, 8}, {"cap", C.cap, 8 * n, 8},
                           {"boff", C.boff, 8 * n, 8}, {"len", C.len, 8 * n, 8}, {"hash", C.hash, 8 * n, 8},
                           {"status", C.status, 4 * n, 4}, {"nblk", C.nblk, 4 * n, 4}, {"bind", C.bind, n, 1},
                           {"flag", C.flag, n, 1}, {"scratch", C.scratch, 8 * scratch_words, 8},
                           {"res", C.res, 8 * res_words, 8}};
  if (prefixes) {
    expect(C.pfx == pfx_at, "pfx", kind, n, C.pfx, pfx_at);
    expect(C.pfx_bytes == pfx_at + 8 * n, "pfx_bytes", kind, n, C.pfx_bytes, pfx_at + 8 * n);
    arrs.push_back({"pfx", C.pfx, 8 * n, 8});
    arrs.push_back({"pfx_bytes", C.pfx_bytes, 8 * n, 8});
  } else {
    expect(C.pfx == BatchCarve::ABSENT, "absent", kind, n, C.pfx, BatchCarve::ABSENT);
    expect(C.pfx_bytes == BatchCarve::ABSENT, "absent", kind, n, C.pfx_bytes, BatchCarve::ABSENT);
  }
  check_arrays(arrs, C.total, kind, n);
}

static uint64_t total_of(uint64_t n, bool on_device, uint64_t npieces, bool prefixes) {
  BatchCarve C;
  C.carve(n, on_device, npieces, prefixes);
  return C.total;
}

int main() {
  const uint64_t ns[] = {1, 7, 8, 9, 255, 256, 257, 65536};
  for (uint64_t n : ns) {
    host_arrays(n, n);
    host_arrays(n, n + 3);
    device_arrays(n, false);
    device_arrays(n, true);
  }
  expect(total_of(1, false, 1, false) == 80, "spot", "host", 1, total_of(1, false, 1, false), 80);
  expect(total_of(9, false, 11, false) == 680, "spot", "host", 9, total_of(9, false, 11, false), 680);
  expect(total_of(1, true, 0, false) == 160, "spot", "device", 1, total_of(1, true, 0, false), 160);
  expect(total_of(1, true, 0, true) == 176, "spot", "device, prefixes", 1, total_of(1, true, 0, true), 176);
  expect(total_of(257, true, 0, false) == 21168, "spot", "device", 257, total_of(257, true, 0, false), 21168);
  expect(total_of(257, true, 0, true) == 25280, "spot", "device, prefixes", 257, total_of(257, true, 0, true), 25280);
  if (failures) return 1;
  printf("ok %ld\n", checks);
  return 0;
}
