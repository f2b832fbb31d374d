// zd_seek.hip — gfx950 kernels of the seekable-archive layer (include/zd.h
// zd_seekable_*): the seek table read where it lies, a read's ranges turned
// into the chunk table of an ordinary device-built batch, and the pass that
// delivers the staged frames' bytes.  The rules -- footer, entry, clamp,
// search, which part of a frame a range wants, in place or staged -- are
// zd_seek.h's, shared with the host.  Compiled as the last part of
// zd_kernels.hip, which includes this file: the library keeps one device
// code object.
//
// A read (zd_seekable_read_create), R ranges over an archive of F frames:
//   zd_k_seek_cover   one lane a range: clamp, destination check, first and
//                     last frame (binary search in d_off), 32 KiB piece count
//   zd_k_seek_mark    one wave a range, lanes striding over its frames:
//                     cover[f]++, partial[f]++ when the range holds only a part
//   zd_k_seek_plan    one lane a frame: needed (0 / 1), staged bytes
//   scans             needed -> the frame's chunk, staged bytes -> its staging
//                     offset, pieces -> the range's first piece
//   zd_k_seek_totals  the words that come back to the host
//   zd_k_seek_chunks  one wave a range: the inner batch's four columns
// A launch (zd_seek_read_decode_async), behind the inner batch's decode:
//   zd_k_seek_verify  (a ZD_SEEK_VERIFY_TABLE read) four lanes a needed entry:
//                     its bytes hashed where they were decoded, the low 32
//                     bits compared with the table's Checksum
//   zd_k_seek_finish  one workgroup a 32 KiB piece of a range's destination
//   zd_k_seek_results one wave a range
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/zd.h"
#include "zd_common.h"
#include "zd_launch.h"
#include "zd_seek.h"

namespace zd {

namespace {
typedef uint32_t s_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t s_u32x4a1 __attribute__((ext_vector_type(4), aligned(1)));
typedef __attribute__((address_space(1))) const s_u32x4a1 sg_cu32x4a1;
typedef __attribute__((address_space(1))) s_u32x4 sg_u32x4;
}  // namespace

// zd_k_seek_table: entry f's sizes into the columns the scans turn into c_off
// and d_off (entry nframes: 0, so the scans leave the totals there), its
// checksum; the largest Decompressed_Size; lane 0 of the grid checks the
// skippable header.  Byte loads at the table's own alignment, nothing outside
// [table, table + table_bytes).
__global__ __launch_bounds__(256) void zd_k_seek_table(const uint8_t* __restrict__ table, SeekFooter ft,
                                                       uint64_t* c_off, uint64_t* d_off, uint32_t* checksum,
                                                       uint64_t* res) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  uint32_t big = 0;
  if (i < ft.nframes) {
    uint32_t c, d, k;
    seek_entry(table, ft, (uint32_t)i, &c, &d, &k);
    c_off[i] = c;
    d_off[i] = d;
    if (checksum) checksum[i] = k;
    big = d;
  } else if (i == ft.nframes) {
    c_off[i] = 0;
    d_off[i] = 0;
  }
  for (int k = 32; k; k >>= 1) {
    const uint32_t o = __shfl_xor(big, k);
    big = o > big ? o : big;
  }
  if ((threadIdx.x & 63) == 0 && big) atomicMax((unsigned long long*)(res + 1), (unsigned long long)big);
  if (i == 0) res[0] = (uint64_t)(int64_t)seek_header(table, ft);
}

hipError_t launch_seek_table(const uint8_t* table, const SeekFooter& f, uint64_t* c_off, uint64_t* d_off,
                             uint32_t* checksum, uint64_t* tot, uint64_t* res, hipStream_t s) {
  const uint64_t n1 = (uint64_t)f.nframes + 1;
  if (d_off != c_off + n1) return hipErrorInvalidValue;       // (the two scanned columns)
  hipError_t e = hipMemsetAsync(res, 0, 2 * 8, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(zd_k_seek_table, dim3((uint32_t)((n1 + 255) / 256)), dim3(256), 0, s, table, f, c_off, d_off,
                     checksum, res);
  return launch_scan64(c_off, nullptr, n1, 2, n1, tot, s);
}

// zd_k_seek_cover: range i clamped, its destination checked (zd_seek.h
// seek_dst_ok; a refused range reads and writes nothing), its frames found,
// its 32 KiB pieces counted.  Entry R of the piece column is 0: the scan
// leaves the total there.
__global__ __launch_bounds__(256) void zd_k_seek_cover(const uint64_t* __restrict__ off,
                                                       const uint64_t* __restrict__ len,
                                                       const uint64_t* __restrict__ dst,
                                                       const uint64_t* __restrict__ d_off, SeekRead A) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i > A.R) return;
  if (i == A.R) { A.piece0[i] = 0; return; }
  const uint64_t content = A.F ? d_off[A.F] : 0;
  const uint64_t o = off[i], d = dst[i];
  uint64_t l = seek_clamp(o, len[i], content);
  uint8_t bad = 0;
  if (!seek_dst_ok(d, l)) { bad = 1; l = 0; }
  uint32_t f0 = 0, f1 = 0;
  if (l) seek_frames(d_off, A.F, o, l, &f0, &f1);
  A.off[i] = l ? o : 0;
  A.len[i] = l;
  A.dst[i] = l ? d : 0;
  A.f0[i] = f0;
  A.f1[i] = f1;
  A.bad[i] = bad;
  A.piece0[i] = (l + COPY_PIECE - 1) / COPY_PIECE;
}

// zd_k_seek_mark: every frame range i touches with at least one byte counts
// the range (cover) and, when the range holds only a part of it, once more
// (partial).  Frames of no bytes between f0 and f1 are not touched.
__global__ __launch_bounds__(256) void zd_k_seek_mark(const uint64_t* __restrict__ d_off, SeekRead A) {
  const uint32_t i = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (i >= A.R) return;
  const uint64_t l = A.len[i];
  if (!l) return;
  const uint64_t o = A.off[i];
  const uint32_t f0 = A.f0[i], f1 = A.f1[i];
  for (uint64_t f = (uint64_t)f0 + lane; f <= f1; f += 64) {
    uint64_t from, bytes, at;
    const bool whole = seek_part(d_off[f], d_off[f + 1], o, l, &from, &bytes, &at);
    if (!bytes) continue;
    atomicAdd(A.cover + f, 1u);
    if (!whole) atomicAdd(A.partial + f, 1u);
  }
}

// zd_k_seek_plan: frame f's two scanned columns -- 1 when some range needs it,
// its staging bytes when it is staged -- and the count of in-place frames.
__global__ __launch_bounds__(256) void zd_k_seek_plan(const uint64_t* __restrict__ d_off, SeekRead A, uint64_t* res) {
  const uint32_t f = blockIdx.x * 256 + threadIdx.x;
  uint32_t inplace = 0;
  if (f < A.F) {
    const uint32_t c = A.cover[f], p = A.partial[f];
    A.idx[f] = c ? 1 : 0;
    A.soff[f] = seek_staged(c, p) ? seek_stage_bytes(d_off[f + 1] - d_off[f]) : 0;
    inplace = seek_in_place(c, p) ? 1 : 0;
  }
  for (int k = 32; k; k >>= 1) inplace += __shfl_xor(inplace, k);
  if ((threadIdx.x & 63) == 0 && inplace) atomicAdd((unsigned long long*)(res + 3), (unsigned long long)inplace);
}

// zd_k_seek_totals: what the creation reads back (res[3] is zd_k_seek_plan's)
__global__ void zd_k_seek_totals(const uint64_t* __restrict__ totF, uint64_t tilesF, const uint64_t* __restrict__ totR,
                                 uint64_t tilesR, uint64_t* res) {
  res[0] = tilesF ? totF[tilesF] : 0;
  res[1] = tilesF ? totF[(tilesF + 1) + tilesF] : 0;
  res[2] = totR[tilesR];
}

hipError_t launch_seek_layout(const uint64_t* off, const uint64_t* len, const uint64_t* dst, const uint64_t* d_off,
                              const SeekRead& A, uint64_t* tot, uint64_t* res, hipStream_t s) {
  if (A.F && A.soff != A.idx + A.F) return hipErrorInvalidValue;   // (the two scanned columns)
  const uint64_t tilesF = ((uint64_t)A.F + 255) / 256, tilesR = ((uint64_t)A.R + 1 + 255) / 256;
  uint64_t* totF = tot;
  uint64_t* totR = tot + 2 * (tilesF + 1);
  hipLaunchKernelGGL(zd_k_seek_cover, dim3((uint32_t)tilesR), dim3(256), 0, s, off, len, dst, d_off, A);
  if (A.F) {
    hipLaunchKernelGGL(zd_k_seek_mark, dim3((A.R + 3) / 4), dim3(256), 0, s, d_off, A);
    hipLaunchKernelGGL(zd_k_seek_plan, dim3((uint32_t)tilesF), dim3(256), 0, s, d_off, A, res);
    hipError_t e = launch_scan64(A.idx, nullptr, A.F, 2, A.F, totF, s);
    if (e != hipSuccess) return e;
  }
  hipError_t e = launch_scan64(A.piece0, nullptr, (uint64_t)A.R + 1, 1, (uint64_t)A.R + 1, totR, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(zd_k_seek_totals, dim3(1), dim3(1), 0, s, (const uint64_t*)totF, A.F ? tilesF : 0,
                     (const uint64_t*)totR, tilesR, res);
  return hipGetLastError();
}

// zd_k_seek_chunks: the inner batch's chunk of every frame range i needs:
// the entry's bytes in the archive, decoded at the range's own destination
// when the frame is in place (then this range is the only one that touches
// it) and at its staging offset otherwise (every range that touches a staged
// frame writes the same four words).  Capacity: the table's Decompressed_Size.
// v_entry / v_addr (a verified read's, else null): the chunk's entry and the
// address it decodes to, which zd_k_seek_verify reads at every launch.
__global__ __launch_bounds__(256) void zd_k_seek_chunks(SeekRead A, const uint8_t* archive,
                                                        const uint64_t* __restrict__ c_off,
                                                        const uint64_t* __restrict__ d_off, uint8_t* staging,
                                                        uint64_t* col_src, uint64_t* col_size, uint64_t* col_dst,
                                                        uint64_t* col_cap, uint32_t* v_entry, uint64_t* v_addr) {
  const uint32_t i = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (i >= A.R) return;
  const uint64_t l = A.len[i];
  if (!l) return;
  const uint64_t o = A.off[i], d = A.dst[i];
  const uint32_t f0 = A.f0[i], f1 = A.f1[i];
  for (uint64_t f = (uint64_t)f0 + lane; f <= f1; f += 64) {
    const uint64_t fa = d_off[f], fb = d_off[f + 1];
    uint64_t from, bytes, at;
    seek_part(fa, fb, o, l, &from, &bytes, &at);
    if (!bytes) continue;
    const uint64_t k = A.idx[f];
    const bool inplace = seek_in_place(A.cover[f], A.partial[f]);
    col_src[k] = (uint64_t)(uintptr_t)archive + c_off[f];
    col_size[k] = c_off[f + 1] - c_off[f];
    const uint64_t to = inplace ? d + at : (uint64_t)(uintptr_t)staging + A.soff[f];
    col_dst[k] = to;
    col_cap[k] = fb - fa;
    if (v_entry) v_entry[k] = (uint32_t)f;
    if (v_addr) v_addr[k] = to;
  }
}

hipError_t launch_seek_chunks(const SeekRead& A, const uint8_t* archive, const uint64_t* c_off, const uint64_t* d_off,
                              uint8_t* staging, uint64_t* col_src, uint64_t* col_size, uint64_t* col_dst,
                              uint64_t* col_cap, uint32_t* v_entry, uint64_t* v_addr, hipStream_t s) {
  if (!A.R || !A.F) return hipSuccess;
  hipLaunchKernelGGL(zd_k_seek_chunks, dim3((A.R + 3) / 4), dim3(256), 0, s, A, archive, c_off, d_off, staging,
                     col_src, col_size, col_dst, col_cap, v_entry, v_addr);
  return hipGetLastError();
}

// zd_k_seek_verify (a ZD_SEEK_VERIFY_TABLE read, between the inner batch's
// decode and zd_k_seek_finish): the table's Checksum, the low 32 bits of XXH64
// of the entry's decoded bytes, compared for every chunk that ended ZD_OK with
// its entry's Decompressed_Size.  zd_k_verify's layout and its 32-byte-row body
// (seek_xx_lines): four lanes a chunk, lane `sub` accumulator `sub`, 16 chunks a
// wave; always the rows, entries being KiB to MiB and few.  The bytes are read
// where the chunk decoded them, v_addr[k]: a range's destination for an entry in
// place, the staging buffer otherwise, at whatever alignment that has, and every
// load lies inside [p, p + Decompressed_Size).  A chunk is an entry, so an entry
// is hashed once however many ranges touch it.  b_ok / b_hash (a
// ZD_F_VERIFY_CHECKSUM read's, else null): a chunk whose frame's own
// Content_Checksum the inner batch verified (b_ok[k] == 1) was hashed there; the
// low half of that digest is compared and the bytes are not read again.  Every
// other chunk is not read: ok -1, hash32 0.  Writes ok and hash32, nothing else.
//
// seek_xx_lines is a copy of the LINES body of zd_k_verify (zd_kernels.hip), not
// a function both call: with the body moved into one __device__ function,
// zd_k_verify<true> compiled to other code for gfx950 (986 against 1,026 lines
// of assembly), so that kernel stays as it was.  The whole 128-byte lines of
// [p, p + 32 nst) into accumulator `sub` of the quad: a line is four 32-byte
// rows of two ldg16, quad_transpose64 hands lane k word k of the four stripes,
// VF_U lines go a trip with the next trip's loads issued before this trip's
// rounds.  Returns the stripes eaten (four a line).
__device__ inline uint64_t seek_xx_lines(const uint8_t* p, uint64_t nst, int sub, uint64_t& v) {
  const uint64_t nl = nst / 4;
  auto row = [&](uint64_t line, u32x4& a, u32x4& b) {
    const uint8_t* q = p + 128 * line + 32 * sub;
    a = ldg16(q);
    b = ldg16(q + 16);
  };
  auto eat = [&](const u32x4& a, const u32x4& b) {
    uint64_t w[4] = {(uint64_t)a.x | ((uint64_t)a.y << 32), (uint64_t)a.z | ((uint64_t)a.w << 32),
                     (uint64_t)b.x | ((uint64_t)b.y << 32), (uint64_t)b.z | ((uint64_t)b.w << 32)};
    quad_transpose64(w, sub);
    v = xx_round(xx_round(xx_round(xx_round(v, w[0]), w[1]), w[2]), w[3]);
  };
  u32x4 ca[VF_U] = {}, cb[VF_U] = {};
  uint64_t t = 0;
  if (VF_U <= nl) {
#pragma unroll
    for (int k = 0; k < VF_U; k++) row(k, ca[k], cb[k]);
  }
  while (t + VF_U <= nl) {
    u32x4 na[VF_U], nb[VF_U];
#pragma unroll
    for (int k = 0; k < VF_U; k++) { na[k] = ca[k]; nb[k] = cb[k]; }
    if (t + 2 * VF_U <= nl) {                       // the next trip's lines, before this trip's rounds
#pragma unroll
      for (int k = 0; k < VF_U; k++) row(t + VF_U + k, na[k], nb[k]);
    }
#pragma unroll
    for (int k = 0; k < VF_U; k++) eat(ca[k], cb[k]);
#pragma unroll
    for (int k = 0; k < VF_U; k++) { ca[k] = na[k]; cb[k] = nb[k]; }
    t += VF_U;
  }
  for (; t < nl; t++) {
    u32x4 a, b;
    row(t, a, b);
    eat(a, b);
  }
  return 4 * nl;
}

__global__ __launch_bounds__(64) void zd_k_seek_verify(const uint32_t* __restrict__ v_entry,
                                                       const uint64_t* __restrict__ v_addr, uint32_t n,
                                                       const uint64_t* __restrict__ d_off,
                                                       const uint32_t* __restrict__ checksum,
                                                       const int32_t* __restrict__ b_status,
                                                       const uint64_t* __restrict__ b_len,
                                                       const uint64_t* __restrict__ b_hash,
                                                       const int8_t* __restrict__ b_ok, int8_t* ok, uint32_t* hash32) {
  const int lane = threadIdx.x, sub = lane & 3;
  const uint32_t k = blockIdx.x * 16 + (lane >> 2);
  uint64_t L = 0, size = 0;
  const uint8_t* p = nullptr;
  uint32_t want = 0, have = 0;
  bool act = false, hashed = false;
  if (k < n) {
    const uint32_t f = v_entry[k];
    size = d_off[f + 1] - d_off[f];
    act = b_status[k] == ZD_OK && b_len[k] == size;
    if (act) {
      want = checksum[f];
      hashed = b_ok && b_ok[k] == 1;
      if (hashed) {
        have = (uint32_t)b_hash[k];
      } else {
        L = size;
        p = (const uint8_t*)(uintptr_t)v_addr[k];
      }
    }
  }
  const uint64_t nst = L / 32;
  uint64_t v = xx_acc_init(sub);
  uint64_t s = seek_xx_lines(p, nst, sub, v);
  for (; s < nst; s++) v = xx_round(v, *(g_cu64a1*)(p + 32 * s + 8 * sub));
  // (the lanes have reconverged: the four accumulators into every lane of the quad)
  const uint64_t acc[4] = {qdpp64<0x00>(v), qdpp64<0x55>(v), qdpp64<0xAA>(v), qdpp64<0xFF>(v)};
  if (k < n && sub == 0) {
    if (act && !hashed) have = (uint32_t)xx_finish(L, acc, p + 32 * nst, (uint32_t)(L - 32 * nst));
    ok[k] = act ? (have == want ? 1 : 0) : -1;
    hash32[k] = act ? have : 0;
  }
}

hipError_t launch_seek_verify(const uint32_t* v_entry, const uint64_t* v_addr, uint32_t n, const uint64_t* d_off,
                              const uint32_t* checksum, const int32_t* b_status, const uint64_t* b_len,
                              const uint64_t* b_hash, const int8_t* b_ok, int8_t* ok, uint32_t* hash32,
                              hipStream_t s) {
  if (!n) return hipSuccess;
  if (!v_entry || !v_addr || !checksum || !b_status || !b_len || !ok || !hash32) return hipErrorInvalidValue;
  hipLaunchKernelGGL(zd_k_seek_verify, dim3((n + 15) / 16), dim3(64), 0, s, v_entry, v_addr, n, d_off, checksum,
                     b_status, b_len, b_hash, b_ok, ok, hash32);
  return hipGetLastError();
}

// zd_k_seek_finish: piece q of the read is piece q - piece0[i] of range i, the
// last range whose first piece is at or below q (zd_k_gather_scan's search;
// ranges of no pieces share their successor's start and are never found).
// The workgroup walks the frames under its 32 KiB of the range, skips the ones
// decoded in place, and copies each staged frame's wanted part: bytewise up to
// the destination's next 16-byte boundary, then 16-byte aligned stores fed by
// 16-byte loads at the source's own alignment, then the tail bytewise.  Every
// load lies inside the frame's own bytes of the staging buffer.
__global__ __launch_bounds__(256) void zd_k_seek_finish(SeekRead A, const uint64_t* __restrict__ d_off,
                                                        const uint8_t* __restrict__ staging, uint64_t npieces) {
  const uint64_t q = blockIdx.x;
  if (q >= npieces || !A.R) return;
  uint32_t lo = 0, hi = A.R;          // piece0[lo] <= q < piece0[hi] (piece0[R] = npieces)
  while (hi - lo > 1) {
    const uint32_t m = lo + (hi - lo) / 2;
    if (A.piece0[m] <= q) lo = m; else hi = m;
  }
  const uint32_t i = lo;
  const uint64_t l = A.len[i], o = A.off[i];
  const uint64_t p0 = (q - A.piece0[i]) * COPY_PIECE;           // the piece: range bytes [p0, p1)
  if (p0 >= l) return;
  const uint64_t p1 = p0 + COPY_PIECE < l ? p0 + COPY_PIECE : l;
  uint8_t* const dst = (uint8_t*)(uintptr_t)A.dst[i];
  const uint32_t t = threadIdx.x;
  const uint32_t fend = A.f1[i];
  for (uint32_t f = seek_frame_of(d_off, A.F, o + p0); f <= fend; f++) {
    const uint64_t fa = d_off[f], fb = d_off[f + 1];
    if (fa >= o + p1) break;
    uint64_t from, bytes, at;
    seek_part(fa, fb, o + p0, p1 - p0, &from, &bytes, &at);
    if (!bytes || !seek_staged(A.cover[f], A.partial[f])) continue;
    const uint8_t* sp = staging + A.soff[f] + from;
    uint8_t* dp = dst + p0 + at;
    const uint32_t n = (uint32_t)bytes;                          // (<= COPY_PIECE)
    uint32_t head = (uint32_t)((16 - ((uintptr_t)dp & 15)) & 15);
    if (head > n) head = n;
    const uint32_t nvec = (n - head) / 16, tail0 = head + 16 * nvec;
    if (t < head) dp[t] = sp[t];
    for (uint32_t v = t; v < nvec; v += 256)
      *(sg_u32x4*)(dp + head + 16 * v) = *(sg_cu32x4a1*)(sp + head + 16 * v);
    if (tail0 + t < n) dp[tail0 + t] = sp[tail0 + t];
  }
}

hipError_t launch_seek_finish(const SeekRead& A, const uint64_t* d_off, const uint8_t* staging, uint64_t npieces,
                              hipStream_t s) {
  if (!npieces || !A.R || !A.F || !staging) return hipSuccess;
  hipLaunchKernelGGL(zd_k_seek_finish, dim3((uint32_t)npieces), dim3(256), 0, s, A, d_off, staging, npieces);
  return hipGetLastError();
}

// zd_k_seek_results: range i's status is that of the lowest-numbered of its
// frames whose chunk did not end ZD_OK; with every chunk ZD_OK but one whose
// decoded length is not the table's Decompressed_Size, ZD_E_SEEK_TABLE.  Its
// length: the clamped length, or 0 on failure.  v_ok (zd_k_seek_verify's
// verdicts, null for a read without ZD_SEEK_VERIFY_TABLE): a frame that was
// compared and differs (0) counts among the frames that did not end ZD_OK, as
// ZD_E_CHECKSUM_WRONG.
__global__ __launch_bounds__(256) void zd_k_seek_results(SeekRead A, const uint64_t* __restrict__ d_off,
                                                         const int32_t* __restrict__ b_status,
                                                         const uint64_t* __restrict__ b_len,
                                                         const int8_t* __restrict__ v_ok) {
  const uint32_t i = blockIdx.x * 4 + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (i >= A.R) return;
  const uint64_t l = A.len[i];
  uint64_t firstbad = ~0ull;
  uint32_t mismatch = 0;
  if (l && b_status) {
    const uint64_t o = A.off[i];
    const uint32_t f0 = A.f0[i], f1 = A.f1[i];
    for (uint64_t f = (uint64_t)f0 + lane; f <= f1; f += 64) {
      const uint64_t fa = d_off[f], fb = d_off[f + 1];
      uint64_t from, bytes, at;
      seek_part(fa, fb, o, l, &from, &bytes, &at);
      if (!bytes) continue;
      const uint64_t k = A.idx[f];
      if (b_status[k]) { if (f < firstbad) firstbad = f; }
      else if (b_len[k] != fb - fa) mismatch = 1;
      else if (v_ok && v_ok[k] == 0) { if (f < firstbad) firstbad = f; }
    }
  }
  for (int k = 32; k; k >>= 1) {
    const uint64_t ob = __shfl_xor((unsigned long long)firstbad, k);
    firstbad = ob < firstbad ? ob : firstbad;
    mismatch |= __shfl_xor(mismatch, k);
  }
  if (lane) return;
  int st = ZD_OK;
  if (A.bad[i]) st = ZD_E_INVALID_ARG;
  else if (firstbad != ~0ull) {
    st = b_status[A.idx[firstbad]];
    if (v_ok && !st) st = ZD_E_CHECKSUM_WRONG;     // (its chunk ended ZD_OK: the entry that was compared and differs)
  } else if (mismatch) st = ZD_E_SEEK_TABLE;
  A.status[i] = st;
  A.out_len[i] = st ? 0 : l;
}

hipError_t launch_seek_results(const SeekRead& A, const uint64_t* d_off, const int32_t* b_status,
                               const uint64_t* b_len, const int8_t* v_ok, hipStream_t s) {
  if (!A.R) return hipSuccess;
  hipLaunchKernelGGL(zd_k_seek_results, dim3((A.R + 3) / 4), dim3(256), 0, s, A, d_off, b_status, b_len, v_ok);
  return hipGetLastError();
}

}  // namespace zd
