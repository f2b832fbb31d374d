// zd_multi.hip — gfx950 kernels of the multi-frame batch (include/zd.h
// zd_multi_*): chunks that hold several concatenated zstd frames, cut into the
// chunk table of an ordinary device-built batch, and the passes that fold the
// sub-chunks' results back and deliver the staged bytes.  The rule -- where a
// sub-chunk ends, in place or staged, offsets, capacities -- is zd_multi.h's,
// shared with the host.  Compiled as a part of zd_kernels.hip, which includes
// this file: the library keeps one device code object.
//
// Creation (zd_multi_create_device), n chunks that hold F sub-chunks:
//   zd_k_multi_count  one lane a chunk: the header walk where the chunk lies;
//                     its sub-chunks, staged bytes, 32 KiB copy pieces, staged
//                     sub-chunks; the chunk's destination copied
//   scans             the four columns -> the chunk's first sub-chunk, staging
//                     offset and copy piece; entry n of each: the total
//   zd_k_multi_fill   one lane a chunk: the same walk again; the inner batch's
//                     four columns and the per-sub-chunk arrays
// A launch (zd_multi_decode_async), behind the inner batch's decode:
//   zd_k_multi_join   one lane a chunk, over its sub-chunks in order
//   zd_k_multi_copy   one workgroup a 32 KiB piece of a staged reserve
// The size query (zd_chunk_sizes_device with ZD_SIZES_MULTI_FRAME):
//   zd_k_multi_sizes  one lane a chunk
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/zd.h"
#include "zd_common.h"
#include "zd_launch.h"
#include "zd_multi.h"

namespace zd {

namespace {
typedef uint32_t m_u32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t m_u32x4a1 __attribute__((ext_vector_type(4), aligned(1)));
typedef __attribute__((address_space(1))) const m_u32x4a1 mg_cu32x4a1;
typedef __attribute__((address_space(1))) m_u32x4 mg_u32x4;
}  // namespace

// zd_k_multi_count: chunk i's sub-chunks counted by the walk of zd_multi.h, 64
// chunks a wave (zd_k_chunk_sizes' shape).  Byte loads at the chunk's own
// alignment, nothing outside [src, src + size).  An entry zd_k_batch_layout
// would refuse is not read: it is one sub-chunk, handed on as it is.  Entry n
// of the four columns is 0: the scans leave the totals there.
__global__ __launch_bounds__(64) void zd_k_multi_count(const uint64_t* __restrict__ src,
                                                      const uint64_t* __restrict__ size,
                                                      const uint64_t* __restrict__ dst,
                                                      const uint64_t* __restrict__ cap, uint32_t wopt, MultiArrays M) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i > M.n) return;
  uint64_t subs = 0, stage = 0, pieces = 0, staged = 0;
  if (i < M.n) {
    const uint64_t s = src[i], z = size[i], d = dst[i], c = cap[i];
    const bool refused = multi_entry_refused(s, z, d, c);
    M.dst[i] = refused ? 0 : d;
    M.cap[i] = refused ? 0 : c;
    if (refused) {
      subs = 1;
    } else {
      MultiWalk w((const uint8_t*)(uintptr_t)s, z, wopt);
      MultiPlace p(c);
      MultiSub sub;
      while (w.next(&sub)) p.place(sub);
      subs = w.k;
      stage = p.stage_bytes;
      pieces = p.pieces;
      staged = p.staged;
    }
  }
  const uint64_t n1 = (uint64_t)M.n + 1;
  M.first[i] = subs;
  M.first[n1 + i] = stage;
  M.first[2 * n1 + i] = pieces;
  M.first[3 * n1 + i] = staged;
}

hipError_t launch_multi_count(const uint64_t* src, const uint64_t* size, const uint64_t* dst, const uint64_t* cap,
                              uint32_t wopt, const MultiArrays& M, uint64_t* tot, hipStream_t s) {
  const uint64_t n1 = (uint64_t)M.n + 1;
  if (M.stage0 != M.first + n1 || M.piece0c != M.first + 2 * n1 || M.nstaged != M.first + 3 * n1)
    return hipErrorInvalidValue;                                    // (the four scanned columns)
  hipLaunchKernelGGL(zd_k_multi_count, dim3((uint32_t)((n1 + 63) / 64)), dim3(64), 0, s, src, size, dst, cap, wopt, M);
  return launch_scan64(M.first, nullptr, n1, 4, n1, tot, s);
}

// zd_k_multi_fill: the walk of zd_k_multi_count again, now with the scanned
// starts: sub-chunk k = first[i] + j of chunk i gets its row of the inner
// batch's chunk table -- its bytes where they lie, and its destination: the
// chunk's own at its offset (in place) or the staging buffer at its staging
// offset, with the capacity of zd_multi.h's MultiPlace -- and chunk[k], soff[k]
// (MULTI_IN_PLACE: not staged), at[k] (in place: its offset), piece0[k].  Lane
// n writes piece0[F].
__global__ __launch_bounds__(64) void zd_k_multi_fill(const uint64_t* __restrict__ src,
                                                     const uint64_t* __restrict__ size,
                                                     const uint64_t* __restrict__ dst,
                                                     const uint64_t* __restrict__ cap, uint32_t wopt, MultiArrays M,
                                                     uint8_t* staging, uint64_t* col_src, uint64_t* col_size,
                                                     uint64_t* col_dst, uint64_t* col_cap) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i > M.n) return;
  uint64_t k = M.first[i];
  if (i == M.n) { M.piece0[k] = M.piece0c[i]; return; }
  const uint64_t kend = M.first[i + 1];
  const uint64_t s = src[i], z = size[i], d = dst[i], c = cap[i];
  if (multi_entry_refused(s, z, d, c)) {
    if (k >= kend) return;
    col_src[k] = s; col_size[k] = z; col_dst[k] = d; col_cap[k] = c;
    M.chunk[k] = i; M.soff[k] = MULTI_IN_PLACE; M.at[k] = 0; M.piece0[k] = M.piece0c[i];
    return;
  }
  const uint64_t stage0 = M.stage0[i];
  uint64_t piece = M.piece0c[i];
  MultiWalk w((const uint8_t*)(uintptr_t)s, z, wopt);
  MultiPlace p(c);
  MultiSub sub;
  // (the chunk's bytes are the caller's and may have changed since the count: never past the chunk's rows,
  // staging bytes or pieces, which the count set)
  const uint64_t stage_end = M.stage0[i + 1], piece_end = M.piece0c[i + 1];
  while (k < kend && w.next(&sub)) {
    MultiSlot o = p.place(sub);
    col_src[k] = sub.end > sub.begin ? s + sub.begin : 0;
    col_size[k] = sub.end - sub.begin;
    if (o.staged() && (stage0 + p.stage_bytes > stage_end || piece + o.pieces > piece_end)) {
      o.cap = 0; o.pieces = 0;
      col_dst[k] = 0;
      M.soff[k] = MULTI_IN_PLACE;
      M.at[k] = 0;
    } else if (o.staged()) {
      col_dst[k] = o.cap ? (uint64_t)(uintptr_t)staging + stage0 + o.stage : 0;
      M.soff[k] = stage0 + o.stage;
      M.at[k] = 0;
    } else {
      col_dst[k] = o.past || !d ? 0 : d + o.offset;           // (capacity 0 then)
      M.soff[k] = MULTI_IN_PLACE;
      M.at[k] = o.offset;
    }
    col_cap[k] = o.cap;
    M.chunk[k] = i;
    M.piece0[k] = piece;
    piece += o.pieces;
    k++;
  }
  for (; k < kend; k++) {                    // (only when the bytes changed: rows of no bytes)
    col_src[k] = 0; col_size[k] = 0; col_dst[k] = 0; col_cap[k] = 0;
    M.chunk[k] = i; M.soff[k] = MULTI_IN_PLACE; M.at[k] = 0; M.piece0[k] = piece;
  }
}

hipError_t launch_multi_fill(const uint64_t* src, const uint64_t* size, const uint64_t* dst, const uint64_t* cap,
                             uint32_t wopt, const MultiArrays& M, uint8_t* staging, uint64_t* col_src,
                             uint64_t* col_size, uint64_t* col_dst, uint64_t* col_cap, hipStream_t s) {
  hipLaunchKernelGGL(zd_k_multi_fill, dim3((uint32_t)(((uint64_t)M.n + 1 + 63) / 64)), dim3(64), 0, s, src, size, dst,
                     cap, wopt, M, staging, col_src, col_size, col_dst, col_cap);
  return hipGetLastError();
}

// zd_k_multi_join: chunk i's sub-chunks first[i] .. first[i + 1) in order, one
// lane a chunk -- the status, the running length and "delivered or not" are a
// chain from one sub-chunk to the next, a chunk has a handful of sub-chunks,
// and the lanes of a wave read neighbouring rows of the inner results.  The
// chunk's status is that of its lowest-numbered sub-chunk that did not end
// ZD_OK; else ZD_E_DST_TOO_SMALL when the decoded lengths, summed in order,
// pass the chunk's capacity at a staged sub-chunk; else ZD_OK with the sum.  A
// sub-chunk in place that starts anywhere but at that running sum (a frame
// before it ended ZD_OK with a length other than its Frame_Content_Size)
// fails the chunk with ZD_E_OUT_OF_DOMAIN.  fdst[k]: a staged sub-chunk's
// final address, MULTI_NOT_DELIVERED from the first failure or overflow on.
__global__ __launch_bounds__(256) void zd_k_multi_join(MultiArrays M, const int32_t* __restrict__ b_status,
                                                      const uint64_t* __restrict__ b_len) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= M.n) return;
  const uint64_t k0 = M.first[i], k1 = M.first[i + 1];
  const uint64_t d = M.dst[i], c = M.cap[i];
  uint64_t off = 0;
  int st = ZD_OK;
  for (uint64_t k = k0; k < k1; k++) {
    const int s = b_status[k];
    const uint64_t l = b_len[k];
    const bool staged = M.soff[k] != MULTI_IN_PLACE;
    if (!st) {
      if (s) st = s;
      else if (staged ? l > c - off : (l && M.at[k] != off)) st = staged ? ZD_E_DST_TOO_SMALL : ZD_E_OUT_OF_DOMAIN;
    }
    if (staged) M.fdst[k] = st ? MULTI_NOT_DELIVERED : d + off;
    if (!st) off += l;                       // (in place: the inner batch held l within its capacity, <= c - off)
  }
  M.status[i] = st;
  M.len[i] = st ? 0 : off;
}

hipError_t launch_multi_join(const MultiArrays& M, const int32_t* b_status, const uint64_t* b_len, hipStream_t s) {
  if (!M.n) return hipSuccess;
  if (!b_status || !b_len) return hipErrorInvalidValue;
  hipLaunchKernelGGL(zd_k_multi_join, dim3((M.n + 255) / 256), dim3(256), 0, s, M, b_status, b_len);
  return hipGetLastError();
}

// zd_k_multi_copy: piece q of the batch is piece q - piece0[k] of sub-chunk k,
// the last one whose first piece is at or below q (zd_k_gather_scan's search;
// sub-chunks of no pieces -- the ones in place, staged ones that reserve
// nothing -- share their successor's start and are never found).  Nothing to do
// past the sub-chunk's decoded length or for one that is not delivered.  The
// copy: bytewise up to the destination's next 16-byte boundary, then 16-byte
// aligned stores fed by 16-byte loads at the source's own alignment, then the
// tail bytewise.  Every load lies inside the sub-chunk's decoded bytes in the
// staging buffer (b_len[k] <= its reserve, its capacity there), every store
// inside [fdst[k], fdst[k] + b_len[k]), which zd_k_multi_join checked against
// the chunk's destination.
__global__ __launch_bounds__(256) void zd_k_multi_copy(MultiArrays M, const uint8_t* __restrict__ staging,
                                                      const uint64_t* __restrict__ b_len, uint64_t npieces) {
  const uint64_t q = blockIdx.x;
  if (q >= npieces || !M.F) return;
  uint64_t lo = 0, hi = M.F;              // piece0[lo] <= q < piece0[hi] (piece0[F] = npieces)
  while (hi - lo > 1) {
    const uint64_t m = lo + (hi - lo) / 2;
    if (M.piece0[m] <= q) lo = m; else hi = m;
  }
  const uint64_t k = lo;
  const uint64_t so = M.soff[k], fd = M.fdst[k];
  if (so == MULTI_IN_PLACE || fd == MULTI_NOT_DELIVERED) return;
  const uint64_t l = b_len[k];
  const uint64_t p0 = (q - M.piece0[k]) * COPY_PIECE;
  if (p0 >= l) return;
  const uint32_t n = (uint32_t)(l - p0 < COPY_PIECE ? l - p0 : COPY_PIECE);
  const uint8_t* sp = staging + so + p0;
  uint8_t* dp = (uint8_t*)(uintptr_t)fd + p0;
  const uint32_t t = threadIdx.x;
  uint32_t head = (uint32_t)((16 - ((uintptr_t)dp & 15)) & 15);
  if (head > n) head = n;
  const uint32_t nvec = (n - head) / 16, tail0 = head + 16 * nvec;
  if (t < head) dp[t] = sp[t];
  for (uint32_t v = t; v < nvec; v += 256)
    *(mg_u32x4*)(dp + head + 16 * v) = *(mg_cu32x4a1*)(sp + head + 16 * v);
  if (tail0 + t < n) dp[tail0 + t] = sp[tail0 + t];
}

hipError_t launch_multi_copy(const MultiArrays& M, const uint8_t* staging, const uint64_t* b_len, uint64_t npieces,
                             hipStream_t s) {
  if (!npieces || !M.F || !staging) return hipSuccess;
  if (!b_len) return hipErrorInvalidValue;
  hipLaunchKernelGGL(zd_k_multi_copy, dim3((uint32_t)npieces), dim3(256), 0, s, M, staging, b_len, npieces);
  return hipGetLastError();
}

// zd_k_multi_sizes (zd_chunk_sizes_device with ZD_SIZES_MULTI_FRAME):
// zd_k_chunk_sizes with the chunk cut into sub-chunks -- the sum of their
// reserves, whether all of them are exact, the first failing one's status.
__global__ __launch_bounds__(64) void zd_k_multi_sizes(const uint64_t* __restrict__ src,
                                                      const uint64_t* __restrict__ size, uint32_t n, uint32_t wopt,
                                                      uint64_t* out_size, int32_t* status, uint8_t* exact) {
  const uint32_t i = blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const uint64_t s = src[i], z = size[i];
  uint64_t r = 0;
  uint8_t ex = 0;
  int st = 0;
  if ((!s && z) || s + z < s) st = ZD_E_INVALID_ARG;
  else if (z >= (1ull << 32)) st = ZD_E_OUT_OF_DOMAIN;
  else st = multi_size_query((const uint8_t*)(uintptr_t)s, (size_t)z, wopt, &r, &ex);
  out_size[i] = r;
  if (status) status[i] = st;
  if (exact) exact[i] = ex;
}

hipError_t launch_multi_sizes(const uint64_t* src, const uint64_t* size, uint32_t n, uint32_t wopt, uint64_t* out_size,
                              int32_t* status, uint8_t* exact, hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(zd_k_multi_sizes, dim3((n + 63) / 64), dim3(64), 0, s, src, size, n, wopt, out_size, status,
                     exact);
  return hipGetLastError();
}

}  // namespace zd
