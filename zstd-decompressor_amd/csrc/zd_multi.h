// zd_multi.h — the rule of a multi-frame batch (zd_multi_create_device): how a
// chunk that holds any number of concatenated zstd frames is cut into
// sub-chunks, each a valid chunk of an ordinary batch, and where each
// sub-chunk decodes -- in place in the chunk's destination, or into the
// staging buffer.  Shared by the host (tests/native/multi_split.cpp: all of
// it) and the device (zd_multi.hip: zd_k_multi_count, zd_k_multi_fill,
// zd_k_multi_sizes): one source, so the passes cannot drift.  It stands on
// index_frame / WalkBound / chunk_reserve of zd_walk.h.
//
// Sub-chunks.  The chunk is walked from its first byte with the walk options
// of the inner batch.  Every zstd frame that walks to its end closes a
// sub-chunk: the bytes from the end of the previous zstd frame (or the chunk's
// start) to the end of this one, so the skippable frames in front of a frame
// travel with it.  Whatever remains -- skippable frames only, bytes that are no
// frame, a frame whose walk fails with everything behind it -- is one last
// sub-chunk when it is not empty.  A chunk in which no zstd frame walks to its
// end is one sub-chunk, the whole chunk (a chunk of no bytes too).  A
// sub-chunk's status in the inner batch is what zd_batch_create_device gives
// that byte range: it holds at most one zstd frame that walks.
//
// Placement.  Sub-chunk k is IN PLACE when every sub-chunk before it in the
// chunk is exact (chunk_reserve's *exact: a usable Frame_Content_Size): its
// offset in the destination is the sum of their Frame_Content_Sizes.  Every
// sub-chunk behind the first inexact one is STAGED: it decodes into the staging
// buffer with its reserve as its capacity, staging offsets rounded up to 16.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zd.h"
#include "zd_common.h"
#include "zd_walk.h"

namespace zd {

constexpr uint64_t MULTI_IN_PLACE = ~0ull;          // a sub-chunk's staging offset: none
constexpr uint64_t MULTI_NOT_DELIVERED = ~0ull;     // a staged sub-chunk's final address: its bytes stay where they are

// One sub-chunk as the walk gives it.
struct MultiSub {
  uint64_t begin = 0, end = 0;   // chunk bytes [begin, end)
  uint64_t reserve = 0;          // chunk_reserve's (0 for a sub-chunk without a zstd frame that walks)
  uint8_t exact = 0;
  int32_t status = 0;            // the header walk's status of the sub-chunk alone
};

// The sub-chunks of [src, src + size) in order.  base = src, and Bytes is
// bounds-checked: no byte outside the chunk is read, at any alignment.
struct MultiWalk {
  const uint8_t* src;
  uint64_t size;
  uint32_t wopt;
  uint64_t pos = 0;
  uint32_t k = 0;               // sub-chunks handed out
  bool done = false;
  ZD_HD MultiWalk(const uint8_t* s, uint64_t n, uint32_t w) : src(s), size(n), wopt(w) {}
  ZD_HD bool next(MultiSub* s) {
    if (done) return false;
    Bytes in{src + pos, (size_t)(size - pos)};
    int st = 0;
    while (in.n) {
      HostFrame hf;
      WalkBound sink;
      st = index_frame(src, in, &hf, sink, wopt);
      if (st) break;
      if (hf.d.kind != ZD_FRAME_ZSTD) continue;       // a skippable frame: it travels with the next frame
      s->begin = pos;
      s->end = (uint64_t)(in.p - src);
      s->reserve = chunk_reserve(hf, sink.bound, &s->exact);
      s->status = 0;
      pos = s->end;
      k++;
      return true;
    }
    // what remains: nothing (and not the only sub-chunk), skippable frames only (st 0), or from a failure on
    done = true;
    if (pos == size && k) return false;
    s->begin = pos;
    s->end = size;
    s->reserve = 0;
    s->exact = 0;
    s->status = st;
    k++;
    return true;
  }
};

// Where a sub-chunk decodes.
struct MultiSlot {
  uint64_t offset = 0;      // in place: its offset in the chunk's destination (meaningful when !past)
  uint64_t cap = 0;         // its capacity in the inner batch
  uint64_t stage = MULTI_IN_PLACE;   // staged: its offset among the chunk's staging bytes; else MULTI_IN_PLACE
  uint64_t pieces = 0;      // staged: the 32 KiB copy pieces of its reserve
  bool past = false;        // in place, and its offset lies past dst_cap (capacity 0)
  ZD_HD bool staged() const { return stage != MULTI_IN_PLACE; }
};

ZD_HD inline uint64_t multi_stage_bytes(uint64_t reserve) { return (reserve + 15) & ~15ull; }
ZD_HD inline uint64_t multi_pieces(uint64_t reserve) { return (reserve + COPY_PIECE - 1) / COPY_PIECE; }

// The running placement of one chunk's sub-chunks, in order.
//   in place, exact:    capacity min(reserve, dst_cap - offset)
//   in place, inexact:  capacity dst_cap - offset   (the first inexact one; everything behind it is staged)
//   both 0 when the offset is past dst_cap: the inner batch's capacity pass then
//   reports ZD_E_DST_TOO_SMALL by itself for a frame that has content.
//   staged:             capacity = reserve, at the next staging offset (a multiple of 16)
struct MultiPlace {
  uint64_t dst_cap;
  uint64_t offset = 0;          // the sum of the exact sub-chunks' Frame_Content_Sizes so far
  uint64_t stage_bytes = 0;     // the chunk's staging bytes so far
  uint64_t pieces = 0;          // the chunk's copy pieces so far
  uint32_t staged = 0;          // its staged sub-chunks so far
  bool in_place = true;
  ZD_HD explicit MultiPlace(uint64_t cap) : dst_cap(cap) {}
  ZD_HD MultiSlot place(const MultiSub& s) {
    MultiSlot o;
    if (in_place) {
      o.past = offset > dst_cap;
      const uint64_t room = o.past ? 0 : dst_cap - offset;
      o.offset = offset;
      o.cap = s.exact ? (s.reserve < room ? s.reserve : room) : room;
      if (s.exact) offset += s.reserve; else in_place = false;
    } else {
      o.stage = stage_bytes;
      o.cap = s.reserve;
      o.pieces = multi_pieces(s.reserve);
      stage_bytes += multi_stage_bytes(s.reserve);
      pieces += o.pieces;
      staged++;
    }
    return o;
  }
};

// An entry zd_k_batch_layout would refuse: a NULL address with a non-zero
// count, a range that wraps (ZD_E_INVALID_ARG there), a chunk of 2^32 bytes or
// more (ZD_E_OUT_OF_DOMAIN there).  Such a chunk is not walked: it goes to the
// inner batch as it is, one sub-chunk, and gets its status there.
ZD_HD inline bool multi_entry_refused(uint64_t src, uint64_t size, uint64_t dst, uint64_t cap) {
  return (!src && size) || (!dst && cap) || src + size < src || dst + cap < dst || size >= (1ull << 32);
}

// zd_chunk_sizes_device with ZD_SIZES_MULTI_FRAME: the sum of the sub-chunks'
// reserves, *exact = every one of them is exact, and the walk status of the
// first sub-chunk that fails.
ZD_HD inline int multi_size_query(const uint8_t* src, size_t size, uint32_t wopt, uint64_t* reserve, uint8_t* exact) {
  MultiWalk w(src, size, wopt);
  MultiSub s;
  uint64_t sum = 0;
  uint8_t all = 1;
  int st = 0;
  while (w.next(&s)) {
    sum += s.reserve;
    all &= s.exact;
    if (!st) st = s.status;
  }
  *reserve = sum;
  *exact = all;
  return st;
}

}  // namespace zd
