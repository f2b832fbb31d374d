// zd_chain.h — the level rule of a chain batch (zd_batch_create_chain): chunk
// i's prefix is the decoded output of chunk parent[i] of the same batch, and a
// chunk's level is the number of its in-batch ancestors.  The executor runs
// once per level, in level order, so every parent is complete before a child
// of it starts: the order comes from the kernel boundaries on the stream,
// never from one workgroup waiting for another.  Shared by the host
// (zd_host.cpp: host arrays, where a bad entry fails the call) and the device
// (zd_kernels.hip zd_k_chain_levels: device arrays, where it fails its chunk):
// one source, so the two cannot drift.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "zd_walk.h"

namespace zd {

constexpr uint32_t CHAIN_MAX_DEPTH = 255;          // ZD_CHAIN_MAX_DEPTH: levels 0..255
constexpr uint32_t CHAIN_LEVELS = CHAIN_MAX_DEPTH + 1;
constexpr int32_t CHAIN_INVALID = -1;

// parent[i] names no chunk and is not -1, or names i itself
ZD_HD inline bool chain_bad_entry(int64_t p, uint64_t i, uint64_t n) {
  return p < -1 || (p >= 0 && ((uint64_t)p >= n || (uint64_t)p == i));
}

// Chunk i's level, or CHAIN_INVALID: its own entry is bad, or its ancestors
// reach no root within CHAIN_MAX_DEPTH hops (a cycle, a tail behind a cycle, a
// chain deeper than the limit).  At most CHAIN_LEVELS entries of parent[] are
// read.  An ANCESTOR with a bad entry ends the walk like a root: that chunk is
// refused itself, and its descendants are not decoded because of its status,
// not because of their own entries.
ZD_HD inline int32_t chain_level(const int64_t* parent, uint64_t n, uint64_t i) {
  if (chain_bad_entry(parent[i], i, n)) return CHAIN_INVALID;
  uint64_t c = i;
  for (uint32_t lvl = 0; lvl < CHAIN_LEVELS; lvl++) {
    const int64_t p = parent[c];
    if (p == -1 || chain_bad_entry(p, c, n)) return (int32_t)lvl;
    c = (uint64_t)p;
  }
  return CHAIN_INVALID;
}

// The chunks grouped by level (host arrays): level[i] as chain_level gives it,
// order[] a permutation of 0..n-1 by ascending level (ascending index inside a
// level; an invalid chunk counts as level 0, where nothing of it runs),
// count[l] the chunks of level l (CHAIN_LEVELS entries, summing to n).
// Returns the number of invalid chunks.
inline uint64_t chain_order(const int64_t* parent, uint64_t n, int32_t* level, uint32_t* order, uint32_t* count) {
  uint64_t bad = 0;
  for (uint32_t l = 0; l < CHAIN_LEVELS; l++) count[l] = 0;
  for (uint64_t i = 0; i < n; i++) {
    level[i] = chain_level(parent, n, i);
    if (level[i] == CHAIN_INVALID) bad++;
    count[level[i] == CHAIN_INVALID ? 0 : level[i]]++;
  }
  uint32_t at[CHAIN_LEVELS];
  uint32_t o = 0;
  for (uint32_t l = 0; l < CHAIN_LEVELS; l++) { at[l] = o; o += count[l]; }
  for (uint64_t i = 0; i < n; i++) order[at[level[i] == CHAIN_INVALID ? 0 : level[i]]++] = (uint32_t)i;
  return bad;
}

// What a chained chunk's prefix is, from its parent's indexed frame: the
// parent's Frame_Content_Size, which the child is planned with; 0 bytes for a
// parent without a zstd frame (no bytes, skippable frames only: the child
// decodes as a plain chunk).  Only the parent's header fields are read, never
// its key, which the passes that run beside this one may still write: a child
// of a parent that fails is not decoded at launch, whatever it was planned with.
// false: the parent's frame carries no Frame_Content_Size, so the child cannot
// be planned (ZD_E_OUT_OF_DOMAIN for the child; the parent is unaffected).
ZD_HD inline bool chain_prefix_bytes(const HostFrame& par, uint64_t* bytes) {
  *bytes = 0;
  if (par.d.kind != ZD_FRAME_ZSTD) return true;
  if (par.d.content_size == UINT64_MAX) return false;
  *bytes = par.d.content_size;
  return true;
}
ZD_HD inline void chain_no_prefix_size(HostFrame& hf) {
  if (hf.key != KEY_NONE) return;            // (a chunk that failed already keeps its own status)
  hf.status = ZD_E_OUT_OF_DOMAIN;
  hf.key = make_key(PH_LIMIT, 0, 0, 0, ZD_E_OUT_OF_DOMAIN);
}

}  // namespace zd
