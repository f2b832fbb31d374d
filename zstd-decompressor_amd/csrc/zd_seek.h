// zd_seek.h — the seek table of a zstd seekable archive (zd_seekable_open_device)
// and the rule that turns a byte range of the content into frames: the footer
// and header checks, the unaligned entry read, the clamp, the range-to-frames
// search and which part of a frame a range wants.  Shared by the host
// (zd_host.cpp: the footer; tests/native/seek_table.cpp: all of it) and the
// device (zd_seek.hip: zd_k_seek_table, zd_k_seek_cover and the kernels behind
// them): one source, so the two cannot drift.
//
// The layout, restated from the published format description:
//   entries ... | 5E 2A 4D 18 | Frame_Size u32 | nframes x entry | footer
//   entry  = Compressed_Size u32, Decompressed_Size u32 [, Checksum u32]
//   footer = Number_Of_Frames u32, descriptor u8, B1 EA 92 8F
// all little endian, at no particular alignment; the footer ends at the
// archive's last byte.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zd.h"
#include "zd_common.h"

namespace zd {

constexpr uint32_t SEEK_MAGIC_SKIP = 0x184D2A5Eu;
constexpr uint32_t SEEK_MAGIC_FOOTER = 0x8F92EAB1u;
constexpr uint32_t SEEK_FOOTER_BYTES = 9;
constexpr uint32_t SEEK_HEADER_BYTES = 8;               // skippable magic, Frame_Size
constexpr uint64_t SEEK_MIN_BYTES = SEEK_HEADER_BYTES + SEEK_FOOTER_BYTES;
constexpr uint32_t SEEK_MAX_FRAMES = 1u << 27;

struct SeekFooter {
  uint32_t nframes = 0;
  uint32_t entry_bytes = 8;     // 8, or 12 with checksums
  uint32_t checksums = 0;
  uint64_t table_bytes = 0;     // header, entries and footer
};

ZD_HD inline uint32_t seek_le32(const uint8_t* p) {
  return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}

// The footer: the last SEEK_FOOTER_BYTES bytes of an archive of n bytes.
ZD_HD inline int seek_footer(const uint8_t* last9, uint64_t n, SeekFooter* out) {
  if (n < SEEK_MIN_BYTES) return ZD_E_NOT_ENOUGH_BYTES;
  if (seek_le32(last9 + 5) != SEEK_MAGIC_FOOTER) return ZD_E_UNRECOGNIZED_MAGIC;
  const uint8_t desc = last9[4];
  if (desc & 0x7C) return ZD_E_FRAME_RESERVED_SET;
  SeekFooter f;
  f.nframes = seek_le32(last9);
  f.checksums = desc >> 7;
  f.entry_bytes = f.checksums ? 12 : 8;
  if (f.nframes > SEEK_MAX_FRAMES) return ZD_E_OUT_OF_DOMAIN;
  // (at most 2^27 entries of 12 bytes: no wrap)
  f.table_bytes = (uint64_t)f.nframes * f.entry_bytes + SEEK_MIN_BYTES;
  if (f.table_bytes > n) return ZD_E_NOT_ENOUGH_BYTES;
  *out = f;
  return ZD_OK;
}

// The skippable header in front of the entries (table: the table's first byte).
ZD_HD inline int seek_header(const uint8_t* table, const SeekFooter& f) {
  if (seek_le32(table) != SEEK_MAGIC_SKIP) return ZD_E_UNRECOGNIZED_MAGIC;
  if ((uint64_t)seek_le32(table + 4) != (uint64_t)f.nframes * f.entry_bytes + SEEK_FOOTER_BYTES) return ZD_E_SEEK_TABLE;
  return ZD_OK;
}

// Entry i of the table, read bytewise where it lies.
ZD_HD inline void seek_entry(const uint8_t* table, const SeekFooter& f, uint32_t i, uint32_t* csize, uint32_t* dsize,
                             uint32_t* checksum) {
  const uint8_t* e = table + SEEK_HEADER_BYTES + (uint64_t)i * f.entry_bytes;
  *csize = seek_le32(e);
  *dsize = seek_le32(e + 4);
  *checksum = f.checksums ? seek_le32(e + 8) : 0;
}

// What the open keeps of the sums: the compressed sizes must add up to exactly
// the bytes in front of the table.
ZD_HD inline int seek_sums(uint64_t compressed, uint64_t n, const SeekFooter& f) {
  return compressed == n - f.table_bytes ? ZD_OK : ZD_E_SEEK_TABLE;
}

// [off, off + len) clamped to a content of `content` bytes, as pread clamps:
// the clamped length (0: nothing to read; off is then not meaningful).
// off + len is never formed.
ZD_HD inline uint64_t seek_clamp(uint64_t off, uint64_t len, uint64_t content) {
  if (off >= content) return 0;
  const uint64_t room = content - off;
  return len < room ? len : room;
}

// The frame that holds content byte pos (pos < d_off[nframes]): the last f
// with d_off[f] <= pos.  Its successor starts past pos, so it is never an
// entry of no bytes.  d_off: nframes + 1 entries, the exclusive sums.
ZD_HD inline uint32_t seek_frame_of(const uint64_t* d_off, uint32_t nframes, uint64_t pos) {
  uint32_t lo = 0, hi = nframes;             // d_off[lo] <= pos < d_off[hi]
  while (hi - lo > 1) {
    const uint32_t m = lo + (hi - lo) / 2;
    if (d_off[m] <= pos) lo = m; else hi = m;
  }
  return lo;
}

// The frames of a clamped range [off, off + len), len > 0:
//   d_off[f0] <= off < d_off[f0 + 1],  d_off[f1] < off + len <= d_off[f1 + 1].
ZD_HD inline void seek_frames(const uint64_t* d_off, uint32_t nframes, uint64_t off, uint64_t len, uint32_t* f0,
                              uint32_t* f1) {
  *f0 = seek_frame_of(d_off, nframes, off);
  *f1 = seek_frame_of(d_off, nframes, off + (len - 1));
}

// Which part of frame [fa, fb) of the content a clamped range [off, off + len)
// wants: frame bytes [*from, *from + *bytes), which land at range byte *at.
// true: the frame lies wholly inside the range (a frame of no bytes: false,
// nothing wanted).
ZD_HD inline bool seek_part(uint64_t fa, uint64_t fb, uint64_t off, uint64_t len, uint64_t* from, uint64_t* bytes,
                            uint64_t* at) {
  const uint64_t end = off + len;            // (a clamped range: <= the content size)
  const uint64_t lo = fa > off ? fa : off, hi = fb < end ? fb : end;
  *from = 0; *bytes = 0; *at = 0;
  if (hi <= lo) return false;
  *from = lo - fa;
  *bytes = hi - lo;
  *at = lo - off;
  return lo == fa && hi == fb;
}

// A needed frame decodes in place when exactly one range touches it and holds
// all of it; every other needed frame is staged.
ZD_HD inline bool seek_in_place(uint32_t cover, uint32_t partial) { return cover == 1 && partial == 0; }
ZD_HD inline bool seek_staged(uint32_t cover, uint32_t partial) { return cover != 0 && !seek_in_place(cover, partial); }
ZD_HD inline uint64_t seek_stage_bytes(uint64_t dsize) { return (dsize + 15) & ~15ull; }

// A range's destination: false for a NULL address with bytes to write, or an
// address range that wraps.
ZD_HD inline bool seek_dst_ok(uint64_t dst, uint64_t clamped) {
  return !clamped || (dst && dst + clamped >= dst);
}

}  // namespace zd
