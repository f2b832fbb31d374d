// zd_walk.h — the frame / block header walk (FrameIterator, Frame::parse,
// Header::parse, Block::parse and the fixed-size parts of
// LiteralsSection::parse and Sequences::parse), shared by the host planner
// (zd_host.cpp: index_frames, one thread per byte range) and the device walk
// (zd_kernels.hip: zd_k_walk, one wave per byte range, for inputs that are
// resident in HBM).  One source for both, so the two walks agree byte for
// byte by construction; tests/test_gpu_walk.py checks the plans they give.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/zd.h"
#include "zd_common.h"

namespace zd {

constexpr uint32_t MAGIC_ZSTD = 0xFD2FB528u;   // frame.rs:41
constexpr uint32_t MAGIC_SKIP = 0x184D2A50u;   // frame.rs:42

struct WalkErr {
  int code = 0;
  uint32_t stage = PS_STRUCT;
};

// ForwardByteParser (parsing.rs:9-112)
struct Bytes {
  const uint8_t* p;
  size_t n;
  ZD_HD int u8(uint8_t* v) {
    if (!n) return ZD_E_NOT_ENOUGH_BYTES;
    *v = *p++; n--; return 0;
  }
  ZD_HD int slice(size_t len, const uint8_t** s) {
    if (len == 0) return ZD_E_EMPTY_SLICE;
    if (n < len) return ZD_E_NOT_ENOUGH_BYTES;
    *s = p; p += len; n -= len; return 0;
  }
  ZD_HD int le(size_t k, uint64_t* v) {
    if (n < k) return ZD_E_NOT_ENOUGH_BYTES;
    uint64_t r = 0;
    for (size_t i = 0; i < k; i++) r |= (uint64_t)p[i] << (8 * i);
    p += k; n -= k; *v = r; return 0;
  }
};

struct HostBlock {
  uint64_t src;          // absolute offset of the block content
  uint32_t size;
  uint8_t type, last, rle;
  // compressed only
  CompBlock cb;
};

// A frame; its blocks are blocks[b0, b0 + nb) of the part that holds it.
struct HostFrame {
  zd_frame_desc d;
  uint32_t b0 = 0, nb = 0;
  uint32_t ncomp = 0;         // compressed blocks
  uint64_t key = KEY_NONE;    // walk-detected parse error (frame stops here)
  int status = 0;
};

ZD_HD inline void zero_bytes(void* p, size_t n) {
  uint8_t* b = (uint8_t*)p;
  for (size_t i = 0; i < n; i++) b[i] = 0;
}

// Literals section header + the walk-visible parts of the section
// (literals.rs:88-206) and of the sequences header (sequences.rs:52-87 and
// the mode byte of 91-143).  The block content is base[off, off + size).
// rfc_empty_lits (dictionary plans, zd_plan_create_dict): a Raw literals
// section of 0 bytes is accepted as RFC 8878 has it -- a record found wholly in
// the dictionary has no literals -- where the reference's zero-length slice is
// an EmptySliceError (parsing.rs, kept everywhere else).
// wopt: the walk's options (zd_common.h walk_opts; WALK_LONG_WINDOW is not read
// here).  WALK_RFC_EMPTY_LITS is the above.  WALK_RFC (ZD_F_RFC) reads the
// headers as RFC 8878 has them: the three-byte Number_of_Sequences adds 0x7F00
// where the reference adds 0x7F (D1); the sizes of Huffman streams are not
// truncated to 16 bits, and a section one of whose streams is empty is
// ZD_E_CORRUPTED_STREAMS_SIZE where the reference decodes the streams before it
// (D8: such a section cannot hold its Regenerated_Size).
ZD_HD inline int parse_compressed(const uint8_t* base, uint64_t off, uint32_t size, CompBlock* cb, WalkErr* e,
                                  uint32_t wopt = 0) {
  const bool rfc_empty_lits = (wopt & WALK_RFC_EMPTY_LITS) != 0, rfc = (wopt & WALK_RFC) != 0;
  Bytes np{base + off, size};
  const uint8_t* start = np.p;
  auto rel = [&]() { return (uint32_t)(np.p - start); };
  e->stage = PS_STRUCT;
  uint8_t h;
  if (int r = np.u8(&h)) return e->code = r;
  int lt = h & 3, sf = (h >> 2) & 3;
  uint32_t regen = 0, csize = 0;
  int nstreams = 1;
  if (lt == LIT_RAW || lt == LIT_RLE) {
    uint8_t b1, b2;
    if (sf == 0 || sf == 2) regen = h >> 3;
    else if (sf == 1) { if (int r = np.u8(&b1)) return e->code = r; regen = (h >> 4) + ((uint32_t)b1 << 4); }
    else {
      if (int r = np.u8(&b1)) return e->code = r;
      if (int r = np.u8(&b2)) return e->code = r;
      regen = (h >> 4) + ((uint32_t)b1 << 4) + ((uint32_t)b2 << 12);
    }
  } else {
    const uint8_t* s;
    uint32_t nb = sf <= 1 ? 2 : (uint32_t)sf + 1;
    if (int r = np.slice(nb, &s)) return e->code = r;
    uint32_t x = 0;
    for (uint32_t i = 0; i < nb; i++) x |= (uint32_t)s[i] << (8 * i);
    if (sf <= 1) { regen = (h >> 4) + ((x & 0x3F) << 4); csize = x >> 6; nstreams = sf == 0 ? 1 : 4; }
    else if (sf == 2) { regen = (h >> 4) + ((x & 0x3FF) << 4); csize = (x >> 10) & 0x3FFF; nstreams = 4; }
    else { regen = (h >> 4) + ((x & 0x3FFF) << 4); csize = (x >> 14) & 0x3FFFF; nstreams = 4; }
  }
  cb->lit_type = (uint8_t)lt;
  cb->lit_regen = regen;
  cb->nstreams = 0;
  if (lt == LIT_RAW) {
    const uint8_t* s;
    cb->lit_data = rel();
    if (regen || !rfc_empty_lits)
      if (int r = np.slice(regen, &s)) return e->code = r;
  } else if (lt == LIT_RLE) {
    if (int r = np.u8(&cb->lit_rle)) return e->code = r;
  } else {
    const uint8_t* cs;
    if (int r = np.slice(csize, &cs)) return e->code = r;
    Bytes ni{cs, csize};
    if (lt == LIT_COMPRESSED) {      // HuffmanDecoder::parse header + description slice (huffman.rs:80-130)
      e->stage = PS_HUF_DESC;
      cb->lit_data = (uint32_t)(cs - start);
      uint8_t hh;
      if (int r = ni.u8(&hh)) return e->code = r;
      size_t dl = hh < 128 ? hh : ((size_t)(hh - 127) / 2 + (hh - 127) % 2);
      const uint8_t* d;
      if (int r = ni.slice(dl, &d)) return e->code = r;
      cb->huf_desc_size = (uint32_t)(1 + dl);
    }
    e->stage = PS_JUMP;
    size_t total = ni.n;
    uint32_t ss[4] = {0, 0, 0, 0};
    if (nstreams == 4) {
      uint64_t s1, s2, s3;
      if (int r = ni.le(2, &s1)) return e->code = r;
      if (int r = ni.le(2, &s2)) return e->code = r;
      if (int r = ni.le(2, &s3)) return e->code = r;
      if (s1 + s2 + s3 > total - 6) return e->code = ZD_E_CORRUPTED_STREAMS_SIZE;
      size_t s4 = total - 6 - s1 - s2 - s3;
      ss[0] = (uint32_t)s1; ss[1] = (uint32_t)s2; ss[2] = (uint32_t)s3; ss[3] = rfc ? (uint32_t)s4 : (uint16_t)s4;
    } else {
      ss[0] = rfc ? (uint32_t)ni.n : (uint16_t)ni.n;
    }
    cb->streams = (uint32_t)(ni.p - start);
    const uint8_t* d;
    if (int r = ni.slice(ni.n, &d)) return e->code = r;
    // literals.rs:70-73: the stream loop stops at the first empty stream
    for (int k = 0; k < 4; k++) {
      if (ss[k] == 0) break;
      cb->stream_size[k] = ss[k];
      cb->nstreams = (uint8_t)(k + 1);
    }
    if (rfc && cb->nstreams != nstreams) return e->code = ZD_E_CORRUPTED_STREAMS_SIZE;
  }
  // Sequences::parse (sequences.rs:52-75)
  e->stage = PS_SEQ_HDR;
  uint8_t b0;
  if (int r = np.u8(&b0)) return e->code = r;
  uint32_t nseq;
  if (b0 == 0) nseq = 0;
  else if (b0 < 128) nseq = b0;
  else if (b0 < 255) { uint8_t b1; if (int r = np.u8(&b1)) return e->code = r; nseq = ((uint32_t)(b0 - 128) << 8) + b1; }
  else {
    uint8_t b1, b2;
    if (int r = np.u8(&b1)) return e->code = r;
    if (int r = np.u8(&b2)) return e->code = r;
    nseq = (uint32_t)b1 + ((uint32_t)b2 << 8) + (rfc ? 0x7F00u : 0x7Fu);     // D1 (sequences.rs:84)
  }
  cb->nseq = nseq;
  cb->modes[0] = cb->modes[1] = cb->modes[2] = M_REPEAT;
  if (nseq) {
    const uint8_t* mb;
    if (int r = np.slice(1, &mb)) return e->code = r;
    if (mb[0] & 3) return e->code = ZD_E_SEQ_RESERVED_SET;
    cb->modes[0] = (mb[0] >> 6) & 3;
    cb->modes[1] = (mb[0] >> 4) & 3;
    cb->modes[2] = (mb[0] >> 2) & 3;
  }
  cb->seq_tables = rel();
  return 0;
}

// Header::parse (frame.rs:111-177)
ZD_HD inline int parse_header(Bytes& in, zd_frame_desc* f) {
  const uint8_t* b;
  if (int r = in.slice(1, &b)) return r;
  unsigned fhd = b[0];
  unsigned dict_flag = fhd & 3, csum = (fhd >> 2) & 1, reserved = (fhd >> 3) & 1;
  unsigned single = (fhd >> 5) & 1, fcs_flag = fhd >> 6;
  if (reserved) return ZD_E_FRAME_RESERVED_SET;
  int fcs_size = (fcs_flag == 0) ? (single ? 1 : -1) : (1 << fcs_flag);
  uint64_t window = 0;
  if (!single) {
    uint8_t wd;
    if (int r = in.u8(&wd)) return r;
    uint64_t base = 1ull << ((wd >> 3) + 10);
    window = base + (base / 8) * (wd & 7);
  }
  f->dict_id = UINT64_MAX;
  if (dict_flag) {
    const uint8_t* a;
    size_t dl = (size_t)1 << (dict_flag - 1);
    if (int r = in.slice(dl, &a)) return r;
    uint64_t v = 0;
    for (size_t i = 0; i < dl; i++) v |= (uint64_t)a[i] << (8 * i);
    f->dict_id = v;
  }
  f->content_size = UINT64_MAX;
  if (fcs_size > 0) {
    const uint8_t* a;
    if (int r = in.slice((size_t)fcs_size, &a)) return r;
    uint64_t v = 0;
    for (int i = 0; i < fcs_size; i++) v |= (uint64_t)a[i] << (8 * i);
    if (fcs_size == 2) v += 256;
    f->content_size = v;
  }
  f->window_size = single ? f->content_size : window;
  f->has_checksum = csum;
  return 0;
}

// Walks one frame at in, handing its blocks to the sink (S.size(): blocks
// so far; S.push(block)).  On error, hf->key/status hold the failure; the
// blocks parsed before (and the failing one, with its host_stage) are kept.
// wopt: WALK_RFC_EMPTY_LITS and WALK_RFC (parse_compressed's) and
// WALK_LONG_WINDOW (ZD_F_LONG_WINDOW: a Window_Size up to MAX_WIN_SIZE_LONG,
// 2 GiB, where the reference's MAX_WIN_SIZE stands otherwise).
template <typename SINK>
ZD_HD inline int index_frame(const uint8_t* base, Bytes& in, HostFrame* hf, SINK& S, uint32_t wopt = 0) {
  zd_frame_desc& f = hf->d;
  zero_bytes(&f, sizeof f);
  f.src_offset = (uint64_t)(in.p - base);
  f.content_size = UINT64_MAX;
  f.dict_id = UINT64_MAX;
  hf->b0 = (uint32_t)S.size();
  hf->nb = 0;
  hf->ncomp = 0;
  hf->key = KEY_NONE;
  hf->status = 0;
  auto push = [&](const HostBlock& hb) {
    S.push(hb);
    hf->nb++;
    hf->ncomp += hb.type == 2;
  };
  auto fail = [&](int code, uint32_t blk, uint32_t stage) {
    hf->status = code;
    hf->key = make_key(PH_PARSE, blk, stage, 0, code);
    f.src_size = (uint64_t)(in.p - base) - f.src_offset;
    return code;
  };
  uint64_t magic;
  if (int r = in.le(4, &magic)) return fail(r, 0, PS_STRUCT);
  f.magic = (uint32_t)magic;
  if (f.magic == MAGIC_ZSTD) {
    f.kind = ZD_FRAME_ZSTD;
    if (int r = parse_header(in, &f)) return fail(r, 0, PS_STRUCT);
    if (f.window_size > ((wopt & WALK_LONG_WINDOW) ? MAX_WIN_SIZE_LONG : MAX_WIN_SIZE))
      return fail(ZD_E_WINDOW_SIZE_TOO_BIG, 0, PS_STRUCT);
    for (uint32_t bi = 0;; bi++) {
      const uint8_t* h;
      if (int r = in.slice(3, &h)) return fail(r, bi, PS_STRUCT);
      uint32_t x = h[0] | (h[1] << 8) | ((uint32_t)h[2] << 16);
      HostBlock hb;
      zero_bytes(&hb, sizeof hb);
      hb.last = x & 1;
      hb.type = (x >> 1) & 3;
      hb.size = x >> 3;
      hb.src = (uint64_t)(in.p - base);
#ifndef __HIP_DEVICE_COMPILE__
      // the next block (or frame) header: a cache miss that now overlaps
      // this block's own header parse
      if (hb.type != 1 && hb.size < in.n) __builtin_prefetch(in.p + hb.size);
#endif
      if (hb.type == 0) {
        const uint8_t* s;
        if (int r = in.slice(hb.size, &s)) return fail(r, bi, PS_STRUCT);
      } else if (hb.type == 1) {
        if (int r = in.u8(&hb.rle)) return fail(r, bi, PS_STRUCT);
      } else if (hb.type == 2) {
        const uint8_t* s;
        if (int r = in.slice(hb.size, &s)) return fail(r, bi, PS_STRUCT);
        CompBlock& cb = hb.cb;
        cb.src = hb.src;
        cb.size = hb.size;
        cb.block_in_frame = bi;
        cb.host_stage = PS_ALL;
        WalkErr e;
        int r = parse_compressed(base, hb.src, hb.size, &cb, &e, wopt);
        if (r) {
          cb.host_stage = (uint8_t)e.stage;
          push(hb);
          return fail(r, bi, e.stage);
        }
      } else {
        return fail(ZD_E_RESERVED_BLOCK_TYPE, bi, PS_STRUCT);
      }
      push(hb);
      if (hb.last) break;
    }
    if (f.has_checksum) {
      uint64_t cs;
      if (in.le(4, &cs)) return fail(ZD_E_MISSING_CHECKSUM, hf->nb, PS_STRUCT);
      f.checksum = (uint32_t)cs;
    }
  } else if ((f.magic ^ MAGIC_SKIP) <= 0x0F) {
    f.kind = ZD_FRAME_SKIPPABLE;
    uint64_t len;
    if (int r = in.le(4, &len)) return fail(r, 0, PS_STRUCT);
    const uint8_t* s;
    HostBlock hb;
    zero_bytes(&hb, sizeof hb);
    hb.src = (uint64_t)(in.p - base);
    if (int r = in.slice((size_t)len, &s)) return fail(r, 0, PS_STRUCT);
    hb.type = 4;
    hb.size = (uint32_t)len;
    hb.last = 1;
    push(hb);
  } else {
    return fail(ZD_E_UNRECOGNIZED_MAGIC, 0, PS_STRUCT);
  }
  f.src_size = (uint64_t)(in.p - base) - f.src_offset;
  return 0;
}

// A block sink that keeps nothing (the frames of a chunk that are walked only
// to be stepped over)
struct NoBlocks {
  ZD_HD size_t size() const { return 0; }
  ZD_HD void push(const HostBlock&) {}
};

// Walks one chunk of a batch (zd_batch_create): `in` is the chunk, bounded by
// its own size.  A chunk is any number of skippable frames around exactly one
// zstd frame; that frame is indexed into *hf with its blocks in S, the
// skippable frames are stepped over.  A chunk without a zstd frame (no bytes,
// or skippable frames only) leaves *hf a frame of no blocks and no output.
// A chunk the walk cannot consume entirely this way fails as a whole -- the
// frame's own parse error, the walk's status at the bytes it stopped at
// (trailing bytes, a truncated frame), ZD_E_OUT_OF_DOMAIN at a second zstd
// frame -- and travels as hf->key, the route of a frame that fails to index.
template <typename SINK>
ZD_HD inline int index_chunk(const uint8_t* base, Bytes& in, HostFrame* hf, SINK& S, uint32_t wopt = 0) {
  zero_bytes(&hf->d, sizeof hf->d);
  hf->d.src_offset = (uint64_t)(in.p - base);
  hf->d.content_size = UINT64_MAX;
  hf->d.dict_id = UINT64_MAX;
  hf->d.kind = ZD_FRAME_SKIPPABLE;
  hf->b0 = (uint32_t)S.size();
  hf->nb = 0;
  hf->ncomp = 0;
  hf->key = KEY_NONE;
  hf->status = 0;
  bool have = false;
  auto fail = [&](int code) {
    hf->status = code;
    hf->key = make_key(PH_PARSE, 0, PS_STRUCT, 0, code);
    return code;
  };
  while (in.n) {
    const bool zstd = in.n >= 4 && ((uint32_t)in.p[0] | ((uint32_t)in.p[1] << 8) | ((uint32_t)in.p[2] << 16) |
                                    ((uint32_t)in.p[3] << 24)) == MAGIC_ZSTD;
    if (zstd) {
      if (have) return fail(ZD_E_OUT_OF_DOMAIN);
      if (int r = index_frame(base, in, hf, S, wopt)) return r;
      have = true;
    } else {
      // a skippable frame, or the walk's own failure (bytes that are no frame)
      HostFrame skip;
      NoBlocks none;
      if (int r = index_frame(base, in, &skip, none, wopt)) return fail(r);
    }
  }
  return 0;
}

// What a chunk needs of its destination: its reserve (zd_chunk_sizes_device,
// zd_batch_create_device_packed; the capacity pass of every batch checks
// against the same numbers).  `bound` is the sum over the frame's blocks of
// MAX_BLOCK_OUT for a compressed block, else the block's size; the frame's
// Frame_Content_Size is usable when present and <= bound.  The reserve is the
// usable Frame_Content_Size (*exact = 1), else bound (*exact = 0); a chunk
// without a zstd frame (no bytes, skippable frames only) or one the walk failed
// reserves nothing (0, *exact = 0).
ZD_HD inline uint64_t frame_bound(const HostFrame& hf, const HostBlock* blocks) {
  uint64_t bound = 0;
  for (uint32_t k = 0; k < hf.nb; k++) {
    const HostBlock& hb = blocks[hf.b0 + k];
    bound += hb.type == 2 ? MAX_BLOCK_OUT : hb.size;
  }
  return bound;
}
ZD_HD inline uint64_t chunk_reserve(const HostFrame& hf, uint64_t bound, uint8_t* exact) {
  *exact = 0;
  if (hf.d.kind != ZD_FRAME_ZSTD || hf.key != KEY_NONE) return 0;
  const bool usable = hf.d.content_size != UINT64_MAX && hf.d.content_size <= bound;
  *exact = usable ? 1 : 0;
  return usable ? hf.d.content_size : bound;
}
// The capacity pass of every batch, for an indexed zstd frame (kind
// ZD_FRAME_ZSTD, key KEY_NONE) and its chunk's capacity: a usable
// Frame_Content_Size above the capacity is ZD_E_DST_TOO_SMALL here (status and
// key), and nothing of the chunk runs.  Returns the chunk's bind flag: the
// capacity is below what the plan reserves for a frame without a usable one.
// (`cap` by reference: zd_k_batch_fit hands in its array's entry, read where
// it is used.)
ZD_HD inline bool chunk_fit(HostFrame& hf, const HostBlock* blocks, const uint64_t& cap) {
  const uint64_t bound = frame_bound(hf, blocks);
  const bool usable = hf.d.content_size != UINT64_MAX && hf.d.content_size <= bound;
  if (usable && hf.d.content_size > cap) {
    hf.status = ZD_E_DST_TOO_SMALL;
    hf.key = make_key(PH_LIMIT, 0, 0, 0, ZD_E_DST_TOO_SMALL);
  }
  return !usable && cap < bound;
}

// A block sink that keeps the frame's bound and block count and no block:
// index_chunk over it gives a chunk's reserve with no index stored (the
// skippable frames of a chunk never reach a chunk's sink, index_chunk steps
// over them with NoBlocks).  It touches no byte of the chunk itself: the walk
// over it reads what Bytes hands out, nothing else.
struct WalkBound {
  uint64_t bound = 0;
  uint32_t n = 0;
  ZD_HD size_t size() const { return n; }
  ZD_HD void push(const HostBlock& hb) {
    n++;
    bound += hb.type == 2 ? MAX_BLOCK_OUT : hb.size;
  }
};

// One chunk's size query: the header walk of [src, src + size) in place
// (base = in.p = src, so every read is inside the chunk: Bytes is bounds-checked
// and index_chunk peeks four bytes only when four are left), the walk's status
// and the reserve.
ZD_HD inline int chunk_size_query(const uint8_t* src, size_t size, uint32_t wopt, uint64_t* reserve,
                                  uint8_t* exact) {
  Bytes in{src, size};
  HostFrame hf;
  WalkBound sink;
  const int st = index_chunk(src, in, &hf, sink, wopt);
  *reserve = chunk_reserve(hf, sink.bound, exact);
  return st;
}

ZD_HD inline bool magic_word(uint32_t m) { return m == MAGIC_ZSTD || (m ^ MAGIC_SKIP) <= 0x0F; }

// The device walk's per-range summary (zd_k_walk, count pass): where the
// range's chain starts and ends, its status and sizes; the fill pass writes
// the range's frames and blocks at f_off / b_off.
struct WalkRange {
  uint64_t p0;          // first frame start of the chain (a magic number in the range), or the range end
  uint64_t end;         // where the chain stopped (first frame start >= range end, or past a failing frame)
  uint64_t f_off, b_off;
  uint32_t nframes, nblocks;
  int32_t status;
  uint32_t pad;
};

}  // namespace zd
