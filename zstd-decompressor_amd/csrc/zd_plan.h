// zd_plan.h — the per-frame descriptor pass of the planner, shared by the
// host planner (zd_host.cpp build_plan, per part on the worker threads) and the
// device planner (zd_kernels.hip zd_k_plan_count / zd_k_plan_fill, one lane per
// frame, zd_plan_create_device): one source, so the two plans cannot drift.
#pragma once
#include <stdint.h>

#include "../../include/zd.h"
#include "zd_common.h"
#include "zd_route.h"
#include "zd_walk.h"

namespace zd {

constexpr uint32_t K4F_CAP_BYTES = 128u << 10;   // frames up to this output size execute in LDS (K4F)

template <typename T>
ZD_HD inline T plan_min(T a, T b) { return a < b ? a : b; }
ZD_HD inline uint64_t plan_align(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// K4J (block-parallel execute, pointer jumping) takes the frames of at least
// K4J_MIN_BLOCKS compressed blocks: the streaming K4 runs a frame's blocks one
// after another on one wave, which a frame of many blocks cannot hide behind
// other frames unless the plan holds thousands of them
// (K4J_MAX_FRAMES).  ZD_K4J=1 / 0 forces it on (every frame with a
// compressed block) / off.
constexpr uint32_t K4J_MIN_BLOCKS = 16;
constexpr uint64_t K4J_MAX_FRAMES = 1024;
// A plan of few frames leaves the GPU nearly idle with one wave per frame on
// the streaming K4 (the reference's moby-dick sample: one frame of 10 blocks,
// 159k sequences on one wave): there K4J takes every frame of 2 or more
// compressed blocks.
constexpr uint64_t K4J_FEW_FRAMES = 64;
constexpr uint32_t K4J_MIN_BLOCKS_FEW = 2;

// Running indices of build_plan: every array it fills grows frame by frame,
// so a frame's entries start at the counts of the frames before it.
// (all u64, so that the device build scans them as PLAN_FIELDS words)
struct PlanCounts {
  uint64_t frames = 0, blocks = 0, comps = 0, luts = 0, fses = 0, lits = 0, nrec = 0, nseq = 0, out = 0;
  uint64_t tables = 0, huf = 0, seq = 0, k4f = 0, copies = 0;
  uint64_t jframes = 0, jblk = 0, jseg = 0;
  uint64_t inexact = 0;          // frames whose capacity is an upper bound (no usable FCS)
  uint64_t jwords = 0;           // K4J state words: a frame's region starts a 16-word piece, 16 words of slack after
  uint64_t jpieces = 0;          // K4J 16-byte pieces over the frames' regions
  uint64_t k0only = 0;           // frames K0 copies whole (every block raw / RLE): no K4 for them
  uint64_t csums = 0;            // zstd frames that carry a Content_Checksum (zd_k_verify runs when there is one)
  ZD_HD bool exact() const { return inexact == 0; }
  ZD_HD void add(const PlanCounts& o) {
    frames += o.frames; blocks += o.blocks; comps += o.comps; luts += o.luts; fses += o.fses; lits += o.lits;
    nrec += o.nrec; nseq += o.nseq; out += o.out; tables += o.tables; huf += o.huf; seq += o.seq; k4f += o.k4f;
    copies += o.copies; jframes += o.jframes; jblk += o.jblk; jseg += o.jseg; inexact += o.inexact;
    jwords += o.jwords; jpieces += o.jpieces; k0only += o.k0only; csums += o.csums;
  }
};
constexpr int PLAN_FIELDS = 22;
static_assert(sizeof(PlanCounts) == PLAN_FIELDS * 8, "PlanCounts: u64 fields only");

// One dictionary of a dictionary-set plan (zd_plan_create_dicts), as the
// per-frame pass needs it.  A plan's table holds the dictionaries that some
// frame of the plan uses, sorted by ID (a raw-content dictionary, ID 0, first).
struct PlanDict {
  uint32_t dict_id;        // 0: raw content (only ever the fallback)
  int32_t comp;            // the prebuilt comp carrying its tables, -1 for raw content
  uint64_t content;        // content size
  uint64_t rep[3];
};

// Plan-wide inputs of the per-frame pass.  `prev_*` seed the Treeless/Repeat
// resolution (context API), -1 when absent.
struct PlanCtx {
  int32_t prev_huf;
  int32_t prev_tab[3];
  uint64_t out_len0, fixed_cap, cap0;
  const HostFrame* cap0_frame;   // the plan's first frame (cap0 applies to it)
  uint64_t rep0[3];
  uint32_t flags;
  bool k4f_on, k4j_auto;
  bool fused;              // zd_k_fused plan: no K4F, 128-byte aligned literal and record slots
  int k4j_mode;
  uint32_t k4j_min;        // compressed blocks a frame needs for K4J (automatic mode)
  // ZD_F_AUTO_EXECUTOR in a prefix or chain batch without a forcing flag
  // (zd_route.h auto_exec; k4j_mode is 0 then): each frame is routed by
  // plan_auto_j, with k4j_min the rule's minimum at the batch's width
  // (auto_min_blocks) and k4j_auto its candidates within the cap
  // (auto_candidates_ok); a chain batch has j_at below as well
  bool auto_exec;
  // A dictionary plan (zd_plan_create_dict): out_len0 is the dictionary's
  // content size, positions before the frame that live in the dictionary's
  // buffer, not in the output: a frame's region starts at its own first byte
  // (K0's destinations, FrameState::out_len and the capacity count the
  // frame's own bytes).  dict_id: the dictionary's ID (0: raw content).
  bool dict;
  uint32_t dict_id;
  // A dictionary or dictionary-set plan created with ZD_F_DICT_BLOCK_PARALLEL
  // (zd_route.h dict_j; false everywhere else, and never with prefix_bytes):
  // a frame with a compressed block may go to K4J behind its dictionary -- all
  // of them with k4j_mode 1, with auto_exec those plan_auto_j names (k4j_min
  // the rule's minimum at the plan's frame count, k4j_auto its candidates
  // within the cap), none with neither.  Such a J frame keeps out_len0, the
  // repeat offsets and the previous tables of its dictionary (the plan-wide
  // fields, or its own PlanDict entry), and JFrame::src names the entry.
  bool dict_j;
  // Optional per-frame placement (a batch; null everywhere else): host arrays
  // in the host planner (zd_batch_create), device arrays in the device planner
  // (zd_batch_create_device).  Frame fi's output starts at
  // place_out[fi] from the output base instead of the running offset, and its
  // capacity is at most place_cap[fi].
  const uint64_t* place_out;
  const uint64_t* place_cap;
  // Optional dictionary table (a dictionary-set plan, zd_plan_create_dicts /
  // zd_batch_create_dicts, and on the device zd_batch_create_device_dicts; null
  // everywhere else; `dict` is set with it): every frame takes out_len0, its first repeat
  // offsets and its previous tables from the entry of its own Dictionary_ID
  // instead of the plan-wide fields above.  A frame without an ID (or with ID
  // 0) takes entry dset_fallback, or none at all when that is -1: it then
  // decodes like a frame of a plan without a dictionary.  Frame fi's entry
  // index goes to Sink::frame_dict (ndset: none).
  const PlanDict* dset;
  uint32_t ndset;
  int32_t dset_fallback;
  // Optional per-frame prefix sizes (a prefix batch, zd_batch_create_prefix:
  // host array; zd_batch_create_device_prefix: device array; null everywhere
  // else; `dict` is set with it, never `dset`): frame fi decodes against its own
  // raw-content prefix of prefix_bytes[fi] bytes (0: none) -- out_len0 is that
  // size, the first repeat offsets are 1, 4, 8, there are no previous tables,
  // and a frame that names a Dictionary_ID is ZD_E_DICT_MISMATCH.  With
  // k4j_mode 1 (a batch created with ZD_F_BLOCK_PARALLEL, no chain: zd_route.h
  // k4j_mode_behind; a chain batch created with ZD_F_CHAIN_BLOCK_PARALLEL:
  // k4j_mode_plan, with j_at below) every such frame with a compressed block
  // goes to K4J; with auto_exec the frames that plan_auto_j names.
  const uint64_t* prefix_bytes;
  // Optional K4J numbering (a chain batch created with ZD_F_CHAIN_BLOCK_PARALLEL
  // or routed by ZD_F_AUTO_EXECUTOR; null everywhere else): frame fi's K4J
  // entries start at j_at[PLAN_J_COLS * fi ...] -- its JFrame, first J block, first segment, first state word, first
  // piece (PlanJ order) -- instead of at the running counts, so that the J
  // frames are numbered level-major (plan_j_order) and every level of the chain
  // owns one contiguous range of each.  The running counts advance as ever
  // (the totals, and the per-frame counts that plan_j_order scans).
  const uint64_t* j_at;
};

// The K4J fields of a plan's PlanCtx from its flags and shape (plan_ctx; host
// only).  `width`: the chunks that execute together, what ZD_F_AUTO_EXECUTOR's
// minimum reads (a prefix batch's count, a chain batch's widest level; unused
// elsewhere).  plan_k4j_min is known before the walk's frames are looked at;
// `candidates` are the frames without a walk-found error and with at least that
// many compressed blocks, counted where plan_k4j_counts says a rule reads them.
inline uint32_t plan_k4j_min(uint32_t flags, bool prefix, bool chain, uint64_t nframes, uint64_t width,
                             bool dict_j = false) {
  return auto_exec(flags, prefix, chain) || dict_j ? auto_min_blocks(width)
         : nframes <= K4J_FEW_FRAMES    ? K4J_MIN_BLOCKS_FEW
                                        : K4J_MIN_BLOCKS;
}
inline bool plan_k4j_counts(uint32_t flags, const RouteEnv& E, bool prefix, bool chain, uint64_t out_len0,
                            bool dict_j = false) {
  if (dict_j) return dict_j_mode(flags) < 0;
  return auto_exec(flags, prefix, chain) || (k4j_mode_of(flags, E) < 0 && out_len0 == 0);
}
inline void plan_k4j_fields(PlanCtx& X, uint32_t flags, const RouteEnv& E, bool dict, bool prefix, bool chain,
                            uint64_t out_len0, uint64_t nframes, uint64_t width, uint64_t candidates,
                            bool dict_j = false) {
  X.dict_j = dict_j;
  X.k4j_mode = k4j_mode_of(flags, E);
  X.k4j_min = plan_k4j_min(flags, prefix, chain, nframes, width, dict_j);
  X.k4j_auto = X.k4j_mode < 0 && out_len0 == 0 && candidates > 0 && candidates <= K4J_MAX_FRAMES;
  X.auto_exec = false;
  if (dict) {
    X.auto_exec = auto_exec(flags, prefix, chain);
    X.k4j_auto = X.auto_exec && auto_candidates_ok(candidates);
    X.k4j_mode = k4j_mode_plan(X.k4j_mode, flags, true, prefix, chain);
  }
  if (dict_j) {
    // (the rule's width is the plan's frame count, its candidates the whole plan's)
    const int m = dict_j_mode(flags);
    X.auto_exec = m < 0;
    X.k4j_auto = X.auto_exec && auto_dict_candidates_ok(candidates);
    X.k4j_mode = m == 1 ? 1 : 0;
  }
}

// The K4J columns of PlanCounts, in j_at's order
constexpr int PLAN_J_COLS = 5;
enum PlanJ : int { PJ_FRAMES = 0, PJ_BLK = 1, PJ_SEG = 2, PJ_WORDS = 3, PJ_PIECES = 4 };

ZD_HD inline void plan_j_get(const PlanCounts& c, uint64_t j[PLAN_J_COLS]) {
  j[PJ_FRAMES] = c.jframes; j[PJ_BLK] = c.jblk; j[PJ_SEG] = c.jseg; j[PJ_WORDS] = c.jwords; j[PJ_PIECES] = c.jpieces;
}
// One level's share of K4J's grids in a flagged chain plan: its J frames,
// scatter segments and 16-byte pieces, each one contiguous range
struct JLevel { uint64_t jf0, njf, seg0, nseg, piece0, npieces; };
// Level-major K4J numbering: jcnt holds each frame's own K4J counts
// (PLAN_J_COLS words a frame, plan_frame's count pass), order[] the frames
// grouped by level with the levels ascending (count[l] frames of level l).
// j_at gets each frame's starts -- an exclusive scan of the counts in order[]
// order, which is what the device planner does with zd_k_scan_* over the
// gathered columns -- and lev[l] level l's ranges.  Returns the totals in tot.
inline void plan_j_order(const uint64_t* jcnt, const uint32_t* order, const uint32_t* count, uint32_t levels,
                         uint64_t* j_at, JLevel* lev, uint64_t tot[PLAN_J_COLS]) {
  uint64_t run[PLAN_J_COLS] = {0, 0, 0, 0, 0};
  uint64_t q = 0;
  for (uint32_t l = 0; l < levels; l++) {
    JLevel L{run[PJ_FRAMES], 0, run[PJ_SEG], 0, run[PJ_PIECES], 0};
    for (uint32_t k = 0; k < count[l]; k++, q++) {
      const uint64_t f = order[q];
      for (int w = 0; w < PLAN_J_COLS; w++) { j_at[PLAN_J_COLS * f + w] = run[w]; run[w] += jcnt[PLAN_J_COLS * f + w]; }
    }
    L.njf = run[PJ_FRAMES] - L.jf0; L.nseg = run[PJ_SEG] - L.seg0; L.npieces = run[PJ_PIECES] - L.piece0;
    lev[l] = L;
  }
  for (int w = 0; w < PLAN_J_COLS; w++) tot[w] = run[w];
}
// The levels' ranges from their first entries (the device planner reads back
// start[3 * l + {0, 1, 2}] = level l's first J frame, segment and piece, set for
// the levels that have a frame) and the plan's totals
inline void plan_j_levels(const uint64_t* start, const uint32_t* count, uint32_t levels, uint64_t jframes,
                          uint64_t jseg, uint64_t jpieces, JLevel* lev) {
  uint64_t end[3] = {jframes, jseg, jpieces};
  for (uint32_t l = levels; l-- > 0;) {
    if (!count[l]) { lev[l] = JLevel{end[0], 0, end[1], 0, end[2], 0}; continue; }
    const uint64_t* s = start + 3 * (uint64_t)l;
    lev[l] = JLevel{s[0], end[0] - s[0], s[1], end[1] - s[1], s[2], end[2] - s[2]};
    end[0] = s[0]; end[1] = s[1]; end[2] = s[2];
  }
}

// ZD_F_AUTO_EXECUTOR's rule for one frame that K4J could take behind a prefix
// (plan_frame's j_ok): (a) at least min_blocks compressed blocks while the
// batch's candidates are within the cap (cand_ok), or (b) a frame the streaming
// executor's int32 positions cannot hold behind its prefix.  The one copy of the
// rule: both planners take it from plan_frame.
ZD_HD inline bool plan_auto_j(uint32_t ncomp, uint32_t min_blocks, bool cand_ok, uint64_t prefix, uint64_t cap) {
  return (cand_ok && ncomp >= min_blocks) || (prefix <= K4_MAX_FRAME_OUT && prefix + cap > K4_MAX_FRAME_OUT);
}

// The entry of Dictionary_ID id (non-zero) in a table sorted by ID, or -1.
ZD_HD inline int32_t plan_dict_find(const PlanDict* t, uint32_t n, uint64_t id) {
  uint32_t lo = 0, hi = n;
  while (lo < hi) {
    const uint32_t m = lo + (hi - lo) / 2;
    if (t[m].dict_id < id) lo = m + 1; else hi = m;
  }
  return (lo < n && t[lo].dict_id == id) ? (int32_t)lo : -1;
}

// Where the filling pass writes: the plan's host vectors (small plans, the
// context API) or the pinned upload staging at the workspace offsets.
struct Sink {
  CompBlock* comps;
  BlockRec* blocks;
  FrameDesc* fdesc;
  FrameState* fstate0;
  uint32_t *list_tables, *list_huf, *list_seq, *list_k4f;
  CopyDesc* copies;
  JFrame* jframes;
  JBlkDesc* jblkd;
  JSegDesc* jsegd;
  uint64_t *frame_out, *frame_cap;
  uint32_t* frame_dict;    // a dictionary-set plan: the frame's entry in the plan's table (PlanCtx::dset), else null
  uint64_t* frame_csum;    // a ZD_F_VERIFY_CHECKSUM plan: has << 32 | the frame's Content_Checksum, else null
};

// One frame's descriptors at the running indices c (build_plan).  FILL: the
// entries are written to S; otherwise c only advances (the counting pass).
// A K4J frame's descriptors (JFrame, its JBlkDesc and JSegDesc entries) are
// written here too, at the running K4J indices, so the host and the device
// build them alike; jm->note(n) gets each K4J frame's sequence count (the
// plan's pointer-jumping rounds follow the largest).
template <bool FILL, typename JOUT>
ZD_HD void plan_frame(const PlanCtx& X, const HostFrame& hf, const HostBlock* hblocks, PlanCounts& c, const Sink& S,
                      JOUT* jm) {
  const uint32_t fi = (uint32_t)c.frames;
  FrameDesc fd{};
  FrameState fs{};
  fs.key = hf.key;
  fs.rep[0] = X.rep0[0]; fs.rep[1] = X.rep0[1]; fs.rep[2] = X.rep0[2];
  fd.first_block = (uint32_t)c.blocks;
  uint64_t out_len0 = X.out_len0;
  int32_t huf_prev = X.prev_huf;
  int32_t tab_prev[3] = {X.prev_tab[0], X.prev_tab[1], X.prev_tab[2]};
  uint64_t bound = 0;
  bool seqs_in_frame = false;
  const bool names_dict = hf.d.kind == ZD_FRAME_ZSTD && hf.d.dict_id != UINT64_MAX && hf.d.dict_id != 0;
  uint32_t jsrc = 0;             // JFrame::src: the frame's entry among the plan's dictionary addresses
  if (X.dset) {
    // the frame's own dictionary: by its ID, else the fallback, else none (a
    // skippable frame: none, nothing of it reads one)
    int32_t e = -1;
    if (names_dict) e = plan_dict_find(X.dset, X.ndset, hf.d.dict_id);
    else if (hf.d.kind == ZD_FRAME_ZSTD) e = X.dset_fallback;
    if (names_dict && e < 0)
      fs.key = plan_min(fs.key, make_key(PH_PARSE, 0, PS_STRUCT, 0, ZD_E_DICT_MISMATCH));
    out_len0 = 0;
    fs.rep[0] = 1; fs.rep[1] = 4; fs.rep[2] = 8;
    huf_prev = tab_prev[0] = tab_prev[1] = tab_prev[2] = -1;
    if (e >= 0) {
      const PlanDict& d = X.dset[e];
      out_len0 = d.content;
      fs.rep[0] = d.rep[0]; fs.rep[1] = d.rep[1]; fs.rep[2] = d.rep[2];
      huf_prev = tab_prev[0] = tab_prev[1] = tab_prev[2] = d.comp;
    }
    jsrc = e >= 0 ? (uint32_t)e : X.ndset;
    if (FILL) S.frame_dict[fi] = jsrc;
  } else if (X.prefix_bytes) {
    // the frame's own prefix: raw content, so no ID fits it
    if (names_dict) fs.key = plan_min(fs.key, make_key(PH_PARSE, 0, PS_STRUCT, 0, ZD_E_DICT_MISMATCH));
    out_len0 = X.prefix_bytes[fi];
    fs.rep[0] = 1; fs.rep[1] = 4; fs.rep[2] = 8;
    huf_prev = tab_prev[0] = tab_prev[1] = tab_prev[2] = -1;
  } else if (X.dict && names_dict && hf.d.dict_id != X.dict_id) {
    // a frame that names another dictionary stops the plan like a frame that
    // failed to index (no block of it is planned to run)
    fs.key = plan_min(fs.key, make_key(PH_PARSE, 0, PS_STRUCT, 0, ZD_E_DICT_MISMATCH));
  }
  fd.out_len0 = out_len0;
  const bool frame_failed_host = fs.key != KEY_NONE;
  const bool rfc = (X.flags & ZD_F_RFC) != 0;
  // bytes of the frame's region before its first own byte (the context API's existing output)
  const uint64_t own0 = X.dict ? 0 : out_len0;
  uint64_t jseg = 0;
  // a re-plan of a frame that overran (zd_plan_decompress): by identity, the
  // counting pass numbers each part's frames from 0
  const bool replanned = X.cap0 && &hf == X.cap0_frame && hf.d.kind == ZD_FRAME_ZSTD;
  for (uint32_t bi = 0; bi < hf.nb; bi++) {
    const HostBlock& hb = hblocks[hf.b0 + bi];
    BlockRec br{};
    br.src = hb.src; br.size = hb.size; br.type = hb.type; br.last = hb.last; br.rle = hb.rle; br.comp = -1;
    if (hb.type == 2) {
      CompBlock cb = hb.cb;
      cb.frame = fi;
      cb.block_in_frame = bi;
      cb.prebuilt = 0;
      cb.rfc = rfc ? 1 : 0;
      cb.huf_src = -1;
      cb.tab_src[0] = cb.tab_src[1] = cb.tab_src[2] = -1;
      const uint32_t ci = (uint32_t)c.comps;
      const bool failing = cb.host_stage != PS_ALL;
      // literals: Treeless resolution (literals.rs:59-66)
      if (!failing && (cb.lit_type == LIT_COMPRESSED || cb.lit_type == LIT_TREELESS)) {
        if (cb.lit_type == LIT_COMPRESSED) { cb.huf_src = (int32_t)ci; huf_prev = (int32_t)ci; }
        else cb.huf_src = huf_prev;
        if (cb.huf_src < 0)
          fs.key = plan_min(fs.key, make_key(PH_DECODE, bi, DS_LITERALS, 0, ZD_E_HUFFMAN_DECODER_MISSING));
      }
      if (cb.lit_type == LIT_COMPRESSED && cb.host_stage > PS_HUF_DESC) cb.lut_slot = (uint32_t)c.luts++;
      // sequences: Repeat resolution (sequences.rs:147-187, 232-234)
      if (!failing) {
        if (cb.nseq == 0 && rfc) {
          // RFC 8878 (D2): the block's literals are its output; it builds no
          // table and leaves tab_prev, so a later Repeat_Mode reaches across it
          // (huf_prev above moves only with a tree of the block's own)
        } else if (cb.nseq == 0) {
          int code = ZD_E_EMPTY_INPUT_DATA;
          for (int k = 0; k < 3; k++) if (tab_prev[k] < 0) { code = ZD_E_NO_PREVIOUS_DECODER; break; }
          fs.key = plan_min(fs.key, make_key(PH_DECODE, bi, DS_SEQUENCES, 0, code));
        } else {
          cb.fse_slot = (uint32_t)c.fses++;
          bool miss = false;
          for (int k = 0; k < 3; k++) {
            if (cb.modes[k] == M_REPEAT) {
              if (tab_prev[k] < 0) { miss = true; break; }
              cb.tab_src[k] = tab_prev[k];
            } else {
              cb.tab_src[k] = (int32_t)ci;
            }
          }
          if (miss) fs.key = plan_min(fs.key, make_key(PH_DECODE, bi, DS_SEQUENCES, 0, ZD_E_NO_PREVIOUS_DECODER));
          else for (int k = 0; k < 3; k++) tab_prev[k] = cb.tab_src[k];
        }
      } else if (cb.nseq) {
        cb.fse_slot = (uint32_t)c.fses++;
      }
      // workspace
      if (cb.lit_type == LIT_COMPRESSED || cb.lit_type == LIT_TREELESS) {
        cb.lit_extra = 0;
        if (replanned) {             // a symbol is at least one bit: <= 8 literals per stream byte
          uint64_t most = 0;
          for (int k = 0; k < cb.nstreams; k++) most += 8ull * cb.stream_size[k];
          if (most > cb.lit_regen) cb.lit_extra = (uint32_t)(most - cb.lit_regen);
        }
        cb.lit_out = c.lits;
        c.lits += plan_align((uint64_t)cb.lit_regen + 32 + cb.lit_extra, X.fused ? 128 : 16);   // + K2's 16-byte slack
      }
      if (X.fused) c.nrec = plan_align(c.nrec, 16);   // a block's records start a 128-byte line
      cb.seq_out = c.nrec;
      c.nseq += cb.nseq;
      c.nrec += rec_slots(cb.nseq);              // record pairs, a spare pair past the block's last
      seqs_in_frame |= cb.nseq > 0;
      br.comp = (int32_t)ci;
      jseg += cb.nseq > J_SEG ? (cb.nseq + J_SEG - 1) / J_SEG : 1;
      const bool needs_tables = (cb.lit_type == LIT_COMPRESSED && cb.host_stage > PS_HUF_DESC) ||
                                (cb.nseq > 0 && cb.host_stage > PS_SEQ_TABLES);
      if (needs_tables) { if (FILL) S.list_tables[c.tables] = ci; c.tables++; }
      if (!frame_failed_host) {
        if ((cb.lit_type == LIT_COMPRESSED || cb.lit_type == LIT_TREELESS) && cb.nstreams && cb.huf_src >= 0) {
          if (FILL) S.list_huf[c.huf] = ci;
          c.huf++;
        }
        if (cb.nseq > 0 && cb.tab_src[0] >= 0 && cb.tab_src[1] >= 0 && cb.tab_src[2] >= 0) {
          if (FILL) S.list_seq[c.seq] = ci;
          c.seq++;
        }
      }
      if (FILL) S.comps[ci] = cb;
      c.comps++;
      bound += MAX_BLOCK_OUT;
    } else {
      bound += hb.size;
      jseg += 1;
    }
    if (FILL) S.blocks[c.blocks] = br;
    c.blocks++;
  }
  if (X.fused) c.nrec = plan_align(c.nrec, 16);   // (the next frame's records start a line: per-frame counts scan)
  fd.nblocks = hf.nb;
  uint64_t cap;
  if (hf.d.kind == ZD_FRAME_SKIPPABLE) {
    // a truncated skippable frame fails to index and keeps no payload block
    cap = ((X.flags & ZD_F_SKIPPABLE) && hf.nb) ? hblocks[hf.b0].size : 0;
    if (!(X.flags & ZD_F_SKIPPABLE)) fd.nblocks = 0;
  } else if (hf.d.content_size != UINT64_MAX && hf.d.content_size <= bound) {
    cap = hf.d.content_size;
  } else {
    cap = bound;
    c.inexact = 1;
  }
  if (frame_failed_host) fd.nblocks = 0;
  if (X.fixed_cap) cap = X.fixed_cap;
  if (replanned) {
    cap = X.cap0;
    c.inexact = 1;
  }
  uint64_t out = c.out;
  if (X.place_out) {
    out = X.place_out[fi];
    cap = plan_min(cap, X.place_cap[fi]);
  }
  // a prefix the streaming K4's int32 positions cannot hold (with the frame's
  // capacity, sequences or not: the frame starts at the prefix's size): no
  // block of the frame runs, and a size past the limit itself is not even kept
  // (K4 truncates out_len0 to 32 bits).  A frame that a prefix batch created
  // with ZD_F_BLOCK_PARALLEL sends to K4J keeps only the prefix's own limit:
  // K4J's state words number the frame's own bytes from 0 and never hold a
  // prefix position.  ZD_F_AUTO_EXECUTOR (j_auto): of the frames the flag could
  // send there, those the rule names.
  // A dictionary plan created with ZD_F_DICT_BLOCK_PARALLEL (dict_j): the same
  // three lines with the dictionary's content for the prefix -- it is at most
  // ZD_DICT_MAX_CONTENT, so only the capacity can keep a frame off K4J, and the
  // limit below stays the prefix batches' alone (a dictionary frame K4J does
  // not take is keyed further down, as it always was)
  const bool j_ok = (X.prefix_bytes || X.dict_j) && !frame_failed_host && fd.nblocks && hf.ncomp &&
                    hf.d.kind == ZD_FRAME_ZSTD && cap <= K4J_MAX_FRAME_OUT;
  const bool j_auto = X.auto_exec && j_ok && plan_auto_j(hf.ncomp, X.k4j_min, X.k4j_auto, out_len0, cap);
  const bool j_pfx = j_ok && (X.k4j_mode == 1 || j_auto);
  if (X.prefix_bytes && out_len0 &&
      (out_len0 > K4_MAX_FRAME_OUT || (!j_pfx && cap + out_len0 > K4_MAX_FRAME_OUT))) {
    fs.key = plan_min(fs.key, make_key(PH_LIMIT, 0, 0, 0, ZD_E_OUT_OF_DOMAIN));
    fd.nblocks = 0;
    if (out_len0 > K4_MAX_FRAME_OUT) fd.out_len0 = out_len0 = 0;
  }
  fd.out = out;
  fd.out_cap = cap;
  // K4J: frames of many compressed blocks, and any frame past the streaming
  // K4's int32 positions (distances, zd_common.h); behind a prefix only on
  // request (j_pfx: the scatter writes the bytes that come from the prefix)
  const bool to_j = (out_len0 == 0 || j_pfx) && !frame_failed_host && fd.nblocks && hf.ncomp && hf.d.kind == ZD_FRAME_ZSTD &&
                    cap <= K4J_MAX_FRAME_OUT &&
                    (j_auto || (X.k4j_mode >= 0 ? X.k4j_mode == 1
                                                : ((X.k4j_auto && hf.ncomp >= X.k4j_min) || cap > K4_MAX_FRAME_OUT)));
  // larger frames with sequences that K4J does not take (forced off, or past
  // its 32 GiB) are outside the GPU path's domain
  if (!to_j && cap + (X.dict ? out_len0 : 0) > K4_MAX_FRAME_OUT && seqs_in_frame)
    fs.key = plan_min(fs.key, make_key(PH_LIMIT, 0, 0, 0, ZD_E_OUT_OF_DOMAIN));
  if (to_j) {
    fd.lds = 2;
    // the frame's K4J indices: the running ones, or its level-major places
    uint64_t J[PLAN_J_COLS];
    plan_j_get(c, J);
    if (X.j_at) for (int w = 0; w < PLAN_J_COLS; w++) J[w] = X.j_at[PLAN_J_COLS * (uint64_t)fi + w];
    uint64_t nseq = 0;
    uint32_t njs = (uint32_t)J[PJ_SEG];
    for (uint32_t k = 0; k < fd.nblocks; k++) {
      const HostBlock& hb = hblocks[hf.b0 + k];
      const uint32_t bn = hb.type == 2 ? hb.cb.nseq : 0u;
      nseq += bn;
      if (FILL) {
        JBlkDesc d{};
        d.block = fd.first_block + k;
        d.jframe = (uint32_t)J[PJ_FRAMES];
        d.j = k;
        d.seg0 = njs;
        for (uint32_t g = 0; g == 0 || g * J_SEG < bn; g++) S.jsegd[njs++] = JSegDesc{(uint32_t)J[PJ_BLK] + k, g};
        S.jblkd[J[PJ_BLK] + k] = d;
      }
    }
    if (FILL) {
      JFrame jf{};
      jf.base = J[PJ_WORDS];                   // word index: frame pieces of 16 words are 64-byte lines
      jf.cap = cap;
      jf.piece0 = J[PJ_PIECES];
      jf.frame = fi;
      jf.jb0 = (uint32_t)J[PJ_BLK];
      jf.njb = fd.nblocks;
      jf.src = jsrc;
      S.jframes[J[PJ_FRAMES]] = jf;
    }
    if (jm) jm->note(nseq);
    c.jframes++;
    c.jblk += fd.nblocks;
    c.jseg += jseg;
    c.jwords += plan_align(cap + 16, 16);
    c.jpieces += (cap + 15) / 16;
  } else {
    // K4F (whole frame resident in LDS, one 1024-thread workgroup per frame)
    // executes the frames that fit it in plans of 256-768 frames, where the
    // streaming K4 runs one round at its batch latency (C3: 0.64 vs 0.75 ms);
    // it is slower on C4 (EXPERIMENTS.md).  ZD_K4F=1 / 0 forces it on / off.
    fd.lds = (X.k4f_on && out_len0 == 0 && cap <= K4F_CAP_BYTES) ? 1u : 0u;
  }
  if (fd.lds == 1) { if (FILL) S.list_k4f[c.k4f] = fi; c.k4f++; }
  // Leading raw / RLE blocks (skippable payloads too) have output offsets
  // known here: K0 copies them in parallel pieces, the streaming K4 starts
  // after them (a frame of raw/RLE blocks only never reaches K4's loop).
  if (!fd.lds && fd.nblocks && cap < 0x7FF00000ull) {
    uint64_t pre = 0;
    uint32_t k = 0;
    for (; k < fd.nblocks; k++) {
      const HostBlock& hb = hblocks[hf.b0 + k];
      if (hb.type != 0 && hb.type != 1 && hb.type != 4) break;
      if (own0 + pre + hb.size > cap) break;
      for (uint64_t x = 0; x < hb.size; x += COPY_PIECE) {
        if (FILL) {
          CopyDesc cd{};
          cd.src = hb.src + (hb.type == 1 ? 0 : x);
          cd.dst = out + own0 + pre + x;
          cd.size = (uint32_t)plan_min<uint64_t>(COPY_PIECE, hb.size - x);
          cd.fill = hb.type == 1 ? (0x100u | hb.rle) : 0u;
          S.copies[c.copies] = cd;
        }
        c.copies++;
      }
      pre += hb.size;
    }
    fd.skip = k;
    fd.skip_bytes = pre;
    // every block copied by K0: the frame's length is known here, and no
    // executor runs it (a launch less when no frame needs the streaming K4)
    if (k == fd.nblocks && fs.key == KEY_NONE) {
      fd.lds = 3;
      fs.out_len = own0 + pre;
      c.k0only++;
    }
  }
  // the stored Content_Checksum, for zd_k_verify (a frame that failed to index has none to check)
  const bool has_csum = hf.d.kind == ZD_FRAME_ZSTD && hf.d.has_checksum && !frame_failed_host;
  if (has_csum) c.csums++;
  if (FILL && S.frame_csum) S.frame_csum[fi] = has_csum ? (1ull << 32) | hf.d.checksum : 0;
  if (FILL) {
    S.frame_out[fi] = out;
    S.frame_cap[fi] = cap;
    S.fdesc[fi] = fd;
    S.fstate0[fi] = fs;
  }
  c.out += cap;
  c.frames++;
}

// A batch's per-chunk arrays (zd_host.cpp zd_batch::d_arr): one allocation,
// carved here into byte offsets, array after array (n entries each unless
// said otherwise).  Host arrays (zd_batch_create): src | size | off | out |
// pieces (npieces GatherPiece slots of 8 bytes) are the head the host uploads,
// [head_bytes, total) is zeroed and written by the device.  Device arrays
// (zd_batch_create_device): piece0 follows off (BatchArrays: the layout scans
// the two as adjacent columns), cap and flag are the chunks' capacities and
// CHUNK_* flags, scratch the scans' 2 * (tiles + 1) + 1 words (tiles of 256
// chunks), res the four words that come back, and a prefix batch keeps the
// checked prefix addresses and sizes after everything else.  ABSENT: an
// array the kind of batch does not have.
struct BatchCarve {
  static constexpr uint64_t ABSENT = UINT64_MAX;
  uint64_t src = 0, size = 0, off = 0, out = 0;           // u64
  uint64_t boff = 0, len = 0, hash = 0;                   // u64
  uint64_t status = 0, nblk = 0;                          // i32, u32
  uint64_t bind = 0;                                      // u8
  uint64_t pieces = ABSENT, head_bytes = 0;               // host arrays
  uint64_t piece0 = ABSENT, cap = ABSENT;                 // device arrays: u64
  uint64_t flag = ABSENT;                                 //   u8
  uint64_t scratch = ABSENT, res = ABSENT;                //   u64 words
  uint64_t pfx = ABSENT, pfx_bytes = ABSENT;              //   u64, a prefix batch
  // a chain batch (zd_batch_create_chain), last of all so that every other
  // batch's carve is what it was: the checked parent of each chunk (i32, -1:
  // none), the chunks grouped by level (u32), and with device arrays the
  // levels' counts and fill cursors (2 * 256 u32), the links (u32, and one of
  // padding) and each chunk's level (u8)
  uint64_t par = ABSENT, order = ABSENT, lcount = ABSENT, lvl = ABSENT;
  uint64_t scratch_words = 0;
  uint64_t total = 0;

  void carve(uint64_t n, bool on_device, uint64_t npieces, bool prefixes, bool chain = false) {
    uint64_t o = 0;
    auto take = [&o](uint64_t bytes) { const uint64_t at = o; o += bytes; return at; };
    src = take(8 * n); size = take(8 * n); off = take(8 * n);
    if (on_device) {
      piece0 = take(8 * n); out = take(8 * n); cap = take(8 * n);
    } else {
      out = take(8 * n); pieces = take(8 * npieces);
      head_bytes = o;
    }
    boff = take(8 * n); len = take(8 * n); hash = take(8 * n);
    status = take(4 * n); nblk = take(4 * n);
    bind = take(n);
    if (on_device) {
      flag = take(n);
      o = plan_align(o, 8);
      scratch_words = 2 * ((n + 255) / 256 + 1) + 1;
      scratch = take(8 * scratch_words); res = take(8 * 4);
      if (prefixes) { pfx = take(8 * n); pfx_bytes = take(8 * n); }
    } else {
      o = bind + plan_align(n, 8);
    }
    if (chain) {
      par = take(4 * n); order = take(4 * n);
      if (on_device) { lcount = take(4 * (2 * 256 + 2)); lvl = take(n); }
      o = plan_align(o, 8);
    }
    total = o;
  }
};


}  // namespace zd
