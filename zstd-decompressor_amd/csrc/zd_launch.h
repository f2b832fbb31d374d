// zd_launch.h — host-side entry points of the gfx950 kernels: launch_pipeline,
// launch_reset, launch_dict_tables and launch_compact in zd_pipeline.hip, the
// seekable layer's in zd_seek.hip, the multi-frame batch's in zd_multi.hip,
// the others beside their kernels in zd_kernels.hip (the one translation
// unit, which includes the three files).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "zd_common.h"
#include "zd_plan.h"
#include "zd_route.h"

namespace zd {

struct LaunchArgs {
  const uint8_t* src;      // d_src
  uint64_t src_size;
  uint8_t* out;            // output base (d_dst or the plan's staging buffer)
  uint8_t* ws;             // workspace base
  Workspace W;
  uint32_t n_tables, n_huf, n_seq, n_frames, n_k4f, n_copies;
  hipStream_t stream;
  LaunchRoute route;       // what to launch and where (zd_route.h); the resources below only serve it
  hipEvent_t* events = nullptr;   // route.profiling 1: N_KERNELS + 1 events recorded around the kernels
  hipStream_t aux = nullptr;      // route.fork / route.k1_fork: the second stream and its two events
  hipEvent_t fork = nullptr, join = nullptr;
  uint32_t n_jframes = 0, n_jblk = 0, n_jseg = 0;   // K4J frames / their blocks / scatter segments
  uint32_t n_k0only = 0;                   // frames K0 copies whole (FrameDesc::lds 3)
  uint32_t j_rounds = 0;                   // K4J pointer-jumping rounds launched
  uint64_t j_pieces = 0;                   // 16-byte pieces over the K4J frames' regions
  uint32_t cus = 256;                      // compute units of the device (K4J rounds' grid)
  // route.profiling 2 (zd_plan_set_profiling mode 2): an event pair recorded
  // on `stream` around each launch group that can carry a plan's work -- K0,
  // zd_k_fused, K4, K4F, the K4J kernels (kDomNames) -- with the fork and
  // fusion kept; bit g of *dom_used is set when group g launched
  hipEvent_t* dom_events = nullptr;
  uint32_t* dom_used = nullptr;
  // route.k4 == K4_DICT (zd_plan_create_dict): the dictionary's content on the
  // device (frame positions [0, FrameDesc::out_len0)).  A dictionary-set plan
  // (K4_DICT_SET) takes each frame's from the workspace's table
  // (Workspace::dict_ptrs, ::frame_dict), a prefix batch (K4_PREFIX) frame f's
  // prefix from dict_ptrs[f]
  const uint8_t* dict = nullptr;
  // K4_DICT with K4J frames (ZD_F_DICT_BLOCK_PARALLEL): that address in device
  // memory, the one-entry table zd_k_jscatter reads through JFrame::src (a set
  // plan's table is Workspace::dict_ptrs)
  const uint8_t* const* dict_tab = nullptr;
  // route.k4 == K4_CHAIN (zd_batch_create_chain): the frames grouped by level
  // (device, n_frames entries), each frame's parent (device, -1: none) and the
  // levels' frame counts (host, chain_levels entries; level l's frames are
  // chain_order[sum of the counts below l ...]).  Prefix addresses as K4_PREFIX.
  const uint32_t* chain_order = nullptr;
  const int32_t* chain_parent = nullptr;
  const uint32_t* chain_count = nullptr;
  uint32_t chain_levels = 0;
  // a chain batch created with ZD_F_CHAIN_BLOCK_PARALLEL (null otherwise): level
  // l's J frames, scatter segments and pieces (host, chain_levels entries), one
  // contiguous range each (zd_plan.h plan_j_order); W.jpend then holds
  // jpend_chain_words(chain_levels) words, three a level
  const JLevel* chain_j = nullptr;
};
// W.jpend's u32 words: a pointer-jumping counter per round, or three per level of a flagged chain plan
constexpr uint32_t JPEND_WORDS = (uint32_t)(J_MAX_ROUNDS + 1);
inline uint32_t jpend_chain_words(uint32_t levels) { return 3 * (levels ? levels : 1u); }

// K1 table parse/build -> K2 Huffman literals -> K3 FSE sequences -> K4 execute.
hipError_t launch_pipeline(const LaunchArgs& a);

// zd_decode_async's state reset (frame / block states, K1 and K4J counters, K4J done flags).
// keep_comps: the leading block states left as they are (a dictionary plan's prebuilt comps)
hipError_t launch_reset(uint8_t* ws, const Workspace& W, uint64_t n_frames, uint64_t n_comps, bool k4j,
                        uint64_t j_pieces, hipStream_t s, uint32_t keep_comps = 0,
                        uint32_t jpend_words = (uint32_t)(J_MAX_ROUNDS + 1));

// zd_k_dict_tables' result (zd_dict_create reads it once)
struct DictTables {
  int32_t status;          // ZD_OK or the failing description's code
  uint32_t rep_off;        // byte offset of the three repeat offsets in the dictionary
  uint32_t huf_bits;       // maxBits of the Huffman tree
  uint8_t al[3];           // accuracy logs, LL | OF | ML
  uint8_t pad;
};
// The tables of a formatted dictionary d_dict[0, n) into a LUT slot (LUT_ENTRIES
// u16) and an FSE slot (FSE_SLOT u16), as a prebuilt comp's.
hipError_t launch_dict_tables(const uint8_t* d_dict, uint32_t n, uint16_t* d_lut, uint16_t* d_fse, DictTables* d_res,
                              hipStream_t s);

// Copies frame outputs from staging (at cap offsets) to exact offsets.
hipError_t launch_compact(const uint8_t* staging, uint8_t* dst, const uint64_t* d_from,
                          const uint64_t* d_to, const uint64_t* d_len, uint32_t n, hipStream_t s);

// XXH64 of n byte ranges [base + off[i], + len[i]) -> hash[i] (device arrays)
hipError_t launch_xxh64(const uint8_t* base, const uint64_t* d_off, const uint64_t* d_len, uint32_t n,
                        uint64_t* d_hash, hipStream_t s);

// zd_k_verify (a ZD_F_VERIFY_CHECKSUM plan, the last launch of decode_launch):
// every zstd frame that carries a Content_Checksum (W.csum) and whose key is
// KEY_NONE is hashed where the route left it, out + FrameDesc::out for
// FrameState::out_len bytes; digest and ok go to W.vhash / W.vok, and a
// mismatch writes the frame's key (DS_CHECKSUM, ZD_E_CHECKSUM_WRONG).
// cus: the device's compute units (the load pattern follows the waves a CU gets).
hipError_t launch_verify(uint8_t* ws, const Workspace& W, const uint8_t* out, uint32_t n_frames, uint32_t cus,
                         hipStream_t s);

// Device header walk (zd_walk.h): ranges [first + k chunk, + chunk) of src[0, n),
// count pass (fill = false: WalkRange summaries) or fill pass (frames/blocks at
// the summaries' f_off / b_off).
struct WalkRange;
struct HostFrame;
struct HostBlock;
hipError_t launch_walk(const uint8_t* src, uint64_t n, uint64_t first, uint64_t chunk, uint32_t nranges, WalkRange* wr,
                       HostFrame* frames, HostBlock* blocks, bool fill, hipStream_t s, uint32_t wopt = 0);

// Device descriptors (zd_plan_create_device): the shape pass (PlanShape
// zeroed first), the count pass + exclusive scan (cnt: nf x PLAN_FIELDS
// words, scanned within 256-frame tiles; tot: (tiles + 1) x PLAN_FIELDS
// words, the tiles' starts and then the plan's totals), the fill pass.
struct PlanShape { uint32_t multi, jcand; uint64_t jmaxseq; };
hipError_t launch_plan_shape(const HostFrame* frames, uint64_t nf, uint32_t k4j_min, PlanShape* out, hipStream_t s);
hipError_t launch_plan_count(const PlanCtx& X, const HostFrame* frames, const HostBlock* blocks, uint64_t nf,
                             uint64_t* cnt, uint64_t* tot, PlanShape* shape, hipStream_t s, uint32_t dict_comps = 0);
hipError_t launch_plan_fill(const PlanCtx& X, const HostFrame* frames, const HostBlock* blocks, uint64_t nf,
                            const uint64_t* cnt, const uint64_t* tot, const Sink& S, hipStream_t s);
// The level-major K4J numbering of a chain batch created with
// ZD_F_CHAIN_BLOCK_PARALLEL (zd_plan.h plan_j_order, on the device), between
// the count pass and its scan: launch_plan_count's `jo` gathers the frames' K4J
// counts in order[] order into PLAN_J_COLS columns of nf words (col), scans
// them (zd_k_scan_*; scratch: PLAN_J_COLS x (tiles + 1) words), writes every
// frame's starts to j_at (PLAN_J_COLS words a frame: PlanCtx::j_at of the fill
// pass) and the levels' first J frame, segment and piece to lev (3 words a
// level, for the levels lcount -- BatchCarve::lcount after zd_k_chain_bucket --
// gives a frame).
struct PlanJOrder {
  const uint32_t* order;     // device: the frames grouped by level
  const uint32_t* lcount;    // device: counts | cursors (the levels' ends)
  uint64_t *col, *scratch, *j_at, *lev;
};
hipError_t launch_plan_count(const PlanCtx& X, const HostFrame* frames, const HostBlock* blocks, uint64_t nf,
                             uint64_t* cnt, uint64_t* tot, PlanShape* shape, hipStream_t s, uint32_t dict_comps,
                             const PlanJOrder* jo);

// A batch's chunks (zd_batch_create), device arrays of n entries: where chunk
// i lies (src, size) and where its copy sits in the gathered buffer (off, a
// multiple of 16; the copy is followed by zero bytes up to the next chunk's).
struct ChunkList {
  const uint64_t* src;     // device addresses
  const uint64_t* size;
  const uint64_t* off;
};
// One piece (<= COPY_PIECE bytes) of a chunk, zd_k_gather's unit of work
struct GatherPiece { uint32_t chunk, piece; };
// zd_k_gather: the chunks' bytes into the gathered buffer, piece by piece.
hipError_t launch_gather(const ChunkList& L, uint8_t* gathered, const GatherPiece* d_pieces, uint64_t npieces,
                         hipStream_t s);
// zd_k_walk_chunks: one lane per chunk of the gathered buffer.  Count pass
// (fill = false): nblocks[i] = the blocks chunk i's walk keeps; fill pass:
// frames[i] and its blocks at blocks[b_off[i]...] (block indices global).
hipError_t launch_walk_chunks(const uint8_t* gathered, const ChunkList& L, uint32_t n, uint32_t wopt,
                              uint32_t* nblocks, const uint64_t* b_off, HostFrame* frames, HostBlock* blocks, bool fill,
                              hipStream_t s);
// zd_k_batch_results: chunk i's status and length from frame i's state (bind[i]:
// the caller's capacity is the frame's binding limit, so reaching it is
// ZD_E_DST_TOO_SMALL).
hipError_t launch_batch_results(const FrameState* fstate, const uint8_t* bind, uint32_t n, int32_t* status,
                                uint64_t* len, hipStream_t s);
// zd_k_chain_results: zd_k_batch_results for a chain batch.  A chunk with an
// ancestor (parent[], at most 255 hops over the read-only frame states) whose
// own status is not ZD_OK -- a checksum that zd_k_verify found wrong included
// -- is ZD_E_NOT_DECODED with length 0.
hipError_t launch_chain_results(const FrameState* fstate, const uint8_t* bind, const int32_t* parent, uint32_t n,
                                int32_t* status, uint64_t* len, hipStream_t s);

// A chain batch made from device arrays (zd_batch_create_device_chain), after
// zd_k_batch_layout.  zd_k_chain_levels, one lane per chunk: the caller's
// parent entry checked (zd_chain.h chain_level; a bad entry, no root within 255
// hops, or a prefix size on a chunk with a parent: flag[i] = CHUNK_INVALID, its
// prefix entry dropped and taken off *pfx_total), par[i] = the checked parent
// (-1: none or refused), lvl[i] its level, lcount[l] the chunks of level l and
// lcount[512] the links.  zd_k_chain_bucket: order[] = the chunks by level,
// through the cursors lcount[256 + l] (one wave scans the counts first).
// lcount: 2 * 256 + 2 u32, zeroed before.
hipError_t launch_chain_levels(const int64_t* parent, uint32_t n, uint8_t* flag, uint64_t* pfx, uint64_t* pfx_bytes,
                               unsigned long long* pfx_total, int32_t* par, uint8_t* lvl, uint32_t* order,
                               uint32_t* lcount, hipStream_t s);
// zd_k_chain_prefix, after the capacity pass and before the planner: a chained
// chunk's prefix entry from its parent's indexed frame (zd_chain.h
// chain_prefix_bytes) -- the parent's destination, outbase + out[parent], and
// its Frame_Content_Size; a child whose parent's frame has none is
// ZD_E_OUT_OF_DOMAIN (its frame's key).
hipError_t launch_chain_prefix(HostFrame* frames, const int32_t* par, const uint64_t* out, const uint8_t* outbase,
                               uint32_t n, uint64_t* pfx, uint64_t* pfx_bytes, hipStream_t s);

// A batch made from device arrays (zd_batch_create_device).  The batch's own
// per-chunk arrays, n entries each; off and piece0 are adjacent (piece0 == off
// + n: the layout scans them as two columns).
struct BatchArrays {
  uint64_t *src, *size;    // the caller's entries, or 0 / 0 for a refused chunk (flag)
  uint64_t* off;           // ChunkList::off
  uint64_t* piece0;        // the chunk's first piece among the batch's (zd_k_gather_scan)
  uint64_t* out;           // the destination's offset from the lowest destination
  uint64_t* cap;           // the caller's capacity (0 for a refused chunk)
  uint8_t* flag;           // CHUNK_*
  // a prefix batch (zd_batch_create_device_prefix; null otherwise): the chunk's
  // prefix address and size, 0 / 0 for a refused chunk or an empty prefix
  uint64_t* pfx = nullptr;
  uint64_t* pfx_bytes = nullptr;
};
enum : uint8_t { CHUNK_OK = 0, CHUNK_INVALID = 1, CHUNK_TOO_LARGE = 2 };
// zd_k_batch_layout, the scans of off / piece0, zd_k_batch_place.  scratch: 2 *
// (tiles + 1) + 1 words (tiles of 256 chunks); res[0..3): gathered bytes,
// pieces, the lowest destination.  pfx / pfx_bytes (a prefix batch): the
// caller's prefix entries, checked with the rest (a NULL address with a size,
// a range that wraps: CHUNK_INVALID) and copied to A.pfx / A.pfx_bytes; res[3]:
// the prefixes' bytes in all.
hipError_t launch_batch_layout(const uint64_t* src, const uint64_t* size, const uint64_t* dst, const uint64_t* cap,
                               uint32_t n, const BatchArrays& A, uint64_t* scratch, uint64_t* res, hipStream_t s,
                               const uint64_t* pfx = nullptr, const uint64_t* pfx_bytes = nullptr);
// Exclusive scan of n entries of ncols u64 arrays in place (column c at a + c *
// stride; in32: one column's input instead); tot: ncols x (tiles + 1) words,
// a column's total last.
hipError_t launch_scan64(uint64_t* a, const uint32_t* in32, uint64_t n, uint32_t ncols, uint64_t stride, uint64_t* tot,
                         hipStream_t s);
// zd_k_batch_pack (a packed batch): cap[i] = chunk i's reserve from the filled
// device index (0 for a refused chunk), out[i] = it rounded up to `align` (a
// power of two), to be scanned into the chunk's offset.
hipError_t launch_batch_pack(const HostFrame* frames, const HostBlock* blocks, const uint8_t* flag, uint32_t n,
                             uint32_t align, uint64_t* cap, uint64_t* out, hipStream_t s);
// zd_k_chunk_sizes: one lane per chunk, read in place: reserve, walk status and
// exact flag per chunk (status / exact may be null).
hipError_t launch_chunk_sizes(const uint64_t* src, const uint64_t* size, uint32_t n, uint32_t wopt,
                              uint64_t* out_size, int32_t* status, uint8_t* exact, hipStream_t s);
// zd_k_gather over the scanned piece starts instead of a piece list
hipError_t launch_gather_scan(const ChunkList& L, uint8_t* gathered, const uint64_t* d_piece0, uint32_t n,
                              uint64_t npieces, hipStream_t s);
// zd_k_batch_fit: the capacity pass over the device index (frames' status /
// key, bind[]), the refused chunks' statuses, and with set_ids the used flags
// of a dictionary set's entries.
hipError_t launch_batch_fit(HostFrame* frames, const HostBlock* blocks, const uint64_t* cap, const uint8_t* flag,
                            uint32_t n, uint8_t* bind, const uint32_t* set_ids, uint32_t nset, int32_t fallback,
                            uint8_t* used, hipStream_t s);

// ---------------------------------------------------------------------------
// Seekable archives (zd_seekable_*, zd_seek.hip; the rules: zd_seek.h)
// ---------------------------------------------------------------------------
struct SeekFooter;
// zd_k_seek_table over the table at `table` (its skippable header's first
// byte): c_off[f] / d_off[f] = entry f's sizes (nframes + 1 entries each, the
// last 0; d_off == c_off + nframes + 1), checksum[f] when present, then the
// two columns scanned into exclusive sums (tot: 2 x (tiles + 1) words).
// res[0]: the header's verdict (a status), res[1]: the largest Decompressed_Size
// (both zeroed here first).
hipError_t launch_seek_table(const uint8_t* table, const SeekFooter& f, uint64_t* c_off, uint64_t* d_off,
                             uint32_t* checksum, uint64_t* tot, uint64_t* res, hipStream_t s);

// A read's device arrays (zd_seekable_read_create): R ranges over F frames.
struct SeekRead {
  // per range
  uint64_t *off, *len;         // clamped (len 0: nothing to read, or a refused destination)
  uint64_t* dst;
  uint64_t* piece0;            // the range's first 32 KiB copy piece (exclusive scan; R + 1 entries)
  uint32_t *f0, *f1;           // its first and last frame (len > 0)
  uint8_t* bad;                // 1: ZD_E_INVALID_ARG
  int32_t* status;             // the results
  uint64_t* out_len;
  // per frame
  uint32_t *cover, *partial;   // ranges that touch the frame / that hold only a part of it
  uint64_t *idx, *soff;        // the frame's chunk in the inner batch / its staging offset (soff == idx + F)
  uint32_t R, F;
};
// zd_k_seek_cover (one lane a range: clamp, destination check, search, piece
// count), zd_k_seek_mark (one wave a range: the cover counts), zd_k_seek_plan
// (one lane a frame: needed, staged bytes), the scans (tot: 3 x (tiles + 1)
// words, tiles of max(R + 1, F) entries) and zd_k_seek_totals: res[0..4) =
// needed frames, staging bytes, copy pieces, frames in place.  cover, partial
// and res are zeroed by the caller before.
hipError_t launch_seek_layout(const uint64_t* off, const uint64_t* len, const uint64_t* dst, const uint64_t* d_off,
                              const SeekRead& A, uint64_t* tot, uint64_t* res, hipStream_t s);
// zd_k_seek_chunks: the inner batch's chunk table, four columns of `needed`
// entries (src, size, dst, cap), one wave a range.  v_entry / v_addr (both or
// neither; `needed` entries): the chunk's entry in the table and the address
// it decodes to, kept by a verified read.
hipError_t launch_seek_chunks(const SeekRead& A, const uint8_t* archive, const uint64_t* c_off, const uint64_t* d_off,
                              uint8_t* staging, uint64_t* col_src, uint64_t* col_size, uint64_t* col_dst,
                              uint64_t* col_cap, uint32_t* v_entry, uint64_t* v_addr, hipStream_t s);
// zd_k_seek_verify (a ZD_SEEK_VERIFY_TABLE read, behind the inner batch's
// decode): chunk k of n, entry v_entry[k] decoded at v_addr[k], is compared when
// it ended ZD_OK (b_status) with its Decompressed_Size (b_len): ok[k] = 1 / 0
// and hash32[k] = the low 32 bits of XXH64 of its bytes; else ok[k] = -1,
// hash32[k] = 0 and nothing of it is read.  b_hash / b_ok: the inner batch's
// zd_batch_device_checksums arrays or null; a chunk with b_ok[k] == 1 is
// compared by b_hash[k] and not read again.  Four lanes a chunk.
hipError_t launch_seek_verify(const uint32_t* v_entry, const uint64_t* v_addr, uint32_t n, const uint64_t* d_off,
                              const uint32_t* checksum, const int32_t* b_status, const uint64_t* b_len,
                              const uint64_t* b_hash, const int8_t* b_ok, int8_t* ok, uint32_t* hash32,
                              hipStream_t s);
// zd_k_seek_finish: the staged frames' wanted parts to the destinations, one
// workgroup a 32 KiB piece of a range.
hipError_t launch_seek_finish(const SeekRead& A, const uint64_t* d_off, const uint8_t* staging, uint64_t npieces,
                              hipStream_t s);
// zd_k_seek_results: the ranges' statuses and lengths from the inner batch's
// (b_status / b_len, null when no frame is needed), one wave a range.  v_ok:
// zd_k_seek_verify's verdicts, or null (a read without ZD_SEEK_VERIFY_TABLE);
// a chunk of verdict 0 counts as ZD_E_CHECKSUM_WRONG.
hipError_t launch_seek_results(const SeekRead& A, const uint64_t* d_off, const int32_t* b_status,
                               const uint64_t* b_len, const int8_t* v_ok, hipStream_t s);

// ---------------------------------------------------------------------------
// Multi-frame batches (zd_multi_*, zd_multi.hip; the rule: zd_multi.h)
// ---------------------------------------------------------------------------
// A multi-frame batch's device arrays: n chunks that hold F sub-chunks, each a
// chunk of the inner batch.
struct MultiArrays {
  // per chunk
  uint64_t *dst, *cap;         // the caller's destination (0 / 0 for a refused entry)
  uint64_t* first;             // its first sub-chunk (exclusive scan; n + 1 entries, entry n = F)
  uint64_t* stage0;            // its first staging byte         (first + (n + 1))
  uint64_t* piece0c;           // its first 32 KiB copy piece    (first + 2 (n + 1))
  uint64_t* nstaged;           // staged sub-chunks before it    (first + 3 (n + 1))
  int32_t* status;             // the results
  uint64_t* len;
  // per sub-chunk (null until F is known)
  uint32_t* chunk;             // the chunk it belongs to
  uint64_t* soff;              // its staging offset, or MULTI_IN_PLACE
  uint64_t* at;                // in place: its offset in the chunk's destination
  uint64_t* piece0;            // its first copy piece (F + 1 entries)
  uint64_t* fdst;              // staged: its final address (zd_k_multi_join), or MULTI_NOT_DELIVERED
  uint32_t n, F;
};
// zd_k_multi_count (one lane a chunk: the header walk where the chunk lies) and
// the scans of the four columns (tot: 4 x (tiles + 1) words, tiles of n + 1
// entries); entry n of first / stage0 / piece0c / nstaged is then the total.
hipError_t launch_multi_count(const uint64_t* src, const uint64_t* size, const uint64_t* dst, const uint64_t* cap,
                              uint32_t wopt, const MultiArrays& M, uint64_t* tot, hipStream_t s);
// zd_k_multi_fill: the inner batch's chunk table, four columns of F entries
// (src, size, dst, cap), and the per-sub-chunk arrays; one lane a chunk.
hipError_t launch_multi_fill(const uint64_t* src, const uint64_t* size, const uint64_t* dst, const uint64_t* cap,
                             uint32_t wopt, const MultiArrays& M, uint8_t* staging, uint64_t* col_src,
                             uint64_t* col_size, uint64_t* col_dst, uint64_t* col_cap, hipStream_t s);
// zd_k_multi_join: the chunks' statuses and lengths from the inner batch's
// (b_status / b_len, F entries), the staged sub-chunks' final addresses; one
// lane a chunk.
hipError_t launch_multi_join(const MultiArrays& M, const int32_t* b_status, const uint64_t* b_len, hipStream_t s);
// zd_k_multi_copy: the delivered staged sub-chunks' decoded bytes to their final
// addresses, one workgroup a 32 KiB piece of a staged reserve.
hipError_t launch_multi_copy(const MultiArrays& M, const uint8_t* staging, const uint64_t* b_len, uint64_t npieces,
                             hipStream_t s);
// zd_k_multi_sizes: launch_chunk_sizes for chunks of several frames
// (ZD_SIZES_MULTI_FRAME).
hipError_t launch_multi_sizes(const uint64_t* src, const uint64_t* size, uint32_t n, uint32_t wopt, uint64_t* out_size,
                              int32_t* status, uint8_t* exact, hipStream_t s);

constexpr int N_KERNELS = 6;
// mode-2 launch groups (LaunchArgs::dom_events: events 2g, 2g + 1)
constexpr int N_DOM = 5;
enum { DOM_K0 = 0, DOM_FUSED = 1, DOM_K4 = 2, DOM_K4F = 3, DOM_K4J = 4 };
extern const char* const kDomNames[N_DOM];
constexpr uint32_t K4F_CAP = K4F_CAP_BYTES;   // frames up to this output size execute in LDS (K4F)
extern const char* const kKernelNames[N_KERNELS];

}  // namespace zd
