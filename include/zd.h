/*
 * zd.h — C ABI of the MI355X-native ZSTD block-decode path.
 *
 * This is the drop-in boundary for the hot path of the reference crate
 * AchilleBailly/zstd-decompressor (Rust).  The reference has no FFI of its own;
 * its boundary is the public Rust API, and each entry point below names the
 * reference item it replaces (paths relative to the reference repo,
 * zstd-decompressor/src/…).  A Rust crate binds these with `extern "C"` blocks
 * (see INTEGRATION.md); the Python mirror in zstd-decompressor_amd/ binds them
 * with ctypes.
 *
 * Conventions
 *   - Every function returns ZD_OK (0) or a negative ZD_E_* code; nothing
 *     aborts across the ABI.
 *   - Plain pointers and sizes only.  `stream` parameters are hipStream_t
 *     passed as void* (NULL = default stream).
 *   - "d_" prefixed pointers are device (HBM) pointers, all others host.
 *   - The caller owns every buffer it passes; objects created by *_create /
 *     *_new own their own device memory and are released by *_destroy/_free.
 *   - Objects are not thread-safe; distinct objects may be used from
 *     distinct threads.
 */
#ifndef ZD_H
#define ZD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ZD_ABI_VERSION 8

/* ------------------------------------------------------------------ */
/* Status codes: one per reference error variant (leaf of the          */
/* thiserror chain), plus codes for behaviour beyond the reference.    */
/* ------------------------------------------------------------------ */
#define ZD_OK 0
/* parsing::Error (parsing.rs:12-25) */
#define ZD_E_NOT_ENOUGH_BYTES              (-1)
#define ZD_E_NOT_ENOUGH_BITS               (-2)
#define ZD_E_MAX_READABLE_BITS_EXCEEDED    (-3)
#define ZD_E_EMPTY_INPUT_DATA              (-4)
#define ZD_E_NULL_BYTE                     (-5)
#define ZD_E_EMPTY_SLICE                   (-6)
/* decoders::Error (decoders/mod.rs:10-23) */
#define ZD_E_LARGE_ACCURACY_LOG            (-12)
#define ZD_E_CORRUPTED_TABLE               (-13)
#define ZD_E_SEQUENCE_CODE_MAX_EXCEEDED    (-14)
/* literals::Error (literals.rs:8-17) */
#define ZD_E_HUFFMAN_DECODER_MISSING       (-20)
#define ZD_E_CORRUPTED_STREAMS_SIZE        (-21)
/* sequences::Error (sequences.rs:14-23) */
#define ZD_E_SEQ_RESERVED_SET              (-30)
#define ZD_E_NO_PREVIOUS_DECODER           (-31)
/* decoding_context::Error (decoding_context.rs:8-15) */
#define ZD_E_CTX_WINDOW_SIZE_TOO_BIG       (-40)
#define ZD_E_NULL_OFFSET                   (-41)
#define ZD_E_IMPOSSIBLE_VALUE              (-42)
/* block::Error (block.rs:12-25) */
#define ZD_E_RESERVED_BLOCK_TYPE           (-50)
/* frame::Error (frame.rs:14-39) */
#define ZD_E_UNRECOGNIZED_MAGIC            (-60)
#define ZD_E_FRAME_RESERVED_SET            (-61)
#define ZD_E_MISSING_CHECKSUM              (-64)
#define ZD_E_WINDOW_SIZE_TOO_BIG           (-66)
/* Beyond the reference */
#define ZD_E_REF_PANIC       (-90) /* the reference would panic / not terminate here; from a
                                      ZD_F_RFC plan only for input that RFC 8878 forbids as well */
#define ZD_E_OUT_OF_DOMAIN   (-91) /* input outside the GPU path's parity domain */
#define ZD_E_DST_TOO_SMALL   (-92)
#define ZD_E_INVALID_ARG     (-93)
#define ZD_E_HIP             (-94) /* a HIP runtime call failed */
#define ZD_E_NO_MEMORY       (-95)
#define ZD_E_NOT_DECODED     (-96) /* frame skipped: an earlier frame failed (FrameIterator stops, frame.rs:94-99);
                                      in a chain batch: a chunk whose parent, or an ancestor further up, failed */
#define ZD_E_COMM            (-97) /* an RCCL call failed, or RCCL is not loadable */
#define ZD_E_DICT_CORRUPTED  (-98) /* zd_dict_create: a formatted dictionary truncated before its content, with
                                      a repeat offset of 0 or past the content, or without content */
#define ZD_E_DICT_MISMATCH   (-99) /* a frame names a Dictionary_ID other than the plan's dictionary's
                                      (a dictionary set: an ID the set does not hold) */
#define ZD_E_CHECKSUM_WRONG  (-100) /* ZD_F_VERIFY_CHECKSUM: the frame decoded, and its bytes do not hash to its
                                       Content_Checksum (libzstd: "Restored data doesn't match checksum") */
#define ZD_E_SEEK_TABLE      (-101) /* a seekable archive's seek table contradicts itself or the archive
                                       (zd_seekable_open_device); a range of a read: a frame decoded to another
                                       length than the table's Decompressed_Size */

/* Device workspaces of destroyed plans are kept for reuse by later plans of
 * the process (bounded by ZD_WS_CACHE_MB, default 8 GiB; 0 disables it).
 * zd_trim_cache frees them (every device): PyTorch's caching allocator does
 * not see this memory. */
void zd_trim_cache(void);

/* Human-readable name of a status code (static storage). */
const char* zd_status_name(int status);
int zd_abi_version(void);

/* ------------------------------------------------------------------ */
/* Frame index — replaces FrameIterator::next + Frame::parse +        */
/* Header::parse + Block::parse (frame.rs:61-99,111-177,198-230;       */
/* block.rs:43-72).  Host-side, O(frames+blocks), reads only headers.  */
/* ------------------------------------------------------------------ */
#define ZD_FRAME_ZSTD      0
#define ZD_FRAME_SKIPPABLE 1

typedef struct zd_frame_desc {
  uint64_t src_offset;     /* offset of the 4-byte magic in src */
  uint64_t src_size;       /* bytes of the whole frame (header, blocks, checksum) */
  uint64_t content_size;   /* Frame_Content_Size, UINT64_MAX if absent */
  uint64_t window_size;    /* Header::window_size (frame.rs:105) */
  uint64_t dict_id;        /* Header::dictionnary_id, UINT64_MAX if absent */
  uint32_t magic;
  uint32_t kind;           /* ZD_FRAME_ZSTD / ZD_FRAME_SKIPPABLE */
  uint32_t first_block;    /* index into the block array */
  uint32_t num_blocks;
  uint32_t has_checksum;
  uint32_t checksum;       /* ZStandard::checksum() (frame.rs:268) */
} zd_frame_desc;

#define ZD_BLOCK_RAW        0
#define ZD_BLOCK_RLE        1
#define ZD_BLOCK_COMPRESSED 2

typedef struct zd_block_desc {
  uint64_t src_offset;     /* first byte after the 3-byte block header */
  uint32_t block_size;     /* Block_Size field (block.rs:50) */
  uint8_t  type;           /* ZD_BLOCK_* */
  uint8_t  last;
  uint8_t  rle_byte;       /* RLEBlock::byte */
  uint8_t  _pad;
} zd_block_desc;

/*
 * Walk the frames of src[0..n).  With frames == NULL (or cap_frames == 0) the
 * whole input is walked and *nframes / *nblocks receive the totals (size
 * query); otherwise at most cap_frames frames are indexed, and blocks beyond
 * cap_blocks are counted but not stored.  *consumed = bytes of the indexed
 * frames (Frame::parse advances the parser the same way).  Stops at the first frame that fails
 * to parse, like FrameIterator + the CLI loop (src/main.rs:43-53): the
 * return value is that frame's status and *consumed the byte offset of the
 * failing frame (n on full success).  Table-level parse errors (FSE/Huffman
 * descriptions) are found on the GPU, not here.
 */
int zd_frames_index(const uint8_t* src, size_t n,
                    zd_frame_desc* frames, size_t cap_frames, size_t* nframes,
                    zd_block_desc* blocks, size_t cap_blocks, size_t* nblocks,
                    size_t* consumed);

/* ------------------------------------------------------------------ */
/* Batch decode (the hot path): a plan over a byte range of frames.    */
/* Replaces Frame::decode / ZStandard::decode (frame.rs:79-84,232-260) */
/* and, per block, Block::decode (block.rs:74-99) with HIP kernels.    */
/* ------------------------------------------------------------------ */
typedef struct zd_plan zd_plan;

#define ZD_F_SKIPPABLE  1u  /* append skippable-frame payloads to the output (CLI -p, src/main.rs:45-48) */
/* Executor choice for frames of many blocks; default:
 * automatic.  Same output either way; tests run both.  Plans with a
 * dictionary or a dictionary set, chain batches and zd_context ignore both
 * flags (the streaming executor only; a chain batch has a flag of its own,
 * ZD_F_CHAIN_BLOCK_PARALLEL, and so have dictionary plans,
 * ZD_F_DICT_BLOCK_PARALLEL, under which the two flags mean what they say); a prefix batch (zd_batch_create_prefix,
 * zd_batch_create_device_prefix) ignores the plain plans' automatic rule and
 * takes K4J when ZD_F_BLOCK_PARALLEL asks for it -- large deltas, whose
 * hundreds of blocks one wave would decode one after another -- or chunk by
 * chunk by the batches' own rule, ZD_F_AUTO_EXECUTOR. */
#define ZD_F_BLOCK_PARALLEL 2u  /* every frame with a compressed block -> K4J (block-parallel execute);
                                   prefix batches included */
#define ZD_F_FRAME_SERIAL   4u  /* no frame -> K4J (the streaming per-frame executor) */
/* Sequence-decode choice: K3 with one lane per block instead of four (the
 * default, K3Q).  Same records either way; tests run both. */
#define ZD_F_SEQ_ONE_LANE   8u
/* Launch choice for plans of 256-1024 single-block frames:
 * K3 and K4 run fused per frame group (zd_k_fused) by default; this flag
 * keeps them as two launches.  Same output either way; tests run both. */
#define ZD_F_NO_FUSE      32u
/* Table-build choice for plans of up to 16,384 tables: K1's sequence half
 * runs one wave per block by default; this flag keeps K1's serial lanes.
 * Same tables either way; tests run both. */
#define ZD_F_K1_LANES     64u
/* Sequence-decode choice for plans of few blocks (<= 8 per CU): K3 runs
 * one block per wave (zd_k_sequences_l, latency-first) by default; this flag
 * keeps K3Q.  Same records either way; tests run both. */
#define ZD_F_SEQ_NO_LATENCY 256u
/* Table-build choice: plans past 64 tables per CU run K1 as two passes -- a
 * parse pass, one block per lane, and a build pass, one wave per block
 * (zd_k_tables_parse / zd_k_tables_build) -- unless
 * ZD_F_K1_LANES is given; this flag runs the two passes in a plan of any size
 * (before the wave-per-block route; never the sequence half of a fused
 * plan).  Same tables either way; tests run both. */
#define ZD_F_K1_SPLIT    512u
/* Test switch: K4J runs ONE pointer-jumping round of one hop, so a frame
 * whose match chains are deeper keys LS_JROUNDS and zd_plan_decompress plans
 * it again on the streaming executor (tests/test_large_frames.py). */
#define ZD_F_J_ONE_ROUND 128u
/* Verify Content_Checksums inside the decode launch (opt-in; the default keeps
 * the reference's behaviour, which hashes and never enforces).  A
 * plan / batch flag, accepted wherever plan flags are: zd_plan_create, _dict,
 * _dicts, _device, zd_decompress*, every zd_batch_create*, and the sharded
 * calls, which pass it to their plans.  With it zd_decode_async /
 * zd_batch_decode_async end with one more kernel (zd_k_verify; only when some
 * zstd frame of the plan carries a Content_Checksum) behind everything else
 * they queue: no host work, no allocation, no synchronisation, capturable
 * like a launch without the flag.  After a frame's last block has executed, a
 * zstd frame that carries a Content_Checksum, whose status is ZD_OK, and whose
 * decoded bytes' XXH64 (seed 0) differs in its low 32 bits from the stored
 * value gets ZD_E_CHECKSUM_WRONG:
 *  - in a plan it is a failing frame like any other: the output stops before
 *    it, later frames are ZD_E_NOT_DECODED, first_error_frame names it
 *    (zd_plan_decompress's re-plans keep the flag);
 *  - in a batch that chunk alone fails, with length 0; the bytes stay in its
 *    buffer, unspecified (the streaming re-decode inside zd_batch_results of a
 *    chunk whose block-parallel execution did not converge verifies too);
 *  - a frame that already failed keeps its own status: the check never
 *    replaces another error and never reads a failed frame's bytes;
 *  - a frame without a Content_Checksum, and a skippable frame, is unaffected;
 *  - an empty checksummed frame verifies (XXH64 of no bytes is
 *    0xEF46DB3751D8E999).
 * Without the flag nothing changes: the same launches, the same statuses.
 * zd_plan_checksums / zd_batch_checksums behave the same with and without it;
 * on a verified plan they report ok = -1 for a frame that failed
 * verification (and for the frames after it), as for any frame that was not
 * decoded.  zd_context / zd_block_decode / zd_execute_sequences take no flags
 * and stay outside the feature. */
#define ZD_F_VERIFY_CHECKSUM 1024u
/* Accept frames whose Window_Size is up to 2 GiB (1 << 31) where the default
 * keeps the reference's 8 MiB limit (frame.rs:44): what `zstd --long` and
 * `zstd --patch-from` write for inputs past 8 MiB.  Above 2 GiB a frame is
 * still ZD_E_WINDOW_SIZE_TOO_BIG.  A plan / batch flag, accepted wherever plan
 * flags are (the host walk, the device walks, zd_plan_decompress's re-plans,
 * the streaming re-decode inside zd_batch_results); zd_chunk_sizes_device has
 * ZD_SIZES_LONG_WINDOW.  Routing is untouched: no executor depends on the
 * window, each checks an offset against the bytes produced so far.  Without
 * the flag nothing changes.  zd_context keeps its own window check. */
#define ZD_F_LONG_WINDOW 2048u
/* A chain batch on the block-parallel executor (zd_batch_create_chain,
 * zd_batch_create_device_chain; opt-in, large deltas): every chunk whose frame
 * has a compressed block executes on K4J, level by level, whether or not it has
 * a parent and whether its prefix is external, a parent's output or none;
 * frames without a compressed block stay on zd_k_execute_chain, and
 * zd_batch_info.executors carries ZD_EXEC_K4J.  The same bytes, statuses and
 * lengths as the batch gives without the flag, with the one exception a prefix
 * batch created with ZD_F_BLOCK_PARALLEL has: a K4J frame needs its prefix to
 * fit 0x7FFF0000 bytes and its capacity K4J's 32 GiB, not the two together to
 * fit 0x7FFF0000.  A chain batch keeps ignoring ZD_F_BLOCK_PARALLEL and
 * ZD_F_FRAME_SERIAL.  Everywhere else the flag is accepted and ignored: plain,
 * dictionary and prefix batches, zd_plan_*, zd_decompress*, the sharded calls.
 * K4J is several times slower than the streaming executor on small frames
 * (16 KiB pages; README), so this flag forces the choice for the whole batch;
 * ZD_F_AUTO_EXECUTOR below chooses chunk by chunk. */
#define ZD_F_CHAIN_BLOCK_PARALLEL 4096u
/* Prefix and chain batches: each chunk's executor chosen by rule (opt-in).  In a
 * prefix batch (zd_batch_create_prefix, zd_batch_create_device_prefix) and in a
 * chain batch (zd_batch_create_chain, zd_batch_create_device_chain) a chunk's
 * frame executes on K4J when it could under the forcing flag -- a zstd frame
 * that did not fail to index, with a compressed block, a capacity within K4J's
 * 32 GiB and a prefix of at most 0x7FFF0000 bytes -- and one of these holds:
 *  (a) it has at least ZD_AUTO_MIN_BLOCKS compressed blocks -- at least
 *      ZD_AUTO_MIN_BLOCKS_FEW when the batch's width is at most
 *      ZD_AUTO_FEW_CHUNKS -- and the batch has at most ZD_AUTO_MAX_CANDIDATES
 *      such frames.  The width is the number of chunks that execute together:
 *      a prefix batch's chunk count, a chain batch's widest level;
 *  (b) the streaming executor cannot hold it: prefix size plus capacity pass
 *      0x7FFF0000 while the prefix alone fits.  Without a forcing flag such a
 *      chunk is ZD_E_OUT_OF_DOMAIN; with this flag it decodes.
 * Every other frame takes the batch's streaming executor.  A chain batch with
 * the flag is laid out and launched like one created with
 * ZD_F_CHAIN_BLOCK_PARALLEL (level by level; a level without a K4J frame queues
 * no K4J launch).  zd_batch_info.executors carries ZD_EXEC_K4J only when some
 * frame went there, and zd_batch_info2.k4j_chunks counts them.  The forcing
 * flags win: in a prefix batch ZD_F_BLOCK_PARALLEL and ZD_F_FRAME_SERIAL behave
 * as without this flag, in a chain batch ZD_F_CHAIN_BLOCK_PARALLEL does (the
 * other two stay ignored there).  A chunk whose pointer jumping does not
 * converge is decoded again inside zd_batch_results, as with the forcing flags.
 * The same bytes, statuses and lengths as without the flag, but for (b).
 * Everywhere else the flag is accepted and ignored: plain, dictionary and
 * dictionary-set batches, zd_plan_*, zd_decompress*, the sharded calls.  Without
 * the flag nothing changes.
 * The four constants (measured on prefix and chain batches of text deltas,
 * scripts/time_auto_exec.py, EXPERIMENTS.md): */
#define ZD_F_AUTO_EXECUTOR 8192u
#define ZD_AUTO_MIN_BLOCKS      4    /* (a): compressed blocks a frame needs for K4J (256 deltas of 4 blocks: K4J
                                        2.3 ms against 2.6 streaming; of 2 blocks: 1.44 against 1.44) */
#define ZD_AUTO_MIN_BLOCKS_FEW  2    /*      ... at a width of at most ZD_AUTO_FEW_CHUNKS (64 deltas of 2 blocks:
                                        0.80 ms against 1.36; of 1 block: 0.73 against 0.75) */
#define ZD_AUTO_FEW_CHUNKS      64
#define ZD_AUTO_MAX_CANDIDATES  256  /* (a) holds only while at most this many frames of the batch meet it (K4J's
                                        time grows with the frames it takes, the streaming executor's with the
                                        longest frame: 256 deltas of 16 blocks 8.2 ms against 10.4, 1,024 of them
                                        33.1 against 11.4; the plain plans' rule has 16 and 1,024 here) */
/* Decode frames as RFC 8878 and libzstd have them (opt-in).  The default is the
 * reference's decoder, its departures from the format included (SURVEY.md §2.1
 * D1-D9); three of them reject or corrupt frames that libzstd writes.  With this
 * flag, and only with it:
 *  - D1: the three-byte Number_of_Sequences is byte1 + (byte2 << 8) + 0x7F00
 *    (the reference adds 0x7F, and decodes such a block to the wrong bytes);
 *  - D2: a compressed block with 0 sequences is valid: its literals are its
 *    output, and it leaves the repeat offsets, the previous FSE tables and the
 *    previous Huffman tree as they were (the reference fails the frame with
 *    ZD_E_NO_PREVIOUS_DECODER or ZD_E_EMPTY_INPUT_DATA);
 *  - D3: Huffman weights follow RFC 8878 4.2.1.1: Max_Number_of_Bits is
 *    highbit(sum of 2^(w-1)) + 1, the last weight fills the sum up to
 *    2^Max_Number_of_Bits, and what is left to fill must be a power of two,
 *    else ZD_E_CORRUPTED_TABLE (the reference is ZD_E_REF_PANIC on a sum that is
 *    a power of two, and truncates the rest to 8 bits);
 *  - D8: Regenerated_Size is enforced: Huffman streams that do not decode to
 *    exactly their shares of it, an empty stream among the four, are
 *    ZD_E_CORRUPTED_STREAMS_SIZE (the reference concatenates what the streams
 *    give); stream sizes are not truncated to 16 bits;
 *  - an empty Raw literals section is accepted in every kind of plan.
 * Everything else is as without the flag: the window limit (ZD_F_LONG_WINDOW is
 * its own flag), no window check on offsets, checksums (ZD_F_VERIFY_CHECKSUM),
 * routing and executors.  ZD_E_REF_PANIC may still come out of such a plan, but
 * only for input that RFC 8878 forbids too (an offset that evaluates to 0, a
 * corrupt FSE description, Huffman weights that overflow 32 bits).  Bytes that
 * follow a Number_of_Sequences of 0 inside its block are ignored.
 * A plan / batch flag, accepted wherever plan flags are: zd_plan_create, _dict,
 * _dicts, _device, zd_decompress*, every zd_batch_create*, the re-plans inside
 * zd_plan_decompress and zd_batch_results (which keep it), and the sharded
 * calls, which pass it to their plans; a seekable read takes it as the read
 * option ZD_SEEK_RFC of zd_seekable_read_create_ex; zd_chunk_sizes_device has ZD_SIZES_RFC.  A dictionary's own tables
 * (zd_dict_create takes no flags) are parsed by the reference's rule.
 * zd_context / zd_block_decode / zd_execute_sequences take no flags and stay
 * the reference's.  Without the flag nothing changes. */
#define ZD_F_RFC 16384u
/* Dictionary and dictionary-set plans and batches on the block-parallel
 * executor (opt-in).  Without this flag every frame behind a dictionary runs on
 * the streaming executor, one wave a frame, block after block, and
 * ZD_F_BLOCK_PARALLEL and ZD_F_AUTO_EXECUTOR mean nothing there.  With it --
 * in zd_plan_create_dict / _dicts, zd_decompress_dict / _dicts,
 * zd_batch_create_dicts, zd_batch_create_device_dicts,
 * zd_batch_create_device_packed_dicts and a multi-frame batch with a
 * dictionary or set (zd_multi_create_device hands the flag to its inner batch;
 * without a dictionary it refuses the bit, as it refuses every flag that is
 * not its own) -- a frame may execute
 * on K4J when it is a zstd frame that did not fail to index, has a compressed
 * block, a capacity within K4J's 32 GiB and dictionary content of at most
 * 0x7FFF0000 bytes:
 *  - with ZD_F_FRAME_SERIAL no frame goes to K4J;
 *  - with ZD_F_BLOCK_PARALLEL every such frame does;
 *  - with neither, each such frame is routed by ZD_F_AUTO_EXECUTOR's rule with
 *    the ZD_AUTO_* constants above: (a) with the plan's frame count (a batch's
 *    chunk count) as the width and the candidates counted over the whole plan,
 *    against ZD_AUTO_DICT_MAX_CANDIDATES in ZD_AUTO_MAX_CANDIDATES' place,
 *    (b) dictionary content plus capacity past 0x7FFF0000 while the content
 *    alone fits.  The three other constants were measured on prefix batches
 *    (the same scatter path) and are kept for dictionary plans; the cap is the
 *    one that scripts/time_dict_big.py's grid moved (EXPERIMENTS.md).
 * A frame of a set plan that decodes without a dictionary is routed alike (its
 * source is 0 bytes).  Frames of raw / RLE blocks only stay where they are; the
 * fused kernel and K4F stay off.  K4J's scatter writes the bytes that come from
 * the dictionary; an offset past the content plus the position is
 * ZD_E_IMPOSSIBLE_VALUE as on the streaming executor.  A frame whose pointer
 * jumping does not converge is decoded again on the streaming executor with its
 * dictionary or set: inside zd_batch_results for a batch (zd_batch_device_results
 * shows ZD_E_OUT_OF_DOMAIN until then), by zd_plan_decompress's re-plan for a
 * plan.  zd_plan_info.executors / zd_batch_info.executors carry ZD_EXEC_K4J only
 * when a frame went there; zd_batch_info2.k4j_chunks counts them.  The same
 * bytes, statuses and lengths as without the flag, but for (b).
 * Everywhere else the flag is accepted and ignored: plain plans and batches,
 * prefix and chain batches, the sharded calls.  A seekable read has no
 * dictionary and refuses the bit in its plan flags (ZD_E_INVALID_ARG).  Without
 * the flag nothing changes. */
#define ZD_F_DICT_BLOCK_PARALLEL 32768u
#define ZD_AUTO_DICT_MAX_CANDIDATES 192  /* (a) in a dictionary plan holds only while at most this many frames meet it:
                                            frames behind a dictionary are whole text frames, not deltas, and K4J's
                                            time grows faster with them (192 frames of 16 blocks 10.3 ms against 11.3
                                            streaming, of 4 blocks 3.57 against 3.72; 256 frames 13.2 against 11.3 and
                                            4.32 against 3.69) */

/* zd_plan_info.executors: */
#define ZD_EXEC_FUSED 1u   /* zd_k_fused: tables, FSE chains and execution per group of four
                              single-block frames (not while kernel profiling is on) */
#define ZD_EXEC_K4F   2u   /* some frames execute resident in LDS (zd_k_execute_lds) */
#define ZD_EXEC_K4J   4u   /* some frames execute block-parallel (pointer jumping) */

typedef struct zd_plan_info {
  uint64_t nframes;        /* frames in the plan (skippable included) */
  uint64_t nblocks;
  uint64_t ncompressed;    /* compressed blocks */
  uint64_t src_bytes;      /* bytes of src covered by the plan */
  uint64_t out_bytes;      /* exact decoded size if every frame has a FCS, else an upper bound */
  uint64_t out_exact;      /* 1 if out_bytes is exact */
  uint64_t workspace_bytes;/* device workspace owned by the plan */
  uint64_t nsequences;     /* sum of Number_of_Sequences over compressed blocks */
  uint64_t nliterals;      /* sum of Regenerated_Size over compressed-literal blocks */
  int32_t  index_status;   /* status of the host walk (first failing frame) */
  uint32_t executors;      /* ZD_EXEC_* bits: the executors the plan's frames take */
  uint64_t host_ns;        /* zd_plan_create: header walk + descriptors (host work) */
  uint64_t device_ns;      /* zd_plan_create: workspace allocation + descriptor upload */
  uint64_t walk_serial_bytes; /* input bytes the frame walk had to walk serially (a range whose
                                 parallel walk started at a magic number inside data); 0 normally */
  uint64_t io_h2d_ns;      /* the last zd_plan_decompress: input host -> HBM */
  uint64_t io_decode_ns;   /*   decode + results (kernels, status read-back) */
  uint64_t io_d2h_ns;      /*   output HBM -> host */
  uint64_t error_key;      /* the last zd_plan_results: where the first failing frame stopped,
                              phase << 62 | block in frame << 32 | stage << 28 | sub << 8 | -status
                              (phase 0 parse, 1 decode, 3 a limit of the GPU path; stages
                              csrc/zd_common.h); all ones when every frame decoded */
  uint64_t replans;        /* the last zd_plan_decompress: re-plans past frames that overran
                              their reserved capacity (or K4J rounds), 0 normally */
  uint64_t fused_redo_frames; /* the last zd_plan_results of a zd_k_fused launch: frames its redo
                              pass decoded (a fast-chain reject, or a wait for K2 / the chain
                              past its bound); 0 normally, never a different output */
  uint64_t device_descriptors; /* 1: zd_plan_create_device built the descriptors on the GPU from its
                              own index (only the frames' output offsets and capacities came
                              back); 0: the index came back and the host built them */
} zd_plan_info;

/* The executor routing zd_plan_create / zd_decode_async choose for a plan of
 * this shape on a device of `cus` compute units (host only: diagnostics and
 * tests).  Every bound scales with the CU count (zd_host.cpp route_plan,
 * DESIGN.md §4): single_block_frames = every frame one compressed block.
 * *route = ZD_ROUTE_* bits. */
#define ZD_ROUTE_FUSED        1u   /* zd_k_fused (tables + K3 + K4 per group of four frames) */
#define ZD_ROUTE_K4F          2u   /* frames up to 128 KiB execute resident in LDS */
#define ZD_ROUTE_K1_SEQ_WAVES 4u   /* K1's sequence half one wave per block */
#define ZD_ROUTE_FORK         8u   /* K2 beside K3 on a second stream */
#define ZD_ROUTE_K1_FORK     16u   /* K1's two halves on the two streams */
#define ZD_ROUTE_K1_SPLIT    32u   /* K1 as a parse pass and a build pass */
int zd_route(uint32_t cus, uint64_t nframes, uint64_t n_tables, uint64_t n_seq_blocks, uint64_t n_huf_blocks,
             int single_block_frames, uint32_t flags, uint32_t* route);

/* Index src[0..n) on the host and allocate the plan's device workspace.
 * Host-side work only (no kernel launches).  A frame that fails to index
 * ends the plan (its status is kept and reported by zd_plan_results). */
int zd_plan_create(const uint8_t* src, size_t n, uint32_t flags, zd_plan** out);
/* The same plan from an input resident in device memory only (d_src,
 * readable for n + ZD_SRC_PADDING bytes): the frame / block header walk runs
 * on the GPU (zd_k_walk, one wave per byte range, the host walk's own code in
 * zd_walk.h), and only its index -- frames and blocks, about 150 bytes per
 * block -- comes back to the host for the descriptors.  Replaces the host
 * pre-pass of FrameIterator / Frame::parse / Header::parse / Block::parse
 * and the section headers (frame.rs:61-230, block.rs:43-72,
 * literals.rs:88-206, sequences.rs:52-143) for input that never was in host
 * memory (e.g. a frame range received from another GPU).  The plan equals
 * zd_plan_create's on the same bytes.  Synchronises `stream`. */
int zd_plan_create_device(const uint8_t* d_src, size_t n, uint32_t flags, void* stream, zd_plan** out);
int zd_plan_info_get(const zd_plan* plan, zd_plan_info* info);
/* Waits for the work the plan launched, then returns its device workspace to
 * the process cache (zd_trim_cache). */
void zd_plan_destroy(zd_plan* plan);

/* Bitstream readers fetch aligned 16-byte windows and may touch up to
 * ZD_SRC_PADDING bytes past the end of the input: device input buffers must
 * stay readable that far (the contents there do not matter). */
#define ZD_SRC_PADDING 16

/* Launch the decode pipeline on `stream`.  d_src holds the same n bytes
 * given to zd_plan_create, resident in HBM (readable for n + ZD_SRC_PADDING
 * bytes); d_dst receives the
 * concatenated output (>= info.out_bytes).  No host synchronisation, no
 * allocation: safe to capture in a hipGraph. */
int zd_decode_async(zd_plan* plan, const uint8_t* d_src, uint8_t* d_dst,
                    size_t dst_cap, void* stream);

/* After the stream has drained: per-frame status and decoded length
 * (host arrays of plan nframes entries, either may be NULL), the total
 * length of the CLI-style output (frames up to the first failure) and the
 * overall status (first failing frame's status, or ZD_OK).  If some frame
 * had no FCS this also compacts d_dst in place so the frames are
 * contiguous (needs the same d_dst and stream). */
int zd_plan_results(zd_plan* plan, uint8_t* d_dst, void* stream,
                    int32_t* frame_status, uint64_t* frame_len,
                    uint64_t* total_len, int32_t* first_error_frame);

/* Content checksums, an extra beyond the reference: after zd_plan_results
 * (same d_dst and stream), XXH64 (seed 0) of every decoded frame's output,
 * computed on the GPU.  ok[i] = 1 when frame i carries a Content_Checksum and
 * it equals the digest's low 32 bits, 0 when it differs, -1 when the frame has
 * none or was not decoded; hash[i] = the digest (0 if not decoded).  The
 * reference computes the hash but never enforces it (frame.rs:239-255,
 * SURVEY D5), so a mismatch never changes the decode status (a plan made with
 * ZD_F_VERIFY_CHECKSUM enforces it inside the launch instead; this call is
 * the same with and without the flag, and there reports -1 for the frame that
 * failed verification, which was not decoded).  Host arrays of
 * plan nframes entries, either may be NULL. */
int zd_plan_checksums(zd_plan* plan, const uint8_t* d_dst, void* stream, int32_t* ok, uint64_t* hash);

/* Kernel times of the last zd_decode_async on the plan, in ms (HIP events on
 * the plan's stream).  zd_plan_set_profiling mode 1: every kernel timed, the
 * launches one after another (no K2 | K3 fork, no fused kernel); mode 2: the
 * pipeline exactly as it runs unprofiled, with events around each launch
 * group that can carry the plan's work and did launch, one entry each, in
 * this order: "zd_k_rawcopy" (K0, raw/RLE blocks), "zd_k_fused", "zd_k_execute"
 * (only when some frame runs on it), "zd_k_execute_lds" (K4F), and the K4J
 * kernels together ("zd_k_jsum+...+zd_k_jround"); the largest is the
 * dominant launch.  0: off.  names/ms arrays of cap entries. */
int zd_plan_set_profiling(zd_plan* plan, int enable);
/* The blocks of the last zd_decode_async whose Huffman tree / sequence tables
 * K1's fast passes left to the large-scratch lane kernels (a table of more
 * than 64 symbols, a weight table past AL 6, more than 255 weights, maxBits >
 * 11, a tree that is not complete): waits for `stream`, reads the blocks'
 * state back and counts the flags.  Nothing on the decode path counts them.
 * libzstd's frames give (0, 0).  Either pointer may be NULL. */
int zd_plan_k1_fallbacks(zd_plan* plan, void* stream, uint64_t* huf_blocks, uint64_t* seq_blocks);
int zd_plan_kernel_times(zd_plan* plan, const char** names, float* ms, int cap, int* n);

/* zd_decompress with a plan already made for the same n bytes (so a caller
 * that sized dst from zd_plan_info_get does not plan twice).  The plan keeps
 * the device buffers for the next call (freed by zd_plan_destroy); input and
 * output move through pinned chunks (zd_plan_info io_*_ns: the phases of the
 * last call).  A frame that decodes past the capacity the plan reserved for
 * it (its Frame_Content_Size, or 128 KiB per block) is planned again from its
 * own start with more room, as often as needed (info.replans); the reference
 * checks neither (decoding_context.rs:29-47, block.rs:50).  Calls on distinct
 * plans may run on distinct threads (thread safe: they share one
 * process-wide pair of pinned chunks only while copying).  Every call runs on
 * the device's legacy null stream, so concurrent calls do not overlap on the
 * GPU; a caller that wants overlap uses zd_decode_async on its own streams.
 * One plan is not used from two threads at once. */
int zd_plan_decompress(zd_plan* plan, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len);
/* Per-frame outcome of the last zd_plan_decompress on the plan (its re-plans
 * included): frame f's status (ZD_OK, the frame's error, or
 * ZD_E_NOT_DECODED after the first failing frame) and where its bytes sit in
 * dst (offset, length; length 0 unless ZD_OK).  *n = the plan's frames
 * (0 before any call); arrays of cap entries, any may be NULL.  This is what
 * a FrameIterator-style caller (frame.rs:86-99) hands out frame by frame
 * from one decode of the whole buffer. */
int zd_plan_frame_outputs(const zd_plan* plan, int32_t* status, uint64_t* offset, uint64_t* length, size_t cap,
                          size_t* n);
/* Convenience: host in, host out (H2D + decode + D2H on the default
 * stream).  Mirrors the CLI (src/main.rs:43-58) minus the UTF-8 step. */
int zd_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap,
                  size_t* out_len, uint32_t flags);

/* ------------------------------------------------------------------ */
/* Dictionaries (RFC 8878 5; beyond the reference, which parses a       */
/* frame's Dictionary_ID and ignores it, frame.rs:143-152).             */
/* ------------------------------------------------------------------ */
typedef struct zd_dict zd_dict;

/* A dictionary from host bytes, on the current device.  A formatted
 * dictionary starts with the magic number 0xEC30A437: a 4-byte ID, the Huffman
 * tree description, the FSE descriptions of the offset, match length and
 * literal length tables, three 4-byte little-endian repeat offsets, then the
 * content.  Any other byte string is a raw-content dictionary: ID 0, no
 * tables, repeat offsets 1, 4, 8, the whole string content.  The content is
 * copied into device memory the object owns and the four tables are built on
 * the GPU once (zd_k_dict_tables); the call synchronises.
 *   ZD_E_DICT_CORRUPTED  truncated anywhere before the content; a repeat
 *                        offset of 0 or larger than the content; no content
 *   the table's own code (ZD_E_CORRUPTED_TABLE, ZD_E_LARGE_ACCURACY_LOG, ...)
 *                        when a description fails as it would in a block
 *   ZD_E_OUT_OF_DOMAIN   a Huffman tree deeper than 11 bits (libzstd writes
 *                        none), or more than ZD_DICT_MAX_CONTENT bytes of content */
#define ZD_DICT_MAX_CONTENT (1ull << 30)
int  zd_dict_create(const uint8_t* dict, size_t n, zd_dict** out);
/* Legal before the plans made with it are destroyed: they share ownership. */
void zd_dict_destroy(zd_dict* d);
/* raw_content: 1 for a raw-content dictionary.  Any pointer may be NULL. */
int  zd_dict_info(const zd_dict* d, uint32_t* dict_id, uint64_t* content_size,
                  uint64_t rep[3], int* raw_content);
/* zd_plan_create with a dictionary (dict == NULL: zd_plan_create).  Every
 * zstd frame of the plan decodes with it: its tables stand for the block
 * before the frame's first (Treeless literals, Repeat modes), its repeat
 * offsets are the frame's first, and a match may reach into its content
 * however far the frame has advanced (no window check, as everywhere here:
 * DESIGN.md D4); an offset larger than content size + position is
 * ZD_E_IMPOSSIBLE_VALUE.  A frame that names a non-zero Dictionary_ID other
 * than the dictionary's gets ZD_E_DICT_MISMATCH and the plan stops there like
 * at any failing frame; a frame without an ID decodes with the dictionary,
 * as in libzstd.  One quirk of the reference is not kept in these plans, whose
 * yardstick is libzstd: a Raw literals section of 0 bytes (a record found
 * wholly in the dictionary) is accepted, where the reference's zero-length
 * slice is an EmptySliceError.  The output holds the frames' own bytes only, contiguous;
 * every zd_plan_* call and zd_decode_async work as on any plan (no host copy
 * or allocation per launch; capturable).  A dictionary made on another
 * device: ZD_E_INVALID_ARG.
 * Limits: without ZD_F_DICT_BLOCK_PARALLEL (see the flag) dictionary plans run
 * on the streaming executor only -- never the
 * fused kernel, K4F or K4J, ZD_F_BLOCK_PARALLEL is ignored and
 * zd_plan_info.executors is 0; a frame whose dictionary content plus
 * capacity passes the streaming executor's int32 positions is
 * ZD_E_OUT_OF_DOMAIN.  zd_plan_create_device, the sharded calls and zd_context
 * take no dictionary. */
int  zd_plan_create_dict(const uint8_t* src, size_t n, uint32_t flags, const zd_dict* dict, zd_plan** out);
/* zd_decompress with a dictionary. */
int  zd_decompress_dict(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len,
                        uint32_t flags, const zd_dict* dict);

/* Dictionary sets (libzstd: ZSTD_d_refMultipleDDicts): many dictionaries in
 * one plan or batch, each frame choosing its own by the Dictionary_ID in its
 * header -- one dictionary per column, table or message type, and records
 * without any, decoded together instead of one plan per dictionary.
 *
 * zd_dict_set_create: ndicts >= 1 dictionaries made by zd_dict_create on the
 * current device.  fallback: index of the dictionary for frames that carry no
 * Dictionary_ID (or ID 0), or -1: such frames decode with no dictionary,
 * exactly as in a plan made without one.  The set shares ownership of its
 * dictionaries' device data (the zd_dict handles may be destroyed at once),
 * plans and batches share ownership of the set: any order of destroy calls is
 * legal.  The call allocates 32 bytes of device memory and copies nothing.
 * ZD_E_INVALID_ARG, before any HIP call: a NULL argument, ndicts == 0 or above
 * ZD_DICT_SET_MAX, a NULL or destroyed entry, fallback outside [-1, ndicts),
 * two entries with the same ID, a dictionary of ID 0 (raw content) anywhere
 * but at `fallback` (no frame can name it), dictionaries of different
 * devices; and a set made on another device than the current one.
 * ZD_DICT_SET_MAX bounds what one plan can be made to pay for its
 * dictionaries: a plan keeps tables (a Huffman and an FSE slot, about 11 KiB,
 * filled by three small copies at creation) for every formatted dictionary
 * that one of ITS frames uses, at most 4096 x 11 KiB = 44 MiB and 12,288
 * copies; dictionaries of the set that no frame of the plan names cost it
 * nothing. */
typedef struct zd_dict_set zd_dict_set;
#define ZD_DICT_SET_MAX 4096
int  zd_dict_set_create(const zd_dict* const* dicts, size_t ndicts, int fallback, zd_dict_set** out);
/* Legal before the plans / batches made with it are destroyed. */
void zd_dict_set_destroy(zd_dict_set* set);
/* ndicts and fallback as given to zd_dict_set_create.  Either pointer may be NULL. */
int  zd_dict_set_info(const zd_dict_set* set, size_t* ndicts, int* fallback);
/* zd_plan_create with a dictionary set.  A zstd frame with a non-zero
 * Dictionary_ID decodes with the set's dictionary of that ID, as in
 * zd_plan_create_dict (tables, repeat offsets, content); when the set holds
 * none, the frame gets ZD_E_DICT_MISMATCH and the plan stops there like at
 * any failing frame (ZD_E_NOT_DECODED after it).  A frame without an ID, or
 * with ID 0, decodes with the fallback dictionary; with fallback -1 with none:
 * first repeat offsets 1, 4, 8, no previous tables, a match before the
 * frame's start is ZD_E_IMPOSSIBLE_VALUE -- the bytes and status a plain plan
 * gives it.  The relaxation of zd_plan_create_dict (a Raw literals section of
 * 0 bytes is accepted) is plan-wide: it holds for every frame of the plan, the
 * ones that decode without a dictionary included.  A set of one dictionary
 * with fallback 0 gives the bytes and statuses of zd_plan_create_dict.  A frame
 * that zd_plan_decompress plans again (capacity) keeps its own dictionary.
 * Limits, as in zd_plan_create_dict and for every frame of the plan, the ones
 * without a dictionary included: without ZD_F_DICT_BLOCK_PARALLEL the streaming
 * executor only -- never the
 * fused kernel, K4F or K4J, ZD_F_BLOCK_PARALLEL is ignored and
 * zd_plan_info.executors is 0; a frame whose own dictionary's content plus
 * capacity passes the streaming executor's int32 positions is
 * ZD_E_OUT_OF_DOMAIN.  zd_plan_info.ncompressed does not count the
 * dictionaries' tables.  zd_plan_create_device, the sharded calls and
 * zd_context take no set.  ZD_E_INVALID_ARG: a NULL or destroyed set, or one
 * made on another device than the current one. */
int  zd_plan_create_dicts(const uint8_t* src, size_t n, uint32_t flags, const zd_dict_set* set, zd_plan** out);
/* zd_decompress with a dictionary set (set must not be NULL). */
int  zd_decompress_dicts(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len,
                         uint32_t flags, const zd_dict_set* set);

/* ------------------------------------------------------------------ */
/* Batches of scattered chunks (beyond the reference, whose input is    */
/* one byte range of frames): N independently compressed chunks at N    */
/* device addresses, each decoded into its own device buffer with its   */
/* own status.                                                          */
/* ------------------------------------------------------------------ */
typedef struct zd_batch zd_batch;

typedef struct zd_batch_info {
  uint64_t nchunks;
  uint64_t gathered_bytes;  /* the batch's own copy of the chunks (16-byte aligned, padded tails) */
  uint64_t nblocks;
  uint64_t nsequences;
  uint64_t workspace_bytes; /* device memory the batch owns besides that copy */
  uint32_t executors;       /* ZD_EXEC_* bits, as zd_plan_info.executors */
  uint32_t device_built;    /* 1: made by zd_batch_create_device(_dicts), else 0 */
  uint64_t gather_ns;       /* zd_batch_create: pointer-list upload + zd_k_gather */
  uint64_t walk_ns;         /*   zd_k_walk_chunks (count, fill) + the index's way back */
  uint64_t host_ns;         /*   descriptors (host work) */
  uint64_t upload_ns;       /*   workspace allocation + descriptor upload */
  /* zd_batch_create_device, the same four phases (host wall clock):
   *   gather_ns   the layout kernels (zd_k_batch_layout, the scans) + zd_k_gather,
   *               to the wait after it
   *   walk_ns     zd_k_walk_chunks count, the scan of the blocks' places and the
   *               wait for their total; the fill pass and the capacity pass
   *               (zd_k_batch_fit) are queued here and waited for in host_ns
   *   host_ns     the device planner's launches (zd_k_plan_*) and their waits
   *   upload_ns   workspace allocation, dictionary tables and small uploads */
  uint64_t prefix_bytes_total; /* a prefix batch: the sum of prefix_bytes[i] over the chunks that
                                * kept their prefix (0 for any other batch) */
} zd_batch_info;
/* zd_batch_info with what came after prefix_bytes_total (zd_batch_info_get_sized
 * writes it when info_bytes covers it: pass &x.info and sizeof x). */
typedef struct zd_batch_info2 {
  zd_batch_info info;
  uint64_t k4j_chunks;      /* chunks whose frame executes on K4J (any batch kind; 0 without ZD_EXEC_K4J) */
} zd_batch_info2;

/* A batch over nchunks chunks: chunk i is the src_bytes[i] bytes at device
 * address d_src[i] and decodes into [d_dst[i], d_dst[i] + dst_cap[i]).  The
 * four arrays are host arrays of nchunks entries.  A chunk holds exactly one
 * zstd frame, with any number of skippable frames (skipped, never output)
 * before and after it; a chunk of zero bytes or of skippable frames only is
 * ZD_OK with length 0.  Chunks are independent: every chunk gets its own
 * status, no chunk's failure touches another (ZD_E_NOT_DECODED never appears,
 * but in a chain batch, zd_batch_create_chain, for a chunk behind a failed
 * ancestor) and a failing chunk's length is 0:
 *   the walk's own code        the chunk is not consumed entirely that way
 *                              (ZD_E_UNRECOGNIZED_MAGIC, ZD_E_NOT_ENOUGH_BYTES,
 *                              ...: trailing bytes, a truncated frame)
 *   ZD_E_OUT_OF_DOMAIN         a second zstd frame in the chunk
 *   ZD_E_DST_TOO_SMALL         a Frame_Content_Size above dst_cap[i] (found here:
 *                              nothing of the chunk runs), or a frame that
 *                              reaches dst_cap[i] while decoding
 *   anything else              what a plan gives the same frame
 * A frame's capacity is the smaller of dst_cap[i] and what a plan reserves
 * (its Frame_Content_Size when usable, else 128 KiB per block); a frame
 * without a Frame_Content_Size decodes in place in its own buffer.  No byte
 * outside [d_dst[i], d_dst[i] + dst_cap[i]) is written.
 * The call copies the chunks into one buffer the batch owns (zd_k_gather:
 * exactly the bytes [d_src[i], d_src[i] + src_bytes[i]) are read, at any
 * alignment, so the caller owes no ZD_SRC_PADDING and may release the sources
 * when the call returns), walks the chunks' headers on the GPU
 * (zd_k_walk_chunks, one lane per chunk) and builds the descriptors on the
 * host.  Synchronises `stream`.
 * flags: the executor and chain flags of a plan, with a plan's routing;
 * ZD_F_SKIPPABLE is ZD_E_INVALID_ARG.  dict (may be NULL): every chunk decodes
 * with it, under zd_plan_create_dict's limits (the streaming executor only,
 * unless flags has ZD_F_DICT_BLOCK_PARALLEL).
 * ZD_E_INVALID_ARG, before any HIP call: a NULL array with nchunks > 0, a NULL
 * d_src[i] with src_bytes[i] > 0, a NULL d_dst[i] with dst_cap[i] > 0,
 * destination ranges that overlap. */
int  zd_batch_create(const void* const* d_src, const uint64_t* src_bytes,
                     void* const* d_dst, const uint64_t* dst_cap, size_t nchunks,
                     uint32_t flags, const zd_dict* dict, void* stream, zd_batch** out);
/* zd_batch_create with a dictionary set (must not be NULL) in place of the one
 * dictionary: every chunk's frame chooses its dictionary as in
 * zd_plan_create_dicts, under its limits; a chunk whose frame names an ID the
 * set does not hold is ZD_E_DICT_MISMATCH, alone.  The other arguments, checks
 * and costs are zd_batch_create's; a set made on another device than the
 * current one is ZD_E_INVALID_ARG. */
int  zd_batch_create_dicts(const void* const* d_src, const uint64_t* src_bytes,
                           void* const* d_dst, const uint64_t* dst_cap, size_t nchunks,
                           uint32_t flags, const zd_dict_set* set, void* stream, zd_batch** out);
/* zd_batch_create / zd_batch_create_dicts for a chunk table that is itself on
 * the device: the four arrays are DEVICE arrays of nchunks entries, readable
 * on `stream` when the call is made; they may be released when it returns (the
 * batch keeps its own copies).  Layout, gather, header walk, capacity checks
 * and descriptors are all built on the GPU: no per-block data and no frame /
 * block index comes to the host, which reads back a few words per phase and
 * 16 bytes a chunk.  The result is an ordinary batch (zd_batch_info.
 * device_built = 1): every zd_batch_* call works on it with the meaning, the
 * routing and the executors of the batch zd_batch_create makes from the same
 * entries, and everything zd_batch_create says about a chunk holds.
 * Synchronises `stream`.  What differs:
 *  - ZD_E_INVALID_ARG for the whole call, before any HIP call: out NULL,
 *    ZD_F_SKIPPABLE in flags, nchunks >= 2^31, a NULL array with nchunks > 0, a
 *    destroyed dictionary or set.  (A dictionary or set of another device:
 *    ZD_E_INVALID_ARG as in zd_batch_create.)  nchunks == 0 is ZD_OK without a
 *    HIP call.
 *  - The entries cannot be read without a round trip, so what zd_batch_create
 *    refuses the whole batch for is a per-chunk outcome here: a NULL source
 *    with a non-zero size, a NULL destination with a non-zero capacity, or an
 *    address range that wraps makes that chunk ZD_E_INVALID_ARG (length 0);
 *    nothing of it is read or written and no other chunk is touched.
 *  - A chunk of 2^32 bytes or more is ZD_E_OUT_OF_DOMAIN, alone (the layout's
 *    64-bit sums cannot wrap at any legal nchunks).
 *  - Overlapping destinations are NOT checked (that needs a sort): keeping the
 *    destination ranges disjoint is the caller's duty.  Overlapping ranges give
 *    unspecified bytes in them; still no byte outside the union of the
 *    destination ranges is written.
 *  - ZD_E_OUT_OF_DOMAIN for the whole call when the chunks' 32 KiB pieces pass
 *    zd_k_gather's grid (as zd_batch_create), known here once the layout's
 *    totals are back. */
int  zd_batch_create_device(const void* const* d_src_ptrs, const uint64_t* d_src_bytes,
                            void* const* d_dst_ptrs, const uint64_t* d_dst_cap, size_t nchunks,
                            uint32_t flags, const zd_dict* dict, void* stream, zd_batch** out);
/* zd_batch_create_device with a dictionary set (must not be NULL): the plan
 * pays only for the dictionaries its own chunks use, as zd_batch_create_dicts. */
int  zd_batch_create_device_dicts(const void* const* d_src_ptrs, const uint64_t* d_src_bytes,
                                  void* const* d_dst_ptrs, const uint64_t* d_dst_cap, size_t nchunks,
                                  uint32_t flags, const zd_dict_set* set, void* stream, zd_batch** out);
/* Deltas: a batch whose chunk i decodes against its own PREFIX, the
 * prefix_bytes[i] bytes at device address d_prefix[i] -- what
 * ZSTD_DCtx_refPrefix gives one frame and `zstd --patch-from` one file, for
 * every chunk of a batch at once.  The six arrays are host arrays of nchunks
 * entries; the first four are zd_batch_create's.
 *  - Prefix content.  A prefix is raw content, always (ZSTD_dct_rawContent, as
 *    refPrefix): a leading dictionary magic (37 a4 30 ec) is just bytes.
 *  - Decode model.  Chunk i's frame starts at position prefix_bytes[i]; its
 *    first repeat offsets are 1, 4, 8 and it has no previous tables.  A match
 *    may reach any prefix byte, however far the frame has advanced (no window
 *    check, as everywhere here); an offset larger than the prefix size plus the
 *    position is ZD_E_IMPOSSIBLE_VALUE.  The output holds the frame's own bytes
 *    only.
 *  - No prefix.  prefix_bytes[i] == 0 (d_prefix[i] may then be NULL): the chunk
 *    decodes with no prefix, exactly as in a plain batch -- but for the
 *    batch-wide relaxation every dictionary batch has: an empty Raw literals
 *    section is accepted.
 *  - Dictionary_ID.  A frame that names a non-zero Dictionary_ID is
 *    ZD_E_DICT_MISMATCH, for that chunk alone.
 *  - Everything else zd_batch_create says about a chunk holds unchanged: one
 *    zstd frame per chunk with skippable frames skipped, a status of its own for
 *    every chunk, length 0 on failure, nothing written outside [d_dst[i],
 *    d_dst[i] + dst_cap[i]).
 *  - Executors.  Without ZD_F_BLOCK_PARALLEL the streaming executor only,
 *    like dictionary batches: zd_batch_info.executors is 0.  A chunk whose
 *    prefix size plus capacity passes that executor's int32 positions
 *    (0x7FFF0000) is ZD_E_OUT_OF_DOMAIN, alone, whether or not its frame has
 *    sequences.  With ZD_F_BLOCK_PARALLEL every frame of the batch with a
 *    compressed block executes block-parallel (K4J; executors carries
 *    ZD_EXEC_K4J), the others on the streaming executor as before.  For a K4J
 *    frame the prefix alone must fit 0x7FFF0000 bytes and the capacity K4J's
 *    32 GiB: a 1.5 GiB shard decodes against its 1.5 GiB predecessor.  A chunk
 *    whose block-parallel execution did not converge is decoded again on the
 *    streaming executor inside zd_batch_results, with its prefix; there a
 *    prefix plus capacity past 0x7FFF0000 ends ZD_E_OUT_OF_DOMAIN.  The same
 *    bytes and statuses either way.
 *  - Window.  Frames keep the reference's 8 MiB window limit unless the batch
 *    has ZD_F_LONG_WINDOW (up to 2 GiB): a --patch-from archive of a file
 *    past 8 MiB needs it.
 *  - Read bounds.  No byte outside [d_prefix[i], d_prefix[i] + prefix_bytes[i])
 *    is ever read through a prefix pointer, at any alignment: the caller owes
 *    no padding on either side.
 *  - When prefixes are read.  By zd_batch_decode_async, not here: addresses and
 *    sizes are fixed at creation, the CONTENTS may change between launches (not
 *    during one), and the buffers must stay valid until zd_batch_destroy.  The
 *    sources are gathered at creation, as in zd_batch_create.
 *  - Overlap.  Prefixes may overlap one another and the sources.  A prefix range
 *    that overlaps any destination range of the batch is ZD_E_INVALID_ARG.
 *  - Flags.  ZD_F_VERIFY_CHECKSUM works and hashes the frame's own bytes;
 *    ZD_F_SKIPPABLE is ZD_E_INVALID_ARG.
 *  - A prefix batch takes no dictionary and no dictionary set.
 * The result is an ordinary batch: every zd_batch_* call works on it;
 * zd_batch_info.prefix_bytes_total is the prefixes' bytes in all.
 * ZD_E_INVALID_ARG, before any HIP call: what zd_batch_create refuses; a NULL
 * d_prefix or prefix_bytes with nchunks > 0; a NULL d_prefix[i] with
 * prefix_bytes[i] > 0; a prefix range that wraps; a prefix range that overlaps
 * a destination range.  nchunks == 0 is ZD_OK.
 * Limits (not in this interface): no packed prefix batches; prefixes cannot be
 * re-pointed after creation; no prefixes on the LDS-resident or fused
 * executors, and on the block-parallel one by ZD_F_BLOCK_PARALLEL or, chunk by
 * chunk, by ZD_F_AUTO_EXECUTOR; none in zd_plan_*, the sharded calls or zd_context;
 * no window past 2 GiB.  (A
 * chunk whose prefix is another chunk's output of the same launch: a chain
 * batch, zd_batch_create_chain.) */
int  zd_batch_create_prefix(const void* const* d_src, const uint64_t* src_bytes,
                            void* const* d_dst, const uint64_t* dst_cap,
                            const void* const* d_prefix, const uint64_t* prefix_bytes,
                            size_t nchunks, uint32_t flags, void* stream, zd_batch** out);
/* zd_batch_create_prefix for a chunk table on the device: the six arrays are
 * DEVICE arrays of nchunks entries, under zd_batch_create_device's terms (the
 * batch keeps its own copies; device_built = 1).  The per-entry cases are a
 * per-chunk outcome: a NULL d_prefix[i] with prefix_bytes[i] > 0 or a prefix
 * range that wraps makes that chunk ZD_E_INVALID_ARG (length 0), and nothing of
 * the chunk or its prefix is read.  A prefix range that overlaps a destination
 * range is NOT checked: keeping them apart is the caller's duty, as for the
 * destinations themselves. */
int  zd_batch_create_device_prefix(const void* const* d_src_ptrs, const uint64_t* d_src_bytes,
                                   void* const* d_dst_ptrs, const uint64_t* d_dst_cap,
                                   const void* const* d_prefix_ptrs, const uint64_t* d_prefix_bytes,
                                   size_t nchunks, uint32_t flags, void* stream, zd_batch** out);
/* Delta chains: a prefix batch in which a chunk's prefix may be ANOTHER CHUNK'S
 * OUTPUT OF THE SAME LAUNCH -- page versions v1 <- v2 <- v3, a record and its
 * patches, a shard patched every step -- decoded by one batch instead of one
 * batch per link.  The seven arrays are host arrays of nchunks entries; the
 * first six are zd_batch_create_prefix's.
 *  - parent[i] == -1: chunk i is exactly a chunk of a prefix batch, its prefix
 *    d_prefix[i] / prefix_bytes[i] (0 bytes: none).  d_prefix and prefix_bytes
 *    may BOTH be NULL: no external prefix anywhere.  parent must not be NULL
 *    when nchunks > 0.
 *  - parent[i] == j, j in [0, nchunks), j != i: chunk i's prefix is chunk j's
 *    decoded output of the same launch, at d_dst[j]; its size is j's
 *    Frame_Content_Size; prefix_bytes[i] must be 0.  The order of the chunks is
 *    free (a child may come before its parent) and many children may share a
 *    parent.  A chunk's LEVEL is the number of its in-batch ancestors, at most
 *    ZD_CHAIN_MAX_DEPTH.
 *  - How it runs.  Tables, literals and sequence chains of every chunk run once,
 *    together, as in a prefix batch: only execution reads a prefix.  The
 *    streaming executor (zd_k_execute_chain) is then launched once per level, in
 *    level order on the stream, so a parent is complete before its children
 *    start: no workgroup ever waits for another.
 *  - Statuses.  A chunk whose parent's final status is not ZD_OK is
 *    ZD_E_NOT_DECODED with length 0 -- final includes ZD_E_CHECKSUM_WRONG from
 *    ZD_F_VERIFY_CHECKSUM and a parent whose decoded length is not the size the
 *    child was planned with -- and so, transitively, is every chunk behind it.
 *    No prefix byte is read for such a chunk (with ZD_F_VERIFY_CHECKSUM a child
 *    has run against its parent's bytes, inside the parent's buffer, before the
 *    parent's checksum is known); its leading raw / RLE blocks may have been
 *    copied into its own destination already: nothing outside the destination
 *    ranges is ever written.  zd_batch_device_checksums' entries of such a
 *    chunk are unspecified.  A chunk whose parent's frame carries no
 *    Frame_Content_Size is ZD_E_OUT_OF_DOMAIN at creation (the size is needed
 *    to plan it); the parent is unaffected.  A parent that is an empty chunk or
 *    holds skippable frames only (ZD_OK, length 0) gives its child a prefix of
 *    0 bytes: the child decodes as a plain chunk.  Prefix size plus capacity
 *    above 0x7FFF0000 is ZD_E_OUT_OF_DOMAIN for that chunk, as in a prefix
 *    batch.
 *  - ZD_E_INVALID_ARG for the whole call, before any HIP call: what
 *    zd_batch_create_prefix refuses (its prefix-overlaps-destination rule for
 *    the external prefixes only; exactly one of d_prefix / prefix_bytes NULL);
 *    a parent outside [-1, nchunks); parent[i] == i; a cycle; a chunk with more
 *    than ZD_CHAIN_MAX_DEPTH ancestors; prefix_bytes[i] != 0 on a chunk with a
 *    parent.  nchunks == 0 is ZD_OK.
 *  - ZD_F_CHAIN_BLOCK_PARALLEL (large deltas, a checkpoint shard patched every
 *    step): the frames with a compressed block execute on K4J instead.  Per
 *    level, in level order on the stream: zd_k_execute_chain over the level's
 *    frames, then K4J's scatter over the level's segments and its
 *    pointer-jumping rounds over the level's pieces -- still no workgroup that
 *    waits for another.  A chunk whose pointer jumping does not converge shows
 *    ZD_E_OUT_OF_DOMAIN in zd_batch_device_results and its descendants
 *    ZD_E_NOT_DECODED until zd_batch_results, which decodes that chunk and every
 *    chunk behind it again on the streaming executor (one internal chain batch)
 *    and updates the device arrays.
 *  - ZD_F_AUTO_EXECUTOR: the same layout and launches, with each chunk's frame
 *    routed by the rule at the flag (the width is the widest level's chunk
 *    count); page links stay on zd_k_execute_chain, large links go to K4J, and a
 *    failure crosses the executors as it crosses levels.
 * Everything else is a prefix batch's: the streaming executor only (but for
 * ZD_F_CHAIN_BLOCK_PARALLEL and ZD_F_AUTO_EXECUTOR; ZD_F_BLOCK_PARALLEL is ignored), no
 * dictionary or set, not packed, ZD_F_SKIPPABLE refused, the sources gathered
 * at creation, zd_batch_decode_async free of allocation and host
 * synchronisation, capturable and re-launchable; every zd_batch_* call works on
 * the result (zd_batch_info.prefix_bytes_total counts the external prefixes).
 * Limits (not in this interface): no packed chain batches, no re-pointing, no
 * chains through dictionaries, none in zd_plan_*, the sharded calls or
 * zd_context. */
#define ZD_CHAIN_MAX_DEPTH 255   /* in-batch ancestors a chunk may have: levels 0..255 */
int  zd_batch_create_chain(const void* const* d_src, const uint64_t* src_bytes,
                           void* const* d_dst, const uint64_t* dst_cap,
                           const void* const* d_prefix, const uint64_t* prefix_bytes,
                           const int64_t* parent, size_t nchunks, uint32_t flags,
                           void* stream, zd_batch** out);
/* zd_batch_create_chain for a chunk table on the device: the seven arrays are
 * DEVICE arrays of nchunks entries (d_prefix_ptrs and d_prefix_bytes may both
 * be NULL), under zd_batch_create_device_prefix's terms and with its host
 * waits, none more.  What the host-array call refuses the call for is a
 * per-chunk outcome: a parent outside [-1, nchunks), a chunk that names itself,
 * a prefix size on a chunk with a parent, and a chunk that reaches no root
 * within ZD_CHAIN_MAX_DEPTH hops -- on a cycle, behind one, or deeper than the
 * limit -- make that chunk ZD_E_INVALID_ARG (length 0); the chunks behind a
 * refused chunk that are not refused themselves are ZD_E_NOT_DECODED. */
int  zd_batch_create_device_chain(const void* const* d_src_ptrs, const uint64_t* d_src_bytes,
                                  void* const* d_dst_ptrs, const uint64_t* d_dst_cap,
                                  const void* const* d_prefix_ptrs, const uint64_t* d_prefix_bytes,
                                  const int64_t* d_parent, size_t nchunks, uint32_t flags,
                                  void* stream, zd_batch** out);
/* A chain batch's shape: the number of levels (1 when no chunk has a parent, or
 * the batch has no chunks) = the executor launches of a decode at most, and the
 * number of chunks with a parent.  Either pointer may be NULL.  ZD_E_INVALID_ARG
 * for a NULL batch or one that was not made by a chain call. */
int  zd_batch_chain_info(const zd_batch* batch, uint32_t* levels, uint64_t* links);
/* What chunks need of their destinations, asked on the device: chunk i is the
 * d_src_bytes[i] bytes at d_src_ptrs[i], as in zd_batch_create_device.  All
 * five arrays are DEVICE arrays of nchunks entries; d_status and d_exact may be
 * NULL.  The call queues one kernel (zd_k_chunk_sizes, one lane per chunk) on
 * `stream` and returns: no allocation, no copy, no host synchronisation, so it
 * can be captured like zd_decode_async.  The chunks are read where they lie, at
 * any alignment, and exactly the bytes [src, src + size) at most: the caller
 * owes no ZD_SRC_PADDING.  Per chunk:
 *   d_size[i]    the chunk's reserve: its frame's Frame_Content_Size when that
 *                is usable (present and not above `bound`), else `bound` = 128
 *                KiB per compressed block + the sizes of the raw and RLE
 *                blocks.  It is the capacity a batch gives the chunk at most,
 *                so a destination of d_size[i] bytes never makes the chunk
 *                ZD_E_DST_TOO_SMALL.  0 for a chunk without a zstd frame (no
 *                bytes, skippable frames only) and for a chunk whose status is
 *                not ZD_OK.
 *   d_exact[i]   1: d_size[i] is the Frame_Content_Size (the decoded length of
 *                a frame that decodes); 0: it is the bound (the decoded length
 *                is at most that), or 0.
 *   d_status[i]  what the header walk of that chunk alone gives, with the
 *                meanings of zd_batch_create_device: ZD_OK; the walk's own code
 *                (a truncated frame, trailing bytes, a section header that does
 *                not parse); ZD_E_OUT_OF_DOMAIN at a second zstd frame or for a
 *                chunk of 2^32 bytes or more; ZD_E_INVALID_ARG for a NULL
 *                address with a non-zero size or a range that wraps (nothing of
 *                such a chunk is read).
 * Errors that only decoding finds are NOT seen here -- a corrupt table
 * description, a frame that overruns its Frame_Content_Size, a dictionary the
 * batch does not have: such a chunk is ZD_OK here with its reserve, and fails
 * when it is decoded.
 * flags: ZD_SIZES_DICT when the chunks will be decoded with a dictionary or a
 * set (an empty Raw literals section is then accepted, as in a dictionary
 * plan; without it such a chunk is ZD_E_EMPTY_SLICE), a prefix batch included;
 * ZD_SIZES_LONG_WINDOW when they will be decoded with ZD_F_LONG_WINDOW (a
 * Window_Size up to 2 GiB is then no failure; the bit is that flag's own);
 * ZD_SIZES_RFC when they will be decoded with ZD_F_RFC (the walk then reads
 * section headers as that flag does: the long-form Number_of_Sequences, an
 * empty Raw literals section, an empty Huffman stream; the bit is that flag's own).
 * ZD_E_INVALID_ARG, before any HIP call: a NULL d_src_ptrs, d_src_bytes or
 * d_size with nchunks > 0, nchunks >= 2^31, unknown flag bits.  nchunks == 0 is
 * ZD_OK without a HIP call. */
#define ZD_SIZES_DICT 1u
#define ZD_SIZES_LONG_WINDOW 2048u   /* the chunks will be decoded with ZD_F_LONG_WINDOW (the same bit) */
#define ZD_SIZES_RFC 16384u          /* the chunks will be decoded with ZD_F_RFC (the same bit) */
/* ZD_SIZES_MULTI_FRAME: the chunks will be decoded by a multi-frame batch
 * (zd_multi_create_device), so a chunk may hold any number of concatenated zstd
 * frames.  It is cut into sub-chunks as that call cuts it; d_size[i] is the sum
 * of the sub-chunks' reserves (a destination of that many bytes never makes the
 * chunk ZD_E_DST_TOO_SMALL), d_exact[i] is 1 when every sub-chunk's reserve is
 * its frame's Frame_Content_Size (0 for a chunk that ends in skippable frames,
 * or of no bytes), d_status[i] the walk status of the first sub-chunk that
 * fails: a second zstd frame is no failure here.  Without the flag every output
 * is as it always was.  (Bits 2 and 4 of the word stay ZD_E_INVALID_ARG.) */
#define ZD_SIZES_MULTI_FRAME 8u
int  zd_chunk_sizes_device(const void* const* d_src_ptrs, const uint64_t* d_src_bytes, size_t nchunks,
                           uint32_t flags, uint64_t* d_size, int32_t* d_status, uint8_t* d_exact, void* stream);
/* zd_batch_create_device without destinations: a PACKED batch lays its outputs
 * out itself, in one buffer that is bound to it afterwards
 * (zd_batch_bind_output).  Chunk i's capacity is its reserve (what
 * zd_chunk_sizes_device reports for it) and its place is offset[i] from the
 * buffer's base: the offsets ascend with i, each is a multiple of `align` (a
 * power of two in [1, 4096]) and offset[i + 1] >= offset[i] + cap[i];
 * out_bytes = the sum of the reserves each rounded up to `align`
 * (zd_batch_output_layout).  Creation is zd_batch_create_device's -- layout,
 * gather, the two walk passes, then zd_k_batch_pack and one scan for the
 * places, the capacity pass and the device planner on those two columns -- and
 * the result is an ordinary batch (device_built = 1) with the routing,
 * executors, dictionary handling and per-chunk statuses of the batch
 * zd_batch_create_device makes from the same sources with d_dst[i] = base +
 * offset[i] and dst_cap[i] = cap[i].  A packed batch never reports
 * ZD_E_DST_TOO_SMALL from creation.  A frame without a usable
 * Frame_Content_Size gets its bound and decodes in place at its offset: the
 * buffer has slack after it, and the lengths (zd_batch_device_results) say how
 * much; offsets and lengths together are a complete index of the output.
 * A frame whose reserve passes the executors' limits is that chunk's
 * ZD_E_OUT_OF_DOMAIN, as in any batch; the 64-bit total cannot wrap (a chunk of
 * z < 2^32 bytes reserves less than z / 3 * 128 KiB).
 * Synchronises `stream`: the waits of zd_batch_create_device and none more --
 * the five that read words back (layout totals, block count, routing shape,
 * plan totals, the frames' offsets and capacities) and the one after the
 * gather: the one word of out_bytes comes back with the routing shape.
 * ZD_E_INVALID_ARG, before any HIP call: what zd_batch_create_device refuses
 * the call for (without the destination arrays), and an `align` that is not a
 * power of two in [1, 4096]. */
int  zd_batch_create_device_packed(const void* const* d_src_ptrs, const uint64_t* d_src_bytes, size_t nchunks,
                                   uint32_t align, uint32_t flags, const zd_dict* dict, void* stream,
                                   zd_batch** out);
/* zd_batch_create_device_packed with a dictionary set (must not be NULL). */
int  zd_batch_create_device_packed_dicts(const void* const* d_src_ptrs, const uint64_t* d_src_bytes, size_t nchunks,
                                         uint32_t align, uint32_t flags, const zd_dict_set* set, void* stream,
                                         zd_batch** out);
/* A packed batch's layout: the bytes its output buffer needs and two device
 * arrays of nchunks uint64 entries, the chunks' offsets from the base and
 * their capacities.  The batch owns the arrays; they are valid until
 * zd_batch_destroy, and work queued on the creation's stream reads them without
 * a round trip.  Any of the three pointers may be NULL.  ZD_E_INVALID_ARG for a
 * NULL batch or one that was not made packed. */
int  zd_batch_output_layout(const zd_batch* batch, uint64_t* out_bytes,
                            const uint64_t** d_offset, const uint64_t** d_cap);
/* Binds the packed batch's output buffer: the cap bytes at d_out.  No HIP
 * call: the base travels as a kernel argument at the next
 * zd_batch_decode_async.  No alignment is required of d_out (the offsets are
 * multiples of `align` from the base).  cap < out_bytes is ZD_E_DST_TOO_SMALL
 * and the previous binding stays; d_out may be NULL only when out_bytes == 0;
 * a range that wraps, a NULL batch or a batch that was not made packed is
 * ZD_E_INVALID_ARG.  Binding again is legal and takes effect at the next
 * zd_batch_decode_async.  zd_batch_results (which decodes a chunk again whose
 * block-parallel execution did not converge) and zd_batch_checksums work on
 * the CURRENT binding: call them for a decode before binding another buffer.
 * zd_batch_decode_async on a packed batch with out_bytes > 0 and no binding is
 * ZD_E_INVALID_ARG. */
int  zd_batch_bind_output(zd_batch* batch, void* d_out, uint64_t cap);
/* The batch's figures.  zd_batch_info grew by prefix_bytes_total without a new
 * ZD_ABI_VERSION, so the exported zd_batch_info_get keeps writing the 80 bytes
 * up to and including upload_ns -- a caller built against the earlier header
 * passes no more -- and zd_batch_info_get_sized writes the first info_bytes
 * bytes of the current struct (at most all of it; fewer than 80 is
 * ZD_E_INVALID_ARG).  C and C++ code that includes this header gets the sized
 * call under the old name, so its whole struct is filled.  What came later
 * (zd_batch_info2: k4j_chunks at byte 88) follows the struct in the same
 * call: zd_batch_info_get_sized(b, &x.info, sizeof x) with a zd_batch_info2 x. */
int  zd_batch_info_get(const zd_batch* batch, zd_batch_info* info);
int  zd_batch_info_get_sized(const zd_batch* batch, zd_batch_info* info, size_t info_bytes);
#ifndef ZD_NO_SIZED_INFO_MACRO
#define zd_batch_info_get(batch, info) zd_batch_info_get_sized((batch), (info), sizeof(zd_batch_info))
#endif
/* Launches the decode of every chunk on `stream`, ending with a kernel that
 * writes the batch's device result arrays (zd_batch_device_results).  No
 * allocation, no host synchronisation, like zd_decode_async; may be called
 * again (the destinations are decoded again). */
int  zd_batch_decode_async(zd_batch* batch, void* stream);
/* The device result arrays, owned by the batch (nchunks entries each): after
 * the work zd_batch_decode_async queued, d_status[i] is chunk i's status and
 * d_len[i] its decoded length (0 unless ZD_OK).  Work queued behind it on the
 * same stream reads them without a host round trip. */
int  zd_batch_device_results(const zd_batch* batch, const int32_t** d_status, const uint64_t** d_len);
/* A ZD_F_VERIFY_CHECKSUM batch's device checksum arrays, owned by the batch
 * (nchunks entries each) and written by the verification pass of
 * zd_batch_decode_async, before the result arrays: d_hash[i] is the full 64-bit
 * XXH64 of chunk i's decoded bytes, or 0 for a chunk that did not decode or
 * carries no Content_Checksum (the pass reads only the frames it checks; a
 * chunk that fails verification keeps its digest); d_ok[i] is 1 / 0 / -1 with
 * zd_batch_checksums' meanings (matches / differs / no Content_Checksum or not
 * decoded).  Work queued behind the decode on the same stream reads them
 * without a host round trip.  Either pointer may be NULL; a batch of no chunks
 * gives NULL arrays.  ZD_E_INVALID_ARG for a NULL batch or one made without
 * the flag. */
int  zd_batch_device_checksums(const zd_batch* batch, const uint64_t** d_hash, const int8_t** d_ok);
/* Waits for `stream` and returns the same arrays (host arrays of cap >=
 * nchunks entries, either may be NULL) and the number of chunks that are not
 * ZD_OK.  A chunk whose block-parallel execution did not converge (K4J's
 * rounds, the case zd_plan_decompress plans again) is decoded again here on
 * the streaming executor, and the device arrays are updated. */
int  zd_batch_results(zd_batch* batch, void* stream, int32_t* status, uint64_t* len, size_t cap, uint64_t* nfailed);
/* zd_plan_checksums per chunk, after zd_batch_results: ok[i] = 1 / 0 / -1
 * (matches / differs / no Content_Checksum or not decoded), hash[i] = XXH64. */
int  zd_batch_checksums(zd_batch* batch, void* stream, int32_t* ok, uint64_t* hash);
void zd_batch_destroy(zd_batch* batch);

/* ------------------------------------------------------------------ */
/* Random access (beyond the reference): byte ranges of a zstd          */
/* SEEKABLE archive that lies on the device.  A seekable archive is an  */
/* ordinary multi-frame .zst whose last frame is a skippable frame      */
/* holding a seek table: every entry's compressed and decompressed size */
/* and, optionally, a checksum (csrc/zd_seek.h restates the layout).    */
/* An entry is treated as a batch chunk: one zstd frame with any number */
/* of skippable frames around it; an entry of two zstd frames is that   */
/* chunk's ZD_E_OUT_OF_DOMAIN, as in any batch (a documented limit).    */
/* The table's per-entry checksums are verified inside the launch by a  */
/* read made with ZD_SEEK_VERIFY_TABLE (zd_seekable_read_create_ex).    */
/* Limits: no dictionary, prefix or chain reads; a read's destinations  */
/* cannot be re-pointed; the ranges come as device arrays only; nothing */
/* of this in zd_plan_*, the sharded calls or zd_context.               */
/* ------------------------------------------------------------------ */
typedef struct zd_seekable zd_seekable;
typedef struct zd_seek_read zd_seek_read;

typedef struct zd_seekable_info {
  uint64_t nframes;            /* entries of the seek table */
  uint64_t content_bytes;      /* the sum of the Decompressed_Sizes */
  uint64_t compressed_bytes;   /* the sum of the Compressed_Sizes: the archive without its table */
  uint64_t table_bytes;        /* the seek table's frame: header, entries, footer */
  uint32_t has_checksums;      /* the entries carry a Checksum */
  uint32_t max_frame_content;  /* the largest Decompressed_Size */
} zd_seekable_info;

/* Opens the archive of n bytes at device address d_archive.  The last 9
 * bytes come to the host (one small copy, one wait) and are checked; then
 * zd_k_seek_table reads the entries where they lie -- at any alignment,
 * never outside the table -- into three device arrays the object owns,
 * c_off[nframes + 1] and d_off[nframes + 1] (u64: entry f occupies archive
 * bytes [c_off[f], c_off[f + 1]) and holds content bytes [d_off[f],
 * d_off[f + 1]); the sums cannot wrap at any legal table) and
 * checksum[nframes] (u32, when present), and checks the skippable header;
 * one more wait brings back the two totals and the header's verdict.  Two
 * host waits on `stream` in all.
 *   ZD_E_NOT_ENOUGH_BYTES    n < 17 (before any HIP call); a table larger
 *                            than the archive
 *   ZD_E_UNRECOGNIZED_MAGIC  the footer's or the skippable header's magic
 *   ZD_E_FRAME_RESERVED_SET  reserved descriptor bits set
 *   ZD_E_OUT_OF_DOMAIN       more than 2^27 entries
 *   ZD_E_SEEK_TABLE          Frame_Size is not nframes * entry_bytes + 9, or
 *                            the compressed sizes do not sum to exactly the
 *                            bytes before the table
 *   ZD_E_INVALID_ARG         d_archive or out NULL (before any HIP call)
 * The archive must stay valid and unchanged until zd_seekable_close: it is
 * read here and at each read's creation, never by a decode.  It needs no
 * padding. */
int  zd_seekable_open_device(const void* d_archive, size_t n, void* stream, zd_seekable** out);
int  zd_seekable_info_get(const zd_seekable* z, zd_seekable_info* info);
/* The three device arrays, for callers that plan their own reads; the object
 * owns them (d_checksum: NULL without checksums; any pointer may be NULL). */
int  zd_seekable_table(const zd_seekable* z, const uint64_t** d_c_off, const uint64_t** d_d_off,
                       const uint32_t** d_checksum);
/* Reads made from the archive stay usable; no new read can be made. */
void zd_seekable_close(zd_seekable* z);

/* A read of nranges ranges: range i is content bytes [d_off[i], d_off[i] +
 * d_len[i]), clamped to the content's end as pread clamps (a range that
 * starts at or past the end, or of length 0, is ZD_OK with length 0), and is
 * written to [d_dst[i], d_dst[i] + clamped length): no other byte is written,
 * d_dst[i] may have any alignment.  The three arrays are DEVICE arrays of
 * nranges entries, readable on `stream`; they may be released when the call
 * returns.  A NULL d_dst[i] with a non-zero clamped length, or an address range
 * that wraps, makes that range ZD_E_INVALID_ARG, alone (it needs no frame:
 * nothing is read or written for it).  Overlapping
 * destinations are the caller's duty, as in zd_batch_create_device.
 * flags: a plain batch's flags, handed to the inner batch
 * (ZD_F_VERIFY_CHECKSUM verifies the frames' own Content_Checksums,
 * ZD_F_LONG_WINDOW works); ZD_F_SKIPPABLE is ZD_E_INVALID_ARG.
 * ZD_E_INVALID_ARG for the whole call, before any HIP call: out NULL, a NULL
 * array with nranges > 0, nranges >= 2^31, unknown flag bits, a NULL archive
 * (what a closed one's handle is to its owner: the Python mirror passes it).
 * Every needed frame is decoded once per launch, however many ranges touch
 * it.  A frame that lies wholly inside exactly one range decodes IN PLACE, at
 * d_dst[i] + (d_off[f] - off_i) with capacity Decompressed_Size: a sequential
 * read of a long range stages nothing but its two edge frames.  Every other
 * needed frame -- a partial frame at a range's edge, a frame more than one
 * range touches -- decodes into a staging buffer the read owns (offsets
 * rounded to 16, from the workspace cache).  Built on the GPU
 * (zd_k_seek_cover, zd_k_seek_mark, zd_k_seek_plan, the scans,
 * zd_k_seek_chunks) and handed to the device creation of a batch.  Host waits:
 * one of its own (the needed frames, the staging bytes, the 32 KiB copy pieces
 * come back) and those of zd_batch_create_device, none more.
 * ZD_E_OUT_OF_DOMAIN for the whole call: 2^31 copy pieces or more. */
int  zd_seekable_read_create(zd_seekable* z, const uint64_t* d_off, const uint64_t* d_len,
                             void* const* d_dst, size_t nranges, uint32_t flags,
                             void* stream, zd_seek_read** out);
/* A read's own options (read_flags; not plan flags, which go to the inner
 * batch).  ZD_SEEK_VERIFY_TABLE: every launch compares the seek table's
 * Checksum -- the low 32 bits of XXH64, seed 0, of the entry's decoded bytes,
 * the archive format's integrity mechanism -- of every needed entry, as zstd's
 * own seekable reader does on every read. */
#define ZD_SEEK_VERIFY_TABLE 1u
/* ZD_SEEK_RFC: the inner batch is created with ZD_F_RFC, so the archive's
 * frames decode as RFC 8878 and libzstd have them.  A read option and not the
 * plan flag: bit 16384 of `flags` has been ZD_E_INVALID_ARG in both calls since
 * they exist, and stays so; the option's own bit is 4, bits 2 and 3 of
 * read_flags being rejected likewise. */
#define ZD_SEEK_RFC 4u
/* zd_seekable_read_create with a read option word; read_flags 0 is that call.
 * Two more ZD_E_INVALID_ARG cases for the whole call, both before any HIP call
 * of this function: unknown read_flags bits; ZD_SEEK_VERIFY_TABLE on an
 * archive whose table carries no checksums (zd_seekable_info.has_checksums 0:
 * a caller who asks for verification never silently gets none).  No host wait
 * is added to the creation.
 * A verified read's zd_seek_read_decode_async queues the inner batch's decode,
 * zd_k_seek_verify, zd_k_seek_finish and the result pass; zd_seek_read_finish_
 * async and the re-run inside zd_seek_read_results include the verify pass.
 * An entry is COMPARED when it is a needed entry whose chunk ended ZD_OK with
 * a decoded length equal to its Decompressed_Size: its bytes are hashed where
 * they were decoded (the destination or the staging buffer, at any alignment,
 * never a byte outside them), once per launch however many ranges touch it.
 * Every other entry is never read (verdict -1); entries of no content bytes
 * are never decoded and never compared.  With ZD_F_VERIFY_CHECKSUM in flags,
 * an entry whose frame's own Content_Checksum the inner batch verified
 * (d_ok[k] == 1 in zd_batch_device_checksums) is compared by the low 32 bits
 * of that digest and not read again.
 * Range status: among the frames "that did not end ZD_OK" now also counts an
 * entry that was compared and differs, as ZD_E_CHECKSUM_WRONG; the range's
 * status is still that of the lowest-numbered such frame, and ZD_E_SEEK_TABLE
 * what it gets when no frame failed but a length differs. */
int  zd_seekable_read_create_ex(zd_seekable* z, const uint64_t* d_off, const uint64_t* d_len,
                                void* const* d_dst, size_t nranges, uint32_t flags,
                                uint32_t read_flags, void* stream, zd_seek_read** out);
/* A verified read's per-entry verdicts, device arrays the read owns (allocated
 * at creation), *n = frames_decoded entries each, indexed by the inner batch's
 * chunk: d_entry[k] the entry's index in the table, d_ok[k] 1 (matches) / 0
 * (differs) / -1 (not compared), d_hash32[k] the computed low 32 bits, 0 when
 * d_ok[k] is -1.  Valid behind the work a launch queued; a loader learns from
 * them which entry to fetch again.  A read made without ZD_SEEK_VERIFY_TABLE:
 * NULL arrays, *n = 0.  Any pointer may be NULL. */
int  zd_seek_read_device_verdicts(const zd_seek_read* r, const uint32_t** d_entry, const int8_t** d_ok,
                                  const uint32_t** d_hash32, uint64_t* n);
/* Queues, in this order: the inner batch's decode; zd_k_seek_finish, which
 * copies the staged frames' wanted parts to the ranges' destinations (the
 * grid runs over 32 KiB pieces of the destinations; in-place frames are
 * skipped; nothing outside the staging buffer is read, nothing outside the
 * destination ranges written); the result pass, the last launch.  Range i's
 * status is that of the lowest-numbered of its frames that did not end ZD_OK;
 * with every frame ZD_OK but one whose decoded length differs from its
 * Decompressed_Size, ZD_E_SEEK_TABLE; else ZD_OK.  Its length is the clamped
 * length, or 0 on failure; a failed range's destination bytes are unspecified.
 * A ZD_SEEK_VERIFY_TABLE read queues zd_k_seek_verify between the decode and
 * zd_k_seek_finish (zd_seekable_read_create_ex).
 * No allocation, no host synchronisation: capturable, and may be called again. */
int  zd_seek_read_decode_async(zd_seek_read* r, void* stream);
/* The finish and result passes alone (a verified read: the verify pass in
 * front of them), behind whatever `stream` holds: what
 * zd_seek_read_results runs after the inner batch's own results, for a caller
 * that reads the inner batch's state itself, and what a timing run puts between
 * two events.  ZD_E_INVALID_ARG before the first zd_seek_read_decode_async. */
int  zd_seek_read_finish_async(zd_seek_read* r, void* stream);
/* The per-range device arrays (nranges entries each), owned by the read. */
int  zd_seek_read_device_results(const zd_seek_read* r, const int32_t** d_status, const uint64_t** d_len);
/* Waits and returns the same on the host (arrays of cap >= nranges entries,
 * either may be NULL) and the number of ranges that are not ZD_OK.  Runs the
 * inner zd_batch_results -- a K4J frame that did not converge is decoded again
 * there -- and then the finish and result passes once more. */
int  zd_seek_read_results(zd_seek_read* r, void* stream, int32_t* status, uint64_t* len, size_t cap,
                          uint64_t* nfailed);
typedef struct zd_seek_read_info {
  uint64_t nranges;
  uint64_t frames_decoded;     /* distinct needed entries: the inner batch's chunks */
  uint64_t frames_in_place;    /*   of them, decoded at a range's own destination */
  uint64_t staged_bytes;       /* the staging buffer (every staged frame rounded up to 16) */
  uint64_t copy_pieces;        /* zd_k_seek_finish's grid: 32 KiB pieces of the destinations */
  zd_batch_info2 batch;        /* the inner batch (zeroed when no frame is needed) */
} zd_seek_read_info;
int  zd_seek_read_info_get(const zd_seek_read* r, zd_seek_read_info* info);
/* What zd_seek_read_info_get_sized writes behind zd_seek_read_info when the
 * caller's size covers it. */
typedef struct zd_seek_read_info2 {
  zd_seek_read_info info;
  uint64_t read_flags;         /* the read's option word (ZD_SEEK_VERIFY_TABLE) */
  uint64_t verify_entries;     /* zd_k_seek_verify's entries: frames_decoded with the option, else 0 */
} zd_seek_read_info2;
/* The first `bytes` bytes of zd_seek_read_info2 (as zd_batch_info_get_sized);
 * fewer than sizeof(zd_seek_read_info) is ZD_E_INVALID_ARG. */
int  zd_seek_read_info_get_sized(const zd_seek_read* r, zd_seek_read_info* info, size_t bytes);
void zd_seek_read_destroy(zd_seek_read* r);

/* ------------------------------------------------------------------ */
/* Multi-frame batches: a batch whose chunks hold any number of         */
/* concatenated zstd frames (RFC 8878: a zstd payload), as a streaming  */
/* compressor that closes a frame at every flush, `cat a.zst b.zst`,    */
/* pzstd or a log appended to frame by frame write them.  zd_batch_*    */
/* keeps ZD_E_OUT_OF_DOMAIN for a second frame in a chunk; this object  */
/* is an ordinary device-built batch over the chunks' SUB-CHUNKS, made  */
/* on the GPU, plus two passes behind its decode.                       */
/* ------------------------------------------------------------------ */
typedef struct zd_multi zd_multi;

/* zd_batch_create_device's four DEVICE arrays (readable on `stream`, released
 * when the call returns if the caller likes; the sources too: the inner batch
 * gathers them), its flags, and at most one of dict / set.
 * SUB-CHUNKS.  A chunk is walked from its first byte with the walk the inner
 * batch uses.  Each zstd frame that walks to its end closes a sub-chunk: the
 * bytes from the end of the previous zstd frame (or the chunk's start) to the
 * end of this frame, so skippable frames travel with the frame behind them.
 * Whatever remains -- skippable frames only, bytes that are no frame, a frame
 * whose walk fails with everything behind it -- is one last sub-chunk when it
 * is not empty; a chunk in which no zstd frame walks to its end is one
 * sub-chunk, the whole chunk.  A sub-chunk's status is what
 * zd_batch_create_device gives that byte range.
 * PLACEMENT.  A sub-chunk's reserve and exactness are zd_chunk_sizes_device's.
 * Sub-chunk k of chunk i is IN PLACE when every sub-chunk before it in the
 * chunk is exact: it decodes at d_dst_ptrs[i] + the sum of their
 * Frame_Content_Sizes, with capacity min(reserve, dst_cap_i - offset) when it
 * is exact itself and dst_cap_i - offset when not (0 when the offset is past
 * dst_cap_i: the inner batch's capacity pass then reports ZD_E_DST_TOO_SMALL).
 * Every sub-chunk behind the first inexact one is STAGED: it decodes into a
 * staging buffer the object owns (its reserve as its capacity, offsets rounded
 * up to 16, from the workspace cache) and is copied behind the chunk's earlier
 * bytes by every launch.  Frames that all carry a Frame_Content_Size stage
 * nothing.
 * RESULTS.  A chunk's status is that of its lowest-numbered sub-chunk that did
 * not end ZD_OK; else ZD_E_DST_TOO_SMALL when the decoded lengths, summed in
 * order, pass dst_cap_i at a staged sub-chunk; else ZD_OK with the summed
 * length.  (A frame that ends ZD_OK with a length other than its
 * Frame_Content_Size, with a frame in place behind it: ZD_E_OUT_OF_DOMAIN.)
 * A failed chunk's length is 0 and its destination bytes are unspecified;
 * nothing outside [dst_i, dst_i + dst_cap_i) is ever written and a failing
 * chunk touches no other.  An entry zd_batch_create_device would refuse (a
 * NULL address with a non-zero count, a range that wraps: ZD_E_INVALID_ARG; a
 * chunk of 2^32 bytes or more: ZD_E_OUT_OF_DOMAIN) fails its chunk alone, and
 * none of it is read or written.  Overlapping destinations are the caller's
 * duty.
 * Built on the GPU: zd_k_multi_count (one lane a chunk walks the headers where
 * the chunk lies, at any alignment, no byte outside it), the scans,
 * zd_k_multi_fill, then zd_batch_create_device (or its dictionary forms) with
 * the caller's flags.  Host waits: one of its own (the sub-chunks, the staging
 * bytes, the 32 KiB copy pieces come back) and the inner creation's.
 * ZD_E_INVALID_ARG for the whole call, before any HIP call: out NULL, a NULL
 * array with nchunks > 0, nchunks >= 2^31, both dict and set, ZD_F_SKIPPABLE,
 * unknown flag bits.  ZD_E_OUT_OF_DOMAIN for the whole call: 2^31 sub-chunks
 * or copy pieces, or more.
 * Limits: no prefix, chain or packed multi-frame batches; device arrays only;
 * the destinations are fixed at creation; one lane walks a chunk's headers, so
 * one huge multi-frame file belongs in zd_plan_create_device. */
int  zd_multi_create_device(const void* const* d_src_ptrs, const uint64_t* d_src_bytes,
                            void* const* d_dst_ptrs, const uint64_t* d_dst_cap, size_t nchunks,
                            uint32_t flags, const zd_dict* dict, const zd_dict_set* set,
                            void* stream, zd_multi** out);
/* Queues, in this order: the inner batch's decode; zd_k_multi_join, one lane a
 * chunk over its sub-chunks' results (the chunk's status and length, each
 * staged sub-chunk's final address, "not delivered" from the first failure or
 * overflow on); zd_k_multi_copy over the 32 KiB pieces of the staged reserves
 * (not queued by a batch that stages nothing), which loads only a sub-chunk's
 * own decoded bytes in the staging buffer and stores only inside the chunk's
 * destination.  The device result arrays are final behind these.  No
 * allocation, no host synchronisation: capturable, and may be called again. */
int  zd_multi_decode_async(zd_multi* m, void* stream);
/* The join and copy passes alone, behind whatever `stream` holds (as
 * zd_seek_read_finish_async).  ZD_E_INVALID_ARG before the first
 * zd_multi_decode_async. */
int  zd_multi_finish_async(zd_multi* m, void* stream);
/* The per-chunk device arrays (nchunks entries each), owned by the object. */
int  zd_multi_device_results(const zd_multi* m, const int32_t** d_status, const uint64_t** d_len);
/* Waits and returns the same on the host (arrays of cap >= nchunks entries,
 * either may be NULL) and the number of chunks that are not ZD_OK.  Runs the
 * inner zd_batch_results -- a K4J frame that did not converge is decoded again
 * there -- and then the join and copy passes once more. */
int  zd_multi_results(zd_multi* m, void* stream, int32_t* status, uint64_t* len, size_t cap,
                      uint64_t* nfailed);
/* The sub-chunks: d_first has nchunks + 1 entries, chunk i's sub-chunks are
 * d_first[i] .. d_first[i + 1) of the inner batch's result arrays
 * d_frame_status / d_frame_len (NULL for a batch of no chunks).  Device arrays
 * the object owns; any pointer may be NULL. */
int  zd_multi_device_frames(const zd_multi* m, const uint64_t** d_first,
                            const int32_t** d_frame_status, const uint64_t** d_frame_len);
typedef struct zd_multi_info {
  uint64_t nchunks;
  uint64_t frames;             /* F: the sub-chunks, the inner batch's chunks */
  uint64_t frames_in_place;    /*   of them, decoded in their chunk's destination */
  uint64_t staged_frames;      /*   and decoded into the staging buffer */
  uint64_t staged_bytes;       /* the staging buffer (every staged reserve rounded up to 16) */
  uint64_t copy_pieces;        /* zd_k_multi_copy's grid: 32 KiB pieces of the staged reserves */
  zd_batch_info2 batch;        /* the inner batch (zeroed for a batch of no chunks) */
} zd_multi_info;
/* The first `bytes` bytes of zd_multi_info (as zd_batch_info_get_sized); fewer
 * than the six counters is ZD_E_INVALID_ARG. */
int  zd_multi_info_get_sized(const zd_multi* m, zd_multi_info* info, size_t bytes);
void zd_multi_destroy(zd_multi* m);

/* ------------------------------------------------------------------ */
/* Multi-GPU: frame-range sharding + RCCL gather.      */
/* Frames are independent (a fresh DecodingContext each, frame.rs:     */
/* 232-237) and the CLI concatenates their outputs, stopping at the    */
/* first failing frame (src/main.rs:43-53).  One process per GPU; each */
/* rank decodes a contiguous frame range into its own HBM (no data-    */
/* path collective), then the ranges are gathered to rank 0.           */
/* ------------------------------------------------------------------ */

/* Contiguous frame ranges balanced by compressed bytes: rank k takes
 * frames [cuts[k], cuts[k+1]) (cuts has world + 1 entries; every rank gets a
 * frame while there are at least `world`).  Host only. */
int zd_shard_partition(const uint64_t* frame_bytes, size_t nframes, int world, size_t* cuts);

/* Rank's share of src: byte range [*src_begin, *src_end) and frame range
 * (frames indexed on the host with zd_frames_index).  A frame that fails
 * to index and the rest of the input go to the last rank, whose plan then
 * reports it.  Host only. */
int zd_shard_range(const uint8_t* src, size_t n, int rank, int world, uint64_t* src_begin, uint64_t* src_end,
                   uint64_t* frame_begin, uint64_t* frame_end);

/* Every rank's share at once, from one walk of the input: rank k's bytes are
 * [src_cuts[k], src_cuts[k+1]) and its frames [frame_cuts[k],
 * frame_cuts[k+1]) (world + 1 entries each), exactly zd_shard_range's.  Made
 * once (on one rank, or ahead of time and kept beside the input) and handed
 * to the ranks, so that no rank walks frames outside its own range.  Host
 * only. */
int zd_shard_cuts(const uint8_t* src, size_t n, int world, uint64_t* src_cuts, uint64_t* frame_cuts);

/* zd_shard_range from given cuts, in time O(the rank's own range): walks only
 * the rank's frames and checks that they tile its byte range with its frame
 * count (the last rank's range may end in a frame that fails to index).
 * ZD_E_INVALID_ARG when they do not, i.e. the cuts are not this input's.
 * Host only. */
int zd_shard_range_at(const uint8_t* src, size_t n, const uint64_t* src_cuts, const uint64_t* frame_cuts, int rank,
                      int world, uint64_t* src_begin, uint64_t* src_end, uint64_t* frame_begin,
                      uint64_t* frame_end);

typedef struct zd_comm zd_comm;
#define ZD_COMM_ID_BYTES 128

/* An RCCL communicator over `world` ranks, one GPU each (the calling
 * thread's current HIP device).  Rank 0 makes the id and shares it out of
 * band (e.g. a torch.distributed broadcast); every rank then calls
 * zd_comm_create with it.  RCCL is loaded on first use. */
int zd_comm_unique_id(uint8_t id[ZD_COMM_ID_BYTES]);
int zd_comm_create(const uint8_t id[ZD_COMM_ID_BYTES], int world, int rank, zd_comm** out);
void zd_comm_destroy(zd_comm* comm);
/* The device buffers zd_decode_sharded keeps in the communicator between
 * calls (its input copy and its own output buffer), in bytes: memory
 * accounting.  A rank-0 decode that outgrows the caller's d_root_out moves to
 * an output buffer sized from what it needs, never from root_cap. */
int zd_comm_buffers(const zd_comm* comm, uint64_t* src_bytes, uint64_t* out_bytes);

typedef struct zd_gather_result {
  uint64_t total_len;         /* bytes gathered on rank 0 */
  int32_t status;             /* the whole input's status: the first failing rank's */
  int32_t failed_rank;        /* that rank, or world when none failed */
  int64_t first_error_frame;  /* global index of the first failing frame, -1 if none */
} zd_gather_result;

/* Host only: the outcome merge every rank of zd_comm_gather performs on the
 * all-gathered outcomes.  meta = world x 4 int64 {status, first failing frame
 * (global, -1 if none), local length, root capacity (rank 0's entry; 0
 * elsewhere)}.  The output stops at the first failing rank's failure: that
 * rank keeps its frames before the failure (its local length), later ranks
 * contribute nothing (src/main.rs:43-53).  Fills off[r] / len[r] (world
 * entries: where rank r's bytes land on rank 0, and how many) and *res;
 * returns ZD_E_DST_TOO_SMALL (res->total_len 0: nothing may be sent) when the
 * kept bytes exceed rank 0's capacity. */
int zd_gather_layout(const int64_t* meta, int world, uint64_t* off, uint64_t* len, zd_gather_result* res);

/* Collective (every rank calls it): each rank's outcome — status, first
 * failing frame (global index), decoded length — is all-gathered; the output
 * stops at the first failing rank's failure (its frames before the failure
 * kept, later ranks contribute nothing), and rank 0 receives the ranks'
 * d_local bytes in rank order at d_root_out (capacity root_cap; rank 0's own
 * bytes are copied unless d_local == d_root_out) with RCCL point-to-point
 * transfers on `stream`.  The same *res on every rank.  ZD_E_DST_TOO_SMALL
 * (on every rank, nothing sent) when rank 0's capacity is short. */
int zd_comm_gather(zd_comm* comm, const uint8_t* d_local, uint64_t local_len, int32_t status,
                   int64_t first_error_frame, uint8_t* d_root_out, uint64_t root_cap, zd_gather_result* res,
                   void* stream);

/* The whole multi-GPU decode (the reference's `decode every frame of a
 * file`, sharded): every rank passes the same host input; rank `comm`'s
 * frame range is planned, copied to HBM, decoded (with zd_plan_decompress's
 * re-plans past frames that overran their reserved capacity), and gathered
 * to rank 0 (zd_comm_gather).  Returns the local call's status (ZD_OK when
 * the collective completed); the input's status is res->status. */
int zd_decode_sharded(zd_comm* comm, const uint8_t* src, size_t n, uint32_t flags, uint8_t* d_root_out,
                      uint64_t root_cap, zd_gather_result* res, void* stream);

/* zd_decode_sharded with the ranks' cuts given (zd_shard_cuts): each rank
 * walks and plans only its own range.  A rank whose range does not fit the
 * cuts still joins the collective: res->status is then ZD_E_INVALID_ARG on
 * every rank. */
int zd_decode_sharded_at(zd_comm* comm, const uint8_t* src, size_t n, const uint64_t* src_cuts,
                         const uint64_t* frame_cuts, uint32_t flags, uint8_t* d_root_out, uint64_t root_cap,
                         zd_gather_result* res, void* stream);

/* ------------------------------------------------------------------ */
/* DecodingContext mirror (decoding_context.rs:17-106): GPU-resident    */
/* per-frame state across Block::decode calls.                         */
/* ------------------------------------------------------------------ */
typedef struct zd_context zd_context;

/* DecodingContext::new (decoding_context.rs:29-47): fails with
 * ZD_E_CTX_WINDOW_SIZE_TOO_BIG above 8 MiB. */
int zd_context_new(uint64_t window_size, zd_context** out);
void zd_context_free(zd_context* ctx);

/* Block::parse + Block::decode (block.rs:43-99) on the GPU: parses one
 * block (3-byte header + content) from src[0..n), decodes it on the
 * device appending to the context.  *consumed / *last as Block::parse. */
int zd_block_decode(zd_context* ctx, const uint8_t* src, size_t n,
                    size_t* consumed, int* last);

/* DecodingContext::execute_sequences (decoding_context.rs:78-106) on the
 * GPU: sequences are (literals_length, offset_value, match_length), any u32
 * values.  ZD_E_OUT_OF_DOMAIN when the context's output would pass
 * 2^31 - 64 KiB (the streaming executor's positions). */
int zd_execute_sequences(zd_context* ctx, const uint32_t* ll,
                         const uint32_t* offset_value, const uint32_t* ml,
                         size_t nseq, const uint8_t* literals, size_t nlits);

/* DecodingContext::decoded / ::offsets (decoding_context.rs:19-20). */
int zd_context_decoded(const zd_context* ctx, uint8_t* dst, size_t cap, size_t* len);
int zd_context_offsets(const zd_context* ctx, uint64_t offsets[3]);

#ifdef __cplusplus
}
#endif
#endif /* ZD_H */
