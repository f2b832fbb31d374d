// zd_host.cpp — host planner and C ABI (include/zd.h).
//
// The host does what the reference's parse phase does with headers only
// (FrameIterator / Frame::parse / Header::parse / Block::parse and the
// fixed-size parts of LiteralsSection::parse and Sequences::parse), resolves
// which block's Huffman/FSE tables every block uses (Treeless literals,
// Repeat_Mode) and carves the device workspace.  Everything that reads
// entropy-coded data — Huffman/FSE table descriptions, literal streams,
// sequence bitstreams, the LZ77 execute — runs in the HIP kernels.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <functional>
#include <memory>
#include <mutex>
#include <new>
#include <thread>
#include <vector>

#include "../../include/zd.h"
#include "zd_chain.h"
#include "zd_common.h"
#include "zd_internal.h"
#include "zd_launch.h"
#include "zd_plan.h"
#include "zd_seek.h"
#include "zd_walk.h"

using namespace zd;

namespace {

// Frames indexed by one thread of the host walk: a contiguous run of the
// input's frames and their blocks, stored flat.
struct HostPart {
  std::vector<HostFrame> frames;
  std::vector<HostBlock> blocks;
};

// The host walk's block sink: a part's block vector
struct VecSink {
  std::vector<HostBlock>& v;
  size_t size() const { return v.size(); }
  void push(const HostBlock& b) { v.push_back(b); }
};

#define HIPCHK(x) do { hipError_t _e = (x); if (_e != hipSuccess) { \
  fprintf(stderr, "zd: %s failed: %s\n", #x, hipGetErrorString(_e)); return ZD_E_HIP; } } while (0)

using TimePoint = std::chrono::steady_clock::time_point;
uint64_t ns(TimePoint a, TimePoint b) { return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(b - a).count(); }

// hipFree as a deleter
struct Free { void operator()(void* p) const { if (p) (void)hipFree(p); } };

}  // namespace

// ===========================================================================
// Dictionary (zd_dict_create): the content and the four tables on the device,
// shared by the zd_dict handle and every plan made with it.
// ===========================================================================
namespace {
constexpr uint32_t DICT_MAGIC = 0xEC30A437u;
constexpr size_t DICT_PAD = 16;          // readable bytes on both sides of the content (K4's 16-byte pieces)
struct DictData {
  int dev = -1;
  uint8_t* d_buf = nullptr;              // DICT_PAD zero bytes, the dictionary's bytes, zero bytes to the end
  const uint8_t* d_content = nullptr;    // inside d_buf
  uint64_t content = 0;
  uint32_t id = 0;
  bool raw = true;
  uint64_t rep[3] = {1, 4, 8};
  uint16_t* d_lut = nullptr;             // formatted: one LUT slot (the pair table) and one FSE slot
  uint16_t* d_fse = nullptr;
  uint8_t huf_bits = 0, al[3] = {0, 0, 0};
  // d_content in device memory, eight bytes at the end of d_buf: the one-entry table of content addresses that
  // K4J's scatter reads in a zd_plan_create_dict plan created with ZD_F_DICT_BLOCK_PARALLEL (a set plan has its
  // workspace's table)
  const uint8_t** d_self = nullptr;
  ~DictData() {
    if (d_buf) (void)hipFree(d_buf);
    if (d_lut) (void)hipFree(d_lut);
    if (d_fse) (void)hipFree(d_fse);
  }
};
}  // namespace
struct zd_dict {
  std::shared_ptr<DictData> p;
};
// Dictionary set (zd_dict_set_create): the dictionaries sorted by ID (a
// raw-content one, ID 0, only ever the fallback), shared by the zd_dict_set
// handle and every plan and batch made with it.
namespace {
struct DictSetData {
  int dev = -1;
  std::vector<std::shared_ptr<DictData>> d;   // sorted by ID
  int fallback = -1;                          // index into d, or -1
  int fallback_arg = -1;                      // as given to zd_dict_set_create
  // what a frame without a dictionary gets for one: DICT_PAD zero bytes on
  // both sides of d_none (its positions [0, 0) are never read, the window
  // preload reads up to 15 bytes below and 1 byte above it)
  uint8_t* d_none_buf = nullptr;
  ~DictSetData() {
    if (d_none_buf) (void)hipFree(d_none_buf);
  }
  const uint8_t* d_none() const { return d_none_buf + DICT_PAD; }
  // the set's dictionary of a frame: by its Dictionary_ID, else the fallback; -1: none
  int find(const zd_frame_desc& f) const {
    if (f.kind != ZD_FRAME_ZSTD) return -1;
    if (f.dict_id == UINT64_MAX || f.dict_id == 0) return fallback;
    size_t lo = 0, hi = d.size();
    while (lo < hi) {
      const size_t m = lo + (hi - lo) / 2;
      if (d[m]->id < f.dict_id) lo = m + 1; else hi = m;
    }
    return (lo < d.size() && d[lo]->id == f.dict_id) ? (int)lo : -1;
  }
};
}  // namespace
struct zd_dict_set {
  std::shared_ptr<DictSetData> p;
};

// ===========================================================================
// Plan
// ===========================================================================
struct zd_plan {
  uint32_t flags = 0;
  std::shared_ptr<DictData> dict;       // a dictionary plan (zd_plan_create_dict): kept alive by the plan
  // a dictionary-set plan (zd_plan_create_dicts; never with `dict`): the set,
  // and the dictionaries this plan's frames use -- PlanCtx::dset, sorted by ID,
  // entry k's tables the prebuilt comp PlanDict::comp (the formatted ones
  // are comps 0..n_dict_comps-1) and its content address dict_ptrs[k]; the
  // last of dict_ptrs is the address of frames without a dictionary
  std::shared_ptr<DictSetData> dset;
  std::vector<PlanDict> dset_tab;
  std::vector<const DictData*> dset_used;
  int32_t dset_fallback = -1;
  uint32_t n_dict_comps = 0;            // prebuilt comps at the head of the plan (a dictionary plan: 0 or 1)
  std::vector<uint32_t> frame_dict;     // Sink::frame_dict of a plan that is not staged
  std::vector<uint64_t> frame_csum;     // Sink::frame_csum of a ZD_F_VERIFY_CHECKSUM plan that is not staged
  bool verify() const { return (flags & ZD_F_VERIFY_CHECKSUM) != 0; }
  // a prefix batch (zd_batch_create_prefix; never with `dict` or `dset`): frame
  // f's own raw-content prefix, prefix_bytes[f] bytes at the caller's address
  // prefix_ptrs[f] (host vectors; a batch made from device arrays leaves them
  // empty and has d_prefix_ptrs / d_prefix_bytes, the batch's own copies)
  bool prefix = false;
  std::vector<uint64_t> prefix_ptrs, prefix_bytes;
  const uint64_t *d_prefix_ptrs = nullptr, *d_prefix_bytes = nullptr;
  // a chain batch (zd_batch_create_chain; a prefix batch in everything above):
  // the frames grouped by level and each frame's parent, device arrays the
  // batch owns, and the levels' frame counts (K4_CHAIN: one launch a level)
  bool chain = false;
  const uint32_t* d_chain_order = nullptr;
  const int32_t* d_chain_parent = nullptr;
  std::vector<uint32_t> chain_count;
  // a chain batch created with ZD_F_CHAIN_BLOCK_PARALLEL, or routed frame by
  // frame under ZD_F_AUTO_EXECUTOR (zd_route.h chain_j_layout; there any level,
  // or every level, may be without a J frame):
  // its J frames are numbered level-major (zd_plan.h plan_j_order), chain_j[l]
  // level l's ranges of K4J's grids.  What the planners need for that: the
  // frames by level on the host (host arrays), or the batch's level counters on
  // the device (device arrays; d_chain_order is order[] there)
  std::vector<JLevel> chain_j;
  std::vector<uint32_t> h_chain_order;
  const uint32_t* d_chain_lcount = nullptr;
  bool chain_on_j() const { return zd::chain_j_layout(flags, chain); }
  // the width ZD_F_AUTO_EXECUTOR's rule reads (the chunks that execute together)
  // and the block minimum of the plan's rule (zd_plan.h plan_k4j_min)
  uint64_t auto_width() const {
    uint64_t w = nframes;
    if (chain) { w = 0; for (uint32_t c : chain_count) w = std::max<uint64_t>(w, c); }
    return w;
  }
  // a dictionary or dictionary-set plan created with ZD_F_DICT_BLOCK_PARALLEL (zd_route.h dict_j)
  bool dict_j() const { return zd::dict_j(flags, (dict != nullptr || dset != nullptr) && !prefix); }
  uint32_t k4j_min() const { return plan_k4j_min(flags, prefix, chain, nframes, auto_width(), dict_j()); }
  uint32_t jpend_words() const {
    return chain_on_j() ? jpend_chain_words((uint32_t)chain_count.size()) : JPEND_WORDS;
  }
  bool with_dict() const { return dict != nullptr || dset != nullptr || prefix; }
  // the walk's options (zd_walk.h): parse_compressed's rfc_empty_lits, ZD_F_LONG_WINDOW, ZD_F_RFC
  uint32_t walk_opts() const {
    return zd::walk_opts(with_dict(), (flags & ZD_F_LONG_WINDOW) != 0, (flags & ZD_F_RFC) != 0);
  }
  std::vector<HostPart> parts;          // the host walk's frames, in input order
  std::vector<size_t> part_f0;          // plan frame index of each part's first frame
  size_t nframes = 0;
  std::vector<CompBlock> comps;
  std::vector<BlockRec> blocks;
  std::vector<FrameDesc> fdesc;
  std::vector<FrameState> fstate0;
  std::vector<uint32_t> list_tables, list_huf, list_seq, list_k4f;
  std::vector<CopyDesc> copies;         // K0 pieces
  std::vector<JFrame> jframes;          // K4J frames, their blocks and the scatter's segments
  std::vector<JBlkDesc> jblkd;
  std::vector<JSegDesc> jsegd;
  uint64_t j_bytes = 0, j_pieces = 0;
  uint32_t j_rounds = 0;
  // counts of the descriptor arrays (large plans keep their descriptors only
  // in the pinned staging until the upload: the vectors above stay empty)
  uint64_t n_comps = 0, n_blocks = 0, n_frames = 0, n_tables = 0, n_huf = 0, n_seq = 0, n_k4f = 0, n_copies = 0;
  uint64_t n_jframes = 0, n_jblk = 0, n_jseg = 0, n_k0only = 0;
  uint64_t n_csums = 0;                         // zstd frames with a Content_Checksum (zd_k_verify's work)
  bool fused = false;                           // zd_k_fused plan (build_plan fuse_plan)
  bool last_fused = false;                      // the last zd_decode_async launched zd_k_fused
  std::vector<uint64_t> frame_out, frame_cap;   // output offset and capacity per frame
  std::vector<uint64_t> place_out, place_cap;   // a batch's per-frame placement (PlanCtx::place_out), else empty
  bool staged = false;
  std::unique_lock<std::mutex> stage_lock;      // the pinned staging, from build_plan to upload_plan
  zd_plan_info info{};
  Workspace W{};
  uint8_t* d_ws = nullptr;
  uint64_t ws_bytes = 0;                 // size of the d_ws allocation (>= W.total: a cached block)
  int dev = -1;                          // the device d_ws and the aux stream belong to (upload_plan)
  uint32_t cus = 256;                    // the CU count the plan was made for and is routed by (build_plan)
  uint64_t desc_bytes = 0;               // the host-filled head of the workspace (one upload)
  uint8_t* d_staging = nullptr;          // the output of a non-exact layout, or the copy an exact one is compacted from
  uint64_t staging_bytes = 0;
  int index_status = 0;
  uint64_t cap0 = 0;                     // capacity of frame 0 instead of its own (a re-plan, zd_plan_decompress)
  // the first failing frame of the last zd_plan_results when its failure is
  // a limit of the GPU path the host can lift (LS_CAPACITY, LS_JROUNDS)
  int64_t limit_frame = -1;
  uint32_t limit_stage = 0;
  size_t index_stop = 0;                 // frame index that failed to index (== nframes - 1) or nframes
  // a plan whose descriptors the GPU built (zd_plan_create_device): its
  // frame index stays in the workspace (W.hframes) until a caller needs it
  bool dev_built = false;
  zd::FrameOuts io_fo;                   // per-frame outcome of the last zd_plan_decompress
  mutable std::vector<HostFrame> dev_frames;
  // the frame index on the host (a device-built plan's comes back once);
  // false when it cannot be read -- nothing is kept then, a later call retries
  bool frames_ready() const {
    if (!dev_built || dev_frames.size() == nframes) return true;
    std::vector<HostFrame> v(nframes);
    if (nframes && hipMemcpy(v.data(), d_ws + W.hframes, nframes * sizeof(HostFrame), hipMemcpyDeviceToHost) !=
                       hipSuccess) {
      (void)hipGetLastError();
      return false;
    }
    dev_frames = std::move(v);
    return true;
  }
  // (callers check frames_ready() first)
  const HostFrame& frame(size_t f) const {
    if (dev_built) return dev_frames[f];
    const size_t k = (size_t)(std::upper_bound(part_f0.begin(), part_f0.end(), f) - part_f0.begin()) - 1;
    return parts[k].frames[f - part_f0[k]];
  }
  void set_parts(std::vector<HostPart>&& p) {
    parts = std::move(p);
    part_f0.clear();
    nframes = 0;
    for (const HostPart& hp : parts) { part_f0.push_back(nframes); nframes += hp.frames.size(); }
  }
  bool profile = false;                  // mode 1: every kernel timed, one after another
  bool profile_dom = false;              // mode 2: the launch groups that carry work, timed in the pipeline as it runs
  uint32_t dom_used = 0;                 // the groups (kDomNames) the last mode-2 launch recorded
  hipEvent_t dom_ev[2 * N_DOM] = {};
  hipEvent_t ev[N_KERNELS + 1] = {};
  hipEvent_t ev_verify = nullptr;        // mode 1, a verified plan: after zd_k_verify (ev[N_KERNELS] is before it)
  bool ev_made = false;
  bool launched = false;
  hipStream_t last_stream = nullptr;     // the stream of the last zd_decode_async
  // context API hook: comp 0 is a prebuilt "previous block" carrying tables
  bool has_prebuilt = false;
  // second stream for K2 beside K3 (created on first launch)
  hipStream_t aux = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
  // output layout of the last zd_plan_results (frames before the first failure)
  std::vector<uint64_t> res_off, res_len;
  uint64_t* d_meta = nullptr;            // zd_plan_results' compaction / zd_plan_checksums' arrays
  uint64_t meta_cap = 0;                 // (u64 entries)
  // zd_plan_decompress (host in, host out): device buffers kept between calls
  uint8_t* io_src = nullptr;
  uint64_t io_src_cap = 0;
  uint8_t* io_dst = nullptr;
  uint64_t io_dst_cap = 0;
};

namespace {

uint64_t align_up(uint64_t x, uint64_t a) { return (x + a - 1) / a * a; }

// The routing overrides (zd_route.h RouteEnv; experiments only), read once per process
const RouteEnv& route_env() {
  static const RouteEnv e = RouteEnv::from_process();
  return e;
}
constexpr size_t PAR_INDEX_MIN_BYTES = 4u << 20;    // the host walk in parallel from 4 MiB of input (>= 512 frames)
constexpr size_t FRAMES_INDEX_SERIAL_MAX = 4096;     // zd_frames_index asked for at most this many frames: walk only them

// A process-wide pool of host worker threads (created on first use, kept:
// spawning 15 threads per planner pass cost ~0.3 ms each time).
class WorkerPool {
 public:
  static WorkerPool& get() {
    static WorkerPool* p = new WorkerPool();   // never destroyed: workers idle on the cv at exit
    return *p;
  }
  // f(k) for k in [0, n): k = 0 on the calling thread, the rest on the
  // workers (n - 1 <= size()); returns when all ran.  Not reentrant from f.
  void run(size_t n, const std::function<void(size_t)>& f) {
    std::unique_lock<std::mutex> lk(m_);
    while (busy_) idle_.wait(lk);              // one job at a time
    busy_ = true;
    job_ = &f;
    next_ = 1;
    end_ = n;
    left_ = n - 1;
    gen_++;
    go_.notify_all();
    lk.unlock();
    f(0);
    lk.lock();
    done_.wait(lk, [&] { return left_ == 0; });
    job_ = nullptr;
    busy_ = false;
    idle_.notify_one();
  }
  size_t size() const { return th_.size(); }

 private:
  WorkerPool() {
    const unsigned n = std::max(1u, std::min(16u, std::thread::hardware_concurrency())) - 1;
    for (unsigned i = 0; i < n; i++) th_.emplace_back([this] { loop(); });
    for (auto& t : th_) t.detach();
  }
  void loop() {
    uint64_t seen = 0;
    std::unique_lock<std::mutex> lk(m_);
    for (;;) {
      go_.wait(lk, [&] { return gen_ != seen && job_ && next_ < end_; });
      seen = gen_;
      while (job_ && next_ < end_) {
        const size_t k = next_++;
        const std::function<void(size_t)>* f = job_;
        lk.unlock();
        (*f)(k);
        lk.lock();
        if (--left_ == 0) done_.notify_all();
      }
    }
  }
  std::mutex m_;
  std::condition_variable go_, done_, idle_;
  std::vector<std::thread> th_;
  const std::function<void(size_t)>* job_ = nullptr;
  size_t next_ = 0, end_ = 0, left_ = 0;
  uint64_t gen_ = 0;
  bool busy_ = false;
};

// Runs f(k) for k in [0, n) in parallel (the calling thread takes k = 0;
// n - 1 must not exceed the pool's workers, else the rest run inline).
template <typename F>
void run_parts(size_t n, F f) {
  if (n <= 1) { if (n) f(0); return; }
  WorkerPool& pool = WorkerPool::get();
  const size_t par = std::min(n, pool.size() + 1);
  const std::function<void(size_t)> g = [&](size_t k) { for (size_t j = k; j < n; j += par) f(j); };
  pool.run(par, g);
}

// Pinned host staging for the descriptor upload, kept between plans: large
// plans write their descriptors straight into it at the workspace offsets
// (pinned pages never fault) and upload them with one DMA.
struct HostStage {
  std::mutex m;
  uint8_t* p = nullptr;
  size_t cap = 0;
  bool pinned = false;     // hipHostMalloc (else malloc: no device to pin for)
  void release() {
    if (p) { if (pinned) (void)hipHostFree(p); else free(p); }
    p = nullptr;
    cap = 0;
  }
};
HostStage& host_stage() {
  static HostStage h;
  return h;
}
constexpr uint64_t STAGE_MIN_BYTES = 1u << 20;     // smaller plans fill host vectors

// The current device's CU count, which a plan keeps and is routed by (zd_plan::cus)
uint32_t device_cus() {
  int dev = 0, cus = 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) {
    (void)hipGetLastError();
    return 256;
  }
  return (uint32_t)cus;
}

// Every frame of the host walk a zstd frame of one compressed block, with no
// walk-found error (the fused kernel's plans)
bool host_single_block_frames(const zd_plan* P) {
  for (const HostPart& hp : P->parts)
    for (const HostFrame& hf : hp.frames)
      if (hf.d.kind != ZD_FRAME_ZSTD || hf.key != KEY_NONE || hf.nb != 1) return false;
  return true;
}

// The per-frame pass's plan-wide inputs (routing included): `single` =
// every frame a single-block zstd frame, `j_candidates` = frames K4J would
// take in automatic mode (frames without a walk-found error and with at
// least k4j_min compressed blocks; counted only when the mode is automatic,
// or for ZD_F_AUTO_EXECUTOR's rule).
PlanCtx plan_ctx(const zd_plan* P, int32_t prev_huf, const int32_t prev_tab[3], uint64_t out_len0,
                 const uint64_t rep0[3], uint64_t fixed_cap, bool single, uint64_t j_candidates) {
  PlanCtx X{};
  X.prev_huf = prev_huf;
  for (int k = 0; k < 3; k++) { X.prev_tab[k] = prev_tab[k]; X.rep0[k] = rep0[k]; }
  X.out_len0 = out_len0;
  X.fixed_cap = fixed_cap;
  X.cap0 = P->cap0;
  X.cap0_frame = nullptr;
  for (const HostPart& hp : P->parts)
    if (!hp.frames.empty()) { X.cap0_frame = hp.frames.data(); break; }
  X.flags = P->flags;
  X.dict = P->with_dict();
  X.dict_id = P->dict ? P->dict->id : 0;
  if (P->dset) {
    // (never null in a set plan, whose workspace carries the per-frame table
    // and whose K4 reads it: a plan none of whose frames uses a dictionary has
    // an empty table, and an empty vector's data() may be null)
    static const PlanDict no_entry{};
    X.dset = P->dset_tab.empty() ? &no_entry : P->dset_tab.data();
    X.ndset = (uint32_t)P->dset_tab.size();
    X.dset_fallback = P->dset_fallback;
  }
  X.place_out = P->place_out.empty() ? nullptr : P->place_out.data();
  X.place_cap = P->place_out.empty() ? nullptr : P->place_cap.data();
  if (P->prefix) X.prefix_bytes = P->d_prefix_bytes ? P->d_prefix_bytes : P->prefix_bytes.data();
  RouteIn in{};
  in.cus = P->cus;
  in.nframes = P->nframes;
  // (a dictionary plan routes like a context plan: the streaming executor only)
  in.context = out_len0 != 0 || P->has_prebuilt || X.dict;
  in.flags = P->flags;
  in.single_block_frames = single;
  const PlanRoute r = plan_route(in, X.dict, route_env());
  X.fused = r.fused;
  X.k4f_on = r.k4f;
  plan_k4j_fields(X, P->flags, route_env(), X.dict, P->prefix, P->chain, out_len0, P->nframes, P->auto_width(),
                  j_candidates, P->dict_j());
  return X;
}

// The descriptor arrays at the head of the workspace (a host-filled plan
// uploads them at once)
void carve_head(Workspace& W, const PlanCounts& T, uint64_t& o) {
  auto carve = [&](uint64_t bytes) { uint64_t r = o; o = align_up(o + bytes, 256); return r; };
  W.comp = carve(sizeof(CompBlock) * std::max<uint64_t>(T.comps, 1));
  W.blocks = carve(sizeof(BlockRec) * std::max<uint64_t>(T.blocks, 1));
  W.frames = carve(sizeof(FrameDesc) * std::max<uint64_t>(T.frames, 1));
  W.frame_state0 = carve(sizeof(FrameState) * std::max<uint64_t>(T.frames, 1));
  W.list_tables = carve(4 * std::max<uint64_t>(T.tables, 1));
  W.list_huf = carve(4 * std::max<uint64_t>(T.huf, 1));
  W.list_seq = carve(4 * std::max<uint64_t>(T.seq, 1));
  W.list_k4f = carve(4 * std::max<uint64_t>(T.k4f, 1));
  W.copies = carve(sizeof(CopyDesc) * std::max<uint64_t>(T.copies, 1));
  W.jframes = carve(sizeof(JFrame) * std::max<uint64_t>(T.jframes, 1));
  W.jblkd = carve(sizeof(JBlkDesc) * std::max<uint64_t>(T.jblk, 1));
  W.jsegd = carve(sizeof(JSegDesc) * std::max<uint64_t>(T.jseg, 1));
}
// The device-only arrays after them (K4J's sizes from its descriptors)
void carve_tail(zd_plan* P, Workspace& W, const PlanCounts& T, uint64_t& o, uint64_t j_base, uint64_t j_pieces,
                uint64_t j_maxseq) {
  auto carve = [&](uint64_t bytes) { uint64_t r = o; o = align_up(o + bytes, 256); return r; };
  W.comp_state = carve(sizeof(CompState) * std::max<uint64_t>(T.comps, 1));
  W.huge = carve(4 * (std::max<uint64_t>(T.tables, 1) + 1));
  W.deep = carve(16 + (T.luts ? DEEP_POOL_BYTES : 0));
  W.frame_state = carve(sizeof(FrameState) * std::max<uint64_t>(T.frames, 1));
  W.lits = carve(T.lits + 64);
  W.seqs = carve(8 * T.nrec + 64);
  W.luts = carve((uint64_t)LUT_ENTRIES * 2 * std::max<uint64_t>(T.luts, 1));
  W.fses = carve((uint64_t)FSE_SLOT * 2 * std::max<uint64_t>(T.fses, 1));
  // K4J: pointer jumping resolves every match byte within ceil(log2(matches
  // + 1)) rounds (each pointer chain ends at a literal after at most one hop
  // per earlier match; each round halves the hops left)
  P->j_bytes = T.jframes ? j_base + 16 : 0;
  P->j_pieces = j_pieces;
  P->j_rounds = 0;
  if (T.jframes) {
    uint32_t r = 1;
    while (r < (uint32_t)J_MAX_ROUNDS - 1 && (1ull << r) <= j_maxseq + 1) r++;
    // a hop whose composed distance would reach 2^31 (J_FINAL) keeps its
    // word until its source is final, so a chain spanning k windows of
    // 2 GiB resolves within k times the rounds of one (by induction on k:
    // the bytes of the windows below are final by then, and the rest of
    // the chain is one window of hops ending at them); j_base (the plan's
    // K4J words) bounds the largest frame.  Rounds past the first are
    // sweeps that stop when nothing is pending: the bound costs nothing
    // on frames that converge sooner.
    const uint64_t k = std::max<uint64_t>(1, (j_base + (1ull << 31) - 1) >> 31);
    P->j_rounds = (uint32_t)((r + 1) * k);
  }
  W.jblk = carve(sizeof(JBlk) * std::max<uint64_t>(T.jblk, 1));
  W.jseg = carve(sizeof(JSeg) * std::max<uint64_t>(T.jseg, 1));
  W.jpend = carve(4 * (uint64_t)P->jpend_words());
  W.jdone = carve(std::max<uint64_t>(j_pieces, 1));
  W.jst = carve(4 * P->j_bytes + 64);
  W.redo = carve(std::max<uint64_t>(T.frames, 1));
  W.k2done = carve(4);
}
// A ZD_F_VERIFY_CHECKSUM plan's arrays: the stored checksums among the
// descriptors the planner fills (after carve_head), zd_k_verify's results
// among the device-only arrays (after carve_tail).  Other plans carve nothing.
void carve_verify_head(const zd_plan* P, Workspace& W, const PlanCounts& T, uint64_t& o) {
  if (!P->verify()) return;
  W.csum = o; o = align_up(o + 8 * std::max<uint64_t>(T.frames, 1), 256);
}
void carve_verify_tail(const zd_plan* P, Workspace& W, const PlanCounts& T, uint64_t& o) {
  if (!P->verify()) return;
  W.vhash = o; o = align_up(o + 8 * std::max<uint64_t>(T.frames, 1), 256);
  W.vok = o; o = align_up(o + std::max<uint64_t>(T.frames, 1), 256);
}
// zd_k_verify's results before any launch wrote them (and for a plan whose
// frames carry no checksum, where it never runs): no digest, nothing checked
int init_verify(zd_plan* P) {
  if (!P->verify()) return 0;
  const uint64_t n = std::max<uint64_t>(P->n_frames, 1);
  HIPCHK(hipMemset(P->d_ws + P->W.vhash, 0, 8 * n));
  HIPCHK(hipMemset(P->d_ws + P->W.vok, 0xFF, n));
  return 0;
}
// The plan's array counts from the totals
void plan_totals(zd_plan* P, const PlanCounts& T, bool fused) {
  P->n_comps = T.comps; P->n_blocks = T.blocks; P->n_frames = T.frames;
  P->n_tables = T.tables; P->n_huf = T.huf; P->n_seq = T.seq; P->n_k4f = T.k4f; P->n_copies = T.copies;
  P->n_jframes = T.jframes; P->n_jblk = T.jblk; P->n_jseg = T.jseg; P->n_k0only = T.k0only;
  P->n_csums = T.csums;
  P->fused = plan_fused(fused, T.jframes, T.k4f);
}
void plan_info(zd_plan* P, const PlanCounts& T) {
  zd_plan_info& I = P->info;
  I.nframes = T.frames;
  I.nblocks = T.blocks;
  I.ncompressed = T.comps - P->n_dict_comps;   // (not the dictionaries' prebuilt comps)
  I.out_bytes = T.out;
  I.out_exact = T.exact();
  I.workspace_bytes = P->W.total;
  I.nsequences = T.nseq;
  I.nliterals = T.lits;
  I.index_status = P->index_status;
  I.executors = (P->fused ? ZD_EXEC_FUSED : 0u) | (P->n_k4f ? ZD_EXEC_K4F : 0u) | (P->n_jframes ? ZD_EXEC_K4J : 0u);
}

// The largest K4J frame's sequence count (plan_frame's jm)
struct JMax {
  uint64_t m = 0;
  void note(uint64_t n) { m = std::max(m, n); }
};

// The prebuilt comps at the head of a dictionary plan and, for a dictionary
// set, the plan's table: the set's entries that some frame of the plan uses
// (used[k] per entry of the set, in its order).
void plan_dict_comps(zd_plan* P, const uint8_t* used) {
  P->n_dict_comps = (P->dict && !P->dict->raw) ? 1u : 0u;
  if (!P->dset) return;
  const DictSetData& D = *P->dset;
  P->dset_tab.clear();
  P->dset_used.clear();
  P->dset_fallback = -1;
  for (size_t k = 0; k < D.d.size(); k++) {
    if (!used[k]) continue;
    const DictData& dd = *D.d[k];
    PlanDict e{};
    e.dict_id = dd.id;
    e.comp = dd.raw ? -1 : (int32_t)P->n_dict_comps++;
    e.content = dd.content;
    for (int q = 0; q < 3; q++) e.rep[q] = dd.rep[q];
    if ((int)k == D.fallback) P->dset_fallback = (int32_t)P->dset_tab.size();
    P->dset_tab.push_back(e);
    P->dset_used.push_back(&dd);
  }
}
// Prebuilt comp k: the tables of the k-th formatted dictionary a plan uses (LUT slot k, FSE slot k)
CompBlock prebuilt_comp(uint32_t k) {
  CompBlock pb{};
  pb.lit_type = LIT_COMPRESSED;
  pb.host_stage = PS_ALL;
  pb.nseq = 1;
  pb.modes[0] = pb.modes[1] = pb.modes[2] = M_FSE;
  pb.prebuilt = 1;
  pb.huf_src = (int32_t)k;
  pb.tab_src[0] = pb.tab_src[1] = pb.tab_src[2] = (int32_t)k;
  pb.lut_slot = k;
  pb.fse_slot = k;
  return pb;
}

// Builds device-side descriptors from the host frames: one counting pass and
// one filling pass over the parts in parallel (each part's entries start at
// the counts of the parts before it), then the K4J descriptors in frame order.
// `staged`: a large plan may fill the pinned staging (zd_plan_create); the
// context API keeps host vectors it edits afterwards.
int build_plan(zd_plan* P, int32_t prev_huf, const int32_t prev_tab[3], uint64_t out_len0,
               const uint64_t rep0[3], uint64_t fixed_cap, bool staged = false) {
  P->cus = device_cus();
  uint64_t j_candidates = 0;
  if (plan_k4j_counts(P->flags, route_env(), P->prefix, P->chain, out_len0, P->dict_j())) {
    const uint32_t k4j_min = P->k4j_min();
    for (const HostPart& hp : P->parts)
      for (const HostFrame& hf : hp.frames) j_candidates += hf.key == KEY_NONE && hf.ncomp >= k4j_min;
  }
  // a formatted dictionary's tables: the plan-level prebuilt comp 0 with LUT
  // slot 0 and FSE slot 0, before every frame's (X.prev_huf / X.prev_tab name
  // it); a dictionary set: one such comp per formatted dictionary that a frame
  // of this plan uses, comps 0..U-1 with LUT and FSE slots 0..U-1
  {
    std::vector<uint8_t> used(P->dset ? P->dset->d.size() : 0, 0);
    if (P->dset)
      for (const HostPart& hp : P->parts)
        for (const HostFrame& hf : hp.frames) {
          const int k = P->dset->find(hf.d);
          if (k >= 0) used[(size_t)k] = 1;
        }
    plan_dict_comps(P, used.data());
  }
  PlanCtx X = plan_ctx(P, prev_huf, prev_tab, out_len0, rep0, fixed_cap, host_single_block_frames(P), j_candidates);

  const size_t np = P->parts.size();
  std::vector<PlanCounts> cnt(np + 1);
  const uint32_t dict_comps = P->n_dict_comps;
  cnt[0].comps = cnt[0].luts = cnt[0].fses = dict_comps;
  const Sink none{};
  // a chain batch on K4J: each frame's own K4J counts, for the level-major numbering below
  const bool jlevels = P->chain_on_j() && X.place_out && P->h_chain_order.size() == P->nframes;
  if (P->chain_on_j() && !jlevels && P->nframes) return ZD_E_INVALID_ARG;
  std::vector<uint64_t> jcnt(jlevels ? PLAN_J_COLS * P->nframes : 0), j_at(jcnt.size());
  run_parts(np, [&](size_t k) {
    const HostPart& hp = P->parts[k];
    PlanCounts c;
    // (a batch's placement is by plan frame index: the part counts from its
    // first frame's, taken off again below)
    if (X.place_out) c.frames = P->part_f0[k];
    for (const HostFrame& hf : hp.frames) {
      uint64_t j0[PLAN_J_COLS], j1[PLAN_J_COLS];
      const uint64_t fi = c.frames;
      plan_j_get(c, j0);
      plan_frame<false, JMax>(X, hf, hp.blocks.data(), c, none, nullptr);
      plan_j_get(c, j1);
      if (jlevels) for (int w = 0; w < PLAN_J_COLS; w++) jcnt[PLAN_J_COLS * fi + w] = j1[w] - j0[w];
    }
    if (X.place_out) c.frames -= P->part_f0[k];
    if (X.fused) {          // parts start aligned, so the filling pass pads exactly as this count did
      c.lits = align_up(c.lits, 128);
      c.nrec = align_up(c.nrec, 16);
    }
    cnt[k + 1] = c;
  });
  for (size_t k = 1; k <= np; k++) { PlanCounts t = cnt[k - 1]; t.add(cnt[k]); cnt[k] = t; }
  const PlanCounts T = cnt[np];
  P->chain_j.clear();
  if (jlevels) {
    // the J frames level-major: every level owns one contiguous range of J
    // frames, J blocks, segments, state words and pieces (the fill pass places
    // each frame's K4J entries at j_at instead of the running counts)
    uint64_t tot[PLAN_J_COLS];
    P->chain_j.resize(P->chain_count.size());
    plan_j_order(jcnt.data(), P->h_chain_order.data(), P->chain_count.data(), (uint32_t)P->chain_count.size(),
                 j_at.data(), P->chain_j.data(), tot);
    X.j_at = j_at.data();
  }

  // workspace carve-up: the arrays the host fills first (one upload), then
  // the device-only ones
  Workspace& W = P->W;
  W = Workspace{};
  uint64_t o = 0;
  carve_head(W, T, o);
  if (X.dset) {
    W.frame_dict = o; o = align_up(o + 4 * std::max<uint64_t>(T.frames, 1), 256);
    W.dict_ptrs = o; o = align_up(o + 8 * (uint64_t)(X.ndset + 1), 256);
  }
  if (P->prefix) { W.dict_ptrs = o; o = align_up(o + 8 * std::max<uint64_t>(T.frames, 1), 256); }
  carve_verify_head(P, W, T, o);
  P->desc_bytes = o;
  plan_totals(P, T, X.fused);
  P->frame_out.resize(T.frames);
  P->frame_cap.resize(T.frames);
  Sink S{};
  P->staged = staged && P->desc_bytes >= STAGE_MIN_BYTES;
  if (P->staged) {
    // held until upload_plan has copied the staging out
    P->stage_lock = std::unique_lock<std::mutex>(host_stage().m);
    HostStage& H = host_stage();
    if (H.cap < P->desc_bytes) {
      H.release();
      const size_t want = P->desc_bytes + (P->desc_bytes >> 2);
      H.pinned = hipHostMalloc((void**)&H.p, want, hipHostMallocDefault) == hipSuccess;
      if (!H.pinned) {
        (void)hipGetLastError();
        H.p = (uint8_t*)aligned_alloc(4096, align_up(want, 4096));
      }
      if (!H.p) return ZD_E_NO_MEMORY;
      H.cap = want;
    }
    uint8_t* b = H.p;
    S = Sink{(CompBlock*)(b + W.comp), (BlockRec*)(b + W.blocks), (FrameDesc*)(b + W.frames),
             (FrameState*)(b + W.frame_state0), (uint32_t*)(b + W.list_tables), (uint32_t*)(b + W.list_huf),
             (uint32_t*)(b + W.list_seq), (uint32_t*)(b + W.list_k4f), (CopyDesc*)(b + W.copies),
             (JFrame*)(b + W.jframes), (JBlkDesc*)(b + W.jblkd), (JSegDesc*)(b + W.jsegd), nullptr, nullptr,
             X.dset ? (uint32_t*)(b + W.frame_dict) : nullptr};
    if (X.dset) {
      const uint8_t** dp = (const uint8_t**)(b + W.dict_ptrs);
      for (uint32_t k = 0; k < X.ndset; k++) dp[k] = P->dset_used[k]->d_content;
      dp[X.ndset] = P->dset->d_none();
    }
    if (P->prefix && !P->prefix_ptrs.empty())
      memcpy(b + W.dict_ptrs, P->prefix_ptrs.data(), 8 * P->prefix_ptrs.size());
    if (P->verify()) S.frame_csum = (uint64_t*)(b + W.csum);
    P->frame_dict.clear();
    P->frame_csum.clear();
    P->comps.clear(); P->blocks.clear(); P->fdesc.clear(); P->fstate0.clear();
    P->list_tables.clear(); P->list_huf.clear(); P->list_seq.clear(); P->list_k4f.clear(); P->copies.clear();
    P->jframes.clear(); P->jblkd.clear(); P->jsegd.clear();
  } else {
    P->comps.assign(T.comps, CompBlock{});
    P->blocks.assign(T.blocks, BlockRec{});
    P->fdesc.assign(T.frames, FrameDesc{});
    P->fstate0.assign(T.frames, FrameState{});
    P->list_tables.assign(T.tables, 0);
    P->list_huf.assign(T.huf, 0);
    P->list_seq.assign(T.seq, 0);
    P->list_k4f.assign(T.k4f, 0);
    P->copies.assign(T.copies, CopyDesc{});
    P->jframes.assign(T.jframes, JFrame{});
    P->jblkd.assign(T.jblk, JBlkDesc{});
    P->jsegd.assign(T.jseg, JSegDesc{});
    S = Sink{P->comps.data(), P->blocks.data(), P->fdesc.data(), P->fstate0.data(), P->list_tables.data(),
             P->list_huf.data(), P->list_seq.data(), P->list_k4f.data(), P->copies.data(), P->jframes.data(),
             P->jblkd.data(), P->jsegd.data(), nullptr, nullptr, nullptr};
    P->frame_dict.assign(X.dset ? T.frames : 0, 0);
    if (X.dset) S.frame_dict = P->frame_dict.data();
    P->frame_csum.assign(P->verify() ? T.frames : 0, 0);
    if (P->verify()) S.frame_csum = P->frame_csum.data();
  }
  S.frame_out = P->frame_out.data();
  S.frame_cap = P->frame_cap.data();
  // (the K4J descriptors are written by plan_frame at the running K4J indices)
  std::vector<JMax> jm(np);
  run_parts(np, [&](size_t k) {
    const HostPart& hp = P->parts[k];
    PlanCounts c = cnt[k];
    for (const HostFrame& hf : hp.frames) plan_frame<true, JMax>(X, hf, hp.blocks.data(), c, S, &jm[k]);
  });
  for (uint32_t k = 0; k < dict_comps; k++) S.comps[k] = prebuilt_comp(k);
  uint64_t j_maxseq = 0;
  for (const JMax& m : jm) j_maxseq = std::max(j_maxseq, m.m);
  carve_tail(P, W, T, o, T.jwords, T.jpieces, j_maxseq);
  carve_verify_tail(P, W, T, o);
  W.total = o;

  plan_info(P, T);
  return 0;
}

// build_plan for a plan or a batch, staged.  With one dictionary (P->dict) its
// tables are the prebuilt comp 0 (a raw-content dictionary has none), its
// repeat offsets every frame's first, and its content the positions before
// every frame; a dictionary set gives every frame's from the plan's table
// (PlanCtx::dset).
int build_plan_staged(zd_plan* P) {
  const int32_t none[3] = {-1, -1, -1}, pre[3] = {0, 0, 0};
  const uint64_t rep0[3] = {1, 4, 8};
  const DictData* D = P->dict.get();
  return D ? build_plan(P, D->raw ? -1 : 0, D->raw ? none : pre, D->content, D->rep, 0, true)
           : build_plan(P, -1, none, 0, rep0, 0, true);
}

// Device workspaces of destroyed plans, kept for the next plans of this
// process (a plan's workspace is up to ~1.2x its decoded bytes: K3's
// records, the literals, the tables).  A plan takes a cached block of at
// least its size and at most 1.25x + 64 MiB; zd_trim_cache() frees them all,
// and so does a failed allocation before its retry.  ZD_WS_CACHE_MB caps
// the bytes held (default 8 GiB, at most 4 blocks; 0 disables the cache).
// The cache is invisible to PyTorch's allocator: a torch user that needs the
// memory back calls zd_trim_cache.
struct WsCache {
  struct E { int dev; uint8_t* p; uint64_t bytes; };
  std::mutex m;
  std::vector<E> free;
  uint64_t held = 0;
};
WsCache& ws_cache() {
  static WsCache c;
  return c;
}
uint64_t ws_cache_limit() {
  static const uint64_t lim = getenv("ZD_WS_CACHE_MB") ? strtoull(getenv("ZD_WS_CACHE_MB"), nullptr, 0) << 20
                                                       : 8ull << 30;
  return lim;
}
void ws_trim(int dev) {           // dev < 0: every device
  WsCache& C = ws_cache();
  std::lock_guard<std::mutex> g(C.m);
  for (size_t i = 0; i < C.free.size();) {
    if (dev < 0 || C.free[i].dev == dev) {
      (void)hipFree(C.free[i].p);
      C.held -= C.free[i].bytes;
      C.free.erase(C.free.begin() + (long)i);
    } else {
      i++;
    }
  }
}
hipError_t ws_alloc(int dev, uint64_t bytes, uint8_t** p, uint64_t* got) {
  {
    WsCache& C = ws_cache();
    std::lock_guard<std::mutex> g(C.m);
    size_t best = SIZE_MAX;
    for (size_t i = 0; i < C.free.size(); i++) {
      const WsCache::E& e = C.free[i];
      if (e.dev == dev && e.bytes >= bytes && e.bytes <= bytes + bytes / 4 + (64ull << 20) &&
          (best == SIZE_MAX || e.bytes < C.free[best].bytes))
        best = i;
    }
    if (best != SIZE_MAX) {
      *p = C.free[best].p;
      *got = C.free[best].bytes;
      C.held -= *got;
      C.free.erase(C.free.begin() + (long)best);
      return hipSuccess;
    }
  }
  hipError_t e = hipMalloc(p, bytes);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    ws_trim(dev);
    e = hipMalloc(p, bytes);
  }
  *got = bytes;
  return e;
}
// (dev: the device p was allocated on, whatever device is current now)
void ws_release(uint8_t* p, uint64_t bytes, int dev) {
  if (!p) return;
  const uint64_t lim = ws_cache_limit();
  if (dev < 0 || bytes > lim) { (void)hipFree(p); return; }
  WsCache& C = ws_cache();
  std::lock_guard<std::mutex> g(C.m);
  C.free.push_back(WsCache::E{dev, p, bytes});
  C.held += bytes;
  while (C.held > lim || C.free.size() > 4) {        // oldest first
    (void)hipFree(C.free.front().p);
    C.held -= C.free.front().bytes;
    C.free.erase(C.free.begin());
  }
}

// the output staging of a plan whose frames' sizes are bounds
int upload_staging(zd_plan* P) {
  if (!P->info.out_exact) {
    P->staging_bytes = P->info.out_bytes;
    HIPCHK(hipMalloc(&P->d_staging, std::max<uint64_t>(P->staging_bytes, 16)));
  }
  return 0;
}

// the workspace and the descriptors at its head
int upload_desc(zd_plan* P) {
  HIPCHK(hipGetDevice(&P->dev));
  HIPCHK(ws_alloc(P->dev, P->W.total, &P->d_ws, &P->ws_bytes));
  if (P->staged) {
    // the descriptors are in the pinned staging at their workspace offsets
    const hipError_t e = hipMemcpy(P->d_ws, host_stage().p, P->desc_bytes, hipMemcpyHostToDevice);
    P->stage_lock = std::unique_lock<std::mutex>();
    HIPCHK(e);
  } else {
    const Workspace& W = P->W;
    struct Piece { uint64_t off; const void* p; size_t bytes; };
    const Piece pieces[] = {
        {W.comp, P->comps.data(), P->comps.size() * sizeof(CompBlock)},
        {W.blocks, P->blocks.data(), P->blocks.size() * sizeof(BlockRec)},
        {W.frames, P->fdesc.data(), P->fdesc.size() * sizeof(FrameDesc)},
        {W.frame_state0, P->fstate0.data(), P->fstate0.size() * sizeof(FrameState)},
        {W.list_tables, P->list_tables.data(), P->list_tables.size() * 4},
        {W.list_huf, P->list_huf.data(), P->list_huf.size() * 4},
        {W.list_seq, P->list_seq.data(), P->list_seq.size() * 4},
        {W.list_k4f, P->list_k4f.data(), P->list_k4f.size() * 4},
        {W.copies, P->copies.data(), P->copies.size() * sizeof(CopyDesc)},
        {W.jframes, P->jframes.data(), P->jframes.size() * sizeof(JFrame)},
        {W.jblkd, P->jblkd.data(), P->jblkd.size() * sizeof(JBlkDesc)},
        {W.jsegd, P->jsegd.data(), P->jsegd.size() * sizeof(JSegDesc)},
        {W.frame_dict, P->frame_dict.data(), P->frame_dict.size() * 4},
        {W.csum, P->frame_csum.data(), P->frame_csum.size() * 8},
    };
    for (const Piece& q : pieces)
      if (q.bytes) HIPCHK(hipMemcpy(P->d_ws + q.off, q.p, q.bytes, hipMemcpyHostToDevice));
    if (P->dset) {
      std::vector<const uint8_t*> dp;
      for (const DictData* d : P->dset_used) dp.push_back(d->d_content);
      dp.push_back(P->dset->d_none());
      HIPCHK(hipMemcpy(P->d_ws + W.dict_ptrs, dp.data(), dp.size() * 8, hipMemcpyHostToDevice));
    }
    if (P->prefix && !P->prefix_ptrs.empty())
      HIPCHK(hipMemcpy(P->d_ws + W.dict_ptrs, P->prefix_ptrs.data(), 8 * P->prefix_ptrs.size(), hipMemcpyHostToDevice));
  }
  return init_verify(P);
}

int upload_plan(zd_plan* P) {
  if (int r = upload_desc(P)) return r;
  return upload_staging(P);
}

// The prebuilt comps of the formatted dictionaries a plan uses (comp 0 of a
// dictionary plan, comps 0..U-1 of a dictionary-set plan), once per plan:
// their slots and their states (zd_k_reset leaves those states alone,
// launch_reset keep_comps; no launch writes the slots)
int upload_dict_tables(zd_plan* P) {
  if (!P->n_dict_comps) return 0;
  std::vector<const DictData*> ds;
  if (P->dict) ds.push_back(P->dict.get());
  for (const DictData* d : P->dset_used)
    if (!d->raw) ds.push_back(d);
  std::vector<CompState> pcs(ds.size());
  for (size_t u = 0; u < ds.size(); u++) {
    pcs[u] = CompState{};
    pcs[u].huf_bits = ds[u]->huf_bits;
    for (int k = 0; k < 3; k++) pcs[u].al[k] = ds[u]->al[k];
    if (hipMemcpy(P->d_ws + P->W.luts + u * (LUT_ENTRIES * 2), ds[u]->d_lut, LUT_ENTRIES * 2,
                  hipMemcpyDeviceToDevice) != hipSuccess ||
        hipMemcpy(P->d_ws + P->W.fses + u * (FSE_SLOT * 2), ds[u]->d_fse, FSE_SLOT * 2, hipMemcpyDeviceToDevice) !=
            hipSuccess) {
      (void)hipGetLastError();
      return ZD_E_HIP;
    }
  }
  if (hipMemcpy(P->d_ws + P->W.comp_state, pcs.data(), pcs.size() * sizeof(CompState), hipMemcpyHostToDevice) !=
      hipSuccess) {
    (void)hipGetLastError();
    return ZD_E_HIP;
  }
  return 0;
}

// A plan's second stream and its fork/join events, kept for the next plans
// of the process (creating them took ~0.25 ms per plan).
struct AuxSet { int dev; hipStream_t s; hipEvent_t fork, join; };
std::mutex& aux_mutex() {
  static std::mutex m;
  return m;
}
std::vector<AuxSet>& aux_free() {
  static std::vector<AuxSet>* v = new std::vector<AuxSet>();   // never destroyed (no HIP calls at exit)
  return *v;
}
bool aux_take(zd_plan* P) {
  const int dev = P->dev;                 // upload_plan's device (current here)
  if (dev < 0) return false;
  {
    std::lock_guard<std::mutex> g(aux_mutex());
    auto& v = aux_free();
    for (size_t i = 0; i < v.size(); i++) {
      if (v[i].dev != dev) continue;
      P->aux = v[i].s; P->fork = v[i].fork; P->join = v[i].join;
      v.erase(v.begin() + (long)i);
      return true;
    }
  }
  return hipStreamCreateWithFlags(&P->aux, hipStreamNonBlocking) == hipSuccess &&
         hipEventCreateWithFlags(&P->fork, hipEventDisableTiming) == hipSuccess &&
         hipEventCreateWithFlags(&P->join, hipEventDisableTiming) == hipSuccess;
}
void aux_give(zd_plan* P) {
  const int dev = P->dev;                 // the plan's device, not the current one
  if (P->aux && P->fork && P->join && dev >= 0) {
    std::lock_guard<std::mutex> g(aux_mutex());
    if (aux_free().size() < 8) {
      aux_free().push_back(AuxSet{dev, P->aux, P->fork, P->join});
      P->aux = nullptr; P->fork = P->join = nullptr;
      return;
    }
  }
  if (P->fork) (void)hipEventDestroy(P->fork);
  if (P->join) (void)hipEventDestroy(P->join);
  if (P->aux) (void)hipStreamDestroy(P->aux);
  P->aux = nullptr; P->fork = P->join = nullptr;
}

// Frames from in (FrameIterator::next, frame.rs:94-99) into `part` until the
// input ends, a frame starting at or past `stop` comes up, or one fails (kept,
// with its status).
int index_frames(const uint8_t* src, Bytes& in, size_t stop, HostPart& part, uint32_t wopt) {
  while (in.n && (size_t)(in.p - src) < stop) {
    HostFrame hf;
    VecSink sink{part.blocks};
    int r = index_frame(src, in, &hf, sink, wopt);
    part.frames.push_back(hf);
    if (r) return r;
  }
  return 0;
}

// Index of the frame of a chain (frames in input order) that starts at byte
// `at`, or SIZE_MAX.
template <typename FR>
size_t chain_start(const FR& frames, size_t at, size_t count = SIZE_MAX) {
  size_t lo = 0, hi = std::min(count, (size_t)frames.size());
  while (lo < hi) {
    const size_t m = lo + (hi - lo) / 2;
    if (frames[m].d.src_offset < at) lo = m + 1; else hi = m;
  }
  return (lo < std::min(count, (size_t)frames.size()) && frames[lo].d.src_offset == at) ? lo : SIZE_MAX;
}

inline bool magic_at(const uint8_t* p) {
  uint32_t m;
  memcpy(&m, p, 4);
  return magic_word(m);
}

// The host walk (FrameIterator over the whole input).  Large inputs are cut
// into T byte ranges; thread k finds the first frame magic in its range and
// indexes the chain of frames from there while they start inside the range.
// Each frame's start follows from the one before it, so a chain that reaches
// a position of the true chain (the one from offset 0) is the true chain
// from there on.  The stitch checks exactly that: range k's frames are kept
// from the frame that starts where the kept frames before it end; a range
// whose chain never meets that position (a magic number inside data, or a
// frame longer than a range) is dropped and the walk continues serially.
// The result is the serial walk's, first failing frame included.
int plan_index(zd_plan* P, const uint8_t* src, size_t n) {
  static const char* wt = getenv("ZD_WALK_THREADS");   // experiments
  const unsigned hw = wt ? (unsigned)std::max(1, atoi(wt)) : std::max(1u, std::min(16u, std::thread::hardware_concurrency()));
  const size_t T = n >= PAR_INDEX_MIN_BYTES ? std::min<size_t>(hw, n >> 20) : 1;
  const uint32_t wopt = P->walk_opts();          // (zd_walk.h parse_compressed, the window limit)
  std::vector<HostPart> part(T);
  std::vector<int> st(T, 0);
  std::vector<size_t> end(T, 0), cut(T + 1);
  for (size_t k = 0; k <= T; k++) cut[k] = (size_t)((unsigned __int128)n * k / T);
  std::vector<double> tms(T, 0.0);
  const auto tw0 = std::chrono::steady_clock::now();
  run_parts(T, [&](size_t k) {
    const auto tk0 = std::chrono::steady_clock::now();
    struct Stamp {
      double& out; std::chrono::steady_clock::time_point t0;
      ~Stamp() { out = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }
    } stamp{tms[k], tk0};
    size_t p = cut[k];
    for (;;) {
      if (k) {                                   // the first candidate frame start in the range
        while (p < cut[k + 1] && (p + 4 > n || !magic_at(src + p))) p++;
        if (p >= cut[k + 1]) { end[k] = p; return; }
      }
      part[k].blocks.reserve((cut[k + 1] - cut[k]) / (16u << 10) + 16);
      Bytes in{src + p, n - p};
      st[k] = index_frames(src, in, cut[k + 1], part[k], wopt);
      end[k] = (size_t)(in.p - src);
      // a candidate that fails at once was a magic inside data: look further
      if (k && st[k] && part[k].frames.size() == 1) {
        part[k].frames.clear();
        part[k].blocks.clear();
        st[k] = 0;
        p++;
        continue;
      }
      return;
    }
  });
  std::vector<HostPart> keep;
  int status = 0;
  size_t cur = 0;                                // where the kept frames end
  uint64_t serial = 0;                           // bytes the stitch walked itself
  for (size_t k = 0; k < T && !status;) {
    if (k && cur >= cut[k + 1]) { k++; continue; }   // the range lies inside a kept frame
    const size_t i = k ? chain_start(part[k].frames, cur) : 0;
    if (i != SIZE_MAX) {
      HostPart& hp = part[k];
      if (i) hp.frames.erase(hp.frames.begin(), hp.frames.begin() + (long)i);   // their blocks stay unreferenced
      status = st[k];
      cur = end[k];
      keep.push_back(std::move(hp));
      k++;
      continue;
    }
    // The chains do not meet (range k's walk started at a magic number
    // inside data, or its first frame starts in an earlier range): walk on
    // from cur frame by frame, only until a frame ends where a later range's
    // chain has a frame start, then stitch on from that range.  One planted
    // magic number costs at most the ranges it spoils, never the rest of the
    // input (the walks from a given position are identical).
    HostPart tail;
    Bytes in{src + cur, n - cur};
    size_t kk = k;
    while (in.n) {
      HostFrame hf;
      VecSink sink{tail.blocks};
      const int r = index_frame(src, in, &hf, sink, wopt);
      tail.frames.push_back(hf);
      const size_t p = (size_t)(in.p - src);
      serial += p - cur;
      cur = p;
      if (r) { status = r; break; }
      while (kk + 1 < T && cur >= cut[kk + 1]) kk++;
      if (kk > k && chain_start(part[kk].frames, cur) != SIZE_MAX) break;
    }
    keep.push_back(std::move(tail));
    k = kk > k ? kk : T;
  }
  const auto tw1 = std::chrono::steady_clock::now();
  P->set_parts(std::move(keep));
  if (getenv("ZD_PLAN_TIMES")) {
    fprintf(stderr, "zd walk: %zu threads, threads", T);
    for (double t : tms) fprintf(stderr, " %.1f", t);
    fprintf(stderr, " ms; walk %.2f ms, stitch %.2f ms, serial %llu bytes\n",
            std::chrono::duration<double, std::milli>(tw1 - tw0).count(),
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw1).count(),
            (unsigned long long)serial);
  }
  P->index_status = status;
  P->index_stop = P->nframes;
  P->info.walk_serial_bytes = serial;
  return 0;
}

// The device walk (zd_kernels.hip zd_k_walk): plan_index for an input that
// is resident in HBM.  Byte ranges of >= 256 KiB (at most 16384 of them),
// one wave each; the count pass gives every range's chain (WalkRange), the
// fill pass writes their frames and blocks into one array each, which come
// back to the host through pinned staging.  The stitch is plan_index's, over
// the ranges; where two chains do not meet, the rest of the input is walked
// serially on the device (one range from there to the end).  The kept frames
// are then cut into parts for the parallel descriptor build.
struct DevWalkBufs {                      // device and pinned buffers, kept between plans
  std::mutex m;
  int dev = -1;
  WalkRange* d_wr = nullptr;
  size_t cap_wr = 0;
  uint8_t* d_out = nullptr;              // frames | blocks
  size_t cap_out = 0;
  uint8_t* h_out = nullptr;              // pinned
  size_t cap_h = 0;
  WalkRange* h_wr = nullptr;             // pinned
  size_t cap_hwr = 0;
  size_t fb = 0, bytes = 0;              // the last fill pass: frames | blocks layout in d_out
  // the device descriptor build (build_plan_device): per-frame counts and
  // tile sums, the frames' output offsets and capacities, the shape
  uint64_t* d_cnt = nullptr;
  size_t cap_cnt = 0;
  uint64_t* d_tot = nullptr;
  size_t cap_tot = 0;
  uint64_t* d_fo = nullptr;
  size_t cap_fo = 0;
  PlanShape* d_shape = nullptr;
  uint64_t* h_small = nullptr;           // pinned: shape, totals
  uint32_t* h_chain = nullptr;           // pinned: a chain batch's level counts, cursors and links (BatchCarve::lcount)
  // a chain batch on K4J (build_plan_device): the K4J columns in order[] order,
  // their scan's scratch, the frames' places, the levels' first entries | the pinned copy of the last
  uint64_t* d_jord = nullptr;
  size_t cap_jord = 0;
  uint64_t* h_jlev = nullptr;
  size_t cap_jlev = 0;
};
DevWalkBufs& dev_walk_bufs() {
  static DevWalkBufs* b = new DevWalkBufs();
  return *b;
}
// The walk's device buffers are `dev`'s from here on: those of another device
// start over.  The caller holds B.m.
void walk_bufs_on(DevWalkBufs& B, int dev) {
  if (B.dev == dev) return;
  if (B.d_wr) (void)hipFree(B.d_wr);
  if (B.d_out) (void)hipFree(B.d_out);
  B.d_wr = nullptr; B.cap_wr = 0; B.d_out = nullptr; B.cap_out = 0;
  B.dev = dev;
}

template <typename T>
bool grow_dev(T*& p, size_t& cap, size_t need) {
  if (need <= cap) return true;
  const size_t n = need;
  if (p) (void)hipFree(p);
  p = nullptr;
  cap = 0;
  if (hipMalloc(&p, n * sizeof(T)) != hipSuccess) { (void)hipGetLastError(); return false; }
  cap = n;
  return true;
}
template <typename T>
bool grow_pinned(T*& p, size_t& cap, size_t need) {
  if (need <= cap) return true;
  const size_t n = need;
  if (p) (void)hipHostFree(p);
  p = nullptr;
  cap = 0;
  if (hipHostMalloc(&p, n * sizeof(T), hipHostMallocDefault) != hipSuccess) return false;
  cap = n;
  return true;
}

// zd_plan_decompress's host <-> device path: a process-wide ring of two
// pinned chunks.  H2D: chunk k is copied into its pinned slot by the worker
// pool while chunk k - 1's DMA runs; D2H: chunk k + 1's DMA runs while chunk
// k is copied out.  (A pageable hipMemcpy stages through the runtime's own
// buffers with one thread.)  Without pinned memory it falls back to that.
constexpr uint64_t IO_CHUNK = 32ull << 20;
struct IoRing {
  std::mutex m;
  uint8_t* p[2] = {nullptr, nullptr};
  bool tried = false;
  bool ok() {
    if (!tried) {
      tried = true;
      for (auto& b : p)
        if (hipHostMalloc((void**)&b, IO_CHUNK, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); b = nullptr; }
      if (!p[0] || !p[1]) {
        for (auto& b : p) if (b) (void)hipHostFree(b);
        p[0] = p[1] = nullptr;
      }
    }
    return p[0] != nullptr;
  }
};
IoRing& io_ring() {
  static IoRing* r = new IoRing();   // never destroyed (no HIP calls at exit)
  return *r;
}
struct IoEvents {
  hipEvent_t e[2] = {nullptr, nullptr};
  bool ok = true;
  IoEvents() {
    for (auto& x : e) ok = ok && hipEventCreateWithFlags(&x, hipEventDisableTiming) == hipSuccess;
  }
  ~IoEvents() { for (auto& x : e) if (x) (void)hipEventDestroy(x); }
};
void par_memcpy(uint8_t* d, const uint8_t* s, size_t n) {
  const size_t T = std::min<size_t>(16, std::max<size_t>(1, n >> 21));   // >= 2 MiB a thread
  run_parts(T, [&](size_t k) {
    const size_t a = n * k / T, b = n * (k + 1) / T;
    memcpy(d + a, s + a, b - a);
  });
}
// The ring is held only while its slots are in use: the H2D copy returns
// after its last DMA (the stream synchronised), the D2H copy after its last
// host copy, so decodes on other plans or devices run beside it.
int io_h2d(uint8_t* d, const uint8_t* h, size_t n, hipStream_t s, IoRing& R, hipEvent_t ev[2]) {
  if (!n) return 0;
  std::lock_guard<std::mutex> lk(R.m);
  if (!R.ok()) { HIPCHK(hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, s)); HIPCHK(hipStreamSynchronize(s)); return 0; }
  for (size_t o = 0, k = 0; o < n; o += IO_CHUNK, k++) {
    const size_t c = std::min<size_t>(IO_CHUNK, n - o);
    if (k >= 2) HIPCHK(hipEventSynchronize(ev[k & 1]));   // chunk k - 2's DMA out of this slot
    par_memcpy(R.p[k & 1], h + o, c);
    HIPCHK(hipMemcpyAsync(d + o, R.p[k & 1], c, hipMemcpyHostToDevice, s));
    HIPCHK(hipEventRecord(ev[k & 1], s));
  }
  HIPCHK(hipStreamSynchronize(s));
  return 0;
}
int io_d2h(uint8_t* h, const uint8_t* d, size_t n, hipStream_t s, IoRing& R, hipEvent_t ev[2]) {
  if (!n) return 0;
  std::lock_guard<std::mutex> lk(R.m);
  if (!R.ok()) { HIPCHK(hipMemcpyAsync(h, d, n, hipMemcpyDeviceToHost, s)); HIPCHK(hipStreamSynchronize(s)); return 0; }
  const size_t nk = (n + IO_CHUNK - 1) / IO_CHUNK;
  auto chunk = [&](size_t k) { return std::min<size_t>(IO_CHUNK, n - k * IO_CHUNK); };
  auto issue = [&](size_t k) -> int {
    HIPCHK(hipMemcpyAsync(R.p[k & 1], d + k * IO_CHUNK, chunk(k), hipMemcpyDeviceToHost, s));
    HIPCHK(hipEventRecord(ev[k & 1], s));
    return 0;
  };
  if (int r = issue(0)) return r;
  for (size_t k = 0; k < nk; k++) {
    if (k + 1 < nk) if (int r = issue(k + 1)) return r;
    HIPCHK(hipEventSynchronize(ev[k & 1]));
    par_memcpy(h + k * IO_CHUNK, R.p[k & 1], chunk(k));
  }
  return 0;
}

// The fill pass's index (in B.d_out) -> the pinned copy
int dev_walk_download(DevWalkBufs& B, hipStream_t s, const HostFrame** frames, const HostBlock** blocks) {
  if (hipMemcpyAsync(B.h_out, B.d_out, B.bytes, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return ZD_E_HIP;
  *frames = (const HostFrame*)B.h_out;
  *blocks = (const HostBlock*)(B.h_out + B.fb);
  return 0;
}

// Walks `nranges` ranges from `first`; on return wr (pinned) holds the
// summaries with f_off / b_off, frames / blocks (pinned) the fill pass.
int dev_walk(DevWalkBufs& B, const uint8_t* d_src, uint64_t n, uint64_t first, uint64_t chunk, uint32_t nranges,
             hipStream_t s, uint64_t* F_out, uint64_t* B_out, const HostFrame** frames, const HostBlock** blocks,
             bool download = true, uint32_t wopt = 0) {
  if (!grow_dev(B.d_wr, B.cap_wr, nranges) || !grow_pinned(B.h_wr, B.cap_hwr, nranges)) return ZD_E_HIP;
  if (launch_walk(d_src, n, first, chunk, nranges, B.d_wr, nullptr, nullptr, false, s, wopt) != hipSuccess ||
      hipMemcpyAsync(B.h_wr, B.d_wr, nranges * sizeof(WalkRange), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return ZD_E_HIP;
  uint64_t F = 0, NB = 0;
  for (uint32_t k = 0; k < nranges; k++) {
    B.h_wr[k].f_off = F; B.h_wr[k].b_off = NB;
    F += B.h_wr[k].nframes; NB += B.h_wr[k].nblocks;
  }
  const size_t fb = align_up(F * sizeof(HostFrame), 256), bytes = fb + NB * sizeof(HostBlock);
  *F_out = F;
  *B_out = NB;
  if (!F) return 0;
  if (!grow_dev(B.d_out, B.cap_out, bytes) || !grow_pinned(B.h_out, B.cap_h, bytes)) return ZD_E_HIP;
  HostFrame* d_frames = (HostFrame*)B.d_out;
  HostBlock* d_blocks = (HostBlock*)(B.d_out + fb);
  if (hipMemcpyAsync(B.d_wr, B.h_wr, nranges * sizeof(WalkRange), hipMemcpyHostToDevice, s) != hipSuccess ||
      launch_walk(d_src, n, first, chunk, nranges, B.d_wr, d_frames, d_blocks, true, s, wopt) != hipSuccess)
    return ZD_E_HIP;
  B.fb = fb;
  B.bytes = bytes;
  if (download) return dev_walk_download(B, s, frames, blocks);
  return hipStreamSynchronize(s) != hipSuccess ? ZD_E_HIP : 0;
}

// Frames fr[i] (i in the kept list) with their blocks (global indices into
// bl) -> parts of about equal frame counts, built in parallel, b0 rebased.
void parts_from(const std::vector<const HostFrame*>& kept, const HostBlock* bl, std::vector<HostPart>& out) {
  const size_t nf = kept.size();
  const size_t T = std::max<size_t>(1, std::min<size_t>(16, nf / 512));
  const size_t base = out.size();
  out.resize(base + T);
  run_parts(T, [&](size_t t) {
    const size_t a = nf * t / T, e = nf * (t + 1) / T;
    HostPart& hp = out[base + t];
    size_t nb = 0;
    for (size_t i = a; i < e; i++) nb += kept[i]->nb;
    hp.frames.resize(e - a);
    hp.blocks.resize(nb);
    size_t b = 0;
    for (size_t i = a; i < e; i++) {
      HostFrame f = *kept[i];
      memcpy(hp.blocks.data() + b, bl + f.b0, f.nb * sizeof(HostBlock));
      f.b0 = (uint32_t)b;
      b += f.nb;
      hp.frames[i - a] = f;
    }
  });
}

// The descriptors of a device-walked plan built on the GPU:
// frames [0, F) of the walk's index in B.d_out (block indices global) are the
// plan's frames.  The host reads back the routing shape (two counters), the
// plan's totals (PLAN_FIELDS words) and the frames' output offsets and
// capacities (16 bytes a frame); everything else is written in place in the
// workspace by the planner's own per-frame pass (zd_plan.h plan_frame).
// K4J frames included: plan_frame writes their descriptors at the scanned
// K4J indices, and the count pass reports the largest K4J frame's sequence
// count (the rounds), so no plan falls back to the host build.
// A batch (zd_batch_create_device) adds what DevPlanIn carries: the frames'
// placement as device arrays, and the plan's dictionary or dictionary set
// (P->dict / P->dset): the prebuilt comps at the plan's head, and for a set
// the plan's table, built from the used flags that come back with the shape.
struct DevPlanIn {
  const uint64_t* place_out = nullptr;   // device arrays, one entry a frame (PlanCtx::place_out / place_cap)
  const uint64_t* place_cap = nullptr;
  const uint8_t* d_used = nullptr;       // a dictionary set: the used flag of each of its entries (device)
  PlanDict* d_dset = nullptr;            //   and room for the plan's table on the device (one entry at least)
  uint64_t alloc_ns = 0;                 // out: the workspace allocation and the small uploads
};
int build_plan_device(zd_plan* P, DevWalkBufs& B, uint64_t F, hipStream_t s, DevPlanIn* in = nullptr) {
  const HostFrame* d_frames = (const HostFrame*)B.d_out;
  const HostBlock* d_blocks = (const HostBlock*)(B.d_out + B.fb);
  P->nframes = F;
  P->cus = device_cus();
  const uint32_t k4j_min = P->k4j_min();
  const uint64_t nt = (F + 255) / 256;
  if (!B.d_shape && hipMalloc(&B.d_shape, sizeof(PlanShape)) != hipSuccess) return ZD_E_HIP;
  if (!B.h_small && hipHostMalloc((void**)&B.h_small, 64 * 8, hipHostMallocDefault) != hipSuccess) return ZD_E_HIP;
  if (!grow_dev(B.d_cnt, B.cap_cnt, std::max<uint64_t>(F, 1) * PLAN_FIELDS) ||
      !grow_dev(B.d_tot, B.cap_tot, (nt + 1) * PLAN_FIELDS) || !grow_dev(B.d_fo, B.cap_fo, 2 * std::max<uint64_t>(F, 1)))
    return ZD_E_HIP;
  HIPCHK(launch_plan_shape(d_frames, F, k4j_min, B.d_shape, s));
  HIPCHK(hipMemcpyAsync(B.h_small, B.d_shape, sizeof(PlanShape), hipMemcpyDeviceToHost, s));
  std::vector<uint8_t> used(P->dset ? P->dset->d.size() : 0, 0);
  if (P->dset && !used.empty()) {
    if (!in || !in->d_used || !in->d_dset) return ZD_E_INVALID_ARG;
    HIPCHK(hipMemcpyAsync(used.data(), in->d_used, used.size(), hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  PlanShape shape;
  memcpy(&shape, B.h_small, sizeof shape);
  const int32_t none[3] = {-1, -1, -1}, pre[3] = {0, 0, 0};
  const uint64_t rep0[3] = {1, 4, 8};
  if (P->with_dict()) plan_dict_comps(P, used.data());
  const DictData* D = P->dict.get();
  const bool tabs = D && !D->raw;
  const bool counts = plan_k4j_counts(P->flags, route_env(), P->prefix, P->chain, 0, P->dict_j());
  PlanCtx X = plan_ctx(P, tabs ? 0 : -1, tabs ? pre : none, D ? D->content : 0, D ? D->rep : rep0, 0, shape.multi == 0,
                       counts ? shape.jcand : 0);
  if (in) { X.place_out = in->place_out; X.place_cap = in->place_cap; }
  if (P->dset) {
    if (!in || !in->d_dset) return ZD_E_INVALID_ARG;
    if (!P->dset_tab.empty())
      HIPCHK(hipMemcpy(in->d_dset, P->dset_tab.data(), P->dset_tab.size() * sizeof(PlanDict), hipMemcpyHostToDevice));
    X.dset = in->d_dset;
  }
  // a chain batch on K4J: the frames' K4J counts scanned in order[] order, so
  // that the J frames are numbered level-major; the levels' first entries come
  // back with the totals (no wait of their own)
  const bool jlevels = P->chain_on_j() && F;
  PlanJOrder jo{};
  constexpr size_t JLEV_WORDS = 3 * CHAIN_LEVELS;
  if (jlevels) {
    if (!P->d_chain_order || !P->d_chain_lcount || !X.place_out) return ZD_E_INVALID_ARG;
    // col | scratch | j_at | lev
    const size_t col = PLAN_J_COLS * F, scr = PLAN_J_COLS * (nt + 1);
    if (!grow_dev(B.d_jord, B.cap_jord, 2 * col + scr + JLEV_WORDS) || !grow_pinned(B.h_jlev, B.cap_jlev, JLEV_WORDS))
      return ZD_E_HIP;
    jo = PlanJOrder{P->d_chain_order, P->d_chain_lcount, B.d_jord, B.d_jord + col, B.d_jord + col + scr,
                    B.d_jord + 2 * col + scr};
    HIPCHK(hipMemsetAsync(jo.lev, 0, 8 * JLEV_WORDS, s));
  }
  HIPCHK(launch_plan_count(X, d_frames, d_blocks, F, B.d_cnt, B.d_tot, B.d_shape, s, P->n_dict_comps,
                           jlevels ? &jo : nullptr));
  HIPCHK(hipMemcpyAsync(B.h_small, B.d_tot + nt * PLAN_FIELDS, PLAN_FIELDS * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(B.h_small + PLAN_FIELDS, B.d_shape, sizeof(PlanShape), hipMemcpyDeviceToHost, s));
  if (jlevels) HIPCHK(hipMemcpyAsync(B.h_jlev, jo.lev, 8 * JLEV_WORDS, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  PlanCounts T;
  memcpy(&T, B.h_small, sizeof T);
  memcpy(&shape, B.h_small + PLAN_FIELDS, sizeof shape);
  P->chain_j.clear();
  if (jlevels) {
    P->chain_j.resize(P->chain_count.size());
    plan_j_levels(B.h_jlev, P->chain_count.data(), (uint32_t)P->chain_count.size(), T.jframes, T.jseg, T.jpieces,
                  P->chain_j.data());
    X.j_at = jo.j_at;
  }
  Workspace& W = P->W;
  W = Workspace{};
  uint64_t o = 0;
  carve_head(W, T, o);
  if (X.dset) {
    W.frame_dict = o; o = align_up(o + 4 * std::max<uint64_t>(T.frames, 1), 256);
    W.dict_ptrs = o; o = align_up(o + 8 * (uint64_t)(X.ndset + 1), 256);
  }
  if (P->prefix) { W.dict_ptrs = o; o = align_up(o + 8 * std::max<uint64_t>(T.frames, 1), 256); }
  carve_verify_head(P, W, T, o);
  P->desc_bytes = o;
  plan_totals(P, T, X.fused);
  carve_tail(P, W, T, o, T.jwords, T.jpieces, shape.jmaxseq);
  carve_verify_tail(P, W, T, o);
  W.hframes = o;
  o = align_up(o + sizeof(HostFrame) * std::max<uint64_t>(F, 1), 256);
  W.total = o;
  const auto ta = std::chrono::steady_clock::now();
  HIPCHK(hipGetDevice(&P->dev));
  HIPCHK(ws_alloc(P->dev, W.total, &P->d_ws, &P->ws_bytes));
  uint8_t* b = P->d_ws;
  // (the dictionaries' prebuilt comps 0..U-1 and a set's content addresses: the fill pass writes neither)
  if (P->n_dict_comps) {
    std::vector<CompBlock> pre_comps(P->n_dict_comps);
    for (uint32_t k = 0; k < P->n_dict_comps; k++) pre_comps[k] = prebuilt_comp(k);
    HIPCHK(hipMemcpy(b + W.comp, pre_comps.data(), pre_comps.size() * sizeof(CompBlock), hipMemcpyHostToDevice));
  }
  if (P->dset) {
    std::vector<const uint8_t*> dp;
    for (const DictData* d : P->dset_used) dp.push_back(d->d_content);
    dp.push_back(P->dset->d_none());
    HIPCHK(hipMemcpy(b + W.dict_ptrs, dp.data(), dp.size() * 8, hipMemcpyHostToDevice));
  }
  // (a prefix batch: the checked addresses, from the batch's own array)
  if (P->prefix && F) {
    if (!P->d_prefix_ptrs) return ZD_E_INVALID_ARG;
    HIPCHK(hipMemcpyAsync(b + W.dict_ptrs, P->d_prefix_ptrs, 8 * F, hipMemcpyDeviceToDevice, s));
  }
  if (in) in->alloc_ns = ns(ta, std::chrono::steady_clock::now());
  uint64_t* d_fout = B.d_fo;
  uint64_t* d_fcap = B.d_fo + std::max<uint64_t>(F, 1);
  const Sink S{(CompBlock*)(b + W.comp), (BlockRec*)(b + W.blocks), (FrameDesc*)(b + W.frames),
               (FrameState*)(b + W.frame_state0), (uint32_t*)(b + W.list_tables), (uint32_t*)(b + W.list_huf),
               (uint32_t*)(b + W.list_seq), (uint32_t*)(b + W.list_k4f), (CopyDesc*)(b + W.copies),
               (JFrame*)(b + W.jframes), (JBlkDesc*)(b + W.jblkd), (JSegDesc*)(b + W.jsegd), d_fout, d_fcap,
               X.dset ? (uint32_t*)(b + W.frame_dict) : nullptr,
               P->verify() ? (uint64_t*)(b + W.csum) : nullptr};
  if (int r = init_verify(P)) return r;
  HIPCHK(launch_plan_fill(X, d_frames, d_blocks, F, B.d_cnt, B.d_tot, S, s));
  if (F) HIPCHK(hipMemcpyAsync(b + W.hframes, d_frames, F * sizeof(HostFrame), hipMemcpyDeviceToDevice, s));
  P->frame_out.resize(F);
  P->frame_cap.resize(F);
  if (F) {
    HIPCHK(hipMemcpyAsync(P->frame_out.data(), d_fout, F * 8, hipMemcpyDeviceToHost, s));
    HIPCHK(hipMemcpyAsync(P->frame_cap.data(), d_fcap, F * 8, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipStreamSynchronize(s));
  P->dev_built = true;
  P->staged = false;
  plan_info(P, T);
  P->info.device_descriptors = 1;
  return 0;
}

// ZD_DEV_DESC=0 (read once): device-walked plans take the host's descriptor
// build (the comparison leg of tests/test_gpu_walk.py)
bool dev_host_descriptors() {
  static const bool off = getenv("ZD_DEV_DESC") && atoi(getenv("ZD_DEV_DESC")) == 0;
  return off;
}

int plan_index_dev(zd_plan* P, const uint8_t* d_src, size_t n, hipStream_t s) {
  const auto tw0 = std::chrono::steady_clock::now();
  std::vector<HostPart> keep;
  int status = 0;
  double t_walk = 0, t_tail = 0;
  uint64_t serial_dev = 0;                    // bytes the stitch walked itself (tail walks)
  if (n) {
    DevWalkBufs& B = dev_walk_bufs();
    std::lock_guard<std::mutex> lk(B.m);
    int dev = 0;
    (void)hipGetDevice(&dev);
    walk_bufs_on(B, dev);
    const uint64_t chunk = std::max<uint64_t>(256u << 10, (n + 16383) / 16384);
    const uint32_t T = (uint32_t)((n + chunk - 1) / chunk);
    uint64_t F = 0, NB = 0;
    const HostFrame* fr = nullptr;
    const HostBlock* bl = nullptr;
    if (int r = dev_walk(B, d_src, n, 0, chunk, T, s, &F, &NB, &fr, &bl, false, P->walk_opts())) return r;
    t_walk = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count();
    const auto cut = [&](size_t k) { return std::min<uint64_t>((uint64_t)k * chunk, n); };
    // The common case from the range summaries alone: every range's chain
    // starts where the kept frames before it end (or the range lies inside a
    // kept frame and found none), so the plan's frames are a prefix of the
    // walk's index, and its descriptors are built where the index is
    // (build_plan_device); otherwise the index comes back for the host stitch.
    if (F && !dev_host_descriptors()) {
      uint64_t cur = 0, kept_end = 0;
      int st = 0;
      bool ok = true;
      for (size_t k = 0; k < T && !st && ok; k++) {
        const WalkRange& R = B.h_wr[k];
        if (k && cur >= cut(k + 1)) { ok = R.nframes == 0; continue; }
        if (k && !(R.nframes && R.p0 == cur)) { ok = false; break; }
        kept_end = R.f_off + R.nframes;
        st = R.status;
        cur = R.end;
      }
      if (ok) {
        const int r = build_plan_device(P, B, kept_end, s);
        if (r < 0) return r;
        if (r == 0) {
          P->index_status = st;
          P->info.index_status = st;
          P->info.walk_serial_bytes = 0;
          P->index_stop = P->nframes;
          if (getenv("ZD_PLAN_TIMES"))
            fprintf(stderr, "zd device walk + descriptors: %.2f ms (walk %.2f)\n",
                    std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count(), t_walk);
          return 0;
        }
      }
    }
    if (F)
      if (int r = dev_walk_download(B, s, &fr, &bl)) return r;
    struct Chain {                                   // one range's frames
      const HostFrame* p; size_t n;
      size_t size() const { return n; }
      const HostFrame& operator[](size_t i) const { return p[i]; }
    };
    // the walk's results stay in the pinned buffers unless a tail walk (which
    // reuses them) is needed: then they move to host vectors first
    std::vector<WalkRange> wr_keep;
    std::vector<HostFrame> fr_keep;
    std::vector<HostBlock> bl_keep;
    const WalkRange* wr = B.h_wr;
    auto chain = [&](size_t k) { return Chain{fr + wr[k].f_off, wr[k].nframes}; };
    std::vector<const HostFrame*> kept;
    kept.reserve(F);
    size_t cur = 0;
    for (size_t k = 0; k < T && !status;) {
      const WalkRange& R = wr[k];
      if (k && cur >= cut(k + 1)) { k++; continue; } // the range lies inside a kept frame
      const Chain c = chain(k);
      const size_t i0 = k ? chain_start(c, cur) : 0;
      if (i0 != SIZE_MAX) {
        for (size_t i = i0; i < c.n; i++) kept.push_back(c.p + i);
        status = R.status;
        cur = R.end;
        k++;
        continue;
      }
      // the chains do not meet: walk on from cur one range at a time on the
      // device (frames that start before the range's end), until the chain
      // reaches a frame start of a later range's chain (plan_index's rule)
      const auto tt = std::chrono::steady_clock::now();
      if (wr_keep.empty()) {
        wr_keep.assign(B.h_wr, B.h_wr + T);
        fr_keep.assign(fr, fr + F);
        bl_keep.assign(bl, bl + NB);
        wr = wr_keep.data(); fr = fr_keep.data(); bl = bl_keep.data();
      }
      parts_from(kept, bl, keep);                    // (kept may point into the pinned copy: same bytes)
      kept.clear();
      size_t kk = k;
      for (;;) {
        uint64_t F2 = 0, NB2 = 0;
        const HostFrame* fr2 = nullptr;
        const HostBlock* bl2 = nullptr;
        const uint64_t hi = std::max<uint64_t>(cut(kk + 1), cur + 1);
        if (int r = dev_walk(B, d_src, n, cur, hi - cur, 1, s, &F2, &NB2, &fr2, &bl2, true, P->walk_opts())) return r;
        std::vector<const HostFrame*> t2;
        for (uint64_t i = 0; i < F2; i++) t2.push_back(fr2 + i);
        parts_from(t2, bl2, keep);
        status = B.h_wr[0].status;
        serial_dev += B.h_wr[0].end - cur;
        cur = B.h_wr[0].end;
        if (status || !F2 || cur >= n) break;
        while (kk + 1 < T && cur >= cut(kk + 1)) kk++;
        if (kk > k && chain_start(chain(kk), cur) != SIZE_MAX) break;
      }
      t_tail += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tt).count();
      k = (kk > k && !status && cur < n) ? kk : T;
    }
    parts_from(kept, bl, keep);
  }
  P->set_parts(std::move(keep));
  if (getenv("ZD_PLAN_TIMES"))
    fprintf(stderr, "zd device walk: %.2f ms (kernels + index download %.2f, serial tail %.2f)\n",
            std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tw0).count(), t_walk, t_tail);
  P->index_status = status;
  P->info.walk_serial_bytes = serial_dev;
  P->index_stop = P->nframes;
  return 0;
}

}  // namespace

// ===========================================================================
// C ABI
// ===========================================================================
// Diagnostics (ZD_PLAN_DUMP=path): the plan's descriptor arrays, for
// comparing planner revisions byte for byte.
static void dump_plan_desc(const zd_plan* P) {
  const char* path = getenv("ZD_PLAN_DUMP");
  if (!path) return;
  FILE* f = fopen(path, "wb");
  if (!f) return;
  auto w = [&](const void* p, size_t bytes) { uint64_t b = bytes; fwrite(&b, 8, 1, f); if (bytes) fwrite(p, 1, bytes, f); };
  const Workspace& W = P->W;
  std::vector<uint8_t> dev_head;               // a device-built plan's descriptors, read back
  if (P->dev_built) {
    dev_head.resize(P->desc_bytes);
    if (P->desc_bytes && hipMemcpy(dev_head.data(), P->d_ws, P->desc_bytes, hipMemcpyDeviceToHost) != hipSuccess)
      (void)hipGetLastError();
  }
  auto at = [&](uint64_t off, const void* vec) -> const void* {
    if (P->dev_built) return (const void*)(dev_head.data() + off);
    return P->staged ? (const void*)(host_stage().p + off) : vec;
  };
  w(at(W.comp, P->comps.data()), P->n_comps * sizeof(CompBlock));
  w(at(W.blocks, P->blocks.data()), P->n_blocks * sizeof(BlockRec));
  w(at(W.frames, P->fdesc.data()), P->n_frames * sizeof(FrameDesc));
  w(at(W.frame_state0, P->fstate0.data()), P->n_frames * sizeof(FrameState));
  w(at(W.list_tables, P->list_tables.data()), P->n_tables * 4);
  w(at(W.list_huf, P->list_huf.data()), P->n_huf * 4);
  w(at(W.list_seq, P->list_seq.data()), P->n_seq * 4);
  w(at(W.list_k4f, P->list_k4f.data()), P->n_k4f * 4);
  w(at(W.copies, P->copies.data()), P->n_copies * sizeof(CopyDesc));
  w(at(W.jframes, P->jframes.data()), P->n_jframes * sizeof(JFrame));
  w(at(W.jblkd, P->jblkd.data()), P->n_jblk * sizeof(JBlkDesc));
  w(at(W.jsegd, P->jsegd.data()), P->n_jseg * sizeof(JSegDesc));
  w(P->frame_out.data(), P->frame_out.size() * 8);
  zd_plan_info I = P->info; I.workspace_bytes = 0; I.host_ns = I.device_ns = 0; I.walk_serial_bytes = 0;
  I.device_descriptors = 0;
  w(&I, sizeof I);
  uint64_t x[4] = {P->j_bytes, P->j_pieces, P->j_rounds, (uint64_t)(int64_t)P->index_status};
  w(x, sizeof x);
  fclose(f);
}

extern "C" {

int zd_abi_version(void) { return ZD_ABI_VERSION; }

int zd_route(uint32_t cus, uint64_t nframes, uint64_t n_tables, uint64_t n_seq_blocks, uint64_t n_huf_blocks,
             int single_block_frames, uint32_t flags, uint32_t* route) {
  if (!route || !cus) return ZD_E_INVALID_ARG;
  RouteIn in{};
  in.cus = cus; in.nframes = nframes; in.n_tables = n_tables; in.n_seq = n_seq_blocks; in.n_huf = n_huf_blocks;
  in.single_block_frames = single_block_frames != 0;
  in.flags = flags;
  const Route r = route_plan(in);
  *route = (r.fused ? ZD_ROUTE_FUSED : 0u) | (r.k4f ? ZD_ROUTE_K4F : 0u) | (r.k1_seq_waves ? ZD_ROUTE_K1_SEQ_WAVES : 0u) |
           (r.fork ? ZD_ROUTE_FORK : 0u) | (r.k1_fork ? ZD_ROUTE_K1_FORK : 0u) |
           (r.k1_split ? ZD_ROUTE_K1_SPLIT : 0u);
  return ZD_OK;
}

void zd_trim_cache(void) { ws_trim(-1); }

const char* zd_status_name(int s) {
  switch (s) {
    case ZD_OK: return "Ok";
    case ZD_E_NOT_ENOUGH_BYTES: return "NotEnoughBytes";
    case ZD_E_NOT_ENOUGH_BITS: return "NotEnoughBits";
    case ZD_E_MAX_READABLE_BITS_EXCEEDED: return "MaximumReadableBitsExceeded";
    case ZD_E_EMPTY_INPUT_DATA: return "EmptyInputData";
    case ZD_E_NULL_BYTE: return "NullByte";
    case ZD_E_EMPTY_SLICE: return "EmptySliceError";
    case ZD_E_LARGE_ACCURACY_LOG: return "LargeAccuracyLog";
    case ZD_E_CORRUPTED_TABLE: return "CorruptedTable";
    case ZD_E_SEQUENCE_CODE_MAX_EXCEEDED: return "SequenceCodeMaxValueExceeded";
    case ZD_E_HUFFMAN_DECODER_MISSING: return "HuffmanDecoderMissing";
    case ZD_E_CORRUPTED_STREAMS_SIZE: return "CorruptedStreamsSizeTooBig";
    case ZD_E_SEQ_RESERVED_SET: return "ReservedSet(sequences)";
    case ZD_E_NO_PREVIOUS_DECODER: return "NoPreviousDecoder";
    case ZD_E_CTX_WINDOW_SIZE_TOO_BIG: return "WindowSizeTooBig(context)";
    case ZD_E_NULL_OFFSET: return "NullOffsetError";
    case ZD_E_IMPOSSIBLE_VALUE: return "ImpossibleValue";
    case ZD_E_RESERVED_BLOCK_TYPE: return "ReservedBlockType";
    case ZD_E_UNRECOGNIZED_MAGIC: return "UnrecognizedMagic";
    case ZD_E_FRAME_RESERVED_SET: return "ReservedSet(frame)";
    case ZD_E_MISSING_CHECKSUM: return "MissingChecksum";
    case ZD_E_WINDOW_SIZE_TOO_BIG: return "WindowSizeTooBig";
    case ZD_E_REF_PANIC: return "ReferencePanic";
    case ZD_E_OUT_OF_DOMAIN: return "OutOfDomain";
    case ZD_E_DST_TOO_SMALL: return "DstTooSmall";
    case ZD_E_INVALID_ARG: return "InvalidArgument";
    case ZD_E_HIP: return "HipError";
    case ZD_E_NO_MEMORY: return "NoMemory";
    case ZD_E_NOT_DECODED: return "NotDecoded";
    case ZD_E_COMM: return "CommError";
    case ZD_E_DICT_CORRUPTED: return "DictionaryCorrupted";
    case ZD_E_DICT_MISMATCH: return "DictionaryMismatch";
    case ZD_E_CHECKSUM_WRONG: return "ChecksumWrong";
    case ZD_E_SEEK_TABLE: return "SeekTableWrong";
    default: return "Unknown";
  }
}

int zd_frames_index(const uint8_t* src, size_t n, zd_frame_desc* frames, size_t cap_frames, size_t* nframes,
                    zd_block_desc* blocks, size_t cap_blocks, size_t* nblocks, size_t* consumed) {
  if (!src && n) return ZD_E_INVALID_ARG;
  zd_plan W;                                     // the host walk only (no device state)
  if (frames && cap_frames && cap_frames <= FRAMES_INDEX_SERIAL_MAX) {
    // a few frames asked for: walk only those (serially), not the whole input
    HostPart hp;
    Bytes in{src, n};
    for (size_t f = 0; f <= cap_frames && in.n; f++) {
      HostFrame hf;
      VecSink sink{hp.blocks};
      const int r = index_frame(src, in, &hf, sink);
      hp.frames.push_back(hf);
      if (r) break;
    }
    std::vector<HostPart> v;
    v.push_back(std::move(hp));
    W.set_parts(std::move(v));
  } else {
    plan_index(&W, src, n);
  }
  size_t nf = 0, nb = 0;
  int status = 0;
  size_t stop = n;
  for (const HostPart& hp : W.parts) {
    for (const HostFrame& hf : hp.frames) {
      if (frames && cap_frames && nf >= cap_frames) { stop = (size_t)hf.d.src_offset; goto done; }
      if (hf.status) { status = hf.status; stop = (size_t)hf.d.src_offset; goto done; }
      if (frames && nf < cap_frames) {
        frames[nf] = hf.d;
        frames[nf].first_block = (uint32_t)nb;
        frames[nf].num_blocks = hf.nb;
      }
      for (uint32_t k = 0; k < hf.nb; k++) {
        const HostBlock& b = hp.blocks[hf.b0 + k];
        if (blocks && nb < cap_blocks) {
          zd_block_desc& d = blocks[nb];
          d.src_offset = b.src; d.block_size = b.size; d.type = b.type == 4 ? 0 : b.type;
          d.last = b.last; d.rle_byte = b.rle; d._pad = 0;
        }
        nb++;
      }
      nf++;
    }
  }
done:
  if (nframes) *nframes = nf;
  if (nblocks) *nblocks = nb;
  if (consumed) *consumed = stop;
  return status;
}

}  // extern "C"

int zd::frame_spans(const uint8_t* src, size_t n, std::vector<uint64_t>& off, std::vector<uint64_t>& size,
                    size_t* consumed) {
  zd_plan W;
  plan_index(&W, src, n);
  off.clear();
  size.clear();
  off.reserve(W.nframes);
  size.reserve(W.nframes);
  size_t stop = n;
  int status = 0;
  for (const HostPart& hp : W.parts) {
    for (const HostFrame& hf : hp.frames) {
      if (hf.status) { status = hf.status; stop = (size_t)hf.d.src_offset; goto done; }
      off.push_back(hf.d.src_offset);
      size.push_back(hf.d.src_size);
    }
  }
done:
  if (consumed) *consumed = stop;
  return status;
}

extern "C" {

// zd_plan_create / zd_plan_create_device: the walk (host or device), then
// the descriptors, the workspace and the upload.
static int plan_create(const uint8_t* src, const uint8_t* d_src, size_t n, uint32_t flags, hipStream_t s,
                       zd_plan** out, uint64_t cap0, const std::shared_ptr<DictData>& dict = nullptr,
                       const std::shared_ptr<DictSetData>& dset = nullptr) {
  zd_plan* P = new (std::nothrow) zd_plan();
  if (!P) return ZD_E_NO_MEMORY;
  P->flags = flags;
  P->cap0 = cap0;
  P->dict = dict;
  P->dset = dset;
  const auto t0 = std::chrono::steady_clock::now();
  if (d_src) {
    if (int r = plan_index_dev(P, d_src, n, s)) { zd_plan_destroy(P); return r; }
  } else {
    plan_index(P, src, n);
  }
  const auto ti = std::chrono::steady_clock::now();
  if (dict || !P->dev_built)
    if (int r = build_plan_staged(P)) { zd_plan_destroy(P); return r; }
  P->info.src_bytes = n;
  const auto t1 = std::chrono::steady_clock::now();
  dump_plan_desc(P);
  if (getenv("ZD_PLAN_TIMES"))
    fprintf(stderr, "zd plan: index %.2f ms, descriptors %.2f ms\n",
            std::chrono::duration<double, std::milli>(ti - t0).count(),
            std::chrono::duration<double, std::milli>(t1 - ti).count());
  int r = P->dev_built ? upload_staging(P) : upload_plan(P);
  if (!r) r = upload_dict_tables(P);
  const auto tu = std::chrono::steady_clock::now();
  // the second stream and its events (K2 beside K3) exist
  // from here on, so zd_decode_async creates nothing
  if (!r && !aux_take(P)) r = ZD_E_HIP;
  if (r) { zd_plan_destroy(P); return r; }
  const auto t2 = std::chrono::steady_clock::now();
  if (getenv("ZD_PLAN_TIMES"))
    fprintf(stderr, "zd plan: workspace + upload %.2f ms, streams %.2f ms\n",
            std::chrono::duration<double, std::milli>(tu - t1).count(),
            std::chrono::duration<double, std::milli>(t2 - tu).count());
  P->info.host_ns = ns(t0, t1);
  P->info.device_ns = ns(t1, t2);
  *out = P;
  return ZD_OK;
}

int zd_plan_create(const uint8_t* src, size_t n, uint32_t flags, zd_plan** out) {
  if (!out || (!src && n)) return ZD_E_INVALID_ARG;
  return plan_create(src, nullptr, n, flags, nullptr, out, 0);
}

int zd_plan_create_device(const uint8_t* d_src, size_t n, uint32_t flags, void* stream, zd_plan** out) {
  if (!out || (!d_src && n)) return ZD_E_INVALID_ARG;
  static const uint8_t none = 0;
  return plan_create(nullptr, d_src ? d_src : &none, n, flags, (hipStream_t)stream, out, 0);
}

int zd_plan_info_get(const zd_plan* P, zd_plan_info* info) {
  if (!P || !info) return ZD_E_INVALID_ARG;
  *info = P->info;
  return ZD_OK;
}

void zd_plan_destroy(zd_plan* P) {
  if (!P) return;
  // the workspace and the second stream go back to process caches: work the
  // plan launched must be done with them first (hipFree used to imply that)
  if (P->launched) {
    (void)hipStreamSynchronize(P->last_stream);
    if (P->aux) (void)hipStreamSynchronize(P->aux);
  }
  ws_release(P->d_ws, P->ws_bytes, P->dev);
  if (P->d_staging) (void)hipFree(P->d_staging);
  if (P->d_meta) (void)hipFree(P->d_meta);
  if (P->io_src) (void)hipFree(P->io_src);
  if (P->io_dst) (void)hipFree(P->io_dst);
  if (P->ev_made) {
    for (auto& e : P->ev) (void)hipEventDestroy(e);
    for (auto& e : P->dom_ev) (void)hipEventDestroy(e);
    (void)hipEventDestroy(P->ev_verify);
  }
  aux_give(P);
  delete P;
}

int zd_plan_k1_fallbacks(zd_plan* P, void* stream, uint64_t* huf_blocks, uint64_t* seq_blocks) {
  if (!P || !P->launched) return ZD_E_INVALID_ARG;
  HIPCHK(hipStreamSynchronize((hipStream_t)stream));
  std::vector<CompState> cs(P->n_comps);
  if (P->n_comps)
    HIPCHK(hipMemcpy(cs.data(), P->d_ws + P->W.comp_state, P->n_comps * sizeof(CompState), hipMemcpyDeviceToHost));
  uint64_t h = 0, q = 0;
  for (const CompState& c : cs) { h += c.k1_bigh != 0; q += c.k1_bigs != 0; }
  if (huf_blocks) *huf_blocks = h;
  if (seq_blocks) *seq_blocks = q;
  return ZD_OK;
}

int zd_plan_set_profiling(zd_plan* P, int enable) {
  if (!P || enable < 0 || enable > 2) return ZD_E_INVALID_ARG;
  if (enable && !P->ev_made) {
    for (auto& e : P->ev) HIPCHK(hipEventCreate(&e));
    for (auto& e : P->dom_ev) HIPCHK(hipEventCreate(&e));
    HIPCHK(hipEventCreate(&P->ev_verify));
    P->ev_made = true;
  }
  P->profile = enable == 1;
  P->profile_dom = enable == 2;
  return ZD_OK;
}

int zd_plan_kernel_times(zd_plan* P, const char** names, float* ms, int cap, int* n) {
  if (!P || !P->launched || !(P->profile || P->profile_dom)) return ZD_E_INVALID_ARG;
  if (P->profile_dom) {
    int k = 0;
    for (int g = 0; g < N_DOM && k < cap; g++) {
      if (!(P->dom_used >> g & 1)) continue;
      HIPCHK(hipEventSynchronize(P->dom_ev[2 * g + 1]));
      float t = 0;
      HIPCHK(hipEventElapsedTime(&t, P->dom_ev[2 * g], P->dom_ev[2 * g + 1]));
      if (names) names[k] = kDomNames[g];
      if (ms) ms[k] = t;
      k++;
    }
    if (n) *n = k;
    return ZD_OK;
  }
  HIPCHK(hipEventSynchronize(P->ev[N_KERNELS]));
  int k = 0;
  for (; k < N_KERNELS && k < cap; k++) {
    if (names) names[k] = kKernelNames[k];
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, P->ev[k], P->ev[k + 1]));
    if (ms) ms[k] = t;
  }
  // a verified plan's last launch, after the pipeline's
  if (k == N_KERNELS && k < cap && P->verify() && P->n_csums) {
    HIPCHK(hipEventSynchronize(P->ev_verify));
    float t = 0;
    HIPCHK(hipEventElapsedTime(&t, P->ev[N_KERNELS], P->ev_verify));
    if (names) names[k] = "zd_k_verify";
    if (ms) ms[k] = t;
    k++;
  }
  if (n) *n = k;
  return ZD_OK;
}

// The launch of zd_decode_async: the pipeline over the plan's descriptors,
// frame f's output at out + FrameDesc::out (zd_decode_async: d_dst or the
// plan's staging; a batch: the lowest destination, zd_batch_decode_async).
static int decode_launch(zd_plan* P, const uint8_t* d_src, uint8_t* out, hipStream_t s) {
  // frame and block states are reset every launch (keys, lengths, repeat
  // offsets, flags) from device-resident copies: no host memory is read, so
  // a graph captured around this call replays the reset
  // (one launch, zd_k_reset: frame states, block states, K1's tree list and
  // deep pool counters, K4J's round counters and done flags; ZD_RESET_COPIES
  // builds keep the six copy / fill launches it replaced)
#ifndef ZD_RESET_COPIES
  HIPCHK(launch_reset(P->d_ws, P->W, P->n_frames, P->n_comps, P->n_jframes != 0, P->j_pieces, s, P->n_dict_comps,
                      P->jpend_words()));
#else
  HIPCHK(hipMemcpyAsync(P->d_ws + P->W.frame_state, P->d_ws + P->W.frame_state0,
                        P->n_frames * sizeof(FrameState), hipMemcpyDeviceToDevice, s));
  HIPCHK(hipMemsetAsync(P->d_ws + P->W.comp_state, 0, std::max<uint64_t>(P->n_comps, 1) * sizeof(CompState), s));
  HIPCHK(hipMemsetAsync(P->d_ws + P->W.huge, 0, 4, s));
  HIPCHK(hipMemsetAsync(P->d_ws + P->W.deep, 0, 4, s));
  if (P->n_jframes) {
    HIPCHK(hipMemsetAsync(P->d_ws + P->W.jpend, 0, 4 * (size_t)P->jpend_words(), s));
    HIPCHK(hipMemsetAsync(P->d_ws + P->W.jdone, 0, std::max<uint64_t>(P->j_pieces, 1), s));
  }
#endif
  LaunchArgs a{};
  a.src = d_src;
  a.src_size = P->info.src_bytes;
  a.out = out;
  a.ws = P->d_ws;
  a.W = P->W;
  a.n_tables = (uint32_t)P->n_tables; a.n_huf = (uint32_t)P->n_huf; a.n_seq = (uint32_t)P->n_seq;
  a.n_frames = (uint32_t)P->n_frames; a.n_k4f = (uint32_t)P->n_k4f; a.n_copies = (uint32_t)P->n_copies;
  a.n_jframes = (uint32_t)P->n_jframes; a.n_k0only = (uint32_t)P->n_k0only;
  a.n_jblk = (uint32_t)P->n_jblk; a.n_jseg = (uint32_t)P->n_jseg;
  // ZD_F_J_ONE_ROUND (a test switch, set per plan) cuts the rounds to one
  // of one hop: the path that re-plans a frame whose pointer jumping did not
  // converge, on the streaming executor
  a.j_rounds = (P->flags & ZD_F_J_ONE_ROUND) && P->j_rounds ? 1u : P->j_rounds;
  a.j_pieces = P->j_pieces;
  a.cus = P->cus;
  a.stream = s;
  // the route, resolved every launch (profiling may have been switched since
  // the last one); the rest of `a` is what the route's launches need
  const LaunchIn in{P->cus, P->n_frames, P->n_tables, P->n_huf, P->n_seq, P->flags, P->fused,
                    P->chain ? K4_CHAIN : P->prefix ? K4_PREFIX : P->dset ? K4_DICT_SET : P->dict ? K4_DICT : K4_PLAIN,
                    P->profile ? 1 : P->profile_dom ? 2 : 0};
  const LaunchRoute R = a.route = launch_route(in, route_env());
  if (P->chain) {
    a.chain_order = P->d_chain_order;
    a.chain_parent = P->d_chain_parent;
    a.chain_count = P->chain_count.data();
    a.chain_levels = (uint32_t)P->chain_count.size();
    if (P->chain_on_j() && P->chain_j.size() == P->chain_count.size()) a.chain_j = P->chain_j.data();
    if (P->n_jframes && !a.chain_j) return ZD_E_INVALID_ARG;   // (never: a chain plan has J frames only level by level)
  }
  // (every plan has its second stream, aux_take, and a profiled one its events, zd_plan_set_profiling)
  if (((R.fork || R.k1_fork) && !P->aux) || (R.profiling && !P->ev_made)) return ZD_E_HIP;
  a.aux = P->aux; a.fork = P->fork; a.join = P->join;
  a.events = P->ev; a.dom_events = P->dom_ev; a.dom_used = &P->dom_used;
  P->dom_used = 0;
  if (P->dict) { a.dict = P->dict->d_content; a.dict_tab = P->dict->d_self; }
  P->last_fused = R.fused;
  if (R.fused) {
    HIPCHK(hipMemsetAsync(P->d_ws + P->W.redo, 0, std::max<uint64_t>(P->n_frames, 1), s));
    HIPCHK(hipMemsetAsync(P->d_ws + P->W.k2done, 0, 4, s));
  }
  HIPCHK(launch_pipeline(a));
  // ZD_F_VERIFY_CHECKSUM: the frames' digests against their stored checksums,
  // behind everything the pipeline queued (its second stream has joined `s`)
  // and before whatever reads the frame states next (zd_k_batch_results)
  if (P->verify() && P->n_csums) {
    HIPCHK(launch_verify(P->d_ws, P->W, out, (uint32_t)P->n_frames, P->cus, s));
    if (R.profiling == 1) HIPCHK(hipEventRecord(P->ev_verify, s));
  }
  P->launched = true;
  P->last_stream = s;
  return ZD_OK;
}

int zd_decode_async(zd_plan* P, const uint8_t* d_src, uint8_t* d_dst, size_t dst_cap, void* stream) {
  if (!P) return ZD_E_INVALID_ARG;
  // out_bytes bounds the output in both layouts (the staging layout is
  // compacted into d_dst by zd_plan_results)
  if (dst_cap < P->info.out_bytes) return ZD_E_DST_TOO_SMALL;
  return decode_launch(P, d_src, P->info.out_exact ? d_dst : P->d_staging, (hipStream_t)stream);
}

int zd_plan_results(zd_plan* P, uint8_t* d_dst, void* stream, int32_t* frame_status, uint64_t* frame_len,
                    uint64_t* total_len, int32_t* first_error_frame) {
  if (!P || !P->launched) return ZD_E_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(hipStreamSynchronize(s));
  size_t nf = P->n_frames;
  std::vector<FrameState> st(nf);
  if (nf) HIPCHK(hipMemcpy(st.data(), P->d_ws + P->W.frame_state, nf * sizeof(FrameState), hipMemcpyDeviceToHost));
  int first = -1;
  int overall = 0;
  uint64_t total = 0;
  P->limit_frame = -1;
  P->limit_stage = 0;
  P->info.error_key = KEY_NONE;
  std::vector<uint64_t> from, to, len;
  bool need_compact = !P->info.out_exact;
  for (size_t f = 0; f < nf; f++) {
    int code = key_code(st[f].key);
    uint64_t l = st[f].out_len;
    if (first >= 0) code = ZD_E_NOT_DECODED;
    if (frame_status) frame_status[f] = code;
    if (frame_len) frame_len[f] = code ? 0 : l;
    if (code && first < 0) {
      first = (int)f;
      overall = code;
      const uint64_t k = st[f].key;
      P->info.error_key = k;
      if (code == ZD_E_OUT_OF_DOMAIN && key_phase(k) == PH_LIMIT &&
          (key_stage(k) == LS_CAPACITY || key_stage(k) == LS_JROUNDS)) {
        P->limit_frame = (int64_t)f;
        P->limit_stage = key_stage(k);
      }
      if (code == ZD_E_OUT_OF_DOMAIN && key_phase(k) == PH_DECODE && key_stage(k) == DS_LITERALS &&
          ((k >> 8) & 0xFFFFF) == DS_LIT_OVERFLOW_SUB) {
        P->limit_frame = (int64_t)f;
        P->limit_stage = LS_CAPACITY;          // a re-plan gives its blocks room for every literal
      }
    }
    if (first < 0) {
      if (P->info.out_exact && l != P->frame_cap[f]) need_compact = true;
      from.push_back(P->frame_out[f]);
      to.push_back(total);
      len.push_back(l);
      total += l;
    }
  }
  if (need_compact && !from.empty()) {
    // exact layout but a frame came out shorter than its FCS: move through a staging copy
    const uint8_t* stage = P->d_staging;
    if (P->info.out_exact) {
      // the plan's staging buffer, made on the first such call and kept
      if (!P->d_staging) {
        P->staging_bytes = P->info.out_bytes;
        HIPCHK(hipMalloc(&P->d_staging, std::max<uint64_t>(P->staging_bytes, 16)));
      }
      HIPCHK(hipMemcpyAsync(P->d_staging, d_dst, P->info.out_bytes, hipMemcpyDeviceToDevice, s));
      stage = P->d_staging;
    }
    size_t m = from.size();
    if (!grow_dev(P->d_meta, P->meta_cap, 3 * m)) return ZD_E_HIP;
    uint64_t* d_meta = P->d_meta;
    HIPCHK(hipMemcpy(d_meta, from.data(), m * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_meta + m, to.data(), m * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(d_meta + 2 * m, len.data(), m * 8, hipMemcpyHostToDevice));
    HIPCHK(launch_compact(stage, d_dst, d_meta, d_meta + m, d_meta + 2 * m, (uint32_t)m, s));
    HIPCHK(hipStreamSynchronize(s));
  }
  if (first < 0 && P->index_status) { first = (int)nf; overall = P->index_status; }
  // frames zd_k_fused handed to its redo pass (a fast-chain reject, or a wait
  // past its bound: a slowdown, never a different output)
  P->info.fused_redo_frames = 0;
  if (P->last_fused && nf) {
    std::vector<uint8_t> redo(nf);
    HIPCHK(hipMemcpy(redo.data(), P->d_ws + P->W.redo, nf, hipMemcpyDeviceToHost));
    for (uint8_t r : redo) P->info.fused_redo_frames += r != 0;
  }
  P->res_off = to;
  P->res_len = len;
  if (total_len) *total_len = total;
  if (first_error_frame) *first_error_frame = first;
  return overall;
}

int zd_plan_checksums(zd_plan* P, const uint8_t* d_dst, void* stream, int32_t* ok, uint64_t* hash) {
  if (!P || !P->launched) return ZD_E_INVALID_ARG;
  hipStream_t s = (hipStream_t)stream;
  const size_t nf = P->n_frames, m = P->res_off.size();   // frames 0..m-1 were decoded
  std::vector<uint64_t> h(m, 0);
  if (m) {
    if (!grow_dev(P->d_meta, P->meta_cap, 3 * m)) return ZD_E_HIP;
    uint64_t* d = P->d_meta;
    hipError_t e = hipMemcpy(d, P->res_off.data(), m * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + m, P->res_len.data(), m * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_xxh64(d_dst, d, d + m, (uint32_t)m, d + 2 * m, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e == hipSuccess) e = hipMemcpy(h.data(), d + 2 * m, m * 8, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return ZD_E_HIP;
  }
  if (!P->frames_ready()) return ZD_E_HIP;
  for (size_t f = 0; f < nf; f++) {
    const zd_frame_desc& d = P->frame(f).d;
    const bool have = f < m && d.kind == ZD_FRAME_ZSTD && d.has_checksum;
    if (ok) ok[f] = have ? ((uint32_t)h[f] == d.checksum ? 1 : 0) : -1;
    if (hash) hash[f] = f < m ? h[f] : 0;
  }
  return ZD_OK;
}

}  // extern "C"

namespace {

// Makes o hold `need` bytes, keeping its first `keep`.  When o.p is the
// caller's own allocation (*o.own) it grows by half at least; when o.p is a
// buffer the caller lent (rank 0's gather buffer in zd_decode_sharded) the
// kept allocation *o.own is reused if it holds `need`, else replaced by one of
// `need` bytes (half again over its old size at most) -- never sized from the
// lent buffer.
int devout_reserve(DevOut& o, uint64_t need, uint64_t keep, hipStream_t s) {
  if (need <= o.cap) return 0;
  const bool lent = o.p != *o.own;
  if (lent && *o.own && *o.own_cap >= need) {
    if (keep) HIPCHK(hipMemcpyAsync(*o.own, o.p, keep, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipStreamSynchronize(s));
    o.p = *o.own;
    o.cap = *o.own_cap;
    return 0;
  }
  const uint64_t base = lent ? (*o.own ? *o.own_cap : 0) : o.cap;
  const uint64_t want = std::max<uint64_t>(need, base + base / 2);
  uint8_t* q = nullptr;
  if (hipMalloc(&q, want) != hipSuccess) {
    (void)hipGetLastError();
    ws_trim(-1);
    HIPCHK(hipMalloc(&q, want));
  }
  if (keep) HIPCHK(hipMemcpyAsync(q, o.p, keep, hipMemcpyDeviceToDevice, s));
  HIPCHK(hipStreamSynchronize(s));
  if (*o.own) (void)hipFree(*o.own);        // the old kept allocation (o.p or unused)
  *o.own = q;
  *o.own_cap = want;
  o.p = q;
  o.cap = want;
  return 0;
}

bool call_failed(int st) { return st == ZD_E_HIP || st == ZD_E_INVALID_ARG || st == ZD_E_DST_TOO_SMALL; }

}  // namespace

// Re-plans past a frame that reached a limit the host can lift: a frame that
// decodes past the capacity its plan reserved (its Frame_Content_Size, or
// 128 KiB per block -- the reference checks neither, decoding_context.rs:
// 29-47, block.rs:50) is planned again from its own start with four times the
// capacity (K4_MAX_FRAME_OUT at most); a K4J frame whose pointer jumping did
// not converge is planned again on the streaming executor.  Each re-plan
// covers the input from that frame on (the same resident input, from that
// frame's offset); its output follows the frames before in `out`.
constexpr int LIMIT_RETRIES = 12;

int zd::decode_resident(zd_plan* P, const uint8_t* src, size_t n, const uint8_t* d_src, DevOut& out, void* stream,
                        uint64_t* total_out, int64_t* first_out, uint64_t* replans, FrameOuts* fo) {
  const hipStream_t s = (hipStream_t)stream;
  *total_out = 0;
  *first_out = -1;
  const uint64_t ob = std::max<uint64_t>(P->info.out_bytes, 16);
  if (int r = devout_reserve(out, ob, 0, s)) return r;
  int st = zd_decode_async(P, d_src, out.p, out.cap, s);
  if (st) return st;
  uint64_t produced = 0;
  int32_t first = -1;
  // per-frame outcomes: the current plan's, written into fo from frame fbase on
  std::vector<int32_t> fs;
  std::vector<uint64_t> fl;
  auto want = [&](zd_plan* Q) {
    if (!fo) return;
    fs.assign(Q->n_frames, 0);
    fl.assign(Q->n_frames, 0);
  };
  auto keep = [&](zd_plan* Q, int64_t fb, uint64_t at) {
    if (!fo) return;
    uint64_t o = at;
    for (size_t f = 0; f < Q->n_frames && fb + (int64_t)f < (int64_t)fo->status.size(); f++) {
      fo->status[fb + f] = fs[f];
      fo->off[fb + f] = o;
      fo->len[fb + f] = fl[f];
      o += fl[f];
    }
  };
  if (fo) {
    fo->status.assign(P->n_frames, ZD_E_NOT_DECODED);
    fo->off.assign(P->n_frames, 0);
    fo->len.assign(P->n_frames, 0);
  }
  want(P);
  st = zd_plan_results(P, out.p, s, fo ? fs.data() : nullptr, fo ? fl.data() : nullptr, &produced, &first);
  if (call_failed(st)) return st;
  keep(P, 0, 0);
  zd_plan* cur = P;
  size_t base = 0;                                 // cur's input starts at src + base
  int64_t fbase = 0;                               // and its frame 0 is P's frame fbase
  for (int k = 0; k < LIMIT_RETRIES && st == ZD_E_OUT_OF_DOMAIN && cur->limit_frame >= 0; k++) {
    const size_t f = (size_t)cur->limit_frame;
    const uint64_t old_cap = cur->frame_cap[f];
    uint32_t flags = cur->flags;
    uint64_t cap0 = 0;
    if (cur->limit_stage == LS_CAPACITY) {
      // past K4J's 32 GiB, or with K4J forced off the streaming K4's int32
      // positions (plan_frame keys a larger frame out of domain): stop
      // (a dictionary plan: the streaming K4's, less the content before the
      // frame -- of the frame's own dictionary in a dictionary-set plan)
      uint64_t lim = k4j_mode_of(flags, route_env()) == 0 ? K4_MAX_FRAME_OUT : K4J_MAX_FRAME_OUT;
      if (cur->dict) lim = K4_MAX_FRAME_OUT - cur->dict->content;
      if (cur->dset) {
        if (!cur->frames_ready()) { st = ZD_E_HIP; break; }
        const int k = cur->dset->find(cur->frame(f).d);
        lim = K4_MAX_FRAME_OUT - (k >= 0 ? cur->dset->d[(size_t)k]->content : 0);
      }
      if (old_cap >= lim) break;
      cap0 = std::min<uint64_t>(lim, std::max<uint64_t>(4 * old_cap, old_cap + (1u << 20)));
    } else {
      flags = (flags & ~ZD_F_BLOCK_PARALLEL) | ZD_F_FRAME_SERIAL;
      cap0 = old_cap;
    }
    if (!cur->frames_ready()) { st = ZD_E_HIP; break; }
    const size_t at = base + (size_t)cur->frame(f).d.src_offset;
    zd_plan* Q = nullptr;
    const int r = plan_create(src + at, nullptr, n - at, flags, nullptr, &Q, cap0, cur->dict, cur->dset);
    if (r) { st = r; break; }
    if (replans) (*replans)++;
    const uint64_t qob = std::max<uint64_t>(Q->info.out_bytes, 16);
    uint64_t t2 = 0;
    int32_t qfirst = -1;
    st = devout_reserve(out, produced + qob, produced, s);
    if (!st) st = zd_decode_async(Q, d_src + at, out.p + produced, qob, s);
    want(Q);
    if (!st) st = zd_plan_results(Q, out.p + produced, s, fo ? fs.data() : nullptr, fo ? fl.data() : nullptr, &t2, &qfirst);
    if (cur != P) zd_plan_destroy(cur);
    cur = Q;
    base = at;
    fbase += (int64_t)f;
    first = qfirst;
    if (call_failed(st)) break;
    keep(Q, fbase, produced);
    produced += t2;
  }
  if (cur != P) {
    P->info.error_key = cur->info.error_key;
    zd_plan_destroy(cur);
  }
  if (call_failed(st)) return st;
  *total_out = produced;
  *first_out = first >= 0 ? fbase + first : -1;
  return st;
}

extern "C" {

int zd_plan_decompress(zd_plan* P, const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len) {
  if (!P || (!src && n) || n != P->info.src_bytes) return ZD_E_INVALID_ARG;
  // device buffers owned by the plan (kept for the next call), the input and
  // output through the pinned ring (chunked, the host copies on the worker
  // pool overlapping the DMA), everything on one stream
  if (!grow_dev(P->io_src, P->io_src_cap, n + ZD_SRC_PADDING)) return ZD_E_HIP;
  const hipStream_t s = nullptr;
  IoEvents ev;
  if (!ev.ok) return ZD_E_HIP;
  const auto t0 = std::chrono::steady_clock::now();
  if (int r = io_h2d(P->io_src, src, n, s, io_ring(), ev.e)) return r;
  const auto t1 = std::chrono::steady_clock::now();
  DevOut o{P->io_dst, P->io_dst_cap, &P->io_dst, &P->io_dst_cap};
  uint64_t produced = 0;
  int64_t first = -1;
  P->info.replans = 0;
  const int st = decode_resident(P, src, n, P->io_src, o, s, &produced, &first, &P->info.replans, &P->io_fo);
  if (call_failed(st)) return st;
  const auto t2 = std::chrono::steady_clock::now();
  const size_t copy = (size_t)std::min<uint64_t>(produced, cap);
  if (copy && dst)
    if (int e = io_d2h(dst, o.p, copy, s, io_ring(), ev.e)) return e;
  const auto t3 = std::chrono::steady_clock::now();
  P->info.io_h2d_ns = ns(t0, t1);
  P->info.io_decode_ns = ns(t1, t2);
  P->info.io_d2h_ns = ns(t2, t3);
  if (out_len) *out_len = (size_t)produced;
  if (!st && produced > cap) return ZD_E_DST_TOO_SMALL;
  return st;
}

int zd_plan_frame_outputs(const zd_plan* P, int32_t* status, uint64_t* offset, uint64_t* length, size_t cap,
                          size_t* n) {
  if (!P) return ZD_E_INVALID_ARG;
  const size_t m = P->io_fo.status.size();
  for (size_t f = 0; f < m && f < cap; f++) {
    if (status) status[f] = P->io_fo.status[f];
    if (offset) offset[f] = P->io_fo.off[f];
    if (length) length[f] = P->io_fo.len[f];
  }
  if (n) *n = m;
  return ZD_OK;
}

int zd_decompress(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, uint32_t flags) {
  zd_plan* P = nullptr;
  int r = zd_plan_create(src, n, flags, &P);
  if (r) return r;
  r = zd_plan_decompress(P, src, n, dst, cap, out_len);
  zd_plan_destroy(P);
  return r;
}

// ---------------------------------------------------------------------------
// Dictionaries
// ---------------------------------------------------------------------------
int zd_dict_create(const uint8_t* dict, size_t n, zd_dict** out) {
  if (!dict || !n || !out) return ZD_E_INVALID_ARG;
  auto rd32 = [&](size_t at) {
    return (uint32_t)dict[at] | (uint32_t)dict[at + 1] << 8 | (uint32_t)dict[at + 2] << 16 | (uint32_t)dict[at + 3] << 24;
  };
  const bool formatted = n >= 4 && rd32(0) == DICT_MAGIC;
  if (formatted && n < 8) return ZD_E_DICT_CORRUPTED;
  // (a formatted dictionary's content is smaller than n: one bound for both)
  if (n > ZD_DICT_MAX_CONTENT + (formatted ? (64u << 10) : 0)) return ZD_E_OUT_OF_DOMAIN;
  std::shared_ptr<DictData> D(new (std::nothrow) DictData());
  zd_dict* h = new (std::nothrow) zd_dict();
  if (!D || !h) { delete h; return ZD_E_NO_MEMORY; }
  std::unique_ptr<zd_dict> hold(h);
  HIPCHK(hipGetDevice(&D->dev));
  const size_t bytes = DICT_PAD + n + 2 * DICT_PAD, self_at = (bytes + 7) & ~(size_t)7;
  HIPCHK(hipMalloc(&D->d_buf, self_at + sizeof(const uint8_t*)));
  HIPCHK(hipMemset(D->d_buf, 0, DICT_PAD));
  HIPCHK(hipMemset(D->d_buf + DICT_PAD + n, 0, 2 * DICT_PAD));
  HIPCHK(hipMemcpy(D->d_buf + DICT_PAD, dict, n, hipMemcpyHostToDevice));
  if (!formatted) {
    D->d_content = D->d_buf + DICT_PAD;
    D->content = n;
  } else {
    D->raw = false;
    D->id = rd32(4);
    HIPCHK(hipMalloc(&D->d_lut, LUT_ENTRIES * 2));
    HIPCHK(hipMalloc(&D->d_fse, FSE_SLOT * 2));
    HIPCHK(hipMemset(D->d_lut, 0, LUT_ENTRIES * 2));
    HIPCHK(hipMemset(D->d_fse, 0, FSE_SLOT * 2));
    DictTables* d_res = nullptr;
    HIPCHK(hipMalloc(&d_res, sizeof(DictTables)));
    DictTables res{};
    hipError_t e = launch_dict_tables(D->d_buf + DICT_PAD, (uint32_t)n, D->d_lut, D->d_fse, d_res, nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e == hipSuccess) e = hipMemcpy(&res, d_res, sizeof res, hipMemcpyDeviceToHost);
    (void)hipFree(d_res);
    HIPCHK(e);
    if (res.status) return res.status;
    // the repeat offsets, then the content
    if ((uint64_t)res.rep_off + 12 > n) return ZD_E_DICT_CORRUPTED;
    D->content = n - res.rep_off - 12;
    if (!D->content) return ZD_E_DICT_CORRUPTED;
    if (D->content > ZD_DICT_MAX_CONTENT) return ZD_E_OUT_OF_DOMAIN;
    for (int k = 0; k < 3; k++) {
      D->rep[k] = rd32(res.rep_off + 4 * (size_t)k);
      if (!D->rep[k] || D->rep[k] > D->content) return ZD_E_DICT_CORRUPTED;
    }
    D->d_content = D->d_buf + DICT_PAD + res.rep_off + 12;
    D->huf_bits = (uint8_t)res.huf_bits;
    for (int k = 0; k < 3; k++) D->al[k] = res.al[k];
  }
  D->d_self = (const uint8_t**)(D->d_buf + self_at);
  HIPCHK(hipMemcpy(D->d_self, &D->d_content, sizeof(const uint8_t*), hipMemcpyHostToDevice));
  h->p = std::move(D);
  *out = hold.release();
  return ZD_OK;
}

void zd_dict_destroy(zd_dict* d) { delete d; }

int zd_dict_info(const zd_dict* d, uint32_t* dict_id, uint64_t* content_size, uint64_t rep[3], int* raw_content) {
  if (!d || !d->p) return ZD_E_INVALID_ARG;
  if (dict_id) *dict_id = d->p->id;
  if (content_size) *content_size = d->p->content;
  if (rep) for (int k = 0; k < 3; k++) rep[k] = d->p->rep[k];
  if (raw_content) *raw_content = d->p->raw ? 1 : 0;
  return ZD_OK;
}

int zd_plan_create_dict(const uint8_t* src, size_t n, uint32_t flags, const zd_dict* dict, zd_plan** out) {
  if (!out || (!src && n)) return ZD_E_INVALID_ARG;
  if (!dict) return plan_create(src, nullptr, n, flags, nullptr, out, 0);
  if (!dict->p) return ZD_E_INVALID_ARG;
  int dev = -1;
  HIPCHK(hipGetDevice(&dev));
  if (dev != dict->p->dev) return ZD_E_INVALID_ARG;
  return plan_create(src, nullptr, n, flags, nullptr, out, 0, dict->p);
}

int zd_decompress_dict(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, uint32_t flags,
                       const zd_dict* dict) {
  zd_plan* P = nullptr;
  int r = zd_plan_create_dict(src, n, flags, dict, &P);
  if (r) return r;
  r = zd_plan_decompress(P, src, n, dst, cap, out_len);
  zd_plan_destroy(P);
  return r;
}

// ---------------------------------------------------------------------------
// Dictionary sets
// ---------------------------------------------------------------------------
int zd_dict_set_create(const zd_dict* const* dicts, size_t ndicts, int fallback, zd_dict_set** out) {
  // ---- argument checks: no HIP call before they are done ----
  if (!dicts || !out || !ndicts || ndicts > ZD_DICT_SET_MAX) return ZD_E_INVALID_ARG;
  if (fallback < -1 || (fallback >= 0 && (size_t)fallback >= ndicts)) return ZD_E_INVALID_ARG;
  for (size_t i = 0; i < ndicts; i++) {
    if (!dicts[i] || !dicts[i]->p) return ZD_E_INVALID_ARG;
    if (dicts[i]->p->dev != dicts[0]->p->dev) return ZD_E_INVALID_ARG;
    // a raw-content dictionary (ID 0) that is not the fallback: no frame can name it
    if (dicts[i]->p->id == 0 && (int)i != fallback) return ZD_E_INVALID_ARG;
  }
  std::vector<size_t> order(ndicts);
  for (size_t i = 0; i < ndicts; i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
    return dicts[a]->p->id != dicts[b]->p->id ? dicts[a]->p->id < dicts[b]->p->id : a < b;
  });
  for (size_t k = 1; k < ndicts; k++)
    if (dicts[order[k]]->p->id == dicts[order[k - 1]]->p->id) return ZD_E_INVALID_ARG;   // (ID 0: at most the fallback)
  std::shared_ptr<DictSetData> D(new (std::nothrow) DictSetData());
  zd_dict_set* h = new (std::nothrow) zd_dict_set();
  if (!D || !h) { delete h; return ZD_E_NO_MEMORY; }
  std::unique_ptr<zd_dict_set> hold(h);
  D->fallback_arg = fallback;
  for (size_t k = 0; k < ndicts; k++) {
    if ((int)order[k] == fallback) D->fallback = (int)k;
    D->d.push_back(dicts[order[k]]->p);
  }
  HIPCHK(hipGetDevice(&D->dev));
  if (D->dev != D->d[0]->dev) return ZD_E_INVALID_ARG;
  HIPCHK(hipMalloc(&D->d_none_buf, 2 * DICT_PAD));
  HIPCHK(hipMemset(D->d_none_buf, 0, 2 * DICT_PAD));
  h->p = std::move(D);
  *out = hold.release();
  return ZD_OK;
}

void zd_dict_set_destroy(zd_dict_set* set) { delete set; }

int zd_dict_set_info(const zd_dict_set* set, size_t* ndicts, int* fallback) {
  if (!set || !set->p) return ZD_E_INVALID_ARG;
  if (ndicts) *ndicts = set->p->d.size();
  if (fallback) *fallback = set->p->fallback_arg;
  return ZD_OK;
}

int zd_plan_create_dicts(const uint8_t* src, size_t n, uint32_t flags, const zd_dict_set* set, zd_plan** out) {
  if (!out || (!src && n) || !set || !set->p) return ZD_E_INVALID_ARG;
  int dev = -1;
  HIPCHK(hipGetDevice(&dev));
  if (dev != set->p->dev) return ZD_E_INVALID_ARG;
  return plan_create(src, nullptr, n, flags, nullptr, out, 0, nullptr, set->p);
}

int zd_decompress_dicts(const uint8_t* src, size_t n, uint8_t* dst, size_t cap, size_t* out_len, uint32_t flags,
                        const zd_dict_set* set) {
  zd_plan* P = nullptr;
  int r = zd_plan_create_dicts(src, n, flags, set, &P);
  if (r) return r;
  r = zd_plan_decompress(P, src, n, dst, cap, out_len);
  zd_plan_destroy(P);
  return r;
}

}  // extern "C"

// ===========================================================================
// Batches of scattered chunks (zd_batch_create): the chunks, copied into one
// buffer the batch owns, are the frames of one plan over that buffer -- chunk
// i is frame i -- whose frames are placed at the chunks' own destinations
// (PlanCtx::place_out) and never stop one another.
// ===========================================================================
struct zd_batch {
  zd_plan* P = nullptr;                  // null: a batch of no chunks
  size_t n = 0;
  uint32_t flags = 0;
  std::shared_ptr<DictData> dict;
  std::shared_ptr<DictSetData> dset;     // zd_batch_create_dicts (never with `dict`)
  int dev = -1;
  uint8_t* d_gather = nullptr;           // the chunks' copies, 16-byte aligned, zero bytes between them
  uint64_t gather_alloc = 0;
  uint8_t* outbase = nullptr;            // the lowest destination
  uint8_t* d_arr = nullptr;              // one allocation for the arrays below
  uint64_t arr_bytes = 0;
  uint64_t *d_src = nullptr, *d_size = nullptr, *d_off = nullptr, *d_out = nullptr;   // ChunkList, output offsets
  GatherPiece* d_pieces = nullptr;
  uint64_t *d_boff = nullptr, *d_len = nullptr, *d_hash = nullptr;
  int32_t* d_status = nullptr;
  uint32_t* d_nblk = nullptr;
  uint8_t* d_bind = nullptr;
  std::vector<uint64_t> goff, src_size, dst, dst_cap;
  // a batch made from device arrays (zd_batch_create_device): the four vectors
  // above stay empty until a call needs them (host_arrays), d_arr holds the
  // chunks' capacities, first pieces and CHUNK_* flags too
  bool device_built = false;
  uint64_t *d_cap = nullptr, *d_piece0 = nullptr;
  uint8_t* d_flag = nullptr;
  uint64_t *d_scratch = nullptr, *d_res = nullptr;   // creation's scans and the words that come back
  // a packed batch (zd_batch_create_device_packed): d_out / d_cap are its own
  // layout, outbase the bound buffer (zd_batch_bind_output; null until then)
  bool packed = false;
  uint64_t out_bytes = 0;
  // a prefix batch made from device arrays (zd_batch_create_device_prefix):
  // the checked prefix addresses and sizes, in d_arr
  uint64_t *d_pfx = nullptr, *d_pfx_bytes = nullptr;
  // a chain batch (zd_batch_create_chain): the chunks' checked parents, the
  // chunks grouped by level and (device arrays) the kernels' counters and
  // levels, in d_arr; the levels' counts up to the last one in use, the links
  bool chain = false;
  int32_t* d_par = nullptr;
  uint32_t *d_order = nullptr, *d_lcount = nullptr;
  uint8_t* d_lvl = nullptr;
  std::vector<uint32_t> chain_count;
  uint64_t chain_links = 0;
  int host_arrays() {
    if (!device_built || goff.size() == n) return 0;
    std::vector<uint64_t> o(n), z(n), d(n), c(n);
    if (hipMemcpy(o.data(), d_off, 8 * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(z.data(), d_size, 8 * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(d.data(), d_out, 8 * n, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(c.data(), d_cap, 8 * n, hipMemcpyDeviceToHost) != hipSuccess) {
      (void)hipGetLastError();
      return ZD_E_HIP;
    }
    // (a chunk without a destination has capacity 0: any address serves)
    for (size_t i = 0; i < n; i++) d[i] += (uint64_t)(uintptr_t)outbase;
    goff = std::move(o); src_size = std::move(z); dst = std::move(d); dst_cap = std::move(c);
    return 0;
  }
  std::vector<int32_t> h_status;         // the last zd_batch_results
  std::vector<uint64_t> h_len;
  bool have_results = false;
  bool launched = false;
  zd_batch_info info{};
};

extern "C" {

void zd_batch_destroy(zd_batch* B) {
  if (!B) return;
  if (B->P) zd_plan_destroy(B->P);        // (waits for the work the batch launched)
  ws_release(B->d_gather, B->gather_alloc, B->dev);
  if (B->d_arr) (void)hipFree(B->d_arr);
  delete B;
}

// What a batch is made from: every zd_batch_create* entry point fills one.
struct BatchSpec {
  // one entry a chunk: host arrays, or with on_device device arrays readable on `stream`
  const void* const* src = nullptr;
  const uint64_t* src_bytes = nullptr;
  void* const* dst = nullptr;              // (both null: a packed batch)
  const uint64_t* dst_cap = nullptr;
  const void* const* prefix = nullptr;     // (both null: no prefixes)
  const uint64_t* prefix_bytes = nullptr;
  const int64_t* parent = nullptr;         // a chain batch (the prefix arrays may then both be null); else null
  bool on_device = false;
  size_t n = 0;
  uint32_t flags = 0;
  uint32_t align = 0;                      // a packed batch's alignment (device arrays only); 0: not packed
  std::shared_ptr<DictData> dict;          // one dictionary, a set, prefixes, or none of them
  std::shared_ptr<DictSetData> dset;
  hipStream_t stream = nullptr;
  bool packed() const { return align != 0; }
  bool chain = false;                      // made by a chain call (parent null only with n == 0)
  bool with_prefix() const { return prefix || prefix_bytes || chain; }
};
// (an entry point's handles: false for one without data)
static bool spec_dicts(BatchSpec& S, const zd_dict* dict, const zd_dict_set* set) {
  if ((dict && !dict->p) || (set && !set->p)) return false;
  if (dict) S.dict = dict->p;
  if (set) S.dset = set->p;
  return true;
}

struct Drop { void operator()(zd_batch* b) const { zd_batch_destroy(b); } };

// d_arr and every array in it, as carved
static int batch_arrays(zd_batch* B, const BatchCarve& C) {
  B->arr_bytes = C.total;
  HIPCHK(hipMalloc(&B->d_arr, B->arr_bytes));
  const auto at = [&](uint64_t o) { return o == BatchCarve::ABSENT ? nullptr : B->d_arr + o; };
  B->d_src = (uint64_t*)at(C.src); B->d_size = (uint64_t*)at(C.size); B->d_off = (uint64_t*)at(C.off);
  B->d_out = (uint64_t*)at(C.out);
  B->d_pieces = (GatherPiece*)at(C.pieces);
  static_assert(sizeof(GatherPiece) == 8, "GatherPiece: one u64 slot");
  B->d_boff = (uint64_t*)at(C.boff); B->d_len = (uint64_t*)at(C.len); B->d_hash = (uint64_t*)at(C.hash);
  B->d_status = (int32_t*)at(C.status);
  B->d_nblk = (uint32_t*)at(C.nblk);
  B->d_bind = at(C.bind);
  B->d_piece0 = (uint64_t*)at(C.piece0); B->d_cap = (uint64_t*)at(C.cap);
  B->d_flag = at(C.flag);
  B->d_scratch = (uint64_t*)at(C.scratch); B->d_res = (uint64_t*)at(C.res);
  B->d_pfx = (uint64_t*)at(C.pfx); B->d_pfx_bytes = (uint64_t*)at(C.pfx_bytes);
  B->d_par = (int32_t*)at(C.par); B->d_order = (uint32_t*)at(C.order); B->d_lcount = (uint32_t*)at(C.lcount);
  B->d_lvl = at(C.lvl);
  return 0;
}

// Host arrays: every entry is checked here, and a bad one fails the call
static int check_entries(const BatchSpec& S) {
  std::vector<std::pair<uint64_t, uint64_t>> ranges;      // destinations of at least one byte
  for (size_t i = 0; i < S.n; i++) {
    if ((!S.src[i] && S.src_bytes[i]) || (!S.dst[i] && S.dst_cap[i])) return ZD_E_INVALID_ARG;
    const uint64_t a = (uint64_t)(uintptr_t)S.dst[i];
    if (a + S.dst_cap[i] < a || (uint64_t)(uintptr_t)S.src[i] + S.src_bytes[i] < (uint64_t)(uintptr_t)S.src[i])
      return ZD_E_INVALID_ARG;
    if (S.dst_cap[i]) ranges.push_back({a, S.dst_cap[i]});
  }
  std::sort(ranges.begin(), ranges.end());
  for (size_t k = 1; k < ranges.size(); k++)
    if (ranges[k].first < ranges[k - 1].first + ranges[k - 1].second) return ZD_E_INVALID_ARG;
  // a prefix is read while the destinations are written: no prefix range may
  // meet one (the sorted destinations are disjoint, so of those that start
  // below the prefix's end the last one reaches furthest)
  // (a chain batch: the external prefixes only -- a chained chunk's prefix IS
  // its parent's destination, complete before the chunk's level starts)
  for (size_t i = 0; S.prefix && i < S.n; i++) {
    const uint64_t a = (uint64_t)(uintptr_t)S.prefix[i], z = S.prefix_bytes[i];
    if (S.chain && S.parent[i] != -1 && z) return ZD_E_INVALID_ARG;
    if ((!a && z) || a + z < a) return ZD_E_INVALID_ARG;
    if (!z) continue;
    auto it = std::lower_bound(ranges.begin(), ranges.end(), std::pair<uint64_t, uint64_t>{a + z, 0});
    if (it != ranges.begin() && (it - 1)->first + (it - 1)->second > a) return ZD_E_INVALID_ARG;
  }
  return 0;
}

// What the phases of a creation from host arrays hand on
struct HostArrays {
  std::vector<uint64_t> head;        // d_arr's uploaded head (kept to the end of the call)
  const uint64_t* out = nullptr;     //   its out column: the plan's place_out
  std::vector<uint8_t> bind;         // the capacity pass's flags, uploaded after the descriptors
  std::vector<uint32_t> chain;       // a chain batch: the parents (i32) | the chunks by level, one upload behind the head
};

// Host arrays of a chain batch: every parent entry is checked here (zd_chain.h:
// an index outside [-1, n), a chunk that names itself, a cycle, more than
// ZD_CHAIN_MAX_DEPTH ancestors fail the call), the chunks are grouped by level.
static int chain_host(const BatchSpec& S, zd_batch* B, HostArrays& H) {
  const size_t n = S.n;
  std::vector<int32_t> level(n);
  uint32_t count[CHAIN_LEVELS];
  H.chain.resize(2 * n);
  if (chain_order(S.parent, n, level.data(), H.chain.data() + n, count)) return ZD_E_INVALID_ARG;
  uint32_t levels = 1;
  for (size_t i = 0; i < n; i++) {
    H.chain[i] = (uint32_t)(int32_t)S.parent[i];
    B->chain_links += S.parent[i] >= 0;
    levels = std::max(levels, (uint32_t)level[i] + 1);
  }
  B->chain_count.assign(count, count + levels);
  return 0;
}

// Host arrays: the gathered layout and zd_k_gather's pieces, made here and
// uploaded as d_arr's head; then the gather.  info.gathered_bytes is set.
static int gather_host(const BatchSpec& S, zd_batch* B, HostArrays& H) {
  const size_t n = S.n;
  const hipStream_t s = S.stream;
  B->goff.resize(n);
  B->src_size.assign(S.src_bytes, S.src_bytes + n);
  B->dst.resize(n);
  B->dst_cap.assign(S.dst_cap, S.dst_cap + n);
  uint64_t total = 0, npieces = 0;
  uint64_t lowest = UINT64_MAX;
  for (size_t i = 0; i < n; i++) {
    B->goff[i] = total;
    total += align_up(S.src_bytes[i], 16) + ZD_SRC_PADDING;
    npieces += std::max<uint64_t>(1, (S.src_bytes[i] + COPY_PIECE - 1) / COPY_PIECE);
    B->dst[i] = (uint64_t)(uintptr_t)S.dst[i];
    if (S.dst[i]) lowest = std::min(lowest, B->dst[i]);
  }
  if (lowest == UINT64_MAX) lowest = 0;
  if (npieces * (COPY_PIECE / 4096) >= (1ull << 31)) return ZD_E_OUT_OF_DOMAIN;   // zd_k_gather's grid
  B->outbase = (uint8_t*)(uintptr_t)lowest;
  BatchCarve C;
  C.carve(n, false, npieces, false, S.chain);
  std::vector<uint64_t>& head = H.head;
  head.resize(C.head_bytes / 8);
  uint64_t *h_src = head.data() + C.src / 8, *h_size = head.data() + C.size / 8, *h_off = head.data() + C.off / 8,
           *h_out = head.data() + C.out / 8;
  for (size_t i = 0; i < n; i++) {
    h_src[i] = (uint64_t)(uintptr_t)S.src[i];
    h_size[i] = S.src_bytes[i];
    h_off[i] = B->goff[i];
    h_out[i] = S.dst[i] ? B->dst[i] - lowest : 0;
  }
  H.out = h_out;
  {
    GatherPiece* gp = (GatherPiece*)(head.data() + C.pieces / 8);
    uint64_t k = 0;
    for (size_t i = 0; i < n; i++) {
      const uint64_t np = std::max<uint64_t>(1, (S.src_bytes[i] + COPY_PIECE - 1) / COPY_PIECE);
      if (np >= (1ull << 32)) return ZD_E_OUT_OF_DOMAIN;
      for (uint64_t q = 0; q < np; q++) gp[k++] = GatherPiece{(uint32_t)i, (uint32_t)q};
    }
  }
  if (int r = batch_arrays(B, C)) return r;
  HIPCHK(ws_alloc(B->dev, std::max<uint64_t>(total, 16), &B->d_gather, &B->gather_alloc));
  HIPCHK(hipMemcpyAsync(B->d_arr, head.data(), C.head_bytes, hipMemcpyHostToDevice, s));
  HIPCHK(hipMemsetAsync(B->d_arr + C.head_bytes, 0, C.total - C.head_bytes, s));
  if (S.chain) {                             // (par | order: adjacent in d_arr)
    if ((uint8_t*)B->d_order != (uint8_t*)B->d_par + 4 * n) return ZD_E_INVALID_ARG;
    HIPCHK(hipMemcpyAsync(B->d_par, H.chain.data(), 8 * n, hipMemcpyHostToDevice, s));
  }
  HIPCHK(launch_gather(ChunkList{B->d_src, B->d_size, B->d_off}, B->d_gather, B->d_pieces, npieces, s));
  HIPCHK(hipStreamSynchronize(s));
  B->info.gathered_bytes = total;
  return 0;
}

// Device arrays: zd_k_batch_layout checks the entries (a bad one fails its
// own chunk), lays the gathered buffer out and finds the lowest destination;
// the totals come back, then the gather over the scanned piece starts.  `lk`
// (WB.m) is taken here and held to the end of the call: the rest of the
// creation reads through WB's pinned words and device buffers.
static int gather_device(const BatchSpec& S, zd_batch* B, DevWalkBufs& WB, std::unique_lock<std::mutex>& lk) {
  const size_t n = S.n;
  const hipStream_t s = S.stream;
  BatchCarve C;
  C.carve(n, true, 0, S.with_prefix(), S.chain);
  if (int r = batch_arrays(B, C)) return r;
  HIPCHK(hipMemsetAsync(B->d_arr, 0, B->arr_bytes, s));
  lk.lock();
  walk_bufs_on(WB, B->dev);
  if (!WB.h_small && hipHostMalloc((void**)&WB.h_small, 64 * 8, hipHostMallocDefault) != hipSuccess) return ZD_E_HIP;
  constexpr size_t LCOUNT = 2 * CHAIN_LEVELS + 2;
  if (S.chain && !WB.h_chain && hipHostMalloc((void**)&WB.h_chain, 4 * LCOUNT, hipHostMallocDefault) != hipSuccess)
    return ZD_E_HIP;
  const BatchArrays A{B->d_src, B->d_size, B->d_off, B->d_piece0, B->d_out, B->d_cap, B->d_flag, B->d_pfx, B->d_pfx_bytes};
  HIPCHK(launch_batch_layout((const uint64_t*)S.src, S.src_bytes, (const uint64_t*)S.dst, S.dst_cap, (uint32_t)n, A,
                             B->d_scratch, B->d_res, s, (const uint64_t*)S.prefix, S.prefix_bytes));
  if (S.chain) {
    // the parents checked, the levels and the chunks grouped by them; the
    // levels' counts come back with the layout's totals (no wait of their own)
    HIPCHK(launch_chain_levels(S.parent, (uint32_t)n, B->d_flag, B->d_pfx, B->d_pfx_bytes,
                               (unsigned long long*)(B->d_res + 3), B->d_par, B->d_lvl, B->d_order, B->d_lcount, s));
    HIPCHK(hipMemcpyAsync(WB.h_chain, B->d_lcount, 4 * LCOUNT, hipMemcpyDeviceToHost, s));
  }
  HIPCHK(hipMemcpyAsync(WB.h_small, B->d_res, 4 * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (S.chain) {
    uint32_t levels = 1;
    for (uint32_t l = 0; l < CHAIN_LEVELS; l++)
      if (WB.h_chain[l]) levels = l + 1;
    B->chain_count.assign(WB.h_chain, WB.h_chain + levels);
    B->chain_links = WB.h_chain[2 * CHAIN_LEVELS];
  }
  const uint64_t total = WB.h_small[0], npieces = WB.h_small[1];
  if (S.with_prefix()) B->info.prefix_bytes_total = WB.h_small[3];
  B->outbase = (uint8_t*)(uintptr_t)WB.h_small[2];
  if (npieces * (COPY_PIECE / 4096) >= (1ull << 31)) return ZD_E_OUT_OF_DOMAIN;   // zd_k_gather's grid
  HIPCHK(ws_alloc(B->dev, std::max<uint64_t>(total, 16), &B->d_gather, &B->gather_alloc));
  HIPCHK(launch_gather_scan(ChunkList{B->d_src, B->d_size, B->d_off}, B->d_gather, B->d_piece0, (uint32_t)n, npieces, s));
  HIPCHK(hipStreamSynchronize(s));             // (the sources may be released from here on; gather_ns ends here)
  B->info.gathered_bytes = total;
  return 0;
}

// zd_k_walk_chunks' count pass: d_nblk[i] = the blocks chunk i's walk keeps
static int walk_count(zd_batch* B, hipStream_t s) {
  HIPCHK(launch_walk_chunks(B->d_gather, ChunkList{B->d_src, B->d_size, B->d_off}, (uint32_t)B->n, B->P->walk_opts(),
                            B->d_nblk, nullptr, nullptr, nullptr, false, s));
  return 0;
}
// zd_k_walk_chunks' fill pass over NB blocks in all, into WB.d_out (frames |
// blocks).  h_boff: the blocks' places where the host summed them, uploaded
// here with room made for the index's pinned copy; null: scanned in d_boff.
static int walk_fill(zd_batch* B, DevWalkBufs& WB, uint64_t NB, const uint64_t* h_boff, hipStream_t s) {
  const size_t n = B->n;
  if (NB >= (1ull << 32)) return ZD_E_OUT_OF_DOMAIN;
  const size_t fb = align_up(n * sizeof(HostFrame), 256), bytes = fb + NB * sizeof(HostBlock);
  if (!grow_dev(WB.d_out, WB.cap_out, bytes) || (h_boff && !grow_pinned(WB.h_out, WB.cap_h, bytes))) return ZD_E_HIP;
  WB.fb = fb;
  WB.bytes = bytes;
  if (h_boff) HIPCHK(hipMemcpyAsync(B->d_boff, h_boff, 8 * n, hipMemcpyHostToDevice, s));
  HIPCHK(launch_walk_chunks(B->d_gather, ChunkList{B->d_src, B->d_size, B->d_off}, (uint32_t)n, B->P->walk_opts(),
                            B->d_nblk, B->d_boff, (HostFrame*)WB.d_out, (HostBlock*)(WB.d_out + fb), true, s));
  return 0;
}

// Host arrays: the walk with the blocks' places summed on the host, the index
// back through the pinned copy, the capacity pass (zd_walk.h chunk_fit; bind
// goes up with the descriptors) and the plan's parts.
static int index_host(const BatchSpec& S, zd_batch* B, DevWalkBufs& WB, HostArrays& H) {
  const size_t n = S.n;
  const hipStream_t s = S.stream;
  zd_plan* P = B->P;
  H.bind.assign(n, 0);
  P->place_out.assign(H.out, H.out + n);
  P->place_cap = B->dst_cap;
  std::lock_guard<std::mutex> lk(WB.m);
  walk_bufs_on(WB, B->dev);
  if (int r = walk_count(B, s)) return r;
  std::vector<uint32_t> nblk(n);
  HIPCHK(hipMemcpyAsync(nblk.data(), B->d_nblk, 4 * n, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  std::vector<uint64_t> boff(n);
  uint64_t NB = 0;
  for (size_t i = 0; i < n; i++) { boff[i] = NB; NB += nblk[i]; }
  if (int r = walk_fill(B, WB, NB, boff.data(), s)) return r;
  const HostFrame* cfr = nullptr;
  const HostBlock* bl = nullptr;
  if (int r = dev_walk_download(WB, s, &cfr, &bl)) return r;
  HostFrame* fr = (HostFrame*)WB.h_out;
  std::vector<const HostFrame*> kept(n);
  for (size_t i = 0; i < n; i++) {
    HostFrame& hf = fr[i];
    kept[i] = &hf;
    if (hf.d.kind == ZD_FRAME_ZSTD && hf.key == KEY_NONE) H.bind[i] = chunk_fit(hf, bl, S.dst_cap[i]);
  }
  // a chain batch: the chained chunks' prefix entries, now that the walk has
  // the parents' Frame_Content_Sizes and before the planner reads them
  for (size_t i = 0; S.chain && i < n; i++) {
    const int64_t p = S.parent[i];
    if (p < 0) continue;
    uint64_t z = 0;
    if (!chain_prefix_bytes(fr[p], &z)) chain_no_prefix_size(fr[i]);
    P->prefix_bytes[i] = z;
    P->prefix_ptrs[i] = z ? B->dst[p] : 0;
  }
  std::vector<HostPart> parts;
  parts_from(kept, bl, parts);
  P->set_parts(std::move(parts));
  return 0;
}

// Device arrays: the walk with the blocks' places scanned in d_boff; a packed
// batch's own capacities and places (zd_k_batch_pack and one scan); a set's
// IDs up, in `set_mem` with room for the plan's table and the used flags; then
// the capacity pass, zd_k_batch_fit.  `in`: what build_plan_device takes over.
static int index_device(const BatchSpec& S, zd_batch* B, DevWalkBufs& WB, DevPlanIn& in,
                        std::unique_ptr<void, Free>& set_mem) {
  const size_t n = S.n;
  const hipStream_t s = S.stream;
  const uint64_t nt = (n + 255) / 256;
  if (int r = walk_count(B, s)) return r;
  HIPCHK(launch_scan64(B->d_boff, B->d_nblk, n, 1, n, B->d_scratch, s));
  HIPCHK(hipMemcpyAsync(WB.h_small, B->d_scratch + nt, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (int r = walk_fill(B, WB, WB.h_small[0], nullptr, s)) return r;
  HostFrame* d_frames = (HostFrame*)WB.d_out;
  const HostBlock* d_blocks = (const HostBlock*)(WB.d_out + WB.fb);
  if (S.packed()) {
    // the chunks' reserves and places; the total comes back with the routing shape (build_plan_device's
    // first wait), in a pinned word the planner does not use
    HIPCHK(launch_batch_pack(d_frames, d_blocks, B->d_flag, (uint32_t)n, S.align, B->d_cap, B->d_out, s));
    HIPCHK(launch_scan64(B->d_out, nullptr, n, 1, n, B->d_scratch, s));
    HIPCHK(hipMemcpyAsync(WB.h_small + 63, B->d_scratch + nt, 8, hipMemcpyDeviceToHost, s));
  }
  in.place_out = B->d_out;
  in.place_cap = B->d_cap;
  // a dictionary set: its IDs go up, the used flags of its entries come back with the routing shape
  const uint32_t* d_ids = nullptr;
  uint32_t nset = 0;
  if (B->dset) {
    const DictSetData& D = *B->dset;
    nset = (uint32_t)D.d.size();
    const uint64_t m = std::max<uint32_t>(nset, 1);
    void* p = nullptr;
    HIPCHK(hipMalloc(&p, m * (sizeof(PlanDict) + 4 + 1)));      // table | IDs | used flags
    set_mem.reset(p);
    in.d_dset = (PlanDict*)p;
    uint32_t* ids = (uint32_t*)(in.d_dset + m);
    uint8_t* used = (uint8_t*)(ids + m);
    std::vector<uint32_t> h_ids(m, 0);
    for (uint32_t k = 0; k < nset; k++) h_ids[k] = D.d[k]->id;
    HIPCHK(hipMemcpy(ids, h_ids.data(), 4 * m, hipMemcpyHostToDevice));
    HIPCHK(hipMemsetAsync(used, 0, m, s));
    d_ids = ids;
    in.d_used = used;
  }
  HIPCHK(launch_batch_fit(d_frames, d_blocks, B->d_cap, B->d_flag, (uint32_t)n, B->d_bind, d_ids, nset,
                          B->dset ? B->dset->fallback : -1, (uint8_t*)in.d_used, s));
  // a chain batch: the chained chunks' prefix entries, before the planner reads them
  if (S.chain)
    HIPCHK(launch_chain_prefix(d_frames, B->d_par, B->d_out, B->outbase, (uint32_t)n, B->d_pfx, B->d_pfx_bytes, s));
  return 0;
}

// Every batch is made here.  With device arrays the host reads back only a
// few words a phase (the layout's totals, the block count, the routing shape
// and a set's used flags, the plan's totals) and the frames' output offsets
// and capacities.
static int batch_create(const BatchSpec& S, zd_batch** out) {
  // ---- argument checks: no HIP call before they are done ----
  const size_t n = S.n;
  if (!out || (S.flags & ZD_F_SKIPPABLE) || n >= (1ull << 31)) return ZD_E_INVALID_ARG;
  if (n && (!S.src || !S.src_bytes || (!S.packed() && (!S.dst || !S.dst_cap)))) return ZD_E_INVALID_ARG;
  if (S.packed() && (!S.on_device || S.dst || S.dst_cap)) return ZD_E_INVALID_ARG;
  // (a chain batch may come without external prefixes: both arrays null)
  if (S.with_prefix() && (S.dict || S.dset || S.packed() ||
                          (n && (S.chain ? !S.prefix != !S.prefix_bytes || !S.parent : !S.prefix || !S.prefix_bytes))))
    return ZD_E_INVALID_ARG;
  if (!S.on_device)
    if (int r = check_entries(S)) return r;

  // ---- the batch; one of no chunks is done here ----
  zd_batch* B = new (std::nothrow) zd_batch();
  if (!B) return ZD_E_NO_MEMORY;
  std::unique_ptr<zd_batch, Drop> hold(B);
  B->n = n;
  B->flags = S.flags;
  B->device_built = S.on_device;
  B->packed = S.packed();
  B->info.nchunks = n;
  B->info.device_built = S.on_device;
  B->chain = S.chain;
  if (!n) { *out = hold.release(); return ZD_OK; }
  HostArrays H;
  if (S.chain && !S.on_device)                // (the last of the argument checks)
    if (int r = chain_host(S, B, H)) return r;
  HIPCHK(hipGetDevice(&B->dev));
  if ((S.dict && S.dict->dev != B->dev) || (S.dset && S.dset->dev != B->dev)) return ZD_E_INVALID_ARG;
  B->dict = S.dict;
  B->dset = S.dset;
  DevWalkBufs& WB = dev_walk_bufs();
  std::unique_lock<std::mutex> lk(WB.m, std::defer_lock);   // (gather_device takes it, to the end of the call)
  const auto t0 = std::chrono::steady_clock::now();

  // ---- the gathered layout, the chunks' copies ----
  if (int r = S.on_device ? gather_device(S, B, WB, lk) : gather_host(S, B, H)) return r;
  const auto t1 = std::chrono::steady_clock::now();

  // ---- the plan; zd_k_walk_chunks: count, the blocks' places, fill; the capacity pass ----
  zd_plan* P = new (std::nothrow) zd_plan();
  if (!P) return ZD_E_NO_MEMORY;
  B->P = P;
  P->flags = S.flags;
  P->dict = B->dict;
  P->dset = B->dset;
  P->prefix = S.with_prefix();
  if (P->prefix && S.on_device) {           // the checked entries, in the batch's own arrays
    P->d_prefix_ptrs = B->d_pfx;
    P->d_prefix_bytes = B->d_pfx_bytes;
  } else if (P->prefix) {
    P->prefix_ptrs.assign(n, 0);
    P->prefix_bytes.assign(n, 0);            // (a chained chunk's entry: index_host, from its parent's frame)
    for (size_t i = 0; S.prefix && i < n; i++) {
      P->prefix_bytes[i] = S.prefix_bytes[i];
      P->prefix_ptrs[i] = S.prefix_bytes[i] ? (uint64_t)(uintptr_t)S.prefix[i] : 0;
      B->info.prefix_bytes_total += S.prefix_bytes[i];
    }
  }
  if (S.chain) {
    P->chain = true;
    P->d_chain_order = B->d_order;
    P->d_chain_parent = B->d_par;
    P->chain_count = B->chain_count;
    // ZD_F_CHAIN_BLOCK_PARALLEL, ZD_F_AUTO_EXECUTOR: what the planners number the J frames level-major from
    if (P->chain_on_j()) {
      if (S.on_device) P->d_chain_lcount = B->d_lcount;
      else P->h_chain_order.assign(H.chain.begin() + n, H.chain.end());
    }
  }
  DevPlanIn in;                            // device arrays
  std::unique_ptr<void, Free> set_mem;
  if (int r = S.on_device ? index_device(S, B, WB, in, set_mem) : index_host(S, B, WB, H)) return r;
  P->index_status = 0;
  const auto t2 = std::chrono::steady_clock::now();

  // ---- descriptors (zd_k_plan_*, or the host planner), placed at the chunks' destinations ----
  if (int r = S.on_device ? build_plan_device(P, WB, n, S.stream, &in) : build_plan_staged(P)) return r;
  if (S.packed()) B->out_bytes = WB.h_small[63];
  P->index_stop = P->nframes;
  P->info.src_bytes = B->info.gathered_bytes;
  const auto t3 = std::chrono::steady_clock::now();

  // ---- what the host planner leaves to upload; the dictionaries' tables; the second stream ----
  if (!S.on_device)
    if (int r = upload_desc(P)) return r;
  if (int r = upload_dict_tables(P)) return r;
  if (!S.on_device) HIPCHK(hipMemcpy(B->d_bind, H.bind.data(), n, hipMemcpyHostToDevice));
  if (!aux_take(P)) return ZD_E_HIP;
  const auto t4 = std::chrono::steady_clock::now();
  zd_batch_info& I = B->info;
  I.nblocks = P->info.nblocks;
  I.nsequences = P->info.nsequences;
  I.workspace_bytes = P->W.total + B->arr_bytes;
  I.executors = P->info.executors;
  // (in.alloc_ns: the device planner's workspace allocation and small uploads count as upload)
  I.gather_ns = ns(t0, t1);
  I.walk_ns = ns(t1, t2);
  I.host_ns = ns(t2, t3) - std::min(in.alloc_ns, ns(t2, t3));
  I.upload_ns = ns(t3, t4) + in.alloc_ns;
  *out = hold.release();
  return ZD_OK;
}

int zd_batch_create(const void* const* d_src, const uint64_t* src_bytes, void* const* d_dst, const uint64_t* dst_cap,
                    size_t nchunks, uint32_t flags, const zd_dict* dict, void* stream, zd_batch** out) {
  BatchSpec S{d_src, src_bytes, d_dst, dst_cap};
  S.n = nchunks; S.flags = flags; S.stream = (hipStream_t)stream;
  if (!spec_dicts(S, dict, nullptr)) return ZD_E_INVALID_ARG;
  return batch_create(S, out);
}

int zd_batch_create_prefix(const void* const* d_src, const uint64_t* src_bytes, void* const* d_dst,
                           const uint64_t* dst_cap, const void* const* d_prefix, const uint64_t* prefix_bytes,
                           size_t nchunks, uint32_t flags, void* stream, zd_batch** out) {
  if (nchunks && (!d_prefix || !prefix_bytes)) return ZD_E_INVALID_ARG;
  BatchSpec S{d_src, src_bytes, d_dst, dst_cap, d_prefix, prefix_bytes};
  S.n = nchunks; S.flags = flags; S.stream = (hipStream_t)stream;
  return batch_create(S, out);
}

int zd_batch_create_dicts(const void* const* d_src, const uint64_t* src_bytes, void* const* d_dst,
                          const uint64_t* dst_cap, size_t nchunks, uint32_t flags, const zd_dict_set* set, void* stream,
                          zd_batch** out) {
  BatchSpec S{d_src, src_bytes, d_dst, dst_cap};
  S.n = nchunks; S.flags = flags; S.stream = (hipStream_t)stream;
  if (!set || !spec_dicts(S, nullptr, set)) return ZD_E_INVALID_ARG;
  return batch_create(S, out);
}

int zd_batch_create_device(const void* const* d_src_ptrs, const uint64_t* d_src_bytes, void* const* d_dst_ptrs,
                           const uint64_t* d_dst_cap, size_t nchunks, uint32_t flags, const zd_dict* dict, void* stream,
                           zd_batch** out) {
  BatchSpec S{d_src_ptrs, d_src_bytes, d_dst_ptrs, d_dst_cap};
  S.on_device = true; S.n = nchunks; S.flags = flags; S.stream = (hipStream_t)stream;
  if (!spec_dicts(S, dict, nullptr)) return ZD_E_INVALID_ARG;
  return batch_create(S, out);
}

int zd_batch_create_device_prefix(const void* const* d_src_ptrs, const uint64_t* d_src_bytes, void* const* d_dst_ptrs,
                                  const uint64_t* d_dst_cap, const void* const* d_prefix_ptrs,
                                  const uint64_t* d_prefix_bytes, size_t nchunks, uint32_t flags, void* stream,
                                  zd_batch** out) {
  if (nchunks && (!d_prefix_ptrs || !d_prefix_bytes)) return ZD_E_INVALID_ARG;
  BatchSpec S{d_src_ptrs, d_src_bytes, d_dst_ptrs, d_dst_cap, d_prefix_ptrs, d_prefix_bytes};
  S.on_device = true; S.n = nchunks; S.flags = flags; S.stream = (hipStream_t)stream;
  return batch_create(S, out);
}

int zd_batch_create_chain(const void* const* d_src, const uint64_t* src_bytes, void* const* d_dst,
                          const uint64_t* dst_cap, const void* const* d_prefix, const uint64_t* prefix_bytes,
                          const int64_t* parent, size_t nchunks, uint32_t flags, void* stream, zd_batch** out) {
  if (nchunks && !parent) return ZD_E_INVALID_ARG;
  BatchSpec S{d_src, src_bytes, d_dst, dst_cap, d_prefix, prefix_bytes, parent};
  S.chain = true; S.n = nchunks; S.flags = flags; S.stream = (hipStream_t)stream;
  return batch_create(S, out);
}

int zd_batch_create_device_chain(const void* const* d_src_ptrs, const uint64_t* d_src_bytes, void* const* d_dst_ptrs,
                                 const uint64_t* d_dst_cap, const void* const* d_prefix_ptrs,
                                 const uint64_t* d_prefix_bytes, const int64_t* d_parent, size_t nchunks,
                                 uint32_t flags, void* stream, zd_batch** out) {
  if (nchunks && !d_parent) return ZD_E_INVALID_ARG;
  BatchSpec S{d_src_ptrs, d_src_bytes, d_dst_ptrs, d_dst_cap, d_prefix_ptrs, d_prefix_bytes, d_parent};
  S.chain = true; S.on_device = true; S.n = nchunks; S.flags = flags; S.stream = (hipStream_t)stream;
  return batch_create(S, out);
}

int zd_batch_chain_info(const zd_batch* B, uint32_t* levels, uint64_t* links) {
  if (!B || !B->chain) return ZD_E_INVALID_ARG;
  if (levels) *levels = (uint32_t)std::max<size_t>(B->chain_count.size(), 1);
  if (links) *links = B->chain_links;
  return ZD_OK;
}

int zd_batch_create_device_dicts(const void* const* d_src_ptrs, const uint64_t* d_src_bytes, void* const* d_dst_ptrs,
                                 const uint64_t* d_dst_cap, size_t nchunks, uint32_t flags, const zd_dict_set* set,
                                 void* stream, zd_batch** out) {
  BatchSpec S{d_src_ptrs, d_src_bytes, d_dst_ptrs, d_dst_cap};
  S.on_device = true; S.n = nchunks; S.flags = flags; S.stream = (hipStream_t)stream;
  if (!set || !spec_dicts(S, nullptr, set)) return ZD_E_INVALID_ARG;
  return batch_create(S, out);
}

static bool pack_align_ok(uint32_t align) { return align && align <= 4096 && !(align & (align - 1)); }

int zd_batch_create_device_packed(const void* const* d_src_ptrs, const uint64_t* d_src_bytes, size_t nchunks,
                                  uint32_t align, uint32_t flags, const zd_dict* dict, void* stream, zd_batch** out) {
  BatchSpec S{d_src_ptrs, d_src_bytes};
  S.on_device = true; S.align = align; S.n = nchunks; S.flags = flags; S.stream = (hipStream_t)stream;
  if (!pack_align_ok(align) || !spec_dicts(S, dict, nullptr)) return ZD_E_INVALID_ARG;
  return batch_create(S, out);
}

int zd_batch_create_device_packed_dicts(const void* const* d_src_ptrs, const uint64_t* d_src_bytes, size_t nchunks,
                                        uint32_t align, uint32_t flags, const zd_dict_set* set, void* stream,
                                        zd_batch** out) {
  BatchSpec S{d_src_ptrs, d_src_bytes};
  S.on_device = true; S.align = align; S.n = nchunks; S.flags = flags; S.stream = (hipStream_t)stream;
  if (!set || !pack_align_ok(align) || !spec_dicts(S, nullptr, set)) return ZD_E_INVALID_ARG;
  return batch_create(S, out);
}

int zd_batch_output_layout(const zd_batch* B, uint64_t* out_bytes, const uint64_t** d_offset, const uint64_t** d_cap) {
  if (!B || !B->packed) return ZD_E_INVALID_ARG;
  if (out_bytes) *out_bytes = B->out_bytes;
  if (d_offset) *d_offset = B->d_out;
  if (d_cap) *d_cap = B->d_cap;
  return ZD_OK;
}

int zd_batch_bind_output(zd_batch* B, void* d_out, uint64_t cap) {
  if (!B || !B->packed) return ZD_E_INVALID_ARG;
  const uint64_t a = (uint64_t)(uintptr_t)d_out;
  if ((!d_out && B->out_bytes) || a + cap < a) return ZD_E_INVALID_ARG;
  if (cap < B->out_bytes) return ZD_E_DST_TOO_SMALL;
  B->outbase = (uint8_t*)d_out;
  B->goff.clear();                        // (host_arrays: the chunks' addresses follow the binding)
  return ZD_OK;
}

int zd_chunk_sizes_device(const void* const* d_src_ptrs, const uint64_t* d_src_bytes, size_t nchunks, uint32_t flags,
                          uint64_t* d_size, int32_t* d_status, uint8_t* d_exact, void* stream) {
  if ((flags & ~(ZD_SIZES_DICT | ZD_SIZES_LONG_WINDOW | ZD_SIZES_RFC | ZD_SIZES_MULTI_FRAME)) || nchunks >= (1ull << 31))
    return ZD_E_INVALID_ARG;
  if (nchunks && (!d_src_ptrs || !d_src_bytes || !d_size)) return ZD_E_INVALID_ARG;
  if (!nchunks) return ZD_OK;
  const uint32_t wopt = walk_opts((flags & ZD_SIZES_DICT) != 0, (flags & ZD_SIZES_LONG_WINDOW) != 0,
                                  (flags & ZD_SIZES_RFC) != 0);
  // (chunks of several frames: zd_multi.hip's kernel, the other one untouched)
  HIPCHK((flags & ZD_SIZES_MULTI_FRAME ? launch_multi_sizes : launch_chunk_sizes)(
      (const uint64_t*)d_src_ptrs, d_src_bytes, (uint32_t)nchunks, wopt, d_size, d_status, d_exact,
      (hipStream_t)stream));
  return ZD_OK;
}

// (the exported symbol: the struct as it was before prefix_bytes_total, see include/zd.h)
#undef zd_batch_info_get
int zd_batch_info_get(const zd_batch* B, zd_batch_info* info) {
  return zd_batch_info_get_sized(B, info, offsetof(zd_batch_info, prefix_bytes_total));
}

int zd_batch_info_get_sized(const zd_batch* B, zd_batch_info* info, size_t info_bytes) {
  if (!B || !info || info_bytes < offsetof(zd_batch_info, prefix_bytes_total)) return ZD_E_INVALID_ARG;
  zd_batch_info2 I{};
  I.info = B->info;
  I.k4j_chunks = B->P ? B->P->n_jframes : 0;   // (the plan's total, which both planners bring back)
  memcpy(info, &I, std::min(info_bytes, sizeof I));
  return ZD_OK;
}

int zd_batch_decode_async(zd_batch* B, void* stream) {
  if (!B) return ZD_E_INVALID_ARG;
  if (!B->P) return ZD_OK;
  if (B->packed && !B->outbase && B->out_bytes) return ZD_E_INVALID_ARG;   // (no zd_batch_bind_output yet)
  const hipStream_t s = (hipStream_t)stream;
  zd_plan* P = B->P;
  // every frame at its own destination from the lowest one: never the plan's
  // staging, and no capacity but the frames' own
  if (int r = decode_launch(P, B->d_gather, B->outbase, s)) return r;
  // (a chain batch: a chunk behind a failed ancestor is ZD_E_NOT_DECODED, known once zd_k_verify has run)
  if (B->chain)
    HIPCHK(launch_chain_results((const FrameState*)(P->d_ws + P->W.frame_state), B->d_bind, B->d_par, (uint32_t)B->n,
                                B->d_status, B->d_len, s));
  else
    HIPCHK(launch_batch_results((const FrameState*)(P->d_ws + P->W.frame_state), B->d_bind, (uint32_t)B->n,
                                B->d_status, B->d_len, s));
  B->launched = true;
  B->have_results = false;
  return ZD_OK;
}

int zd_batch_device_results(const zd_batch* B, const int32_t** d_status, const uint64_t** d_len) {
  if (!B) return ZD_E_INVALID_ARG;
  if (d_status) *d_status = B->d_status;
  if (d_len) *d_len = B->d_len;
  return ZD_OK;
}

int zd_batch_device_checksums(const zd_batch* B, const uint64_t** d_hash, const int8_t** d_ok) {
  if (!B || !(B->flags & ZD_F_VERIFY_CHECKSUM)) return ZD_E_INVALID_ARG;
  const zd_plan* P = B->P;               // (null: a batch of no chunks, arrays of no entries)
  if (d_hash) *d_hash = P ? (const uint64_t*)(P->d_ws + P->W.vhash) : nullptr;
  if (d_ok) *d_ok = P ? (const int8_t*)(P->d_ws + P->W.vok) : nullptr;
  return ZD_OK;
}

int zd_batch_results(zd_batch* B, void* stream, int32_t* status, uint64_t* len, size_t cap, uint64_t* nfailed) {
  if (!B || ((status || len) && cap < B->n)) return ZD_E_INVALID_ARG;
  if (nfailed) *nfailed = 0;
  if (!B->P) return ZD_OK;
  if (!B->launched) return ZD_E_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  const size_t n = B->n;
  zd_plan* P = B->P;
  HIPCHK(hipStreamSynchronize(s));
  B->h_status.resize(n);
  B->h_len.resize(n);
  HIPCHK(hipMemcpy(B->h_status.data(), B->d_status, 4 * n, hipMemcpyDeviceToHost));
  HIPCHK(hipMemcpy(B->h_len.data(), B->d_len, 8 * n, hipMemcpyDeviceToHost));
  if (P->n_jframes) {
    // chunks whose pointer jumping did not converge within K4J's rounds: once
    // more on the streaming executor, as an internal batch of just those
    // chunks (from the gathered copies), then into the device arrays
    std::vector<FrameState> st(n);
    HIPCHK(hipMemcpy(st.data(), P->d_ws + P->W.frame_state, n * sizeof(FrameState), hipMemcpyDeviceToHost));
    std::vector<size_t> redo;
    for (size_t i = 0; i < n; i++) {
      const uint64_t k = st[i].key;
      if (key_code(k) == ZD_E_OUT_OF_DOMAIN && key_phase(k) == PH_LIMIT && key_stage(k) == LS_JROUNDS)
        redo.push_back(i);
    }
    // a chain batch (K4J only with ZD_F_CHAIN_BLOCK_PARALLEL or ZD_F_AUTO_EXECUTOR): every chunk behind
    // such a chunk goes with it -- the launch left them ZD_E_NOT_DECODED -- as one
    // streaming chain batch over that set, the parents remapped.  A chunk of the
    // set whose parent is outside it (the parent decoded fine) is a root there:
    // its prefix entry, the parent's destination and Frame_Content_Size or its
    // own external prefix, goes with it as an external prefix.
    std::vector<int64_t> rpar;
    if (B->chain && !redo.empty()) {
      std::vector<int32_t> par(n);
      HIPCHK(hipMemcpy(par.data(), B->d_par, 4 * n, hipMemcpyDeviceToHost));
      // in[i]: 1 in the set, 0 not, -1 unknown; every chunk walks up to a known ancestor
      std::vector<int8_t> in(n, -1);
      for (size_t i : redo) in[i] = 1;
      std::vector<size_t> path;
      for (size_t i = 0; i < n; i++) {
        path.clear();
        int64_t p = (int64_t)i;
        while (p >= 0 && in[(size_t)p] < 0 && path.size() <= n) { path.push_back((size_t)p); p = par[(size_t)p]; }
        const int8_t v = p >= 0 ? in[(size_t)p] : (int8_t)0;
        for (size_t q : path) in[q] = v;
      }
      redo.clear();
      std::vector<int64_t> at(n, -1);
      for (size_t i = 0; i < n; i++)
        if (in[i] == 1) { at[i] = (int64_t)redo.size(); redo.push_back(i); }
      rpar.resize(redo.size());
      for (size_t k = 0; k < redo.size(); k++) {
        const int32_t p = par[redo[k]];
        rpar[k] = p >= 0 ? at[(size_t)p] : -1;
      }
    }
    if (!redo.empty()) {
      if (int r = B->host_arrays()) return r;
      const size_t m = redo.size();
      std::vector<const void*> src(m);
      std::vector<void*> dst(m);
      std::vector<uint64_t> sz(m), dc(m);
      for (size_t k = 0; k < m; k++) {
        const size_t i = redo[k];
        src[k] = B->d_gather + B->goff[i];
        sz[k] = B->src_size[i];
        dst[k] = (void*)(uintptr_t)B->dst[i];
        dc[k] = B->dst_cap[i];
      }
      // a prefix batch (K4J only with ZD_F_BLOCK_PARALLEL or ZD_F_AUTO_EXECUTOR): the redo chunks'
      // checked prefix addresses and sizes go with them -- a chunk whose prefix
      // plus capacity the streaming executor cannot hold ends ZD_E_OUT_OF_DOMAIN.
      // (a chain batch: the roots' entries only.  A dictionary or set batch has
      // n_jframes only with ZD_F_DICT_BLOCK_PARALLEL: its redo batch takes the
      // dictionary or set below and ZD_F_FRAME_SERIAL, which keeps every frame
      // on the streaming executor whatever else the flags say)
      std::vector<const void*> pf;
      std::vector<uint64_t> pz;
      if (P->prefix) {
        std::vector<uint64_t> a = P->prefix_ptrs, z = P->prefix_bytes;
        if (P->d_prefix_ptrs) {
          a.resize(n); z.resize(n);
          HIPCHK(hipMemcpy(a.data(), P->d_prefix_ptrs, 8 * n, hipMemcpyDeviceToHost));
          HIPCHK(hipMemcpy(z.data(), P->d_prefix_bytes, 8 * n, hipMemcpyDeviceToHost));
        }
        pf.resize(m); pz.resize(m);
        for (size_t k = 0; k < m; k++) {
          // (a chunk whose parent is in the redo batch: the parent's output there, no external prefix)
          pz[k] = (B->chain && rpar[k] >= 0) ? 0 : z[redo[k]];
          pf[k] = pz[k] ? (const void*)(uintptr_t)a[redo[k]] : nullptr;
        }
      }
      BatchSpec S{src.data(), sz.data(), dst.data(), dc.data()};
      if (P->prefix) { S.prefix = pf.data(); S.prefix_bytes = pz.data(); }
      if (B->chain) { S.chain = true; S.parent = rpar.data(); }
      S.n = m;
      S.flags = (B->flags & ~(ZD_F_BLOCK_PARALLEL | ZD_F_CHAIN_BLOCK_PARALLEL | ZD_F_AUTO_EXECUTOR | ZD_F_J_ONE_ROUND)) |
                ZD_F_FRAME_SERIAL;
      S.dict = B->dict;
      S.dset = B->dset;
      S.stream = s;
      zd_batch* Q = nullptr;
      int r = batch_create(S, &Q);
      if (r) return r;
      std::vector<int32_t> st2(m);
      std::vector<uint64_t> ln2(m);
      r = zd_batch_decode_async(Q, s);
      if (!r) r = zd_batch_results(Q, s, st2.data(), ln2.data(), m, nullptr);
      // (the internal batch keeps ZD_F_VERIFY_CHECKSUM: its chunks' digests too)
      if (!r && P->verify() && Q->P)
        for (size_t k = 0; k < m && !r; k++) {
          const size_t i = redo[k];
          if (hipMemcpy(P->d_ws + P->W.vhash + 8 * i, Q->P->d_ws + Q->P->W.vhash + 8 * k, 8,
                        hipMemcpyDeviceToDevice) != hipSuccess ||
              hipMemcpy(P->d_ws + P->W.vok + i, Q->P->d_ws + Q->P->W.vok + k, 1, hipMemcpyDeviceToDevice) !=
                  hipSuccess) {
            (void)hipGetLastError();
            r = ZD_E_HIP;
          }
        }
      zd_batch_destroy(Q);
      if (r) return r;
      for (size_t k = 0; k < m; k++) {
        const size_t i = redo[k];
        B->h_status[i] = st2[k];
        B->h_len[i] = ln2[k];
        HIPCHK(hipMemcpy(B->d_status + i, &st2[k], 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(B->d_len + i, &ln2[k], 8, hipMemcpyHostToDevice));
      }
    }
  }
  uint64_t bad = 0;
  for (size_t i = 0; i < n; i++) {
    if (status) status[i] = B->h_status[i];
    if (len) len[i] = B->h_len[i];
    bad += B->h_status[i] != 0;
  }
  if (nfailed) *nfailed = bad;
  B->have_results = true;
  return ZD_OK;
}

int zd_batch_checksums(zd_batch* B, void* stream, int32_t* ok, uint64_t* hash) {
  if (!B) return ZD_E_INVALID_ARG;
  if (!B->P) return ZD_OK;
  if (!B->launched) return ZD_E_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  if (!B->have_results)
    if (int r = zd_batch_results(B, stream, nullptr, nullptr, 0, nullptr)) return r;
  const size_t n = B->n;
  if (!B->P->frames_ready()) return ZD_E_HIP;   // (a device-built batch's frame index comes back here, once)
  std::vector<uint64_t> h(n);
  HIPCHK(launch_xxh64(B->outbase, B->d_out, B->d_len, (uint32_t)n, B->d_hash, s));
  HIPCHK(hipStreamSynchronize(s));
  HIPCHK(hipMemcpy(h.data(), B->d_hash, 8 * n, hipMemcpyDeviceToHost));
  for (size_t i = 0; i < n; i++) {
    const zd_frame_desc& d = B->P->frame(i).d;
    const bool done = B->h_status[i] == 0;
    const bool have = done && d.kind == ZD_FRAME_ZSTD && d.has_checksum;
    if (ok) ok[i] = have ? ((uint32_t)h[i] == d.checksum ? 1 : 0) : -1;
    if (hash) hash[i] = done ? h[i] : 0;
  }
  return ZD_OK;
}

}  // extern "C"

// ===========================================================================
// Seekable archives (zd_seekable_*): the seek table as three device arrays,
// and reads -- R byte ranges of the content -- as an ordinary device-built
// batch over the needed entries, whose chunk table zd_seek.hip's kernels
// write, plus the pass that delivers the staged frames' bytes.  The rules are
// zd_seek.h's.
// ===========================================================================
namespace {
struct SeekData {
  int dev = -1;
  const uint8_t* d_archive = nullptr;
  uint64_t n = 0;
  SeekFooter ft;
  uint8_t* d_mem = nullptr;              // one allocation: c_off | d_off | scan words | res | checksum
  uint64_t *c_off = nullptr, *d_off = nullptr;
  uint32_t* checksum = nullptr;
  zd_seekable_info info{};
  ~SeekData() { if (d_mem) (void)hipFree(d_mem); }
};
constexpr uint32_t SEEK_READ_FLAGS =
    ZD_F_BLOCK_PARALLEL | ZD_F_FRAME_SERIAL | ZD_F_SEQ_ONE_LANE | ZD_F_NO_FUSE | ZD_F_K1_LANES | ZD_F_J_ONE_ROUND |
    ZD_F_SEQ_NO_LATENCY | ZD_F_K1_SPLIT | ZD_F_VERIFY_CHECKSUM | ZD_F_LONG_WINDOW | ZD_F_CHAIN_BLOCK_PARALLEL |
    ZD_F_AUTO_EXECUTOR;
uint64_t up16(uint64_t x) { return (x + 15) & ~15ull; }
}  // namespace

struct zd_seekable {
  std::shared_ptr<SeekData> p;
};

struct zd_seek_read {
  std::shared_ptr<SeekData> a;           // (a read outlives zd_seekable_close: d_off is read at every launch)
  zd_batch* B = nullptr;                 // the needed entries; null: none
  int dev = -1;
  uint8_t* d_mem = nullptr;              // one allocation for A's arrays, the scan words and res
  SeekRead A{};
  uint8_t* d_stage = nullptr;            // the staged frames, from the workspace cache
  uint64_t stage_alloc = 0;
  uint64_t npieces = 0;
  bool launched = false;
  zd_seek_read_info info{};
  // a ZD_SEEK_VERIFY_TABLE read (else all null / 0): one allocation made at creation, frames_decoded entries each
  uint32_t read_flags = 0;
  uint8_t* d_vmem = nullptr;             // v_addr | v_entry | v_hash32 | v_ok
  uint64_t* v_addr = nullptr;            // where the chunk decodes to (the chunk table itself is freed after creation)
  uint32_t *v_entry = nullptr, *v_hash32 = nullptr;
  int8_t* v_ok = nullptr;
};

extern "C" {

int zd_seekable_open_device(const void* d_archive, size_t n, void* stream, zd_seekable** out) {
  if (!out) return ZD_E_INVALID_ARG;
  if (n < SEEK_MIN_BYTES) return ZD_E_NOT_ENOUGH_BYTES;
  if (!d_archive) return ZD_E_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  const uint8_t* base = (const uint8_t*)d_archive;
  // ---- the footer: one small copy, one wait ----
  uint8_t last[SEEK_FOOTER_BYTES];
  HIPCHK(hipMemcpyAsync(last, base + (n - SEEK_FOOTER_BYTES), SEEK_FOOTER_BYTES, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  SeekFooter ft;
  if (int r = seek_footer(last, n, &ft)) return r;
  std::shared_ptr<SeekData> D(new (std::nothrow) SeekData());
  if (!D) return ZD_E_NO_MEMORY;
  HIPCHK(hipGetDevice(&D->dev));
  D->d_archive = base;
  D->n = n;
  D->ft = ft;
  // ---- the entries, where they lie; the sums; the header's verdict ----
  const uint64_t F = ft.nframes, n1 = F + 1, tiles = (n1 + 255) / 256;
  const uint64_t o_tot = 2 * n1 * 8, o_res = o_tot + 2 * (tiles + 1) * 8, o_sum = o_res + 4 * 8;
  HIPCHK(hipMalloc(&D->d_mem, o_sum + std::max<uint64_t>(F, 1) * 4));
  D->c_off = (uint64_t*)D->d_mem;
  D->d_off = D->c_off + n1;
  uint64_t* tot = (uint64_t*)(D->d_mem + o_tot);
  uint64_t* res = (uint64_t*)(D->d_mem + o_res);
  D->checksum = ft.checksums ? (uint32_t*)(D->d_mem + o_sum) : nullptr;
  HIPCHK(launch_seek_table(base + (n - ft.table_bytes), ft, D->c_off, D->d_off, D->checksum, tot, res, s));
  uint64_t h[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(h, res, 2 * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h + 2, D->c_off + F, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(h + 3, D->d_off + F, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  if (const int r = (int)(int64_t)h[0]) return r;
  if (const int r = seek_sums(h[2], n, ft)) return r;
  zd_seekable_info& I = D->info;
  I.nframes = F;
  I.content_bytes = h[3];
  I.compressed_bytes = h[2];
  I.table_bytes = ft.table_bytes;
  I.has_checksums = ft.checksums;
  I.max_frame_content = (uint32_t)h[1];
  zd_seekable* z = new (std::nothrow) zd_seekable();
  if (!z) return ZD_E_NO_MEMORY;
  z->p = std::move(D);
  *out = z;
  return ZD_OK;
}

int zd_seekable_info_get(const zd_seekable* z, zd_seekable_info* info) {
  if (!z || !z->p || !info) return ZD_E_INVALID_ARG;
  *info = z->p->info;
  return ZD_OK;
}

int zd_seekable_table(const zd_seekable* z, const uint64_t** d_c_off, const uint64_t** d_d_off,
                      const uint32_t** d_checksum) {
  if (!z || !z->p) return ZD_E_INVALID_ARG;
  if (d_c_off) *d_c_off = z->p->c_off;
  if (d_d_off) *d_d_off = z->p->d_off;
  if (d_checksum) *d_checksum = z->p->checksum;
  return ZD_OK;
}

void zd_seekable_close(zd_seekable* z) { delete z; }

void zd_seek_read_destroy(zd_seek_read* r) {
  if (!r) return;
  if (r->launched) (void)hipDeviceSynchronize();   // (the passes behind the batch's own work read the staging buffer)
  if (r->B) zd_batch_destroy(r->B);
  ws_release(r->d_stage, r->stage_alloc, r->dev);
  if (r->d_mem) (void)hipFree(r->d_mem);
  if (r->d_vmem) (void)hipFree(r->d_vmem);
  delete r;
}

int zd_seekable_read_create(zd_seekable* z, const uint64_t* d_off, const uint64_t* d_len, void* const* d_dst,
                            size_t nranges, uint32_t flags, void* stream, zd_seek_read** out) {
  return zd_seekable_read_create_ex(z, d_off, d_len, d_dst, nranges, flags, 0, stream, out);
}

int zd_seekable_read_create_ex(zd_seekable* z, const uint64_t* d_off, const uint64_t* d_len, void* const* d_dst,
                               size_t nranges, uint32_t flags, uint32_t read_flags, void* stream,
                               zd_seek_read** out) {
  // ---- argument checks: no HIP call before they are done (z is looked at last) ----
  if (!out || (flags & ZD_F_SKIPPABLE) || (flags & ~(SEEK_READ_FLAGS | ZD_F_SKIPPABLE)) || nranges >= (1ull << 31) ||
      (read_flags & ~(ZD_SEEK_VERIFY_TABLE | ZD_SEEK_RFC)))
    return ZD_E_INVALID_ARG;
  if (read_flags & ZD_SEEK_RFC) flags |= ZD_F_RFC;               // the inner batch's flag (zd.h: why a read option)
  if (nranges && (!d_off || !d_len || !d_dst)) return ZD_E_INVALID_ARG;
  if (!z || !z->p) return ZD_E_INVALID_ARG;
  const bool verify = (read_flags & ZD_SEEK_VERIFY_TABLE) != 0;
  if (verify && !z->p->checksum) return ZD_E_INVALID_ARG;        // (nothing to verify with: never silently none)
  struct DropRead { void operator()(zd_seek_read* r) const { zd_seek_read_destroy(r); } };
  std::unique_ptr<zd_seek_read, DropRead> hold(new (std::nothrow) zd_seek_read());
  zd_seek_read* r = hold.get();
  if (!r) return ZD_E_NO_MEMORY;
  r->a = z->p;
  r->read_flags = read_flags;
  r->info.nranges = nranges;
  if (!nranges) { *out = hold.release(); return ZD_OK; }
  const SeekData& D = *r->a;
  int dev = -1;
  HIPCHK(hipGetDevice(&dev));
  if (dev != D.dev) return ZD_E_INVALID_ARG;
  r->dev = dev;
  const hipStream_t s = (hipStream_t)stream;
  // ---- the read's arrays ----
  const uint64_t R = nranges, F = D.ft.nframes;
  const uint64_t tilesF = (F + 255) / 256, tilesR = (R + 1 + 255) / 256;
  uint64_t o = 0;
  const auto take = [&](uint64_t bytes) { const uint64_t at = o; o += up16(bytes); return at; };
  const uint64_t o_off = take(8 * R), o_len = take(8 * R), o_dst = take(8 * R), o_piece = take(8 * (R + 1)),
                 o_olen = take(8 * R), o_idx = take(2 * 8 * F), o_tot = take(8 * (2 * (tilesF + 1) + tilesR + 1)),
                 o_res = take(8 * 4), o_f0 = take(4 * R), o_f1 = take(4 * R), o_st = take(4 * R),
                 o_cover = take(4 * F), o_part = take(4 * F), o_bad = take(R);
  HIPCHK(hipMalloc(&r->d_mem, o));
  HIPCHK(hipMemsetAsync(r->d_mem, 0, o, s));
  SeekRead& A = r->A;
  uint8_t* m = r->d_mem;
  A.off = (uint64_t*)(m + o_off); A.len = (uint64_t*)(m + o_len); A.dst = (uint64_t*)(m + o_dst);
  A.piece0 = (uint64_t*)(m + o_piece);
  A.f0 = (uint32_t*)(m + o_f0); A.f1 = (uint32_t*)(m + o_f1);
  A.bad = m + o_bad;
  A.status = (int32_t*)(m + o_st); A.out_len = (uint64_t*)(m + o_olen);
  A.cover = (uint32_t*)(m + o_cover); A.partial = (uint32_t*)(m + o_part);
  A.idx = (uint64_t*)(m + o_idx); A.soff = A.idx + F;
  A.R = (uint32_t)R; A.F = (uint32_t)F;
  uint64_t* tot = (uint64_t*)(m + o_tot);
  uint64_t* res = (uint64_t*)(m + o_res);
  // ---- clamp, search, cover counts, the scans; the one wait of this layer ----
  HIPCHK(launch_seek_layout(d_off, d_len, (const uint64_t*)d_dst, D.d_off, A, tot, res, s));
  uint64_t h[4] = {0, 0, 0, 0};
  HIPCHK(hipMemcpyAsync(h, res, 4 * 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const uint64_t needed = h[0], staged = h[1];
  r->npieces = h[2];
  r->info.frames_decoded = needed;
  r->info.frames_in_place = h[3];
  r->info.staged_bytes = staged;
  r->info.copy_pieces = r->npieces;
  if (r->npieces >= (1ull << 31)) return ZD_E_OUT_OF_DOMAIN;    // zd_k_seek_finish's grid
  if (!needed) { *out = hold.release(); return ZD_OK; }
  // ---- the staging buffer, the chunk table, the inner batch ----
  if (staged) HIPCHK(ws_alloc(dev, staged, &r->d_stage, &r->stage_alloc));
  uint64_t* cols = nullptr;
  HIPCHK(hipMalloc(&cols, 4 * 8 * needed));
  std::unique_ptr<void, Free> cols_mem(cols);
  if (verify) {
    // the verdicts and what zd_k_seek_verify needs of every chunk; before the first launch: not compared (-1, 0)
    const uint64_t o_entry = 8 * needed, o_hash = o_entry + up16(4 * needed), o_ok = o_hash + up16(4 * needed);
    HIPCHK(hipMalloc(&r->d_vmem, o_ok + needed));
    HIPCHK(hipMemsetAsync(r->d_vmem, 0, o_ok, s));
    HIPCHK(hipMemsetAsync(r->d_vmem + o_ok, 0xFF, needed, s));
    r->v_addr = (uint64_t*)r->d_vmem;
    r->v_entry = (uint32_t*)(r->d_vmem + o_entry);
    r->v_hash32 = (uint32_t*)(r->d_vmem + o_hash);
    r->v_ok = (int8_t*)(r->d_vmem + o_ok);
  }
  HIPCHK(launch_seek_chunks(A, D.d_archive, D.c_off, D.d_off, r->d_stage, cols, cols + needed, cols + 2 * needed,
                            cols + 3 * needed, r->v_entry, r->v_addr, s));
  BatchSpec S{(const void* const*)cols, cols + needed, (void* const*)(cols + 2 * needed), cols + 3 * needed};
  S.on_device = true; S.n = (size_t)needed; S.flags = flags; S.stream = s;
  if (int e = batch_create(S, &r->B)) return e;
  (void)zd_batch_info_get_sized(r->B, &r->info.batch.info, sizeof(zd_batch_info2));
  *out = hold.release();
  return ZD_OK;
}

// the verify (a ZD_SEEK_VERIFY_TABLE read), finish and result passes, behind the inner batch's work on s
static int seek_passes(zd_seek_read* r, hipStream_t s) {
  const int32_t* b_status = nullptr;
  const uint64_t* b_len = nullptr;
  if (r->B) (void)zd_batch_device_results(r->B, &b_status, &b_len);
  if (r->v_ok && r->B) {
    // (a ZD_F_VERIFY_CHECKSUM read: the frames the inner batch hashed are not hashed again)
    const uint64_t* b_hash = nullptr;
    const int8_t* b_ok = nullptr;
    if (zd_batch_device_checksums(r->B, &b_hash, &b_ok) != ZD_OK || !b_hash || !b_ok) b_hash = nullptr, b_ok = nullptr;
    HIPCHK(launch_seek_verify(r->v_entry, r->v_addr, (uint32_t)r->info.frames_decoded, r->a->d_off, r->a->checksum,
                              b_status, b_len, b_hash, b_ok, r->v_ok, r->v_hash32, s));
  }
  HIPCHK(launch_seek_finish(r->A, r->a->d_off, r->d_stage, r->npieces, s));
  HIPCHK(launch_seek_results(r->A, r->a->d_off, b_status, b_len, r->v_ok, s));
  return 0;
}

int zd_seek_read_decode_async(zd_seek_read* r, void* stream) {
  if (!r) return ZD_E_INVALID_ARG;
  if (!r->A.R) return ZD_OK;
  if (r->B)
    if (int e = zd_batch_decode_async(r->B, stream)) return e;
  if (int e = seek_passes(r, (hipStream_t)stream)) return e;
  r->launched = true;
  return ZD_OK;
}

int zd_seek_read_finish_async(zd_seek_read* r, void* stream) {
  if (!r) return ZD_E_INVALID_ARG;
  if (!r->A.R) return ZD_OK;
  if (!r->launched) return ZD_E_INVALID_ARG;
  return seek_passes(r, (hipStream_t)stream);
}

int zd_seek_read_device_results(const zd_seek_read* r, const int32_t** d_status, const uint64_t** d_len) {
  if (!r) return ZD_E_INVALID_ARG;
  if (d_status) *d_status = r->A.status;
  if (d_len) *d_len = r->A.out_len;
  return ZD_OK;
}

int zd_seek_read_results(zd_seek_read* r, void* stream, int32_t* status, uint64_t* len, size_t cap, uint64_t* nfailed) {
  if (!r || ((status || len) && cap < r->A.R)) return ZD_E_INVALID_ARG;
  if (nfailed) *nfailed = 0;
  const size_t R = r->A.R;
  if (!R) return ZD_OK;
  if (!r->launched) return ZD_E_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  if (r->B) {
    // (a K4J frame that did not converge is decoded again in there: its bytes and
    // its chunk's status are new, so the two passes run once more)
    if (int e = zd_batch_results(r->B, stream, nullptr, nullptr, 0, nullptr)) return e;
    if (int e = seek_passes(r, s)) return e;
  }
  HIPCHK(hipStreamSynchronize(s));
  std::vector<int32_t> st(R);
  HIPCHK(hipMemcpy(st.data(), r->A.status, 4 * R, hipMemcpyDeviceToHost));
  if (len) HIPCHK(hipMemcpy(len, r->A.out_len, 8 * R, hipMemcpyDeviceToHost));
  uint64_t bad = 0;
  for (size_t i = 0; i < R; i++) {
    if (status) status[i] = st[i];
    bad += st[i] != 0;
  }
  if (nfailed) *nfailed = bad;
  return ZD_OK;
}

int zd_seek_read_info_get(const zd_seek_read* r, zd_seek_read_info* info) {
  if (!r || !info) return ZD_E_INVALID_ARG;
  *info = r->info;
  return ZD_OK;
}

int zd_seek_read_info_get_sized(const zd_seek_read* r, zd_seek_read_info* info, size_t bytes) {
  if (!r || !info || bytes < sizeof(zd_seek_read_info)) return ZD_E_INVALID_ARG;
  zd_seek_read_info2 I{};
  I.info = r->info;
  I.read_flags = r->read_flags;
  I.verify_entries = r->v_ok ? r->info.frames_decoded : 0;
  memcpy(info, &I, std::min(bytes, sizeof I));
  return ZD_OK;
}

int zd_seek_read_device_verdicts(const zd_seek_read* r, const uint32_t** d_entry, const int8_t** d_ok,
                                 const uint32_t** d_hash32, uint64_t* n) {
  if (!r) return ZD_E_INVALID_ARG;
  if (d_entry) *d_entry = r->v_entry;
  if (d_ok) *d_ok = r->v_ok;
  if (d_hash32) *d_hash32 = r->v_hash32;
  if (n) *n = r->v_ok ? r->info.frames_decoded : 0;
  return ZD_OK;
}

}  // extern "C"

// ===========================================================================
// Multi-frame batches (zd_multi_*): chunks of several concatenated zstd frames
// as an ordinary device-built batch over their sub-chunks, whose chunk table
// zd_multi.hip's kernels write, plus the pass that folds the sub-chunks'
// results back into the chunks' and the one that delivers the staged bytes.
// The rule is zd_multi.h's.
// ===========================================================================
namespace {
constexpr uint32_t MULTI_FLAGS = SEEK_READ_FLAGS | ZD_F_RFC;
// (with a dictionary or set only, where it means something: the inner batch gets it; without one it stays an
// unknown bit, as it was)
constexpr uint32_t MULTI_DICT_FLAGS = ZD_F_DICT_BLOCK_PARALLEL;
}  // namespace

struct zd_multi {
  zd_batch* B = nullptr;                 // the sub-chunks; null: a batch of no chunks
  int dev = -1;
  uint8_t* d_mem = nullptr;              // one allocation for M's per-chunk arrays and the scan words
  uint8_t* d_sub = nullptr;              // one for its per-sub-chunk arrays
  MultiArrays M{};
  uint8_t* d_stage = nullptr;            // the staged sub-chunks, from the workspace cache
  uint64_t stage_alloc = 0;
  uint64_t npieces = 0;
  bool launched = false;
  zd_multi_info info{};
};

extern "C" {

void zd_multi_destroy(zd_multi* m) {
  if (!m) return;
  if (m->launched) (void)hipDeviceSynchronize();   // (the passes behind the batch's own work read the staging buffer)
  if (m->B) zd_batch_destroy(m->B);
  ws_release(m->d_stage, m->stage_alloc, m->dev);
  if (m->d_mem) (void)hipFree(m->d_mem);
  if (m->d_sub) (void)hipFree(m->d_sub);
  delete m;
}

int zd_multi_create_device(const void* const* d_src_ptrs, const uint64_t* d_src_bytes, void* const* d_dst_ptrs,
                           const uint64_t* d_dst_cap, size_t nchunks, uint32_t flags, const zd_dict* dict,
                           const zd_dict_set* set, void* stream, zd_multi** out) {
  // ---- argument checks: no HIP call before they are done ----
  if (!out || (flags & ZD_F_SKIPPABLE) ||
      (flags & ~(MULTI_FLAGS | ZD_F_SKIPPABLE | (dict || set ? MULTI_DICT_FLAGS : 0u))) || nchunks >= (1ull << 31) ||
      (dict && set))
    return ZD_E_INVALID_ARG;
  if (nchunks && (!d_src_ptrs || !d_src_bytes || !d_dst_ptrs || !d_dst_cap)) return ZD_E_INVALID_ARG;
  BatchSpec S;
  if (!spec_dicts(S, dict, set)) return ZD_E_INVALID_ARG;
  struct DropMulti { void operator()(zd_multi* m) const { zd_multi_destroy(m); } };
  std::unique_ptr<zd_multi, DropMulti> hold(new (std::nothrow) zd_multi());
  zd_multi* m = hold.get();
  if (!m) return ZD_E_NO_MEMORY;
  m->info.nchunks = nchunks;
  if (!nchunks) { *out = hold.release(); return ZD_OK; }
  int dev = -1;
  HIPCHK(hipGetDevice(&dev));
  m->dev = dev;
  const hipStream_t s = (hipStream_t)stream;
  const uint32_t wopt = walk_opts(dict || set, (flags & ZD_F_LONG_WINDOW) != 0, (flags & ZD_F_RFC) != 0);
  // ---- the per-chunk arrays ----
  const uint64_t n = nchunks, n1 = n + 1, tiles = (n1 + 255) / 256;
  uint64_t o = 0;
  const auto take = [&](uint64_t bytes) { const uint64_t at = o; o += up16(bytes); return at; };
  const uint64_t o_dst = take(8 * n), o_cap = take(8 * n), o_len = take(8 * n), o_first = take(4 * 8 * n1),
                 o_tot = take(4 * 8 * (tiles + 1)), o_st = take(4 * n);
  HIPCHK(hipMalloc(&m->d_mem, o));
  HIPCHK(hipMemsetAsync(m->d_mem, 0, o, s));
  MultiArrays& M = m->M;
  uint8_t* b = m->d_mem;
  M.dst = (uint64_t*)(b + o_dst); M.cap = (uint64_t*)(b + o_cap); M.len = (uint64_t*)(b + o_len);
  M.first = (uint64_t*)(b + o_first); M.stage0 = M.first + n1; M.piece0c = M.first + 2 * n1;
  M.nstaged = M.first + 3 * n1;
  M.status = (int32_t*)(b + o_st);
  M.n = (uint32_t)n;
  // ---- the walk where the chunks lie, the scans; the one wait of this layer ----
  const uint64_t *src = (const uint64_t*)d_src_ptrs, *dst = (const uint64_t*)d_dst_ptrs;
  HIPCHK(launch_multi_count(src, d_src_bytes, dst, d_dst_cap, wopt, M, (uint64_t*)(b + o_tot), s));
  uint64_t h[4] = {0, 0, 0, 0};
  for (int c = 0; c < 4; c++)
    HIPCHK(hipMemcpyAsync(h + c, M.first + c * n1 + n, 8, hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  const uint64_t F = h[0], staged = h[1];
  m->npieces = h[2];
  m->info.frames = F;
  m->info.staged_frames = h[3];
  m->info.frames_in_place = F - h[3];
  m->info.staged_bytes = staged;
  m->info.copy_pieces = m->npieces;
  if (F >= (1ull << 31) || m->npieces >= (1ull << 31)) return ZD_E_OUT_OF_DOMAIN;   // the inner batch; zd_k_multi_copy's grid
  // ---- the per-sub-chunk arrays, the staging buffer, the chunk table, the inner batch ----
  M.F = (uint32_t)F;
  o = 0;
  const uint64_t o_soff = take(8 * F), o_at = take(8 * F), o_piece = take(8 * (F + 1)), o_fdst = take(8 * F),
                 o_chunk = take(4 * F);
  HIPCHK(hipMalloc(&m->d_sub, o));
  uint8_t* u = m->d_sub;
  M.soff = (uint64_t*)(u + o_soff); M.at = (uint64_t*)(u + o_at); M.piece0 = (uint64_t*)(u + o_piece);
  M.fdst = (uint64_t*)(u + o_fdst); M.chunk = (uint32_t*)(u + o_chunk);
  HIPCHK(hipMemsetAsync(M.fdst, 0xFF, 8 * F, s));                 // (before the first join: nothing delivered)
  if (staged) HIPCHK(ws_alloc(dev, staged, &m->d_stage, &m->stage_alloc));
  uint64_t* cols = nullptr;
  HIPCHK(hipMalloc(&cols, 4 * 8 * F));
  std::unique_ptr<void, Free> cols_mem(cols);
  HIPCHK(launch_multi_fill(src, d_src_bytes, dst, d_dst_cap, wopt, M, m->d_stage, cols, cols + F, cols + 2 * F,
                           cols + 3 * F, s));
  S.src = (const void* const*)cols; S.src_bytes = cols + F; S.dst = (void* const*)(cols + 2 * F); S.dst_cap = cols + 3 * F;
  S.on_device = true; S.n = (size_t)F; S.flags = flags; S.stream = s;
  if (int e = batch_create(S, &m->B)) return e;
  (void)zd_batch_info_get_sized(m->B, &m->info.batch.info, sizeof(zd_batch_info2));
  *out = hold.release();
  return ZD_OK;
}

// the join and copy passes, behind the inner batch's work on s
static int multi_passes(zd_multi* m, hipStream_t s) {
  const int32_t* b_status = nullptr;
  const uint64_t* b_len = nullptr;
  (void)zd_batch_device_results(m->B, &b_status, &b_len);
  HIPCHK(launch_multi_join(m->M, b_status, b_len, s));
  HIPCHK(launch_multi_copy(m->M, m->d_stage, b_len, m->npieces, s));
  return 0;
}

int zd_multi_decode_async(zd_multi* m, void* stream) {
  if (!m) return ZD_E_INVALID_ARG;
  if (!m->M.n) return ZD_OK;
  if (int e = zd_batch_decode_async(m->B, stream)) return e;
  if (int e = multi_passes(m, (hipStream_t)stream)) return e;
  m->launched = true;
  return ZD_OK;
}

int zd_multi_finish_async(zd_multi* m, void* stream) {
  if (!m) return ZD_E_INVALID_ARG;
  if (!m->M.n) return ZD_OK;
  if (!m->launched) return ZD_E_INVALID_ARG;
  return multi_passes(m, (hipStream_t)stream);
}

int zd_multi_device_results(const zd_multi* m, const int32_t** d_status, const uint64_t** d_len) {
  if (!m) return ZD_E_INVALID_ARG;
  if (d_status) *d_status = m->M.status;
  if (d_len) *d_len = m->M.len;
  return ZD_OK;
}

int zd_multi_device_frames(const zd_multi* m, const uint64_t** d_first, const int32_t** d_frame_status,
                           const uint64_t** d_frame_len) {
  if (!m) return ZD_E_INVALID_ARG;
  const int32_t* b_status = nullptr;
  const uint64_t* b_len = nullptr;
  if (m->B) (void)zd_batch_device_results(m->B, &b_status, &b_len);
  if (d_first) *d_first = m->M.first;
  if (d_frame_status) *d_frame_status = b_status;
  if (d_frame_len) *d_frame_len = b_len;
  return ZD_OK;
}

int zd_multi_results(zd_multi* m, void* stream, int32_t* status, uint64_t* len, size_t cap, uint64_t* nfailed) {
  if (!m || ((status || len) && cap < m->M.n)) return ZD_E_INVALID_ARG;
  if (nfailed) *nfailed = 0;
  const size_t n = m->M.n;
  if (!n) return ZD_OK;
  if (!m->launched) return ZD_E_INVALID_ARG;
  const hipStream_t s = (hipStream_t)stream;
  // (a K4J frame that did not converge is decoded again in there: its bytes and
  // its sub-chunk's status are new, so the two passes run once more)
  if (int e = zd_batch_results(m->B, stream, nullptr, nullptr, 0, nullptr)) return e;
  if (int e = multi_passes(m, s)) return e;
  HIPCHK(hipStreamSynchronize(s));
  std::vector<int32_t> st(n);
  HIPCHK(hipMemcpy(st.data(), m->M.status, 4 * n, hipMemcpyDeviceToHost));
  if (len) HIPCHK(hipMemcpy(len, m->M.len, 8 * n, hipMemcpyDeviceToHost));
  uint64_t bad = 0;
  for (size_t i = 0; i < n; i++) {
    if (status) status[i] = st[i];
    bad += st[i] != 0;
  }
  if (nfailed) *nfailed = bad;
  return ZD_OK;
}

int zd_multi_info_get_sized(const zd_multi* m, zd_multi_info* info, size_t bytes) {
  if (!m || !info || bytes < offsetof(zd_multi_info, batch)) return ZD_E_INVALID_ARG;
  memcpy(info, &m->info, std::min(bytes, sizeof m->info));
  return ZD_OK;
}

// ===========================================================================
// DecodingContext mirror
// ===========================================================================
}  // extern "C"

struct zd_context {
  uint64_t window = 0;
  uint8_t* d_out = nullptr;     // decoded (capacity d_cap)
  uint64_t d_cap = 0;
  uint64_t len = 0;
  uint64_t rep[3] = {1, 4, 8};
  // persisted tables of the previous blocks (one virtual comp block)
  uint16_t* d_lut = nullptr;    // LUT_ENTRIES
  uint16_t* d_fse = nullptr;    // FSE_SLOT entries
  uint8_t huf_bits = 0;
  uint8_t al[3] = {0, 0, 0};
  bool has_huf = false;
  bool has_tab[3] = {false, false, false};
  // the persisted Huffman table's deep-tree pool (a tree with more leaves
  // than a LUT slot holds keeps its symbols there): the pool's counter and
  // bytes as the plan that built it left them, deep_used bytes
  uint8_t* d_deep = nullptr;
  uint32_t deep_used = 0;
  // kept between calls: the stream every block runs on (one synchronisation
  // per block) and the block-input buffer (grown, never freed per call)
  hipStream_t s = nullptr;
  uint8_t* d_in = nullptr;
  uint64_t in_cap = 0;
};

namespace {

// The caller's bytes in the context's input buffer (async on its stream).
int ctx_input(zd_context* c, const uint8_t* src, size_t n) {
  if (n + ZD_SRC_PADDING > c->in_cap) {
    if (c->d_in) (void)hipFree(c->d_in);
    c->d_in = nullptr;
    c->in_cap = 0;
    const uint64_t nc = std::max<uint64_t>(n + ZD_SRC_PADDING, 256u << 10);
    HIPCHK(hipMalloc(&c->d_in, nc));
    c->in_cap = nc;
  }
  if (n) HIPCHK(hipMemcpyAsync(c->d_in, src, n, hipMemcpyHostToDevice, c->s));
  return 0;
}

int ctx_reserve(zd_context* c, uint64_t need) {
  if (need <= c->d_cap) return 0;
  uint64_t nc = std::max<uint64_t>(c->d_cap ? c->d_cap * 2 : (1 << 20), need);
  uint8_t* nd = nullptr;
  HIPCHK(hipMalloc(&nd, nc));
  if (c->len) HIPCHK(hipMemcpy(nd, c->d_out, c->len, hipMemcpyDeviceToDevice));
  if (c->d_out) (void)hipFree(c->d_out);
  c->d_out = nd;
  c->d_cap = nc;
  return 0;
}

}  // namespace

extern "C" {

int zd_context_new(uint64_t window_size, zd_context** out) {
  if (!out) return ZD_E_INVALID_ARG;
  if (window_size > MAX_WIN_SIZE) return ZD_E_CTX_WINDOW_SIZE_TOO_BIG;   // decoding_context.rs:29-35
  zd_context* c = new (std::nothrow) zd_context();
  if (!c) return ZD_E_NO_MEMORY;
  c->window = window_size;
  if (hipMalloc(&c->d_lut, LUT_ENTRIES * 2) != hipSuccess || hipMalloc(&c->d_fse, FSE_SLOT * 2) != hipSuccess ||
      hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking) != hipSuccess) {
    zd_context_free(c);
    return ZD_E_HIP;
  }
  *out = c;
  return ZD_OK;
}

void zd_context_free(zd_context* c) {
  if (!c) return;
  if (c->d_out) (void)hipFree(c->d_out);
  if (c->d_lut) (void)hipFree(c->d_lut);
  if (c->d_fse) (void)hipFree(c->d_fse);
  if (c->d_deep) (void)hipFree(c->d_deep);
  if (c->d_in) (void)hipFree(c->d_in);
  if (c->s) { (void)hipStreamSynchronize(c->s); (void)hipStreamDestroy(c->s); }
  delete c;
}

int zd_context_decoded(const zd_context* c, uint8_t* dst, size_t cap, size_t* len) {
  if (!c) return ZD_E_INVALID_ARG;
  if (len) *len = c->len;
  size_t k = (size_t)std::min<uint64_t>(cap, c->len);
  if (k && dst) HIPCHK(hipMemcpy(dst, c->d_out, k, hipMemcpyDeviceToHost));
  return cap < c->len ? ZD_E_DST_TOO_SMALL : ZD_OK;
}

int zd_context_offsets(const zd_context* c, uint64_t offsets[3]) {
  if (!c || !offsets) return ZD_E_INVALID_ARG;
  for (int i = 0; i < 3; i++) offsets[i] = c->rep[i];
  return ZD_OK;
}

// Runs a one-frame plan whose output continues the context's decoded buffer:
// copies and kernels on the context's stream, one synchronisation (for the
// frame state and the block's table state).
static int ctx_run(zd_context* c, zd_plan* P, const uint8_t* src, size_t n) {
  if (int r = upload_plan(P)) return r;
  if (int r = ctx_input(c, src, n)) return r;
  const hipStream_t s = c->s;
  HIPCHK(hipMemsetAsync(P->d_ws + P->W.comp_state, 0, std::max<size_t>(P->comps.size(), 1) * sizeof(CompState), s));
  HIPCHK(hipMemsetAsync(P->d_ws + P->W.huge, 0, 4, s));
  HIPCHK(hipMemsetAsync(P->d_ws + P->W.deep, 0, 4, s));
  // prebuilt comp 0 carries the context's tables
  CompState pcs{};
  if (P->has_prebuilt) {
    const CompBlock& pb = P->comps[0];
    uint8_t* luts = P->d_ws + P->W.luts + (uint64_t)pb.lut_slot * LUT_ENTRIES * 2;
    uint8_t* fses = P->d_ws + P->W.fses + (uint64_t)pb.fse_slot * FSE_SLOT * 2;
    HIPCHK(hipMemcpyAsync(luts, c->d_lut, LUT_ENTRIES * 2, hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(fses, c->d_fse, FSE_SLOT * 2, hipMemcpyDeviceToDevice, s));
    pcs.huf_bits = c->huf_bits;
    for (int k = 0; k < 3; k++) pcs.al[k] = c->al[k];
    HIPCHK(hipMemcpyAsync(P->d_ws + P->W.comp_state, &pcs, sizeof pcs, hipMemcpyHostToDevice, s));
    // a Treeless block reuses the persisted tree: when its symbols live in
    // the deep pool, the pool comes back too, at the offsets the LUT slot's
    // DEEP_POOL_AT word names (its counter included, so nothing new lands on it)
    if (P->comps.size() > 1 && P->comps[1].lit_type == LIT_TREELESS && c->has_huf && c->deep_used)
      HIPCHK(hipMemcpyAsync(P->d_ws + P->W.deep, c->d_deep, 16 + (size_t)c->deep_used, hipMemcpyDeviceToDevice, s));
  }
  P->info.out_exact = 1;    // output goes straight into the context buffer
  P->fdesc[0].out = 0;
  HIPCHK(hipMemcpyAsync(P->d_ws + P->W.frames, P->fdesc.data(), sizeof(FrameDesc), hipMemcpyHostToDevice, s));
  HIPCHK(hipMemcpyAsync(P->d_ws + P->W.frame_state, P->fstate0.data(), sizeof(FrameState), hipMemcpyHostToDevice, s));
  LaunchArgs a{};
  a.src = c->d_in; a.src_size = n; a.out = c->d_out; a.ws = P->d_ws; a.W = P->W;
  a.n_tables = (uint32_t)P->list_tables.size();
  a.n_huf = (uint32_t)P->list_huf.size();
  a.n_seq = (uint32_t)P->list_seq.size();
  a.n_frames = 1;
  a.n_k4f = (uint32_t)P->list_k4f.size();
  a.n_copies = (uint32_t)P->copies.size();
  a.stream = s;
  a.route = context_route();
  if (launch_pipeline(a) != hipSuccess) return ZD_E_HIP;
  // the frame state and every block's table state in one synchronisation
  const size_t nc = P->comps.size();
  std::vector<CompState> cst(std::max<size_t>(nc, 1));
  FrameState st{};
  uint32_t deep_used = 0;
  HIPCHK(hipMemcpyAsync(&st, P->d_ws + P->W.frame_state, sizeof st, hipMemcpyDeviceToHost, s));
  HIPCHK(hipMemcpyAsync(&deep_used, P->d_ws + P->W.deep, 4, hipMemcpyDeviceToHost, s));
  if (nc) HIPCHK(hipMemcpyAsync(cst.data(), P->d_ws + P->W.comp_state, nc * sizeof(CompState), hipMemcpyDeviceToHost, s));
  HIPCHK(hipStreamSynchronize(s));
  int code = key_code(st.key);
  if (code) return code;
  c->len = st.out_len;
  for (int i = 0; i < 3; i++) c->rep[i] = st.rep[i];
  // persist tables defined by the real block (comp index 1 when prebuilt, else 0);
  // the device copies stay on the stream, ahead of the next block's work
  size_t ci = P->has_prebuilt ? 1 : 0;
  if (ci < nc) {
    const CompBlock& cb = P->comps[ci];
    const CompState& cs = cst[ci];
    if (cb.lit_type == LIT_COMPRESSED) {
      HIPCHK(hipMemcpyAsync(c->d_lut, P->d_ws + P->W.luts + (uint64_t)cb.lut_slot * LUT_ENTRIES * 2, LUT_ENTRIES * 2,
                            hipMemcpyDeviceToDevice, s));
      c->huf_bits = cs.huf_bits;
      c->has_huf = true;
      c->deep_used = 0;
      if (deep_used) {             // the new tree's symbols are in the plan's pool
        if (!c->d_deep && hipMalloc(&c->d_deep, 16 + (size_t)DEEP_POOL_BYTES) != hipSuccess) {
          c->d_deep = nullptr;
          c->has_huf = false;
          return ZD_E_NO_MEMORY;
        }
        HIPCHK(hipMemcpyAsync(c->d_deep, P->d_ws + P->W.deep, 16 + (size_t)deep_used, hipMemcpyDeviceToDevice, s));
        c->deep_used = deep_used;
      }
    }
    for (int k = 0; k < 3 && cb.nseq; k++) {
      int32_t srcc = cb.tab_src[k];
      if (srcc < 0) continue;
      const CompBlock& sb = P->comps[(size_t)srcc];
      if ((size_t)srcc == ci) {
        HIPCHK(hipMemcpyAsync(c->d_fse + k * FSE_TAB,
                              P->d_ws + P->W.fses + ((uint64_t)sb.fse_slot * FSE_SLOT + k * FSE_TAB) * 2, FSE_TAB * 2,
                              hipMemcpyDeviceToDevice, s));
        c->al[k] = cst[(size_t)srcc].al[k];
      }
      c->has_tab[k] = true;
    }
    // the plan's workspace is released after this call: the copies out of it first
    HIPCHK(hipStreamSynchronize(s));
  }
  return ZD_OK;
}

int zd_block_decode(zd_context* c, const uint8_t* src, size_t n, size_t* consumed, int* last) {
  if (!c || (!src && n)) return ZD_E_INVALID_ARG;
  // Block::parse (block.rs:43-72) on the host side
  Bytes in{src, n};
  const uint8_t* h;
  if (int r = in.slice(3, &h)) return r;
  uint32_t x = h[0] | (h[1] << 8) | ((uint32_t)h[2] << 16);
  HostBlock hb;
  memset(&hb, 0, sizeof hb);
  hb.last = x & 1; hb.type = (x >> 1) & 3; hb.size = x >> 3; hb.src = 3;
  if (hb.type == 0) { const uint8_t* s; if (int r = in.slice(hb.size, &s)) return r; }
  else if (hb.type == 1) { if (int r = in.u8(&hb.rle)) return r; }
  else if (hb.type == 2) {
    const uint8_t* s;
    if (int r = in.slice(hb.size, &s)) return r;
    hb.cb.src = 3; hb.cb.size = hb.size; hb.cb.host_stage = PS_ALL;
    WalkErr e;
    if (int r = parse_compressed(src, 3, hb.size, &hb.cb, &e)) return r;
  } else return ZD_E_RESERVED_BLOCK_TYPE;
  size_t used = n - in.n;
  if (consumed) *consumed = used;
  if (last) *last = hb.last;

  zd_plan P;
  HostPart part;
  HostFrame hf;
  memset(&hf.d, 0, sizeof hf.d);
  hf.d.kind = ZD_FRAME_ZSTD;
  hf.d.content_size = UINT64_MAX;
  int32_t prev_huf = -1, prev_tab[3] = {-1, -1, -1};
  bool need_pre = c->has_huf || c->has_tab[0] || c->has_tab[1] || c->has_tab[2];
  if (need_pre) {
    // virtual previous block: a compressed block that is never decoded
    HostBlock pre;
    memset(&pre, 0, sizeof pre);
    pre.type = 2;
    pre.cb.lit_type = LIT_COMPRESSED;
    pre.cb.host_stage = PS_ALL;
    pre.cb.nseq = 1;
    pre.cb.modes[0] = pre.cb.modes[1] = pre.cb.modes[2] = M_FSE;
    part.blocks.push_back(pre);
    P.has_prebuilt = true;
    if (c->has_huf) prev_huf = 0;
    for (int k = 0; k < 3; k++) if (c->has_tab[k]) prev_tab[k] = 0;
  }
  part.blocks.push_back(hb);
  hf.nb = (uint32_t)part.blocks.size();
  for (const HostBlock& b : part.blocks) hf.ncomp += b.type == 2;
  part.frames.push_back(hf);
  {
    std::vector<HostPart> one;
    one.push_back(std::move(part));
    P.set_parts(std::move(one));
  }
  // resolve with the prebuilt block as "previous": build_plan walks the blocks in
  // order, so the virtual block seeds Treeless/Repeat through prev_huf/prev_tab.
  uint64_t cap = c->len + (hb.type == 2 ? (uint64_t)MAX_BLOCK_OUT : (uint64_t)hb.size);
  if (int r = ctx_reserve(c, cap + 16)) return r;
  uint64_t rep0[3] = {c->rep[0], c->rep[1], c->rep[2]};
  build_plan(&P, prev_huf, prev_tab, c->len, rep0, c->d_cap);
  if (P.has_prebuilt) {
    // the virtual block: prebuilt, never executed, tables self-referencing
    CompBlock& pb = P.comps[0];
    pb.prebuilt = 1;
    pb.huf_src = 0;
    for (int k = 0; k < 3; k++) pb.tab_src[k] = 0;
    P.list_tables.erase(std::remove(P.list_tables.begin(), P.list_tables.end(), 0u), P.list_tables.end());
    P.list_huf.erase(std::remove(P.list_huf.begin(), P.list_huf.end(), 0u), P.list_huf.end());
    P.list_seq.erase(std::remove(P.list_seq.begin(), P.list_seq.end(), 0u), P.list_seq.end());
    // the real block resolves Treeless/Repeat against comp 0 (build_plan already
    // chained them through the virtual block's own FSE/Compressed modes)
    P.blocks[0].type = 5;    // skip in execute
    FrameState& fs = P.fstate0[0];
    // build_plan's keys came from the virtual block; keep only a capacity
    // limit (PH_LIMIT: the context past the streaming K4's int32 positions)
    if (fs.key != KEY_NONE && key_phase(fs.key) != PH_LIMIT) fs.key = KEY_NONE;
    // re-derive host decode errors for the real block only
    CompBlock& cb = P.comps[1];
    if (cb.lit_type == LIT_TREELESS && !c->has_huf)
      fs.key = std::min(fs.key, make_key(PH_DECODE, 1, DS_LITERALS, 0, ZD_E_HUFFMAN_DECODER_MISSING));
    if (cb.nseq == 0) {
      int code = ZD_E_EMPTY_INPUT_DATA;
      for (int k = 0; k < 3; k++) if (!c->has_tab[k]) { code = ZD_E_NO_PREVIOUS_DECODER; break; }
      fs.key = std::min(fs.key, make_key(PH_DECODE, 1, DS_SEQUENCES, 0, code));
    } else {
      for (int k = 0; k < 3; k++) {
        if (cb.modes[k] == M_REPEAT) {
          if (!c->has_tab[k]) {
            fs.key = std::min(fs.key, make_key(PH_DECODE, 1, DS_SEQUENCES, 0, ZD_E_NO_PREVIOUS_DECODER));
            cb.tab_src[k] = -1;
            break;
          }
          cb.tab_src[k] = 0;
        }
      }
      bool ok = cb.tab_src[0] >= 0 && cb.tab_src[1] >= 0 && cb.tab_src[2] >= 0;
      P.list_seq.erase(std::remove(P.list_seq.begin(), P.list_seq.end(), 1u), P.list_seq.end());
      if (ok) P.list_seq.push_back(1);
    }
    if (cb.lit_type == LIT_TREELESS) {
      cb.huf_src = c->has_huf ? 0 : -1;
      P.list_huf.erase(std::remove(P.list_huf.begin(), P.list_huf.end(), 1u), P.list_huf.end());
      if (cb.huf_src >= 0 && cb.nstreams) P.list_huf.push_back(1);
    }
  }
  P.info.src_bytes = n;
  int r = ctx_run(c, &P, src, n);
  ws_release(P.d_ws, P.ws_bytes, P.dev);
  P.d_ws = nullptr;
  if (P.d_staging) { (void)hipFree(P.d_staging); P.d_staging = nullptr; }
  return r;
}

int zd_execute_sequences(zd_context* c, const uint32_t* ll, const uint32_t* ofv, const uint32_t* ml, size_t nseq,
                         const uint8_t* lits, size_t nlits) {
  if (!c || (nseq && (!ll || !ofv || !ml)) || (nlits && !lits)) return ZD_E_INVALID_ARG;
  // One synthetic compressed block whose literals are raw (taken from `lits`)
  // and whose sequences are pre-decoded: only the execute kernel runs.
  uint64_t need = c->len + nlits;
  for (size_t i = 0; i < nseq; i++) need += ml[i];
  // the streaming K4's int32 positions bound the context's output
  if (need >= K4_MAX_FRAME_OUT) return ZD_E_OUT_OF_DOMAIN;
  if (int r = ctx_reserve(c, need + 16)) return r;
  zd_plan P;
  HostFrame hf;
  memset(&hf.d, 0, sizeof hf.d);
  hf.d.kind = ZD_FRAME_ZSTD;
  hf.d.content_size = UINT64_MAX;
  HostBlock hb;
  memset(&hb, 0, sizeof hb);
  hb.type = 2; hb.size = (uint32_t)nlits; hb.src = 0; hb.last = 1;
  hb.cb.lit_type = LIT_RAW; hb.cb.lit_regen = (uint32_t)nlits; hb.cb.lit_data = 0;
  hb.cb.nseq = (uint32_t)nseq; hb.cb.host_stage = PS_ALL; hb.cb.seq_direct = 1;
  hb.cb.modes[0] = hb.cb.modes[1] = hb.cb.modes[2] = M_RLE;
  HostPart part;
  part.blocks.push_back(hb);
  hf.nb = 1;
  hf.ncomp = 1;
  part.frames.push_back(hf);
  {
    std::vector<HostPart> one;
    one.push_back(std::move(part));
    P.set_parts(std::move(one));
  }
  int32_t none[3] = {-1, -1, -1};
  uint64_t rep0[3] = {c->rep[0], c->rep[1], c->rep[2]};
  P.flags |= ZD_F_FRAME_SERIAL;         // the streaming K4 (K4J reads no direct records)
  build_plan(&P, -1, none, c->len, rep0, c->d_cap);
  P.list_tables.clear();
  P.list_huf.clear();
  P.list_seq.clear();   // sequences come from the caller
  P.info.src_bytes = nlits;
  // the caller's triples as direct records (zd_common.h): a value past its
  // packed field is an escape with its exact triple in a DirectSide entry
  uint8_t* d_side = nullptr;
  auto fin = [&](int rr) {
    ws_release(P.d_ws, P.ws_bytes, P.dev);
    if (P.d_staging) (void)hipFree(P.d_staging);
    if (d_side) (void)hipFree(d_side);
    P.d_ws = nullptr; P.d_staging = nullptr; d_side = nullptr;
    return rr;
  };
  std::vector<uint64_t> rec(nseq);
  std::vector<DirectSide> side;
  if (nseq) {
    for (size_t i = 0; i < nseq; i++) {
      // K4's literal and offset checks run in 32 bits; a literals_length
      // past every literal the block holds is ImpossibleValue whatever its
      // size (decoding_context.rs:86-90), so it is clamped to nlits + 1:
      // the outcome is the reference's and no batch sum can wrap (nlits and
      // every match length are below K4_MAX_FRAME_OUT < 2^31)
      const uint32_t lli = (uint32_t)std::min<uint64_t>(ll[i], (uint64_t)nlits + 1);
      const bool esc = lli >= 0x1FFFF || ml[i] >= 0x3FFFF || ofv[i] >= DIRECT_GIANT;
      if (esc && side.empty()) side.assign(nseq, DirectSide{});
      if (esc) side[i] = DirectSide{lli, ml[i], ofv[i], 0};
      rec[i] = esc ? DIRECT_ESCAPE : seq_pack(lli, ml[i], ofv[i]);
    }
    if (!side.empty()) {
      if (hipMalloc(&d_side, side.size() * sizeof(DirectSide)) != hipSuccess) { d_side = nullptr; return fin(ZD_E_NO_MEMORY); }
      if (hipMemcpy(d_side, side.data(), side.size() * sizeof(DirectSide), hipMemcpyHostToDevice) != hipSuccess)
        return fin(ZD_E_HIP);
      P.comps[0].seq_side = (uint64_t)(uintptr_t)d_side;
    }
  }
  int r = upload_plan(&P);
  if (r) return fin(r);
  const hipStream_t s = c->s;
  if (int rr = ctx_input(c, lits, nlits)) return fin(rr);
  CompState cs{};
  cs.lit_count = (uint32_t)nlits;
  if (nseq && hipMemcpyAsync(P.d_ws + P.W.seqs, rec.data(), nseq * 8, hipMemcpyHostToDevice, s) != hipSuccess)
    return fin(ZD_E_HIP);
  P.fdesc[0].out = 0;
  if (hipMemcpyAsync(P.d_ws + P.W.comp_state, &cs, sizeof cs, hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(P.d_ws + P.W.frames, P.fdesc.data(), sizeof(FrameDesc), hipMemcpyHostToDevice, s) != hipSuccess ||
      hipMemcpyAsync(P.d_ws + P.W.frame_state, P.fstate0.data(), sizeof(FrameState), hipMemcpyHostToDevice, s) != hipSuccess)
    return fin(ZD_E_HIP);
  LaunchArgs a{};
  a.src = c->d_in; a.src_size = nlits; a.out = c->d_out; a.ws = P.d_ws; a.W = P.W;
  a.n_frames = 1;
  a.n_k4f = (uint32_t)P.list_k4f.size();
  a.n_copies = (uint32_t)P.copies.size();
  a.stream = s;
  a.route = context_route();
  FrameState st{};
  if (launch_pipeline(a) != hipSuccess ||
      hipMemcpyAsync(&st, P.d_ws + P.W.frame_state, sizeof st, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess)
    return fin(ZD_E_HIP);
  int code = key_code(st.key);
  if (code) return fin(code);
  c->len = st.out_len;
  for (int i = 0; i < 3; i++) c->rep[i] = st.rep[i];
  return fin(ZD_OK);
}

}  // extern "C"
