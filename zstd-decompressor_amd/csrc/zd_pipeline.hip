// zd_pipeline.hip — launch_pipeline, the one place that starts a plan's decode
// kernels along its LaunchRoute; the debug exports of the trace / profiling
// builds; zd_k_reset* and launch_reset, launch_dict_tables, launch_compact.
// Compiled only as part of zd_kernels.hip, which includes it inside namespace
// zd where this text stood (behind the decode kernels, before the device
// planner): the library keeps one device code object.
// ---------------------------------------------------------------------------
// launch
// ---------------------------------------------------------------------------
// zd_k_jround's grid over `pieces` pieces: a multiple of 8 (one eighth per XCD)
static dim3 j_grid(uint64_t pieces, uint32_t cus) {
  const uint64_t gw = (pieces + 16 * JW_K - 1) / (16 * JW_K);   // pieces per workgroup sweep
  const uint64_t gmax = 8ull * cus;                              // what fits at once: 8 workgroups per CU
  return dim3((uint32_t)(gw < gmax ? (gw + 7) & ~7ull : (gmax + 7) & ~7ull));
}
// launch_pipeline's view of the workspace: every array it hands to a kernel,
// typed once, here.  What some kernel writes is a plain pointer (it converts
// where another kernel takes it const); what none writes is const.
struct WsView {
  const CopyDesc* copies;
  const CompBlock* comp;
  CompState* cstate;
  const BlockRec* blocks;
  const FrameDesc* frames;
  FrameState* fstate;
  uint16_t *luts, *fses;
  uint64_t* seqs;
  uint8_t* lits;
  const uint32_t *list_tables, *list_huf, *list_seq, *list_k4f;
  uint32_t *huge, *deep, *k2done;
  const uint8_t* deep_pool;                // K2's: the deep pool behind its 16 bytes of counters
  uint8_t *redo, *jdone;
  const uint8_t* const* dict_ptrs;
  const uint32_t* frame_dict;
  const JFrame* jframes;
  const JBlkDesc* jd;
  JBlk* jb;
  JSeg* jseg;
  const JSegDesc* jsd;
  uint32_t *jst, *jpend;
  WsView(uint8_t* ws, const Workspace& W)
      : copies((const CopyDesc*)(ws + W.copies)), comp((const CompBlock*)(ws + W.comp)),
        cstate((CompState*)(ws + W.comp_state)), blocks((const BlockRec*)(ws + W.blocks)),
        frames((const FrameDesc*)(ws + W.frames)), fstate((FrameState*)(ws + W.frame_state)),
        luts((uint16_t*)(ws + W.luts)), fses((uint16_t*)(ws + W.fses)), seqs((uint64_t*)(ws + W.seqs)),
        lits(ws + W.lits), list_tables((const uint32_t*)(ws + W.list_tables)),
        list_huf((const uint32_t*)(ws + W.list_huf)), list_seq((const uint32_t*)(ws + W.list_seq)),
        list_k4f((const uint32_t*)(ws + W.list_k4f)), huge((uint32_t*)(ws + W.huge)), deep((uint32_t*)(ws + W.deep)),
        k2done((uint32_t*)(ws + W.k2done)), deep_pool(ws + W.deep + 16), redo(ws + W.redo), jdone(ws + W.jdone),
        dict_ptrs((const uint8_t* const*)(ws + W.dict_ptrs)), frame_dict((const uint32_t*)(ws + W.frame_dict)),
        jframes((const JFrame*)(ws + W.jframes)), jd((const JBlkDesc*)(ws + W.jblkd)), jb((JBlk*)(ws + W.jblk)),
        jseg((JSeg*)(ws + W.jseg)), jsd((const JSegDesc*)(ws + W.jsegd)), jst((uint32_t*)(ws + W.jst)),
        jpend((uint32_t*)(ws + W.jpend)) {}
};
hipError_t launch_pipeline(const LaunchArgs& a) {
  const WsView w(a.ws, a.W);
  const LaunchRoute& R = a.route;
  hipStream_t s = a.stream;
  hipError_t e;
  // mode 2: events around launch group g on s
  auto dom = [&](int g, int end) -> hipError_t {
    if (R.profiling != 2) return hipSuccess;
    if (end) *a.dom_used |= 1u << g;
    return hipEventRecord(a.dom_events[2 * g + end], s);
  };
  // mode 1: event k on s
  auto ev = [&](int k) -> hipError_t { return R.profiling == 1 ? hipEventRecord(a.events[k], s) : hipSuccess; };
  // One way to start a kernel for each head of arguments the kernels share, the
  // kernel's own arguments behind it (generic lambdas, always inlined: plain
  // launches).  K4's head, which K4F's and zd_k_fused's is too:
  auto run_x = [&](auto kernel, dim3 g, dim3 b, hipStream_t st, auto... tail) __attribute__((always_inline)) {
    hipLaunchKernelGGL(kernel, g, b, 0, st, a.src, a.out, w.frames, w.fstate, w.blocks, w.comp, w.cstate, w.lits,
                       w.seqs, w.fses, tail...);
  };
  // K2's and K3's: a work list and its length behind the block arrays
  auto run_l = [&](auto kernel, dim3 g, dim3 b, hipStream_t st, const uint32_t* list, uint32_t n, auto... tail)
                   __attribute__((always_inline)) {
    hipLaunchKernelGGL(kernel, g, b, 0, st, a.src, w.comp, w.cstate, w.fstate, list, n, tail...);
  };
  // K1's, `lanes` blocks of the table list a workgroup: src_size too, and the tables it fills
  auto run_k1 = [&](auto kernel, uint32_t lanes, hipStream_t st, auto... tail) __attribute__((always_inline)) {
    hipLaunchKernelGGL(kernel, dim3((a.n_tables + lanes - 1) / lanes), dim3(lanes), 0, st, a.src, a.src_size, w.comp,
                       w.cstate, w.fstate, w.list_tables, a.n_tables, w.luts, w.fses, tail...);
  };
  if ((e = ev(0)) != hipSuccess) return e;
  if (a.n_copies) {
    if ((e = dom(DOM_K0, 0)) != hipSuccess) return e;
    hipLaunchKernelGGL(zd_k_rawcopy, dim3(a.n_copies * K0_SPLIT), dim3(256), 0, s, a.src, a.out, w.copies);
    if ((e = dom(DOM_K0, 1)) != hipSuccess) return e;
  }
  if ((e = ev(1)) != hipSuccess) return e;
  // K2 and K3 are independent once their tables exist: with the fork, K1's
  // Huffman half and K2 run on the aux stream beside K1's sequence half and
  // K3; without it, K1's two halves may still run on the two streams (joined
  // before K2)
  const bool fork = R.fork, k1f = R.k1_fork;
  hipStream_t s2 = fork ? a.aux : s;               // K2's stream
  hipStream_t sh = fork || k1f ? a.aux : s;        // K1's Huffman half, where the halves are two launches
  if (fork || k1f) {
    if ((e = hipEventRecord(a.fork, s)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(a.aux, a.fork, 0)) != hipSuccess) return e;
  }
  // the trees of more than 256 symbols the passes before listed, then K2's
  // pair tables from the LUTs of maxBits <= 11
  auto k1_huge_pairs = [&](hipStream_t st, uint32_t only_big) {
    hipLaunchKernelGGL(zd_k_tables_huge, dim3(K1H_GRID), dim3(K1H_LANES), 0, st, a.src, a.src_size, w.comp, w.cstate,
                       w.fstate, w.huge, w.luts, w.deep);
    hipLaunchKernelGGL(zd_k_huf_pairs, dim3((a.n_tables + PR_WAVES - 1) / PR_WAVES), dim3(64 * PR_WAVES), 0, st,
                       w.comp, w.cstate, w.list_tables, a.n_tables, w.luts, only_big);
  };
  auto k1 = [&](auto pass_small, auto pass_big, hipStream_t st, bool huf) {
    run_k1(pass_small, K1_LANES, st, w.huge);
    run_k1(pass_big, K1_LANES, st, w.huge);
    if (huf) k1_huge_pairs(st, 0u);
  };
  // the two passes (ZD_ROUTE_K1_SPLIT), then what they flagged on the lanes
  auto k1s = [&](auto parse, auto build, auto pass_big, hipStream_t st, uint32_t part) {
    run_k1(parse, K1P_LANES, st);
    hipLaunchKernelGGL(build, dim3((a.n_tables + K1B_WAVES - 1) / K1B_WAVES), dim3(64 * K1B_WAVES), 0, st, w.comp,
                       w.cstate, w.list_tables, a.n_tables, w.luts, w.fses);
    run_k1(pass_big, K1_LANES, st, w.huge);
    if (part & 1) k1_huge_pairs(st, part == 3 ? 2u : 1u);
  };
  auto k1s_huf = [&](hipStream_t st) {
    k1s(zd_k_tables_parse<1>, zd_k_tables_build<1>, zd_k_tables<true, 1>, st, 1);
  };
  const bool fz = R.fused;
  if (a.n_tables) switch (R.k1) {
    case K1_HUF_LANES: k1(zd_k_tables<false, 1>, zd_k_tables<true, 1>, s2, true); break;   // (the sequence half
    case K1_HUF_SPLIT: k1s_huf(s2); break;                                                 // runs in zd_k_fused)
    case K1_SPLIT_TWO:                         // the same launch shapes as the lanes' below
      k1s_huf(sh);
      k1s(zd_k_tables_parse<2>, zd_k_tables_build<2>, zd_k_tables<true, 2>, s, 2);
      break;
    case K1_SPLIT_BOTH: k1s(zd_k_tables_parse<3>, zd_k_tables_build<3>, zd_k_tables<true, 3>, s, 3); break;
    case K1_LANES_SEQW:                        // few blocks: the sequence half one wave per block
      k1(zd_k_tables<false, 1>, zd_k_tables<true, 1>, sh, true);
      run_l(zd_k_tables_seqw, dim3(a.n_tables), dim3(64), s, w.list_tables, a.n_tables, w.fses);
      break;
    case K1_LANES_TWO:
      k1(zd_k_tables<false, 1>, zd_k_tables<true, 1>, sh, true);
      k1(zd_k_tables<false, 2>, zd_k_tables<true, 2>, s, false);
      break;
    case K1_LANES_BOTH: k1(zd_k_tables<false, 3>, zd_k_tables<true, 3>, s, true); break;
  }
  if ((e = ev(2)) != hipSuccess) return e;
  if (k1f) {
    if ((e = hipEventRecord(a.join, a.aux)) != hipSuccess) return e;
    if ((e = hipStreamWaitEvent(s, a.join, 0)) != hipSuccess) return e;
  }
  if (a.n_huf)
    run_l(zd_k_huffman, dim3((a.n_huf + K2_BLOCKS - 1) / K2_BLOCKS), dim3(K2_LANES), s2, w.list_huf, a.n_huf, w.luts,
          w.lits, (fz && fork) ? w.k2done : nullptr, w.deep_pool);
  if (fork)
    if ((e = hipEventRecord(a.join, a.aux)) != hipSuccess) return e;
  if ((e = ev(3)) != hipSuccess) return e;
  auto k3 = [&](const uint8_t* redo) {
    const uint32_t n = a.n_seq;
    if (n) switch (R.k3) {
      case K3_L: run_l(zd_k_sequences_l, dim3(n), dim3(64), s, w.list_seq, n, w.fses, w.seqs, redo); break;
      case K3_Q:
        run_l(zd_k_sequences_q, dim3((n + K3Q_CHAINS - 1) / K3Q_CHAINS), dim3(64), s, w.list_seq, n, w.fses, w.seqs,
              redo);
        break;
      case K3_ONE_LANE:
        run_l(zd_k_sequences, dim3((n + K3_LANES - 1) / K3_LANES), dim3(K3_LANES), s, w.list_seq, n, w.fses, w.seqs);
        break;
    }
  };
  // the streaming K4 runs when some frame is not K4F's, K4J's or K0's alone
  // (the others exit at once in it)
  const bool k4_work = a.n_frames > a.n_k4f + a.n_jframes + a.n_k0only;
  // K4J's tables over every J frame of the plan: the segments' sums, the
  // blocks' checkpoints, the frames' scans
  auto k4j_tables = [&](hipStream_t st) {
    hipLaunchKernelGGL(zd_k_jsum, dim3(a.n_jseg), dim3(64), 0, st, a.src, w.fstate, w.blocks, w.comp, w.cstate, w.seqs,
                       w.fses, w.jframes, w.jd, w.jsd, w.jseg);
    hipLaunchKernelGGL(zd_k_jsum_blocks, dim3((a.n_jblk + 63) / 64), dim3(64), 0, st, w.fstate, w.blocks, w.comp,
                       w.cstate, w.jframes, w.jd, a.n_jblk, w.jb, w.jseg);
    hipLaunchKernelGGL(zd_k_jprefix, dim3(a.n_jframes), dim3(64 * JP_WAVES), 0, st, w.frames, w.fstate, w.jframes,
                       w.jd, w.jb);
  };
  // K4J's scatter over segments [seg0, seg0 + nseg), then its pointer-jumping
  // rounds over `pieces` pieces from J frame jf0 on, counted in pend[1], pend[2].
  // The two std::bool_constant arguments choose the kernels' templates.  pfx:
  // the frames read prefixes (the scatter gets no frames / dict_ptrs
  // otherwise).  lvl: the range is one level of a chain batch -- the scatter
  // checks the frames' parents, and a level without a piece gets no round (a
  // whole plan's rounds are launched whatever a.j_pieces is).  dct (with pfx):
  // a dictionary or dictionary-set plan -- the scatter's table holds the plan's
  // dictionaries' content addresses, src_tab (one entry, LaunchArgs::dict_tab,
  // or the workspace's table of a set), not the frames' prefixes.
  auto k4j_range = [&](auto pfx_c, auto lvl_c, auto dct_c, hipStream_t st, uint32_t seg0, uint32_t nseg, uint32_t jf0,
                       uint64_t pieces, uint32_t* pend, const uint8_t* const* src_tab) {
    constexpr bool pfx = decltype(pfx_c)::value, lvl = decltype(lvl_c)::value, dct = decltype(dct_c)::value;
    hipLaunchKernelGGL((zd_k_jscatter<pfx, lvl, dct>), dim3(nseg), dim3(64), 0, st, a.src, w.fstate, w.blocks, w.comp,
                       w.cstate, w.lits, w.seqs, w.fses, w.jframes, w.jd, w.jb, w.jseg, w.jsd, w.jst,
                       pfx ? w.frames : nullptr, pfx ? src_tab : nullptr, seg0, lvl ? a.chain_parent : nullptr);
    const dim3 gr = j_grid(pieces, a.cus);
    // round 1 one launch, the rest as one launch of sweeps
    // (one launch of all the sweeps: 1.43 ms for the rounds of c3s, against
    // 1.38 with the first round launched alone; three launches, 1.38 too)
    const uint32_t nr = a.j_rounds < 2 ? a.j_rounds : 2u;
    for (uint32_t r = 1; r <= nr && (pieces || !lvl); r++)
      hipLaunchKernelGGL(zd_k_jround<lvl>, gr, dim3(256), 0, st, a.out, w.frames, w.fstate, w.jframes, a.n_jframes, jf0,
                         pieces, w.jst, pend, w.jdone, r > 1 ? R.j_hops2 : R.j_hops, r, (uint32_t)(r == nr),
                         r == nr ? a.j_rounds - nr + 1 : 1u);
  };
  // the streaming K4 over every frame of the plan, on s
  auto k4 = [&](const uint8_t* redo) -> hipError_t {
    const uint32_t n = a.n_frames;
    if (R.k4 == K4_CHAIN) {
      // one launch per non-empty level, in level order on this stream: a level's
      // frames find their parents complete.  Levels past the first launch even
      // when K0 copies every frame whole: the workgroups check their parents.
      if (n && k4_work) if ((e = dom(DOM_K4, 0)) != hipSuccess) return e;
      // ZD_F_CHAIN_BLOCK_PARALLEL: K4J's tables once over every J frame (none of
      // them reads a prefix), then per level, behind the level's streaming
      // frames, the scatter over the level's segments and the rounds over the
      // level's pieces (LaunchArgs::chain_j).  A level's frames find every
      // frame of the levels below final, streaming or J: a J frame's bytes are
      // final once its level's last zd_k_jround has emitted them.
      const bool cj = a.chain_j && a.n_jframes;
      if (cj) k4j_tables(s);
      uint32_t begin = 0;
      for (uint32_t l = 0; l < a.chain_levels; begin += a.chain_count[l], l++) {
        if (a.chain_count[l] && (l || k4_work))
          run_x(zd_k_execute_chain, dim3(a.chain_count[l]), dim3(64), s, a.chain_order, begin, a.chain_parent,
                w.dict_ptrs);
        if (!cj || !a.chain_j[l].njf) continue;
        // (the level's own pend slots, 3 a level: rounds 1 and 2 use [1] and [2])
        const JLevel& L = a.chain_j[l];
        k4j_range(std::true_type{}, std::true_type{}, std::false_type{}, s, (uint32_t)L.seg0, (uint32_t)L.nseg,
                  (uint32_t)L.jf0, L.npieces, w.jpend + 3 * l, w.dict_ptrs);
      }
      if (n && k4_work) if ((e = dom(DOM_K4, 1)) != hipSuccess) return e;
      return hipSuccess;
    }
    if (n && k4_work) {  // frames on the streaming K4 (K4F's, K4J's and K0's exit at once)
      const bool tm = !redo && k4_work;
      if (tm) if ((e = dom(DOM_K4, 0)) != hipSuccess) return e;
      const dim3 g(n), b(64);
      // One helper call a kernel, not one behind a choice of (kernel, tail): the tails differ in number and
      // type.  Every K4Kind is named: a new one is a -Wswitch warning here, not a silent zd_k_execute.
      switch (R.k4) {
        case K4_PLAIN: run_x(zd_k_execute, g, b, s, 0u, n, redo); break;
        case K4_DICT: run_x(zd_k_execute_dict, g, b, s, 0u, n, a.dict); break;            // (never fused: no redo pass)
        case K4_DICT_SET: run_x(zd_k_execute_dicts, g, b, s, 0u, n, w.dict_ptrs, w.frame_dict); break;   // each frame's own
        case K4_PREFIX: run_x(zd_k_execute_prefix, g, b, s, 0u, n, w.dict_ptrs); break;   // each frame's own prefix
        case K4_CHAIN: break;                  // (launched above, level by level)
      }
      if (tm) if ((e = dom(DOM_K4, 1)) != hipSuccess) return e;
    }
    return hipSuccess;
  };
  if (fz) {
    // K1's sequence half + K3 + K4 per group of four frames; K2 (forked) signals its workgroups;
    // then the redo pass for the frames the fused kernel flagged (normally none:
    // two launches whose workgroups exit at once)
    const uint32_t k2need = fork ? (a.n_huf + K2_BLOCKS - 1) / K2_BLOCKS : 0;
    const dim3 g((a.n_frames + FZ_FRAMES - 1) / FZ_FRAMES);
    if ((e = dom(DOM_FUSED, 0)) != hipSuccess) return e;
    if (R.k3 == K3_L)
      run_x(zd_k_fused<true>, g, dim3(128 * FZ_FRAMES), s, a.n_frames, w.k2done, k2need, w.redo);
    else
      run_x(zd_k_fused<false>, g, dim3(64 * FZ_WAVES), s, a.n_frames, w.k2done, k2need, w.redo);
    if ((e = dom(DOM_FUSED, 1)) != hipSuccess) return e;
    if (fork)
      if ((e = hipStreamWaitEvent(s, a.join, 0)) != hipSuccess) return e;
    k3(w.redo);
    if ((e = k4(w.redo)) != hipSuccess) return e;
  } else {
    k3(nullptr);
    if (fork)
      if ((e = hipStreamWaitEvent(s, a.join, 0)) != hipSuccess) return e;
    if ((e = ev(4)) != hipSuccess) return e;
    if ((e = k4(nullptr)) != hipSuccess) return e;
    if (a.n_k4f) {
      if ((e = dom(DOM_K4F, 0)) != hipSuccess) return e;
      run_x(zd_k_execute_lds, dim3(a.n_k4f), dim3(K4F_T), s, w.list_k4f);
      if ((e = dom(DOM_K4F, 1)) != hipSuccess) return e;
    }
  }
  if ((e = ev(5)) != hipSuccess) return e;
  if (a.n_jframes && !(R.k4 == K4_CHAIN && a.chain_j)) {   // (a flagged chain batch: level by level, in k4 above)
    if ((e = dom(DOM_K4J, 0)) != hipSuccess) return e;
    k4j_tables(s);
    if (R.k4 == K4_PREFIX)                     // each frame's own prefix, as the streaming launch above reads it
      k4j_range(std::true_type{}, std::false_type{}, std::false_type{}, s, 0u, a.n_jseg, 0u, a.j_pieces, w.jpend,
                w.dict_ptrs);
    else if (R.k4 == K4_DICT || R.k4 == K4_DICT_SET) {   // ZD_F_DICT_BLOCK_PARALLEL: the dictionary, or each frame's own
      const uint8_t* const* tab = R.k4 == K4_DICT ? a.dict_tab : w.dict_ptrs;
      if (!tab) return hipErrorInvalidValue;   // (never: zd_dict_create makes the one-entry table)
      k4j_range(std::true_type{}, std::false_type{}, std::true_type{}, s, 0u, a.n_jseg, 0u, a.j_pieces, w.jpend, tab);
    } else
      k4j_range(std::false_type{}, std::false_type{}, std::false_type{}, s, 0u, a.n_jseg, 0u, a.j_pieces, w.jpend,
                nullptr);
    if ((e = dom(DOM_K4J, 1)) != hipSuccess) return e;
  }
  if ((e = ev(6)) != hipSuccess) return e;
  return hipGetLastError();
}

#ifdef ZD_FZ_TRACE
}  // namespace zd
extern "C" int zd_debug_fz_trace(uint64_t* out, uint64_t* k2end) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(zd::fz_tr), sizeof(zd::fz_tr), 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (hipMemcpyFromSymbol(k2end, HIP_SYMBOL(zd::fz_k2end), 8, 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  return 0;
}
namespace zd {
#endif
#ifdef ZD_K1_PROF
}  // namespace zd
extern "C" int zd_debug_k1_prof(uint64_t out[8], int reset) {
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(zd::k1_prof), 64, 0, hipMemcpyDeviceToHost) != hipSuccess) return -1;
  if (reset) {
    static const uint64_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(zd::k1_prof), z, 64, 0, hipMemcpyHostToDevice) != hipSuccess) return -1;
  }
  return 0;
}
namespace zd {
#endif
// The per-launch state reset of zd_decode_async in one launch: frame states
// from their device copies, block states, K1's tree list and deep-pool
// counters, K4J's round counters and done flags (six copy / fill launches
// before, ~5 us each on the path of a few-frame plan).
// cs_keep: the leading words of the block states that stay (a dictionary
// plan's prebuilt comp 0 -- a dictionary-set plan's prebuilt comps, one per
// dictionary it uses -- written once at plan creation; zd_k_reset_dict).
__device__ __attribute__((always_inline)) inline void reset_body(uint8_t* ws, const Workspace& W, uint64_t fs_words,
                                                                 uint64_t cs_words, uint32_t jp_words,
                                                                 uint64_t jdone_bytes, uint32_t cs_keep) {
  const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x, nt = (uint64_t)gridDim.x * 256;
  uint32_t* fs = (uint32_t*)(ws + W.frame_state);
  const uint32_t* fs0 = (const uint32_t*)(ws + W.frame_state0);
  for (uint64_t i = t; i < fs_words; i += nt) fs[i] = fs0[i];
  uint32_t* cs = (uint32_t*)(ws + W.comp_state);
  for (uint64_t i = t + cs_keep; i < cs_words; i += nt) cs[i] = 0;
  if (t == 0) {
    *(uint32_t*)(ws + W.huge) = 0;
    *(uint32_t*)(ws + W.deep) = 0;
  }
  uint32_t* jp = (uint32_t*)(ws + W.jpend);
  for (uint64_t i = t; i < jp_words; i += nt) jp[i] = 0;
  u32x4* jd = (u32x4*)(ws + W.jdone);
  const uint64_t n16 = jdone_bytes / 16;
  for (uint64_t i = t; i < n16; i += nt) jd[i] = (u32x4){0, 0, 0, 0};
  if (t < jdone_bytes % 16) (ws + W.jdone)[16 * n16 + t] = 0;
}
__global__ __launch_bounds__(256) void zd_k_reset(uint8_t* ws, Workspace W, uint64_t fs_words, uint64_t cs_words,
                                                  uint32_t jp_words, uint64_t jdone_bytes) {
  reset_body(ws, W, fs_words, cs_words, jp_words, jdone_bytes, 0);
}
__global__ __launch_bounds__(256) void zd_k_reset_dict(uint8_t* ws, Workspace W, uint64_t fs_words, uint64_t cs_words,
                                                       uint32_t jp_words, uint64_t jdone_bytes, uint32_t cs_keep) {
  reset_body(ws, W, fs_words, cs_words, jp_words, jdone_bytes, cs_keep);
}
hipError_t launch_reset(uint8_t* ws, const Workspace& W, uint64_t n_frames, uint64_t n_comps, bool k4j,
                        uint64_t j_pieces, hipStream_t s, uint32_t keep_comps, uint32_t jpend_words) {
  const uint64_t fs_words = n_frames * sizeof(FrameState) / 4, cs_words = std::max<uint64_t>(n_comps, 1) * sizeof(CompState) / 4;
  const uint32_t jp_words = k4j ? jpend_words : 0u;
  const uint64_t jdone = k4j ? std::max<uint64_t>(j_pieces, 1) : 0;
  const uint64_t work = std::max(std::max(fs_words, cs_words), jdone / 16 + 16);
  const uint32_t grid = (uint32_t)std::min<uint64_t>(2048, (work + 1023) / 1024);
  static_assert(sizeof(FrameState) % 4 == 0 && sizeof(CompState) % 4 == 0, "zd_k_reset: u32 words");
  if (keep_comps)
    hipLaunchKernelGGL(zd_k_reset_dict, dim3(grid), dim3(256), 0, s, ws, W, fs_words, cs_words, jp_words, jdone,
                       keep_comps * (uint32_t)(sizeof(CompState) / 4));
  else
    hipLaunchKernelGGL(zd_k_reset, dim3(grid), dim3(256), 0, s, ws, W, fs_words, cs_words, jp_words, jdone);
  return hipGetLastError();
}

hipError_t launch_dict_tables(const uint8_t* d_dict, uint32_t n, uint16_t* d_lut, uint16_t* d_fse, DictTables* d_res,
                              hipStream_t s) {
  hipLaunchKernelGGL(zd_k_dict_tables, dim3(1), dim3(64), 0, s, d_dict, n, d_lut, d_fse, d_res);
  return hipGetLastError();
}

hipError_t launch_compact(const uint8_t* staging, uint8_t* dst, const uint64_t* d_from, const uint64_t* d_to,
                          const uint64_t* d_len, uint32_t n, hipStream_t s) {
  if (!n) return hipSuccess;
  hipLaunchKernelGGL(zd_k_compact, dim3(n, COMPACT_SPLIT), dim3(256), 0, s, staging, dst, d_from, d_to, d_len);
  return hipGetLastError();
}
