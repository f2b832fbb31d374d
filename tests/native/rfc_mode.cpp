// Host driver of the three places ZD_F_RFC changes on the host side, no GPU
// needed (tests/test_rfc_native.py reads the lines):
//   N extra nseq_default nseq_rfc
//       parse_compressed (zd_walk.h) over a block whose Number_of_Sequences is
//       the three-byte form 0xFF, extra & 255, extra >> 8, without an option and
//       with walk_opts(.., rfc): D1
//   S status_default nstreams_default status_rfc
//       a four-stream Huffman section whose third stream is empty
//   P flag key_code key_block fses nseq_listed list_seq... | fse_slot(B) tab_src(C) x3 huf_src(C) rfc(A) jseg
//       plan_frame (zd_plan.h) over a frame of three compressed blocks: A with
//       5 sequences, FSE tables and a Huffman tree, B with 0 sequences and Raw
//       literals, C with 3 sequences, every mode Repeat_Mode, Treeless literals.
//       flag 0: the reference keys the frame at B (D2); ZD_F_RFC: no key, B
//       takes no FSE slot and is on no list, C's tables and tree are A's.
//   H sum maxw st_ref bits_ref last_ref st_rfc bits_rfc last_rfc
//       huf_close (zd_huf.h) for every sum in 1..4096 and three values of maxw
// Exit status 4: a counting pass and its filling pass disagree.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_huf.h"
#include "../../zstd-decompressor_amd/csrc/zd_plan.h"

using namespace zd;

struct NoJ {
  void note(uint64_t) {}
};

static void long_count(uint32_t extra) {
  // 1 Raw literal, the long-form count, mode byte 0x54 (all RLE) and its three symbols
  const uint8_t blk[] = {1 << 3, 'Z', 255, (uint8_t)(extra & 255), (uint8_t)(extra >> 8), 0x54, 0, 2, 0, 1};
  uint32_t n[2];
  for (int k = 0; k < 2; k++) {
    CompBlock cb;
    zero_bytes(&cb, sizeof cb);
    WalkErr e;
    const int r = parse_compressed(blk, 0, sizeof blk, &cb, &e, k ? walk_opts(false, false, true) : 0u);
    n[k] = r ? 0xFFFFFFFFu : cb.nseq;
  }
  printf("N %u %u %u\n", extra, n[0], n[1]);
}

static void empty_stream() {
  // Compressed literals, size format 1 (4 streams, 10-bit sizes): regen 8, a
  // direct tree description of 2 weights, jump table 1, 1, 0, a last stream of 1
  std::vector<uint8_t> b;
  const uint32_t regen = 8, csize = 2 + 6 + 3;
  const uint32_t h = 2u | (1u << 2) | (regen << 4) | (csize << 14);
  b.push_back(h & 255); b.push_back((h >> 8) & 255); b.push_back((h >> 16) & 255);
  b.push_back(129); b.push_back(0x11);                     // header byte 129: 2 weights, 1 and 1
  const uint8_t jump[6] = {1, 0, 1, 0, 0, 0};
  b.insert(b.end(), jump, jump + 6);
  b.push_back(1); b.push_back(1); b.push_back(1);          // streams 1, 2 and 4 (3 is empty)
  b.push_back(0);                                          // Number_of_Sequences 0
  int st[2];
  uint32_t ns = 0;
  for (int k = 0; k < 2; k++) {
    CompBlock cb;
    zero_bytes(&cb, sizeof cb);
    WalkErr e;
    st[k] = parse_compressed(b.data(), 0, (uint32_t)b.size(), &cb, &e, k ? walk_opts(false, false, true) : 0u);
    if (!k) ns = cb.nstreams;
  }
  printf("S %d %u %d\n", st[0], ns, st[1]);
}

static int plan_case(uint32_t flags) {
  HostBlock blocks[3];
  for (int i = 0; i < 3; i++) {
    HostBlock& b = blocks[i];
    zero_bytes(&b, sizeof b);
    b.src = 64ull * i + 16;
    b.size = 40;
    b.type = 2;
    b.last = i == 2;
    b.cb.src = b.src;
    b.cb.size = b.size;
    b.cb.lit_regen = 20;
    b.cb.host_stage = PS_ALL;
  }
  blocks[0].cb.lit_type = LIT_COMPRESSED; blocks[0].cb.nstreams = 1; blocks[0].cb.stream_size[0] = 9;
  blocks[0].cb.nseq = 5;
  blocks[0].cb.modes[0] = blocks[0].cb.modes[1] = blocks[0].cb.modes[2] = M_FSE;
  blocks[1].cb.lit_type = LIT_RAW;
  blocks[1].cb.nseq = 0;                                   // (parse_compressed leaves the modes M_REPEAT)
  blocks[1].cb.modes[0] = blocks[1].cb.modes[1] = blocks[1].cb.modes[2] = M_REPEAT;
  blocks[2].cb.lit_type = LIT_TREELESS; blocks[2].cb.nstreams = 1; blocks[2].cb.stream_size[0] = 9;
  blocks[2].cb.nseq = 3;
  blocks[2].cb.modes[0] = blocks[2].cb.modes[1] = blocks[2].cb.modes[2] = M_REPEAT;
  HostFrame f;
  zero_bytes(&f, sizeof f);
  f.d.src_size = 200;
  f.d.content_size = UINT64_MAX;
  f.d.dict_id = UINT64_MAX;
  f.d.kind = ZD_FRAME_ZSTD;
  f.nb = 3;
  f.ncomp = 3;
  f.key = KEY_NONE;

  PlanCtx X{};
  X.prev_huf = X.prev_tab[0] = X.prev_tab[1] = X.prev_tab[2] = -1;
  X.rep0[0] = 1; X.rep0[1] = 4; X.rep0[2] = 8;
  X.flags = flags;
  X.k4j_mode = 1;                                          // K4J: the frame's scatter segments are counted
  PlanCounts cc;
  const Sink none{};
  plan_frame<false, NoJ>(X, f, blocks, cc, none, nullptr);

  const size_t n = 8;
  PlanCounts c;
  std::vector<CompBlock> comps(n);
  std::vector<BlockRec> brec(n);
  std::vector<FrameDesc> fdesc(1);
  std::vector<FrameState> fstate(1);
  std::vector<uint32_t> lt(n), lh(n), ls(n, 99), lk(n);
  std::vector<CopyDesc> copies(n);
  std::vector<JFrame> jf(1);
  std::vector<JBlkDesc> jb(n);
  std::vector<JSegDesc> js(n);
  std::vector<uint64_t> fout(1), fcap(1);
  Sink S{};
  S.comps = comps.data(); S.blocks = brec.data(); S.fdesc = fdesc.data(); S.fstate0 = fstate.data();
  S.list_tables = lt.data(); S.list_huf = lh.data(); S.list_seq = ls.data(); S.list_k4f = lk.data();
  S.copies = copies.data();
  S.jframes = jf.data(); S.jblkd = jb.data(); S.jsegd = js.data();
  S.frame_out = fout.data(); S.frame_cap = fcap.data();
  plan_frame<true, NoJ>(X, f, blocks, c, S, nullptr);
  if (memcmp(&c, &cc, sizeof c) != 0) return 4;
  const uint64_t key = fstate[0].key;
  printf("P %u %d %u %llu %llu", flags, key_code(key), key == KEY_NONE ? 0u : key_block(key),
         (unsigned long long)c.fses, (unsigned long long)c.seq);
  for (uint64_t i = 0; i < c.seq; i++) printf(" %u", ls[i]);
  printf(" | %u %d %d %d %d %u %llu\n", comps[1].fse_slot, comps[2].tab_src[0], comps[2].tab_src[1],
         comps[2].tab_src[2], comps[2].huf_src, comps[0].rfc, (unsigned long long)c.jseg);
  return 0;
}

int main() {
  long_count(0);
  long_count(88);
  long_count(0xFFFF);
  empty_stream();
  if (int r = plan_case(0)) return r;
  if (int r = plan_case(ZD_F_RFC)) return r;
  for (uint32_t sum = 1; sum <= 4096; sum++) {
    const uint32_t maxws[3] = {1, (uint32_t)hb32(sum) + 1, 13};
    for (uint32_t maxw : maxws) {
      int b0 = -1, b1 = -1;
      uint32_t l0 = 0, l1 = 0;
      const int s0 = huf_close(sum, maxw, false, &b0, &l0);
      const int s1 = huf_close(sum, maxw, true, &b1, &l1);
      printf("H %u %u %d %d %u %d %d %u\n", sum, maxw, s0, s0 ? -1 : b0, s0 ? 0 : l0, s1, s1 ? -1 : b1, s1 ? 0 : l1);
    }
  }
  return 0;
}
