// Host driver of the batch chunk walk (zd_walk.h index_chunk, the code
// zd_k_walk_chunks runs one lane per chunk): reads chunks from a file of
// [u32 length][bytes] records, laid out the way zd_batch_create gathers them
// (16-byte aligned offsets, ZD_SRC_PADDING zero bytes after each), walks each
// chunk bounded by its own size and prints one line per chunk:
//   status  frame kind  blocks kept  compressed blocks  content size  bytes left
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_walk.h"

using namespace zd;

struct Sink {
  std::vector<HostBlock> v;
  size_t size() const { return v.size(); }
  void push(const HostBlock& b) { v.push_back(b); }
};

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const bool rfc_empty_lits = argc > 2 && !strcmp(argv[2], "dict");
  std::vector<uint8_t> buf;
  std::vector<uint64_t> off, size;
  uint32_t n;
  while (fread(&n, 4, 1, f) == 1) {
    off.push_back(buf.size());
    size.push_back(n);
    buf.resize(buf.size() + (n + 15) / 16 * 16 + ZD_SRC_PADDING, 0);
    if (n && fread(buf.data() + off.back(), 1, n, f) != n) return 2;
  }
  fclose(f);
  Sink S;
  for (size_t i = 0; i < off.size(); i++) {
    Bytes in{buf.data() + off[i], (size_t)size[i]};
    HostFrame hf;
    const int r = index_chunk(buf.data(), in, &hf, S, rfc_empty_lits);
    if (r != hf.status || (r != 0) != (hf.key != KEY_NONE) || key_code(hf.key) != r) return 3;
    if (hf.b0 + hf.nb != S.size()) return 4;
    printf("%d %u %u %u %lld %zu\n", r, hf.d.kind, hf.nb, hf.ncomp, (long long)hf.d.content_size, in.n);
  }
  return 0;
}
