// Host driver of the frame walk's window limit (zd_walk.h index_frame, the
// call the host walk, zd_k_walk and zd_k_walk_chunks make for every frame;
// index_chunk and chunk_size_query over it): one frame from a file, walked with
// the options given as the second argument (0: none, 2: WALK_LONG_WINDOW, what
// ZD_F_LONG_WINDOW / ZD_SIZES_LONG_WINDOW set).  Three lines, one per call:
//   status  blocks kept  Window_Size  bytes left
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../zstd-decompressor_amd/csrc/zd_walk.h"

using namespace zd;

struct Sink {
  std::vector<HostBlock> v;
  size_t size() const { return v.size(); }
  void push(const HostBlock& b) { v.push_back(b); }
};

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) return 2;
  const uint32_t wopt = (uint32_t)atoi(argv[2]);
  std::vector<uint8_t> buf(1 << 20);
  const size_t n = fread(buf.data(), 1, buf.size() - ZD_SRC_PADDING, f);
  fclose(f);
  {
    Sink S;
    Bytes in{buf.data(), n};
    HostFrame hf;
    const int r = index_frame(buf.data(), in, &hf, S, wopt);
    if (r != hf.status || key_code(hf.key) != r) return 3;
    printf("%d %u %llu %zu\n", r, hf.nb, (unsigned long long)hf.d.window_size, in.n);
  }
  {
    Sink S;
    Bytes in{buf.data(), n};
    HostFrame hf;
    const int r = index_chunk(buf.data(), in, &hf, S, wopt);
    printf("%d %u %llu %zu\n", r, hf.nb, (unsigned long long)hf.d.window_size, in.n);
  }
  {
    uint64_t reserve = 0;
    uint8_t exact = 0;
    const int r = chunk_size_query(buf.data(), n, wopt, &reserve, &exact);
    printf("%d %llu %u 0\n", r, (unsigned long long)reserve, exact);
  }
  return 0;
}
