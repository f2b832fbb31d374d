// zd_huf.h — the end of HuffmanDecoder::from_weights (huffman.rs:177-203):
// from the listed weights' total to Max_Number_of_Bits and the weight of the
// implied last symbol.  One copy of the rule for K1's three tree builders
// (zd_kernels.hip k1_huffman_lane, k1_huffman_huge, k1_huffman_parse; the
// dictionary's tree, zd_k_dict_tables, goes through the first) and for the
// native test (tests/native/huf_close.cpp).
#pragma once
#include <stdint.h>

#include "../../include/zd.h"
#include "zd_common.h"

namespace zd {

// sum: the total of 2^(w - 1) over the listed non-zero weights (the callers
// stop with ZD_E_REF_PANIC themselves at a weight above 32 or a total past 32
// bits); maxw: the largest listed weight.  On 0, *bits is Max_Number_of_Bits
// and *last the last symbol's weight (its code has *bits + 1 - *last bits).
//  rfc == false, the reference: bits = ceil(log2(sum)), so a total that is a
//    power of two leaves nothing to fill and is ZD_E_REF_PANIC (D3); what is
//    left is truncated `as u8` before its highest bit is taken, a 0 after that
//    panics as well, and so does a weight above bits + 1.
//  rfc == true, RFC 8878 4.2.1.1: bits = highbit(sum) + 1, what is left to
//    2^bits must be a power of two, else ZD_E_CORRUPTED_TABLE (so must a total
//    of 0 or one of 2^31 and more be, which no tree of the format has).
ZD_HD inline int huf_close(uint32_t sum, uint32_t maxw, bool rfc, int* bits, uint32_t* last) {
  if (rfc) {
    if (sum == 0 || sum >= (1u << 31)) return ZD_E_CORRUPTED_TABLE;
    const int p = hb32(sum) + 1;
    const uint32_t rest = (1u << p) - sum;            // 1 .. 2^(p - 1)
    if (rest & (rest - 1)) return ZD_E_CORRUPTED_TABLE;
    *bits = p;
    *last = (uint32_t)hb32(rest) + 1;                 // <= p, and every listed weight is (2^(w - 1) <= sum < 2^p)
    return 0;
  }
  if (sum == 0) return ZD_E_REF_PANIC;
  int p = hb32(sum);
  if ((1ull << p) < sum) p++;
  if (p >= 32) return ZD_E_REF_PANIC;
  const uint8_t rest = (uint8_t)((1u << p) - sum);
  if (rest == 0) return ZD_E_REF_PANIC;               // D3
  const uint32_t manquant = (uint32_t)hb32(rest) + 1;
  if (maxw > (uint32_t)p + 1 || manquant > (uint32_t)p + 1) return ZD_E_REF_PANIC;
  *bits = p;
  *last = manquant;
  return 0;
}

}  // namespace zd
