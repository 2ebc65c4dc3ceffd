// Strided [B, H, S, D] addressing shared by the attention kernels
// (attention.hip, attention_decode.hip).
#pragma once

#include <cstdint>

// Strides are in elements; the innermost (D) dim must be contiguous.
// Strided addressing lets the packed qkv layout [B, S, heads, 3*D] feed the
// kernel directly — no permute/contiguous copies on the hot path.
struct AttnStrides {
  int64_t qb, qh, qs;  // q batch/head/seq strides
  int64_t kb, kh, ks;
  int64_t vb, vh, vs;
  int64_t ob, oh, os;
};

// s: the launcher's 12-entry array, q(3) k(3) v(3) o(3)
static inline AttnStrides attn_strides(const int64_t* s) {
  return {s[0], s[1], s[2], s[3], s[4], s[5],
          s[6], s[7], s[8], s[9], s[10], s[11]};
}
