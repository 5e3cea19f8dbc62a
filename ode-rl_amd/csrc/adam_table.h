// adam_table.h -- what the multi-tensor optimizer launches share (adam.hip, adamax.hip): the table of tensor pointers that travels as a
// kernel argument, and the grid of an elementwise launch over one chunk of it.
#pragma once

namespace odehip {

constexpr int kAdamChunk = 24;  // tensors per launch (pointers travel as kernel arguments)
struct AdamTable {
  float* p[kAdamChunk];
  const float* g[kAdamChunk];
  float* m[kAdamChunk];
  float* v[kAdamChunk];   // the second state tensor: Adam's exp_avg_sq, Adamax's exp_inf
  long long n[kAdamChunk];
};

// workgroups per tensor of an elementwise launch over a chunk whose largest tensor has nmax elements (adam_kernel's grid)
static inline int update_blocks(long long nmax) {
  const long long b = (nmax + 255) / 256;
  return b < 1 ? 1 : (b > 1024 ? 1024 : (int)b);
}

}  // namespace odehip
