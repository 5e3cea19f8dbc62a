// dopri5_reduce.h -- the fixed-order reductions behind the adaptive solver's norms, shared by dopri5.hip (which defines the two
// kernels) and adjoint_dopri5.hip.
#pragma once
#include <hip/hip_runtime.h>

namespace odehip {

// Halving tree over the 256 values a 256-thread workgroup has just written to sh[threadIdx.x]; the sum (fixed order) is in sh[0].
__device__ inline float block_tree_sum(float* sh) {
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
    __syncthreads();
  }
  return sh[0];
}

// partial sums of ((a - b) / (atol + |y|*rtol))^2 per workgroup (b may be null)
__global__ __launch_bounds__(256) void scaled_sumsq_kernel(const float* __restrict__ a, const float* __restrict__ b,
                                                           const float* __restrict__ y, float atol, float rtol,
                                                           long long n4, float* __restrict__ partials);

// out[j] = fixed-order sum of partial array j (one workgroup): a strided partial sum per thread, then the halving tree.  If skip is
// non-null and *skip != 0 the kernel does nothing.
struct SumSet {
  const float* p[4];
  int n[4];
  int count;
};
__global__ __launch_bounds__(256) void sum_partials_kernel(SumSet ss, float* __restrict__ out, const int* skip);

}  // namespace odehip
