// reduce.h -- the reproducible sums of the training step (losses, LSGAN, gradient norm, KL, InstanceNorm, metrics): the ONE place
// where their order is defined.  (The solver's float halving tree is a different order and lives in dopri5_reduce.h.)
//
//   thread      a thread adds its own elements in ascending order (the caller's loop)
//   wave        wave_sum: the 64 lanes by an xor-butterfly, offsets 32, 16, .. 1
//   workgroup   group_sum: lane 0 of every wave stores its sum, thread 0 adds them in wave order, starting from 0
//   launch      ordered_sum: a one-workgroup second launch adds the per-workgroup float64 partials in index order, starting from 0
//
// Which elements a thread sees, and how many partials there are, is a function of the sizes alone (sum_groups): no atomics, no
// arrival order, so two calls are bitwise equal on any device.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace odehip {

constexpr int kSumMaxGroups = 1024;      // workgroup partials of a launch at most = the doubles ordered_sum stages in LDS at a time
constexpr int kSumItemsPerGroup = 2048;  // below kSumMaxGroups groups a 256-thread workgroup walks this many items: 8 per thread

// workgroups (= partials) of a sum over `items` items
static inline int sum_groups(long long items) {
  const long long g = (items + kSumItemsPerGroup - 1) / kSumItemsPerGroup;
  return g < 1 ? 1 : (g > kSumMaxGroups ? kSumMaxGroups : (int)g);
}

static inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// float, double or unsigned; every lane gets the sum
template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// The sum of a kThreads-wide workgroup, returned to thread 0 (the others get 0).  red: kThreads / 64 doubles of LDS, which thread 0
// may still be reading on return: a caller that uses red again puts a barrier in between.
template <int kThreads>
__device__ __forceinline__ double group_sum(double v, double* red) {
  v = wave_sum(v);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  double t = 0.0;
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) t += red[w];
  }
  return t;
}

// ... returned to every thread.  red: kThreads / 64 + 1 doubles of LDS, free again on return.
template <int kThreads>
__device__ __forceinline__ double group_sum_all(double v, double* red) {
  const double t = group_sum<kThreads>(v, red);
  if (threadIdx.x == 0) red[kThreads / 64] = t;
  __syncthreads();
  const double all = red[kThreads / 64];
  __syncthreads();
  return all;
}

// One workgroup: partials[0 .. n) added in index order by thread 0, which gets the sum.  They pass through `stage` (kSumMaxGroups
// doubles of LDS, free again on return), kSumMaxGroups at a time, one running sum.
template <int kThreads>
__device__ __forceinline__ double ordered_sum(const double* __restrict__ partials, long long n, double* stage) {
  double s = 0.0;
  for (long long base = 0; base < n; base += kSumMaxGroups) {
    const int m = n - base < kSumMaxGroups ? (int)(n - base) : kSumMaxGroups;
    for (int i = threadIdx.x; i < m; i += kThreads) stage[i] = partials[base + i];
    __syncthreads();
    if (threadIdx.x == 0)
      for (int i = 0; i < m; ++i) s += stage[i];
    __syncthreads();
  }
  return s;
}

}  // namespace odehip
