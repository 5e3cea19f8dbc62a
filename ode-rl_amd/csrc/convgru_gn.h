// convgru_gn.h -- device helpers of the ConvGRU GroupNorm / gate kernels (convgru.hip, convgru_sequence.hip): in the Q4 layout a
// 32-channel group of one sample is 32 KiB contiguous, so a workgroup of 256 threads holds its whole group in registers.
#pragma once
#include "odehip_internal.h"

namespace odehip {

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float block_reduce_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return sh[0] + sh[1] + sh[2] + sh[3];
}

// loads the (sample b, group g) slab: 8 quads x 256 px x 4 ch; thread t owns pixel t of every quad
__device__ __forceinline__ void load_group(const float* src, int b, int groups, int g, f32x4 (&v)[8]) {
  const f32x4* p = (const f32x4*)(src + ((size_t)(b * groups + g) * 8) * kPix * 4) + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = p[q * kPix];
}

__device__ __forceinline__ void group_norm(f32x4 (&v)[8], const float* gamma, const float* beta, int g, float eps, float* sh) {
  float s = 0.0f;
#pragma unroll
  for (int q = 0; q < 8; ++q) s += (v[q].x + v[q].y) + (v[q].z + v[q].w);
  const float mean = block_reduce_sum(s, sh) * (1.0f / 8192.0f);
  float ss = 0.0f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 d = v[q] - mean;
    ss += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
  }
  const float var = block_reduce_sum(ss, sh) * (1.0f / 8192.0f);
  const float rstd = 1.0f / sqrtf(var + eps);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 ga = *(const f32x4*)(gamma + g * 32 + q * 4), be = *(const f32x4*)(beta + g * 32 + q * 4);
    v[q] = (v[q] - mean) * rstd * ga + be;
  }
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }

}  // namespace odehip
