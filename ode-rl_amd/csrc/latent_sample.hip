// latent_sample.hip -- z0 drawn from N(mean_z0, std_z0) by the reparameterisation trick, its KL term against N(0, 1), and the
// backward of both: the mode the reference declares (`opt.z_sample`, configs.yaml; models/ODEConvGRU.py:72-77 "TODO:
// reparametrization trick") and never finishes.  One launch forward, one backward, no host round trip, nothing stored in between.
//
//   forward   z0[k*B + b] = fma(std[b], eps[k, b], mean[b])                         k = 0 .. K-1 (sample-major)
//             kl[b]       = sum_{c,h,w} 0.5 (mean^2 + std^2 - 1) - log std          == kl_divergence(Normal(mean, std), Normal(0, 1))
//   backward  grad_mean[b] = sum_k g[k, b]          + grad_kl[b] mean
//             grad_std[b]  = sum_k g[k, b] eps[k,b] + grad_kl[b] (std - 1 / std)
//
// Noise stream (the definition is the header's, include/odecgru_hip.h: odehip_latent_sample).  Counter-based: element quad q of the
// GLOBAL (K, B_global, C, 16, 16) noise tensor, q = ((k B_global + b_global) C + c) 64 + pixel / 4, is Philox4x32-10 with key = seed
// and counter = (q lo, q hi, offset lo, offset hi): four words -> four uniforms -> two Box-Muller pairs -> four normals, stored with
// one 16-byte store.  A quad never looks at the launch geometry or at the shard it is drawn in: a shard that passes its batch_offset
// gets the rows of the full draw bit for bit, and the backward regenerates exactly what the forward used.
//
// Layout.  Forward: grid (B, K), 1024 threads; workgroup (b, k) walks the C * 64 quads of sample b with 16-byte loads and stores.
// The k = 0 workgroup of every b also forms kl[b]: per element in float64 (the whole term, log included -- 16 elements per thread at
// C = 64, nothing next to the Philox rounds), summed per thread in quad order, then reduce.h's workgroup sum (16 waves); rounded
// to fp32 once.  No atomics: two calls are bitwise equal, and kl[b] depends on nothing but sample b.
// Backward: one thread per quad of (B, C, 16, 16); it walks k = 0 .. K-1 in order with explicit fmas (contraction off), so the
// regenerated-noise call and the eps_in call run the same arithmetic.  No clamp anywhere: std = 0 gives kl = +inf and z0 = mean, a
// NaN stays a NaN in its own sample.
#include <math.h>
#include <stdint.h>

#include "odehip_internal.h"
#include "reduce.h"

namespace odehip {

constexpr int kLatent = 16;                      // the latent map is 16 x 16 (resolution 64, n_downs 2)
constexpr int kQuadsPerPlane = kLatent * kLatent / 4;
constexpr int kSampleThreads = 1024;

typedef float f32x4s __attribute__((ext_vector_type(4)));

struct NoiseKey {
  uint32_t seed_lo, seed_hi, off_lo, off_hi;
};

// Philox4x32-10 (Salmon et al., SC'11), the Random123 constants
__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t out[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    const uint32_t hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0, out[1] = c1, out[2] = c2, out[3] = c3;
}

// word -> uniform in (0, 1): u = ((w >> 9) + 0.5) 2^-23, 24 significant bits, exact in fp32
__device__ __forceinline__ float word_uniform(uint32_t w) { return ((float)(w >> 9) + 0.5f) * 0x1p-23f; }

// the four normals of global quad q: (r0 cos, r0 sin, r1 cos, r1 sin), r_i = sqrt(-2 ln u(w_2i)), angle 2 pi u(w_2i+1)
__device__ __forceinline__ f32x4s noise_quad(unsigned long long q, NoiseKey key) {
  uint32_t w[4];
  philox4x32_10((uint32_t)q, (uint32_t)(q >> 32), key.off_lo, key.off_hi, key.seed_lo, key.seed_hi, w);
  f32x4s e;
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const float r = sqrtf(-2.0f * logf(word_uniform(w[2 * p])));
    float s, c;
    sincospif(2.0f * word_uniform(w[2 * p + 1]), &s, &c);   // the argument is exact; no large-argument reduction is ever needed
    e[2 * p] = r * c;
    e[2 * p + 1] = r * s;
  }
  return e;
}

// grid (batch, n_samples); eps_in / eps_out / kl may be NULL
__global__ __launch_bounds__(kSampleThreads) void latent_sample_kernel(const float* __restrict__ mean, const float* __restrict__ std_, int batch,
                                                                       int channels, NoiseKey key, int batch_offset, int global_batch,
                                                                       const float* __restrict__ eps_in, float* __restrict__ z0,
                                                                       float* __restrict__ kl, float* __restrict__ eps_out) {
#pragma clang fp contract(off)
  __shared__ double red[kSampleThreads / 64];
  const int b = blockIdx.x, k = blockIdx.y, tid = threadIdx.x;
  const int quads = channels * kQuadsPerPlane;
  const f32x4s* const pm = (const f32x4s*)mean + (long long)b * quads;
  const f32x4s* const ps = (const f32x4s*)std_ + (long long)b * quads;
  const long long row = ((long long)k * batch + b) * quads;                                           // of this shard's tensors
  const unsigned long long qrow = ((unsigned long long)k * global_batch + batch_offset + b) * quads;   // of the global noise tensor
  const bool with_kl = kl != nullptr && k == 0;
  double acc = 0.0;
  for (int q = tid; q < quads; q += kSampleThreads) {
    const f32x4s m = pm[q], s = ps[q];
    const f32x4s e = eps_in ? ((const f32x4s*)eps_in)[row + q] : noise_quad(qrow + q, key);
    f32x4s z;
#pragma unroll
    for (int i = 0; i < 4; ++i) z[i] = fmaf(s[i], e[i], m[i]);
    ((f32x4s*)z0)[row + q] = z;
    if (eps_out) ((f32x4s*)eps_out)[row + q] = e;
    if (with_kl) {
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const double md = (double)m[i], sd = (double)s[i];
        acc += 0.5 * (md * md + sd * sd - 1.0) - log(sd);
      }
    }
  }
  if (!with_kl) return;   // uniform over the workgroup
  const double t = group_sum<kSampleThreads>(acc, red);
  if (tid == 0) kl[b] = (float)t;
}

// one thread per quad of (batch, channels, 16, 16); grad_kl / eps_in may be NULL
__global__ __launch_bounds__(256) void latent_sample_backward_kernel(const float* __restrict__ grad_z0, const float* __restrict__ grad_kl,
                                                                     const float* __restrict__ mean, const float* __restrict__ std_, int batch,
                                                                     int channels, int n_samples, NoiseKey key, int batch_offset,
                                                                     int global_batch, const float* __restrict__ eps_in,
                                                                     float* __restrict__ grad_mean, float* __restrict__ grad_std) {
#pragma clang fp contract(off)
  const int quads = channels * kQuadsPerPlane;
  const long long total = (long long)batch * quads;
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int b = (int)(idx / quads), q = (int)(idx - (long long)b * quads);
  f32x4s gm = {0.0f, 0.0f, 0.0f, 0.0f}, gs = gm;
  for (int k = 0; k < n_samples; ++k) {
    const long long at = ((long long)k * batch + b) * quads + q;
    const f32x4s g = ((const f32x4s*)grad_z0)[at];
    const f32x4s e = eps_in ? ((const f32x4s*)eps_in)[at]
                            : noise_quad(((unsigned long long)k * global_batch + batch_offset + b) * quads + q, key);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gm[i] = k ? gm[i] + g[i] : g[i];
      gs[i] = k ? fmaf(g[i], e[i], gs[i]) : g[i] * e[i];
    }
  }
  if (grad_kl) {
    const float w = grad_kl[b];
    const f32x4s m = ((const f32x4s*)mean)[idx], s = ((const f32x4s*)std_)[idx];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      gm[i] = fmaf(w, m[i], gm[i]);
      gs[i] = fmaf(w, s[i] - 1.0f / s[i], gs[i]);
    }
  }
  ((f32x4s*)grad_mean)[idx] = gm;
  ((f32x4s*)grad_std)[idx] = gs;
}

static NoiseKey make_key(unsigned long long seed, unsigned long long offset) {
  return NoiseKey{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32)};
}

// the checks both calls share; 0 or ODEHIP_EINVAL (message set)
static int check_sample_shape(const char* who, int batch, int channels, int height, int width, int n_samples, int batch_offset, int global_batch) {
  ODEHIP_REQUIRE(batch >= 1 && n_samples >= 1, "%s: batch (%d) and n_samples (%d) must be at least 1", who, batch, n_samples);
  ODEHIP_REQUIRE(height == kLatent && width == kLatent && channels >= 4 && channels % 4 == 0,
                 "%s: unsupported latent shape (channels %d, %d x %d): a multiple of 4 channels of 16 x 16 only", who, channels, height, width);
  ODEHIP_REQUIRE(batch_offset >= 0 && global_batch >= 1 && (long long)batch_offset + batch <= global_batch,
                 "%s: the shard [%d, %d + %d) does not lie in the global batch of %d", who, batch_offset, batch_offset, batch, global_batch);
  ODEHIP_REQUIRE(n_samples <= 65535, "%s: n_samples (%d) exceeds the grid limit of 65535", who, n_samples);
  ODEHIP_REQUIRE((long long)n_samples * batch * channels * kQuadsPerPlane <= 0x7fffffffLL * 256,
                 "%s: n_samples * batch * channels (%d x %d x %d) exceeds the grid limit", who, n_samples, batch, channels);
  return ODEHIP_OK;
}

}  // namespace odehip

using namespace odehip;

extern "C" int odehip_latent_sample(const float* mean, const float* std, int batch, int channels, int height, int width, int n_samples,
                                    uint64_t seed, uint64_t offset, int batch_offset, int global_batch, const float* eps_in, float* z0,
                                    float* kl, float* eps_out, void* stream) {
  ODEHIP_REQUIRE(mean && std && z0, "latent_sample: null pointer");
  if (int rc = check_sample_shape("latent_sample", batch, channels, height, width, n_samples, batch_offset, global_batch)) return rc;
  hipLaunchKernelGGL(latent_sample_kernel, dim3((unsigned)batch, (unsigned)n_samples), dim3(kSampleThreads), 0, (hipStream_t)stream, mean, std,
                     batch, channels, make_key(seed, offset), batch_offset, global_batch, eps_in, z0, kl, eps_out);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

extern "C" int odehip_latent_sample_backward(const float* grad_z0, const float* grad_kl, const float* mean, const float* std, int batch,
                                             int channels, int height, int width, int n_samples, uint64_t seed, uint64_t offset,
                                             int batch_offset, int global_batch, const float* eps_in, float* grad_mean, float* grad_std,
                                             void* stream) {
  ODEHIP_REQUIRE(grad_z0 && mean && std && grad_mean && grad_std, "latent_sample_backward: null pointer");
  if (int rc = check_sample_shape("latent_sample_backward", batch, channels, height, width, n_samples, batch_offset, global_batch)) return rc;
  const long long total = (long long)batch * channels * kQuadsPerPlane;
  hipLaunchKernelGGL(latent_sample_backward_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, grad_z0, grad_kl,
                     mean, std, batch, channels, n_samples, make_key(seed, offset), batch_offset, global_batch, eps_in, grad_mean, grad_std);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
