// convgru_cell.h -- the internal interface of the ConvGRU family: what its files share (convgru.hip, convgru_plain.hip, convgru_backward.hip, convgru_sequence.hip): the device
// helpers of the GroupNorm / gate kernels, and the host functions each of them writes ONCE for the others -- the forward cell step, the
// reverse cell step, the encoder's forward loop and its workspace.
// In the Q4 layout a 32-channel group of one sample is 32 KiB contiguous, so a workgroup of 256 threads holds its whole group in
// registers (8 x f32x4 per thread): statistics are exact two-pass fp32.
#pragma once
#include <string.h>

#include "odehip_internal.h"

namespace odehip {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// Sum of v over the 256 threads of the workgroup: wave shuffles, then the four wave sums meet in LDS.  The LAST add exists in two
// orders, and both stay: kPairwise = false is ((s0 + s1) + s2) + s3, what the forward kernels (gn_gates_kernel, gn_update_kernel) have
// always computed; kPairwise = true is (s0 + s1) + (s2 + s3), what the backward kernels (normalise and gn_backward in
// gn_update_bwd_kernel, gn_gates_bwd_kernel) have.  So the statistics the backward recomputes can differ from the forward's in the
// last bit.  Making them one order changes gradient bits (or forward bits) and is a decision of its own.
template <bool kPairwise>
__device__ __forceinline__ float block_sum(float v, float* sh) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
  __syncthreads();
  return kPairwise ? (sh[0] + sh[1]) + (sh[2] + sh[3]) : sh[0] + sh[1] + sh[2] + sh[3];
}

// the (sample b, group g) slab: 8 quads x 256 px x 4 ch; thread t owns pixel t of every quad
__device__ __forceinline__ void load_group(const float* src, int b, int groups, int g, f32x4 (&v)[8]) {
  const f32x4* p = (const f32x4*)(src + ((size_t)(b * groups + g) * 8) * kPix * 4) + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = p[q * kPix];
}
__device__ __forceinline__ void store_group(float* dst, int b, int groups, int g, const f32x4 (&v)[8]) {
  f32x4* p = (f32x4*)(dst + ((size_t)(b * groups + g) * 8) * kPix * 4) + threadIdx.x;
#pragma unroll
  for (int q = 0; q < 8; ++q) p[q * kPix] = v[q];
}

// two-pass statistics of the group in v (8192 values): mean and 1 / sqrt(var + eps)
template <bool kPairwise>
__device__ __forceinline__ void group_stats(const f32x4 (&v)[8], float eps, float* sh, float& mean, float& rstd) {
  float s = 0.0f;
#pragma unroll
  for (int q = 0; q < 8; ++q) s += (v[q].x + v[q].y) + (v[q].z + v[q].w);
  mean = block_sum<kPairwise>(s, sh) * (1.0f / 8192.0f);
  float ss = 0.0f;
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 d = v[q] - mean;
    ss += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
  }
  const float var = block_sum<kPairwise>(ss, sh) * (1.0f / 8192.0f);
  rstd = 1.0f / sqrtf(var + eps);
}

// x -> GroupNorm(x) with its affine, in place (the forward kernels: serial block sum)
__device__ __forceinline__ void group_norm(f32x4 (&v)[8], const float* gamma, const float* beta, int g, float eps, float* sh) {
  float mean, rstd;
  group_stats<false>(v, eps, sh, mean, rstd);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const f32x4 ga = *(const f32x4*)(gamma + g * 32 + q * 4), be = *(const f32x4*)(beta + g * 32 + q * 4);
    v[q] = (v[q] - mean) * rstd * ga + be;
  }
}

// x -> xhat in place, returns rstd (the backward kernels: pairwise block sum, see block_sum)
__device__ __forceinline__ float normalise(f32x4 (&v)[8], float* sh) {
  float mean, rstd;
  group_stats<true>(v, 1e-5f, sh, mean, rstd);
#pragma unroll
  for (int q = 0; q < 8; ++q) v[q] = (v[q] - mean) * rstd;
  return rstd;
}

__device__ __forceinline__ float sigmoidf_(float x) { return 1.0f / (1.0f + __expf(-x)); }
__device__ __forceinline__ f32x4 sigmoid4(const f32x4 v) { return f32x4{sigmoidf_(v.x), sigmoidf_(v.y), sigmoidf_(v.z), sigmoidf_(v.w)}; }
__device__ __forceinline__ f32x4 tanh4(const f32x4 v) { return f32x4{tanhf(v.x), tanhf(v.y), tanhf(v.z), tanhf(v.w)}; }

// the instantiations of gn_update_kernel (convgru.hip): every sample observed, or a mask row
enum UpdateMode { kUpdPlain, kUpdMasked };

// ---- forward (convgru.hip) ------------------------------------------------------------------------------------------------------
int check_cell(const odehip_convgru_cell* c);
// one convolution over one or two Q4 sources.  direct = false: launch_conv's dispatch by kernel size and images.
int conv_layer(const float* src1, const float* src2, int cin1, int cin, int cout, int ks, const float* wp, const float* bias, float* dst,
               int relu, int batch, hipStream_t stream, const void* w_bf16 = nullptr, const float* w_wino = nullptr, bool direct = false);
// One ConvGRU step on Q4 tensors.  x == null or h == null (a zero frame / a zero state; never both) runs one-source convolutions
// over the weight halves of hv, which a sequence passes and a single step leaves null.  h_out_nchw (may be null): the state is also
// written to this NCHW slot, sample b at + b * nchw_batch_stride.  mask_b: the step's B observation mask values on the device or
// null.  Scratch: gates_raw (B,2H), z, rh, cand_raw (B,H).
int cell_forward_step(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv, const float* x, const float* h, float* h_out,
                      float* h_out_nchw, long long nchw_batch_stride, int batch, float* gates_raw, float* z, float* rh, float* cand_raw,
                      const float* mask_b, hipStream_t stream);
// small tables (bytes % 4 == 0) travel as kernel arguments, 256 bytes per launch: asynchronous, no pageable-host copy on the stream
int upload_bytes(void* dst, const void* src, size_t bytes, hipStream_t stream);

// The step-size rule of the reference's loop (ODEConvGRUCell.py:47,73), known here and nowhere else.  Euler step in front of the
// idx-th visited frame: first t[-1] - (t[-1] + 0.01); after visiting frame j the loop sets (prev_t, t_i) = (t[j], t[j-1]) -- Python
// indexing, so j = 0 wraps to t[-1].  Frames are visited T-1 .. 0 (run_backwards, what forward() does, :33) or 0 .. T-1.
inline float frame_dt(const double* t_host, int n_frames, int idx, int run_backwards) {
  if (idx == 0) return (float)(t_host[n_frames - 1] - (t_host[n_frames - 1] + 0.01));
  const int j = run_backwards ? n_frames - idx : idx - 1;  // frame visited at iteration idx - 1
  return (float)(t_host[(j + n_frames - 1) % n_frames] - t_host[j]);
}
inline int visited_frame(int n_frames, int idx, int run_backwards) { return run_backwards ? n_frames - 1 - idx : idx; }

// Workspace of the encoder; one place knows where everything lives.  train = false: two state slots and one step's buffers;
// train = true: a slot per step for everything the reverse sweep reads, and the sweep's own buffers behind them.
struct EncLayout {
  int T, B, C, NH, NG, HH, OUT2;
  bool train;
  size_t hs, fh, hh, ho;
  size_t off_dts, off_frames, off_ping, off_pong, off_hstate, off_hidden, off_hode, off_gates, off_z, off_rh, off_cand, off_headhid,
      off_headout;
  size_t off_gp, off_ggates, off_gcand, off_gx, off_gzpre, off_ghode, off_gxc, off_grh, off_gh, off_gheadout, off_gheadhid, off_pgg,
      off_pgc, off_tab, off_slab, total;
  EncLayout(const odehip_encoder* e, int n_frames, int batch, bool train_) : train(train_) {
    T = n_frames; B = batch; C = e->cell.hidden; NH = e->f_enc.n_convs - 1; NG = grad_slots(&e->f_enc); HH = e->head_hidden; OUT2 = 2 * e->out_ch;
    hs = al256((size_t)B * C * kPix * 4);
    int cmax = max_hidden(&e->f_enc);
    if (train) {  // the gradient slots of the dynamics' input and output have this size too
      const int c_in = e->f_enc.channels[0], c_out = e->f_enc.channels[e->f_enc.n_convs];
      cmax = c_in > cmax ? c_in : cmax;
      cmax = c_out > cmax ? c_out : cmax;
    }
    fh = al256((size_t)B * cmax * kPix * 4);
    hh = al256((size_t)B * HH * kPix * 4);
    ho = al256((size_t)B * OUT2 * kPix * 4);
    size_t o = 0;
    auto take = [&](size_t b) { size_t r = o; o += al256(b); return r; };
    const size_t per = train ? (size_t)T : 1;
    off_dts = take((size_t)T * 4);
    off_frames = take((size_t)T * hs);
    off_ping = take(fh);
    off_pong = take(fh);
    off_hstate = take((train ? (size_t)T + 1 : 2) * hs);
    off_hidden = take(train ? (size_t)T * (NH > 0 ? NH : 1) * fh : 0);
    off_hode = take(per * hs);
    off_gates = take(per * 2 * hs);
    off_z = take(per * hs);
    off_rh = take(per * hs);
    off_cand = take(per * hs);
    off_headhid = take(hh);
    off_headout = take(ho);
    off_gp = off_ggates = off_gcand = off_gx = off_gzpre = off_ghode = off_gxc = off_grh = off_gh = off_gheadout = off_gheadhid = off_pgg =
        off_pgc = off_tab = off_slab = o;
    if (train) {
      off_gp = take((size_t)T * NG * fh);
      off_ggates = take((size_t)T * 2 * hs);
      off_gcand = take((size_t)T * hs);
      off_gx = take((size_t)T * hs);
      off_gzpre = take(hs);
      off_ghode = take(hs);
      off_gxc = take(hs);
      off_grh = take(hs);
      off_gh = take(2 * hs);
      off_gheadout = take(ho);
      off_gheadhid = take(hh);
      off_pgg = take((size_t)2 * T * B * 2 * C * 4);
      off_pgc = take((size_t)2 * T * B * C * 4);
      off_tab = take((size_t)(ODEHIP_MAX_LAYERS + 6) * T * sizeof(WgradPair));  // every weight-gradient table of a backward pass: ONE upload
      off_slab = take(wgrad_slab_bytes(B));
    }
    total = o;
  }
  float* p(void* ws, size_t off) const { return (float*)((char*)ws + off); }
  float* frame(void* ws, int i) const { return p(ws, off_frames + (size_t)i * hs); }
  float* hstate(void* ws, int k) const { return p(ws, off_hstate + (size_t)(train ? k : (k & 1)) * hs); }  // the state BEFORE step k
  float* hidden(void* ws, int idx, int l) const { return p(ws, off_hidden + ((size_t)idx * NH + l) * fh); }
  float* gp(void* ws, int idx, int l) const { return p(ws, off_gp + ((size_t)idx * NG + l) * fh); }
  float* per(void* ws, size_t off, int idx, size_t bytes) const { return p(ws, off + (train ? (size_t)idx * bytes : 0)); }
};

// train: the reverse sweep's kernels need channel counts that are multiples of 64 and 3x3 dynamics on top
int check_encoder(const odehip_encoder* e, bool train, const char* who);
// The encoder's forward loop over the visited frames (Euler combine, observed or not, latent slot, cell), then head and split.
// L.train keeps what the reverse sweep reads.  mask_tb / step_observed_host / cell_steps_run: as odehip_odeconvgru_encode_steps.
int encoder_forward(const odehip_encoder* e, const EncLayout& L, void* ws, const float* inputs_nchw, const double* t_host,
                    int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw, const float* mask_tb,
                    const unsigned char* step_observed_host, int* cell_steps_run, hipStream_t stream);

// ---- reverse (convgru_backward.hip) ---------------------------------------------------------------------------------------------
// input-gradient convolution (transposed + flipped weight images) of one Q4 source; combine 0 stores to dst, 2 / 3 end in *bw
int conv_bwd(const float* src, int cin, int cout, int ks, const float* wt, const void* w_bf16, const float* w_wino, int combine,
             const BwdArgs* bw, float* dst, int batch, hipStream_t stream);
// epilogue target  out = srcA + conv (+ srcB)
inline BwdArgs bwd_target(float* out, const float* srcA, const float* srcB = nullptr) {
  BwdArgs w;
  memset(&w, 0, sizeof(w));
  w.n_targets = 1;
  w.tgt[0].out = out;
  w.tgt[0].srcA = srcA;
  w.tgt[0].a_c = 1.0f;
  w.tgt[0].g_c = 1.0f;
  if (srcB) {
    w.tgt[0].srcB = srcB;
    w.tgt[0].b_c = 1.0f;
  }
  return w;
}
// the four transposed weight halves, in the order gates/x, gates/h, can/x, can/h (odehip_convgru_cell_bwd, odehip_encoder_bwd)
struct CellDgradW {
  const float* packed[4];
  const void* bf16[4];
  const float* wino[4];
};
template <class Bwd>  // odehip_convgru_cell_bwd or odehip_encoder_bwd; with_bf16 = false leaves the bf16 images out
inline CellDgradW dgrad_images(const Bwd* b, bool with_bf16 = true) {
  CellDgradW w;
  const float* packed[4] = {b->w_gates_dx, b->w_gates_dh, b->w_can_dx, b->w_can_dh};
  for (int j = 0; j < 4; ++j) {
    w.packed[j] = packed[j];
    w.bf16[j] = with_bf16 ? b->bf16[j] : nullptr;
    w.wino[j] = b->wino[j];
  }
  return w;
}
struct CellBwdStep {
  const float *cand_raw, *z, *gates_raw, *h_prev;  // what the forward kept; h_prev = the state the cell was given
  const float* gh;                                 // gradient at the state the step left
  float *g_cand, *g_gates;                         // out: gradients of the two conv outputs (the weight gradient reads them later)
  float *gz_pre, *gh_prev, *gx_c, *g_rh;           // scratch; gh_prev and gx_c are srcA of the two targets
  float *pgc_w, *pgc_b, *pgg_w, *pgg_b;            // this step's GroupNorm partial rows (dgamma, dbeta of the candidate / the gates)
  const float* mask_b;                             // the step's observation mask values or null
  bool has_x, has_h;                               // false: a zero frame / a zero state -- its convolutions do not run
};
// The reverse of one ConvGRU step: update backward, the candidate's two input-gradient convs (-> gx_c, g_rh), gates backward, the
// gates' two input-gradient convs, whose epilogues write frame_tgt (the frame's gradient) and state_tgt (the gradient at h_prev).
int cell_backward_step(const odehip_convgru_cell* c, const CellDgradW& w, const CellBwdStep& s, const BwdArgs& frame_tgt,
                       const BwdArgs& state_tgt, int batch, hipStream_t stream);
// fixed-order sums of the GroupNorm affine partials: pgg = [dgamma | dbeta][rows][2H], pgc = [dgamma | dbeta][rows][H]
void reduce_gn_partials(const float* pgg, const float* pgc, int rows, int hidden, float* gn_gates_w, float* gn_gates_b, float* gn_can_w,
                        float* gn_can_b, hipStream_t stream);
// Weight-gradient table entries of the two convs on cat(x, state): four tables [gates/x | gates/h | can/x | can/r*h], `stride` entries
// apart, entry k of each from step k of the list.
struct CatStep {
  const float *g_gates, *g_cand, *x, *h, *rh;
};
inline void cat_wgrad_entries(WgradPair* tab, size_t stride, const CatStep* steps, int n) {
  for (int j = 0; j < 2; ++j)
    for (int half = 0; half < 2; ++half)
      for (int k = 0; k < n; ++k) {
        WgradPair& e = tab[(size_t)(2 * j + half) * stride + k];
        e.g = j == 0 ? steps[k].g_gates : steps[k].g_cand;
        e.a = half == 0 ? steps[k].x : (j == 0 ? steps[k].h : steps[k].rh);
        e.scale = 1.0f;
      }
}

}  // namespace odehip
