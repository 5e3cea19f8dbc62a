// Internal declarations shared by the HIP translation units of libodecgru_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>
#include <time.h>

#include "../../include/odecgru_hip.h"
#include "dopri5_control.h"

namespace odehip {

constexpr int kHW = 16;           // latent maps are 16x16 (models/ODEConvGRU.py:18-20)
constexpr int kPix = kHW * kHW;   // 256 pixels
constexpr int kQuadBytes = kPix * 16;  // one channel-quad plane of the Q4 layout: 256 px * 4 ch * 4 B

void set_error(const char* fmt, ...);
int hip_fail(hipError_t e, const char* what);

#define ODEHIP_CHECK_HIP(expr)                                   \
  do {                                                           \
    hipError_t e__ = (expr);                                     \
    if (e__ != hipSuccess) return ::odehip::hip_fail(e__, #expr); \
  } while (0)

#define ODEHIP_REQUIRE(cond, ...)            \
  do {                                       \
    if (!(cond)) {                           \
      ::odehip::set_error(__VA_ARGS__);      \
      return ODEHIP_EINVAL;                  \
    }                                        \
  } while (0)

// ---- activation codes of ConvArgs::act
constexpr int kActNone = 0;
constexpr int kActRelu = 1;
constexpr int kActTanh = 2;
// reverse sweep of a Tanh head (combine 0 only, per-layer kernels only): the head's conv is evaluated again and
// dst = bwd.mask_src * (1 - tanh(conv)^2), in place (dst == mask_src: the adjoint of f's output becomes that of the head's input)
constexpr int kActTanhSeed = 3;
// combine 2 of a layer whose forward conv ran in bf16 (epilogue() of the 32x32-accumulator kernels only): the Tanh derivative from
// the saved output as that conv consumed it, dst = scale * acc * (1 - bf16(mask_src)^2)
constexpr int kActTanhBf16 = 4;

// ---- stage-combine epilogue of the LAST conv of f (Runge-Kutta bookkeeping fused in) -------
// k_cur = conv output.  Optional outputs, all Q4 unless stated:
//   k_out             <- k_cur
//   out1              <- y + h * ( sum_{j<n_prev} c1[j]*k_prev[j] + c1[n_prev]*k_cur )
//   out2 (+out2_nchw) <- y + h * ( sum c2 ... )            (used for the step result y_{n+1})
// h = *h_ptr (device scalar; the step size of this interval), so one captured graph serves any t.
struct CombineArgs {
  const float* y;
  const float* k_prev[ODEHIP_MAX_STAGES];
  float* k_out;
  float* out1;
  float* out2;
  float* out2_nchw;
  const float* h_ptr;
  int n_prev;
  float c1[ODEHIP_MAX_STAGES + 1];
  float c2[ODEHIP_MAX_STAGES + 1];
  float k_scale;  // k_cur is multiplied by this first (-1 for backwards=True / reversed time)
  // adaptive error norm (dopri5, last stage): err = h * (sum_j ce[j]*k_prev[j] + ce[n_prev]*k_cur),
  // tol = atol + rtol*max(|y|, |err_y1|); every wave writes sum((err/tol)^2) of its 32x32 tile to
  // err_partials[4*workgroup + wave] (no atomics: the controller adds them in a fixed order)
  const float* err_y1;
  float* err_partials;
  float ce[ODEHIP_MAX_STAGES + 1];
  float rtol, atol;
  // Summation order of the stage combine.  0 (fixed-grid drivers): s = c[n]*k_cur, then += c[j]*k_prev[j].  1 (the adaptive
  // solver's drivers): explicit fmas over k_prev[0..n-1] FIRST, k_cur last, out = fma(s, h, y) -- the part that does not depend
  // on the conv output can then be formed while the matrix cores still work on the layer (the persistent walk's adaptive kernel
  // holds three partial sums instead of up to six earlier stages), and every kernel that evaluates the expression rounds it the
  // same way (no contraction left to the compiler), so the walk stays bit-identical to one launch per layer.
  int order;
  const float* c_dev;   // elementwise rows only: if non-null, c1[j] is read from this DEVICE array instead (coefficients a device-side
                        // controller computed, e.g. the dense-output weights of an accepted step)
};
// ---- elementwise rows (ConvArgs::combine == 4): no convolution.  Uses the CombineArgs fields:
//   out1 = (y ? y : 0) + sum_{j < n_prev} (c1[j] * hs) * k_prev[j]        hs = *h_ptr (1 if null)
//   out2 = (y ? y : 0) + sum_{j < n_prev} (c2[j] * hs) * k_prev[j]        (only if out2 != null)
// evaluated as explicit fmas in j order.  In a persistent walk a lane only touches the elements the conv epilogues give it
// (channel quad Q of its 2x2 output tile), i.e. data it wrote itself: no wait, no barrier; the row then announces itself like a layer.

// ---- epilogues of the input-gradient (dgrad) convolutions of the backward sweep
//   combine == 2: dst = scale * acc * (mask_src > 0)            (ReLU backward fused; scale = sc_c + sc_h*h)
//                 dst = scale * acc * (1 - mask_src^2)          (act == kActTanh: Tanh backward; mask_src = the Tanh output)
//   combine == 3: gx = acc; up to 4 targets  out_t = (a_c+a_h*h)*srcA_t + (b_c+b_h*h)*srcB_t + (g_c+g_h*h)*gx
//                 (the reverse Runge-Kutta bookkeeping: gy += gx, gk_j += c*h*gx, next interval's seed, ...)
struct BwdTarget {
  float* out;
  const float* srcA;
  const float* srcB;
  float a_c, a_h, b_c, b_h, g_c, g_h;
};
struct BwdArgs {
  const float* mask_src;
  float sc_c, sc_h;
  int n_targets;
  BwdTarget tgt[4];
  const float* h_ptr;
};

struct ConvArgs {
  const float* src1;
  const float* src2;
  const float* w_packed;
  const float* w_wino;   // Winograd-transformed weights (pack_winograd) or null
  const void* w_bf16;    // bf16 A-operand image (pack_conv_weight_bf16) or null: non-null selects bf16 compute for 3x3 layers
  const float* bias;
  float* dst;
  int q1;      // channel quads in src1
  int qin;     // total input quads
  int qout;    // output quads (cout / 4)
  int batch;
  int act;     // activation code (kAct*): combine 0 / 1 apply it to the conv output (bias included) before the store / stage combine;
               // combine 2 takes the derivative of the layer it masks from it (kActTanh: g * (1 - y^2), else the ReLU mask)
  int combine; // 0: plain store (+act); 1: CombineArgs epilogue; 2/3: BwdArgs epilogues; 4: elementwise row (no conv; see above);
               // 5: norm row (adaptive walk only): err_partials <- per-wave sums of ((k_prev[0] - k_prev[1]) / (atol + |y| rtol))^2
  int debug;   // diagnostic ablation bits (tools/conv_microbench.py): 1 skip DMA, 2 skip MFMA, 4 skip epilogue
  int h_by_value;  // persistent tables of fixed-grid drivers: cmb.atol holds the step size itself (read instead of *h_ptr)
  int dep_back;    // adaptive walk: 1 = this row does NOT depend on the row right in front of it (two independent chains woven into
                   // one table, e.g. the input-gradient chain of a stage and the forward chain of the next): its producers only wait
                   // for the row before that, i.e. they load and transform its input while the consumers still multiply the other
                   // chain's row -- the partner hand-off leaves the critical path
  const int* skip;          // if non-null and *skip != 0 the kernel does nothing (adaptive solver already done)
  unsigned long long* dbg;  // debug & 8: per-workgroup stamps (8 x u64 per workgroup)
  CombineArgs cmb;
  BwdArgs bwd;
};

int launch_conv(const ConvArgs& a, int ks, hipStream_t stream);
// While non-null (set by a driver on its own thread), launch_conv() appends its argument here INSTEAD of launching: the driver
// collects the layer sequence of a whole trajectory and hands it to the persistent kernel (conv_wino.hip).
struct ConvRecorder {
  ConvArgs* items;
  int count, capacity;
};
extern thread_local ConvRecorder* g_conv_recorder;
constexpr int kDoneStride = 64;   // words between the per-sample flag lines of the trajectory walks (a 256-byte line each)
int launch_wino_persist(const ConvArgs* table_dev, int n_layers, int batch, unsigned* done, unsigned* xcc_of, unsigned* host_err_dev,
                        float* out_nchw, int grid, hipStream_t stream, bool wide = false,  // wide: the table has 128-channel layers
                        bool adaptive = false, const int* n_layers_ptr = nullptr,           // adaptive: wino_persist_d_kernel (order-1
                        const unsigned long long* reloc = nullptr,                          // combines, elementwise rows, h on the device;
                        bool strip = false);                                                // {row0, rows} and relocation bases on the device)
                                                                                            // strip: wino_persist_strip_kernel (row strips,
                                                                                            // one sample per group, fixed-grid tables)
int launch_ew_row(const ConvArgs& a, hipStream_t stream);
// forward tables of a 64-channel stack at batch <= 16: sixteen workgroups per sample (conv_wino.hip, wino_persist16_kernel)
int launch_wino_persist16(const ConvArgs* table_dev, int n_layers, int batch, unsigned* done, unsigned* xcc_of, unsigned* host_err_dev,
                          float* out_nchw, hipStream_t stream, const int* n_layers_ptr = nullptr, const unsigned long long* reloc = nullptr);
// error-norm / norm-row partials per sample that a walk of `batch` samples writes: 64 on the sixteen-workgroup walk (batch <= 16, walk
// available and not switched off), else the per-layer kernels' 16 (64-channel stacks).  Decided BEFORE the rows run: a controller must
// know how many partials to add.
int persist_partials_per_sample(int batch);   // an elementwise row (combine == 4) as an ordinary launch
int launch_wino(const ConvArgs& a, hipStream_t stream);
int launch_wino5(const ConvArgs& a, hipStream_t stream);  // 5x5 layers with a.w_wino (conv_wino5.hip); 1 = no such form, run the direct kernel
int launch_bf16(const ConvArgs& a, hipStream_t stream);
int launch_bf16_5x5(const ConvArgs& a, hipStream_t stream);

// whole-stack bf16 launch (fstack_bf16.hip)
struct FusedArgs {
  const float* x;                          // stage input (B,64) Q4 fp32
  const void* w_fused;                     // [layer][tap][cb 4][mb 2][lane 64][8] bf16, execution order
  const float* bias[ODEHIP_MAX_LAYERS];    // per executed layer (null: none)
  float* store[ODEHIP_MAX_LAYERS];         // fp32 Q4 output of executed layer e < n-1 (null: not stored)
  const float* mask[ODEHIP_MAX_LAYERS];    // e < n-1: null -> the activation, else its derivative from the saved output `mask`:
                                           // output *= (mask > 0), or with act == kActTanh output *= 1 - bf16(mask)^2
  int n_layers;
  int act;                                 // hidden activation: kActRelu or kActTanh
  ConvArgs last;                           // epilogue of the last executed layer (qout = 16)
};
int launch_fstack_bf16(const FusedArgs& fa, int batch, hipStream_t stream);
// whole fixed-grid trajectory of a fused-bf16 64-channel stack in one launch (forward only, nothing saved)
int launch_ftraj_bf16(const odehip_convstack* f, int method, const float* z0_nchw, float* out_nchw, const float* hdev, int n_times,
                      int batch, int negate, hipStream_t stream);
extern int g_debug_flags;
extern unsigned long long* g_debug_buf;


// ---- shared host-side helpers (api.hip, wgrad.hip) ---------------------------------------------------------------------------
static inline size_t al256(size_t v) { return (v + 255) / 256 * 256; }

int check_stack(const odehip_convstack* f);
// Gradient slots per evaluation in the backward layouts: one per conv output (n_convs), plus, with a Tanh head, the head's masked
// seed gp * (1 - K^2) (slot n_convs; written by enqueue_dgrad_chain).  Stacks without a head keep their layouts byte for byte.
inline int grad_slots(const odehip_convstack* f) { return f->n_convs + (f->final_tanh ? 1 : 0); }
// the gradient slot the weight gradient of layer l reads: its output's, or for a Tanh head's conv the masked seed
inline int wgrad_slot(const odehip_convstack* f, int l) { return (f->final_tanh && l == f->n_convs - 1) ? f->n_convs : l; }
// every layer 64 -> 64, 3x3: the stacks the adaptive persistent walk takes (their adaptive drivers write order-1 stage combines)
inline bool all_64(const odehip_convstack* f) {
  if (f->ks != 3) return false;
  for (int l = 0; l <= f->n_convs; ++l)
    if (f->channels[l] != 64) return false;
  return true;
}
// prologue of a fixed-grid trajectory in one launch: NCHW -> Q4 + verbatim copy (solution[0] = y0), n_h <= 64 step sizes into hdev,
// n_zero words zeroed (the persistent launch's flag area; may be null)
int traj_prologue(const float* src, float* dst_q4, float* copy_nchw, int batch, int channels, const float* h_host, int n_h, float* hdev,
                  unsigned* zero_words, int n_zero, hipStream_t stream);
int max_hidden(const odehip_convstack* f);
// ---- the norm-free ConvGRU cell (convgru_plain.hip): a descriptor whose four gn_* pointers are all NULL; reset gate first
inline bool cell_is_plain(const odehip_convgru_cell* c) { return !c->gn_gates_w && !c->gn_gates_b && !c->gn_can_w && !c->gn_can_b; }
void launch_plain_gates(const float* gates_raw, const float* h, float* u, float* rh, int hidden, int batch, hipStream_t stream);
void launch_plain_update(const float* cand_raw, const float* h, const float* u, float* h_out, float* h_out_nchw, long long nchw_batch_stride,
                         int hidden, int batch, const float* mask_b, hipStream_t stream);
void launch_plain_update_bwd(const float* cand_raw, const float* gh, const float* u, const float* h, float* g_cand_raw, float* g_gates_raw,
                             float* gh_out, int hidden, int batch, const float* mask_b, hipStream_t stream);
void launch_plain_gates_bwd(const float* gates_raw, const float* g_rh, const float* h, float* gh_io, float* g_gates_raw, int hidden,
                            int batch, const float* mask_b, hipStream_t stream);
// the host step hint of the odehip_odeconvgru_encode*_steps entry points: FRAME i runs the cell unless its byte is 0 (null: every frame)
inline bool step_is_observed(const unsigned char* step_observed_host, int frame) { return !step_observed_host || step_observed_host[frame] != 0; }
// Q4 state (B,hidden) -> the NCHW latent slot of a step whose cell did not run (convgru.hip)
void launch_state_to_latent(const float* h, float* h_out_nchw, long long nchw_batch_stride, int hidden, int batch, hipStream_t stream);
int upload_floats(float* dst, const float* src, int n, hipStream_t stream);  // scalars travel as kernel arguments (async)
// the entries that differentiate NEGATED solves (fixed_grid.hip, dopri5.hip, dopri5_backward.hip) take fp32 images only: no layer of
// f, or of f_dgrad where there is one, may carry a bf16 image
inline int check_fp32_stacks(const odehip_convstack* f, const odehip_convstack* f_dgrad, const char* who) {
  ODEHIP_REQUIRE(f, "%s: null stack", who);
  ODEHIP_REQUIRE(!f->w_fused && !(f_dgrad && f_dgrad->w_fused), "%s: fp32 stacks only (the stack carries a fused bf16 image)", who);
  for (int l = 0; l < f->n_convs && l < ODEHIP_MAX_LAYERS; ++l)
    ODEHIP_REQUIRE(!f->w_bf16[l] && !(f_dgrad && f_dgrad->w_bf16[l]), "%s: fp32 stacks only (layer %d carries a bf16 image)", who, l);
  return ODEHIP_OK;
}
// f(x) with the stage combine fused into the last conv; `hidden` (n_convs-1 buffers) keeps the ReLU outputs for a backward pass
int enqueue_f(const odehip_convstack* f, const float* x_q4, int batch, float* ping, float* pong, const CombineArgs* cmb,
              float* plain_dst, const int* skip, hipStream_t stream);
int enqueue_f_saving(const odehip_convstack* f, const float* x_q4, int batch, float* const* hidden, float* ping, float* pong,
                     const CombineArgs* cmb, float* plain_dst, const int* skip, hipStream_t stream);

// Input-gradient chain of one evaluation of f: gp[n_convs-1] holds the gradient w.r.t. f's output; with a Tanh head it is first
// turned into that of the head's input, written to gp[n_convs] (grad_slots(f) entries; gp[n_convs-1] is left as it was: drivers
// read it again, e.g. as the adjoint state); for l = n_convs-1 .. 1 the
// gradient w.r.t. conv l's input is masked with hidden[l-1] (the activation's derivative) and written to gp[l-1]; conv 0 ends in `last` (combine 3
// with last.bwd, or combine 1 with last.cmb; its src/weights/shape fields are filled here).  One fused bf16 launch when
// f_dgrad carries a fused image, else one launch per layer.
int enqueue_dgrad_chain(const odehip_convstack* f, const odehip_convstack* f_dgrad, int batch, float* const* gp,
                        const float* const* hidden, const ConvArgs& last, hipStream_t stream);

// one (gradient, activation, weight) triple of the batched weight-gradient kernels (wgrad.hip)
struct WgradPair {
  const float* g;  // gradient w.r.t. the layer's output (Q4)
  const float* a;  // the layer's input (Q4)
  float scale;     // weight of this evaluation in the sum (1 for discretise-then-optimise; dt*b_s for the adjoint)
  float pad_[3];
};
// floats per workgroup slab of the weight-gradient kernels: the Winograd-domain tile [16 positions][64][64] + 64 bias sums is the
// largest; every slab region holds batch * esplit of them PLUS ONE (the fixed-order sum before the final G^T . G)
constexpr int kWgradSlabFloats = 16 * 64 * 64 + 64;
// Workgroups per sample of a batched weight-gradient launch (each walks every esplit-th evaluation): 4 at the batches the chip is
// full anyway; small batches split the evaluations further so that the launch still covers the CUs (B = 4: 16 workgroups walked
// nine evaluations each -- 215 us per layer, the time of a B = 64 launch).  At most 256 slabs, as at B = 64.
inline int wgrad_esplit(int batch, int n_eval) {
  int e = batch > 0 ? 256 / batch : 4;
  if (e > n_eval) e = n_eval;
  return e < 4 ? 4 : e;
}
inline int wgrad_esplit_max(int batch) { return batch >= 64 ? 4 : (256 / batch < 4 ? 4 : 256 / batch); }
// bytes of the slab area of every weight-gradient caller: the slabs of the largest esplit and the one of the sum
inline size_t wgrad_slab_bytes(int batch) { return ((size_t)batch * wgrad_esplit_max(batch) + 1) * kWgradSlabFloats * 4; }

// One 64 x 64 tile of dW (cout_total, cin_total, ks, ks): output channels co0.. from G tensors with g_quads quads per sample (tile at
// quad g_quad0), input channels ci0.. of the WEIGHT from A tensors with a_quads quads per sample (tile at a_quad0) -- the A tensor may be
// one half of a concatenated conv input.  esplit workgroups per sample share the n_eval table entries; slabs: wgrad_slab_bytes(batch).
struct WgradTile {
  const WgradPair* table;
  int n_eval, batch, esplit;
  float* slabs;
  float* dw;
  float* db;
  int ks, cin_total, co0, ci0;
  int g_quads, g_quad0, a_quads, a_quad0;
  bool write_bias;
};
// The weight gradient of one conv operand (wgrad.hip), walked in 64 x 64 tiles: G has cout channels, A the cin channels that sit at
// ci_off of the conv's cin_total input channels (a plain layer: cin_total = cin, ci_off = 0).  bias: these launches carry the bias sums
// (db is written with the tiles ci0 == 0).  bf16: operands rounded to bf16 (fp32 accumulation; 3x3 and 5x5), for layers in bf16 compute
// mode.  fp32 3x3 whole layers and fp32 5x5 tiles run in the Winograd domain unless switched off.
int launch_wgrad_layer(const WgradPair* table_dev, int n_eval, int batch, int esplit, float* slabs, float* dw, float* db, int ks, int cout,
                       int cin, int cin_total, int ci_off, bool bf16, bool bias, hipStream_t stream);
// a plain 3x3 layer
inline int launch_wgrad(const WgradPair* table_dev, int n_eval, int batch, int esplit, float* slabs, float* dw, float* db, int cout,
                        int cin, hipStream_t stream, bool bf16 = false) {
  return launch_wgrad_layer(table_dev, n_eval, batch, esplit, slabs, dw, db, 3, cout, cin, cin, 0, bf16, true, stream);
}
int launch_wgrad_q4h(const WgradPair* table_dev, int n_eval, int batch, int esplit, float* slabs, float* dw, int accumulate,
                     hipStream_t stream);
// the fp32 3x3 layer in the Winograd F(2x2,3x3) domain (wgrad_wino.hip); 1 = switched off
int launch_wgrad_wino(const WgradPair* table_dev, int n_eval, int batch, int esplit, float* slabs, float* dw, float* db, int cout,
                      int cin, hipStream_t stream);
// a 64 x 64 tile of a 5x5 weight gradient in the Winograd F(2x2,5x5) domain (wgrad_wino5.hip); 1 = switched off
int launch_wgrad_wino5(const WgradTile& t, hipStream_t stream);
// sum[i] = sum over k < n_slabs of slabs[k * stride + i], i < n_vals, in a fixed order (16 interleaved partial sums of 4 chains each,
// 16-byte loads: bitwise reproducible).  stride and n_vals multiples of 4 floats, slabs and sum 16-byte aligned.  (wgrad.hip)
void launch_slab_sum4(const float* slabs, int n_slabs, int stride, int n_vals, float* sum, hipStream_t stream);
// raises the dynamic-LDS limit of a weight-gradient kernel to 160 KiB, once per kernel (wgrad.hip)
int wgrad_raise_lds(const void* kernel);

int launch_ftraj_bf16_saving(const odehip_convstack* f, const float* z0_nchw, float* out_nchw, const float* hdev, int n_times, int batch,
                             void* save_x, size_t stride_x, void* save_h, size_t stride_h_eval, size_t stride_h_layer,
                             hipStream_t stream);
// reverse sweep over the intervals n_hi-1 .. n_lo (n_hi == n_times-1: starts from grad_out[T-1], else from state_g / state_seed as the
// previous segment left them; n_lo == 0: writes grad_z0, else leaves its state in state_g / state_seed); bias_part: [B][NL][64]
int launch_btraj_bf16_rk4(const odehip_convstack* f_dgrad, const float* grad_out_nchw, float* grad_z0_nchw, const float* hdev, int n_times,
                          int batch, int n_lo, int n_hi, float* state_g, float* state_seed, const void* save_h, size_t stride_h_eval,
                          size_t stride_h_layer, void* save_g, size_t stride_g_eval, size_t stride_g_layer, float* bias_part,
                          hipStream_t stream);
// grad_b[l][ch] = sum over segments and samples of bias_part[seg][b][l][ch], in order
int launch_bias_reduce(const float* bias_part, int n_parts, int n_layers, float* const* grad_b, hipStream_t stream);

// ---- the adaptive solver's drivers (dopri5.hip, dopri5_backward.hip, adjoint_dopri5.hip, adjoint_device.hip) ------------------
// The stage combine behind k_s = f(x_s) of an attempt with tableau tb (S = tb.stages), s = 2 .. S (stage s lives at index s - 1 of
// k): stages 2 .. S - 1 form the next stage input x_{s+1} = y + h * sum beta_{s+1,j} k_j in out_next (s = S - 1: y1 -- c_sol equals
// the last beta row), stage S the error norm against out_next = y1.  The caller sets k_scale and order afterwards.
inline void adaptive_stage_combine(const Tableau& tb, CombineArgs& c, int s, const float* y, const float* h_ptr, float* const* k,
                                   float* out_next, float* err_partials, float rtol, float atol) {
  memset(&c, 0, sizeof(c));
  c.y = y;
  c.h_ptr = h_ptr;
  c.n_prev = s - 1;
  for (int j = 0; j < s - 1; ++j) c.k_prev[j] = k[j];
  c.k_out = k[s - 1];
  if (s < tb.stages) {
    for (int j = 0; j < s; ++j) c.c1[j] = (float)tb.beta[s - 1][j];
    c.out1 = out_next;
  } else {
    for (int j = 0; j < tb.stages; ++j) c.ce[j] = (float)tb.c_err[j];
    c.err_y1 = out_next;
    c.err_partials = err_partials;
    c.rtol = rtol;
    c.atol = atol;
  }
}

// The host's watch on the progress word of a pinned mailbox a device-side controller writes: the limit is on time WITHOUT
// progress, not on the whole integration.
struct MailboxWatch {
  const volatile int* word;
  int seen;
  double t_progress;
  explicit MailboxWatch(const volatile int* w) : word(w), seen(*w), t_progress(now_s()) {}
  static double now_s() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + 1e-9 * ts.tv_nsec;
  }
  bool stalled() {   // true once 120 s have passed without the word changing
    if (*word != seen) {
      seen = *word;
      t_progress = now_s();
    }
    return now_s() - t_progress > 120.0;
  }
};

inline void write_stats(int* stats_host, int nfe, int n_accept, int n_reject) {
  if (!stats_host) return;
  stats_host[0] = nfe;
  stats_host[1] = n_accept;
  stats_host[2] = n_reject;
}

// the status a device-side controller ended on as the error of its entry point (0: none; mname: the tableau's name); returns the status
inline int controller_error(const char* mname, bool adjoint, int status, int max_accept = 0) {
  if (!adjoint) {
    if (status == ODEHIP_ENAN) set_error("odeint_%s: non-finite error ratio (non-finite values in state `y`)", mname);
    else if (status == ODEHIP_ENOTCONV) set_error("odeint_%s: underflow in dt or max_num_steps exceeded", mname);
    else return ODEHIP_OK;
  } else if (status == ODEHIP_ENAN) {
    set_error("odeint_adjoint_%s_backward: non-finite error ratio", mname);
  } else if (status == ODEHIP_ENOTCONV) {
    set_error("odeint_adjoint_%s_backward: underflow in dt", mname);
  } else if (status != 0) {
    set_error("odeint_adjoint_%s_backward: more than max_accept = %d accepted steps", mname, max_accept);
  }
  return status;
}

}  // namespace odehip
