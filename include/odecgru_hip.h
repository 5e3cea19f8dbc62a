/* odecgru_hip.h -- C ABI of the MI355X (gfx950) Neural-ODE hot path.
 *
 * The reference (jithendaraa/ODE-RL) has no FFI: its hot path is Python calling
 * `torchdiffeq.odeint(func, y0, t, rtol=, atol=, method=)` (modules/DiffEqSolver.py:37,45-46)
 * on a conv dynamics `f` built by `utils.create_convnet` (helpers/utils.py:158-183), plus the
 * Euler+ConvGRU encoder loop (modules/ODEConvGRUCell.py:39-78, modules/ConvGRUCell.py:55-86).
 * These entry points are what a native binding for that path would bind:
 * plain pointers and sizes, device pointers are HIP device memory, `stream` is a hipStream_t.
 *
 * Conventions
 *   - every function returns 0 on success, a negative ODEHIP_E* code on failure;
 *     odehip_last_error() returns a static string for the calling thread.
 *   - scratch comes from caller-provided workspaces sized by the *_bytes() queries, and the compute entry points
 *     are enqueue-only on the caller's stream, WITH THESE EXCEPTIONS (each is stated again at its entry point):
 *       * the persistent-launch layer table: the library keeps up to 8 layer tables in device memory it owns; a call
 *         whose table is not cached yet synchronises the stream once, may hipMalloc, and uploads with a blocking copy
 *         (a steady loop re-uses its table: nothing is allocated, copied or synchronised);
 *       * odehip_odeint_dopri5 returns after the device-side controller has reported completion: it polls a pinned
 *         64 KiB host mailbox that the library allocates on first use (hipHostMalloc);
 *       * odehip_odeint_adjoint_dopri5_backward reads one 8-byte verdict per attempted step from pinned host memory it
 *         allocates on first use;
 *       * tables that follow the accepted steps of an adaptive solve (odehip_odeint_dopri5_backward[_saved]: its layer table and its
 *         weight-gradient tables) travel through a library-owned ring of pinned staging buffers and device slots with asynchronous
 *         copies on the caller's stream -- no stream synchronisation (hipHostMalloc / hipMalloc when a slot has to grow);
 *       * odehip_odeint_fixed_backward with saved_format 1 (bf16 whole-trajectory path) runs its weight-gradient launches on a
 *         library-owned side stream, ordered against the caller's stream by events in both directions (the caller's stream
 *         continues only when the side stream is done with the workspace and the gradients).
 *   - library state (table cache, mailbox, error word, flag areas) is process-global and serves ONE stream at a time:
 *     the library assumes one process per GPU driving it from a single stream (the Python binding passes torch's
 *     current stream); concurrent calls from several streams or threads are not supported.
 *   - a persistent launch whose in-kernel wait gives up (never observed; every wait is capped) sets a sticky error
 *     word: the outputs of the call that was running are filled with NaN, odehip_persistent_error() reports the code,
 *     and the next call that could use the persistent path fails with ODEHIP_EINVAL.
 *   - boundary tensors are fp32 NCHW, contiguous, H = W = 16 (the reference's latent map,
 *     models/ODEConvGRU.py:18-20 with resolution 64, n_downs 2).  Internally activations use
 *     the "Q4" layout [B][C/4][256 pixels][4 channels].
 */
#ifndef ODECGRU_HIP_H
#define ODECGRU_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ODEHIP_ABI_VERSION 13 /* == odehip_version(); bumped whenever a struct layout or a signature below changes */
#define ODEHIP_MAX_LAYERS 8
#define ODEHIP_MAX_STAGES 7

enum {
  ODEHIP_OK = 0,
  ODEHIP_EINVAL = -1,   /* bad shape / argument (the Python side raises ValueError) */
  ODEHIP_EHIP = -2,     /* a HIP runtime call failed */
  ODEHIP_ENOTCONV = -3, /* adaptive solver hit max_num_steps / dt underflow (AssertionError in torchdiffeq) */
  ODEHIP_ENAN = -4,     /* non-finite state (the reference asserts: modules/ODEConvGRUCell.py:56,59) */
  ODEHIP_ETRUNC = -5    /* asynchronous dopri5: the attempts enqueued by _start did not finish the solve (see there) */
};

/* fixed-grid methods of torchdiffeq (_impl/fixed_grid.py); rk4 is the 3/8 rule */
enum { ODEHIP_EULER = 0, ODEHIP_MIDPOINT = 1, ODEHIP_RK4 = 2, ODEHIP_DOPRI5 = 3,
       ODEHIP_BOSH3 = 4 /* adaptive entry points only (odehip_*adaptive*) */ };

const char* odehip_last_error(void);
int odehip_version(void);
/* diagnostic ablation bits for tools/conv_microbench.py (1 skip LDS-DMA, 2 skip MFMA, 4 skip epilogue); 0 in production */
void odehip_set_debug_flags(int flags);
/* device buffer of 8 x uint64 per workgroup for in-kernel stamps (flag 8); NULL disables */
void odehip_set_debug_buffer(void* device_buffer);

/* ---- layout + weight packing -------------------------------------------------------------- */

/* number of floats of the MFMA-ordered image of a (cout, cin, ks, ks) conv weight */
size_t odehip_packed_weight_floats(int cout, int cin, int ks);

/* OIHW fp32 -> packed image.  transpose_flip != 0 packs the weights of the input-gradient
 * convolution (dgrad): W'[ci][co][ks-1-dy][ks-1-dx], i.e. a conv with cin/cout swapped.
 * Replaces: the implicit cuDNN/MIOpen weight handling behind nn.Conv2d (helpers/utils.py:167-177). */
int odehip_pack_conv_weight(const float* w_oihw, float* w_packed, int cout, int cin, int ks,
                            int transpose_flip, void* stream);

/* Winograd F(2x2,3x3) form of a 3x3 conv weight (U = G g G^T, 16 values per (cout, cin) pair) in the LDS image of the
 * Winograd kernel.  Optional: a conv with w_wino == NULL runs the direct kernel. */
size_t odehip_winograd_weight_floats(int cout, int cin);
int odehip_pack_conv_weight_winograd(const float* w_oihw, float* w_wino, int cout, int cin, int transpose_flip, void* stream);
/* Several of the two packs above in ONE launch (a training step repacks every weight tensor after the optimizer's update).
 * kind 0 = odehip_pack_conv_weight (cout, cin, ks, transpose_flip), kind 1 = odehip_pack_conv_weight_winograd (ks must be 3),
 * kind 2 = odehip_pack_conv_weight_winograd5 (ks must be 5); the results are identical to those calls'. */
#define ODEHIP_MAX_PACK_JOBS 32
typedef struct odehip_pack_job {
  const float* w; /* (cout, cin, ks, ks) as nn.Conv2d holds it */
  float* out;
  int cout, cin, ks, kind, transpose_flip;
} odehip_pack_job;
int odehip_pack_conv_weights(const odehip_pack_job* jobs, int n_jobs, void* stream);
/* bf16 A-operand image of a 3x3 weight (round to nearest even): cout % 32 == 0, cin % 16 == 0, cin <= 128 is what the
 * bf16 kernel serves; odehip_bf16_weight_bytes(cout, cin) bytes.  transpose_flip as odehip_pack_conv_weight. */
/* Winograd F(2x2,5x5) form of a 5x5 weight (conv_wino5.hip): U = G g G^T for the points 0, +-1, +-2, inf; cout % 32 == 0,
 * cin % 8 == 0.  Set as odehip_conv_desc.w_wino of a ks = 5 layer, or as odehip_convgru_cell.w_gates_wino / w_can_wino. */
size_t odehip_winograd5_weight_floats(int cout, int cin);
int odehip_pack_conv_weight_winograd5(const float* w_oihw, float* w_wino, int cout, int cin, int transpose_flip, void* stream);

size_t odehip_bf16_weight_bytes(int cout, int cin);
int odehip_pack_conv_weight_bf16(const float* w_oihw, void* w_bf16, int cout, int cin, int transpose_flip, void* stream);
/* fused image of a 64 -> 64 3x3 stack: call once per layer with its position `exec_index` in execution order (forward: the
 * layer index; input-gradient chain: n_convs-1-layer with transpose_flip = 1); odehip_fused_bf16_weight_bytes(n_layers) bytes */
size_t odehip_fused_bf16_weight_bytes(int n_layers);
int odehip_pack_convstack_fused_bf16(const float* w_oihw, void* w_fused, int exec_index, int transpose_flip, void* stream);
/* the same for the 5x5 convs of the ConvGRU cell (block-major image, cout*cin*25*2 bytes) */
int odehip_pack_conv_weight_bf16_ks(const float* w_oihw, void* w_bf16, int cout, int cin, int ks, int transpose_flip, void* stream);

int odehip_nchw_to_q4(const float* src_nchw, float* dst_q4, int batch, int channels, void* stream);
int odehip_q4_to_nchw(const float* src_q4, float* dst_nchw, int batch, int channels, void* stream);

/* ---- one convolution layer on 16x16 maps (building block; exposed for tests) ---------------- */

typedef struct odehip_conv_desc {
  const float* src1;      /* Q4 input, channels [0, cin1)                                     */
  const float* src2;      /* Q4 input, channels [cin1, cin); NULL when cin1 == cin (torch.cat) */
  int cin1, cin, cout, ks, batch;
  const float* w_packed;  /* from odehip_pack_conv_weight                                      */
  const float* w_wino;    /* from odehip_pack_conv_weight_winograd (ks 3) / _winograd5 (ks 5), or NULL (direct kernel) */
  const void* w_bf16;     /* from odehip_pack_conv_weight_bf16: non-NULL = bf16 operands, fp32 accumulate (3x3) */
  const float* bias;      /* cout floats or NULL                                               */
  float* dst;             /* Q4 output                                                        */
  int relu;               /* fuse ReLU into the epilogue                                      */
} odehip_conv_desc;

int odehip_conv_q4(const odehip_conv_desc* d, void* stream);
/* diagnostic: n back-to-back evaluations of f on Q4 tensors; scratch holds 2 hidden activations (tools/fused_microbench.py) */
struct odehip_convstack;
int odehip_debug_repeat_f(const struct odehip_convstack* f, const float* x_q4, float* out_q4, float* scratch, int batch, int n,
                          void* stream);
/* diagnostic: n back-to-back launches of the same layer (tools/conv_microbench.py) */
int odehip_debug_repeat_conv(const odehip_conv_desc* d, int n, void* stream);

/* ---- the dynamics f(t, y) = gradient_net(y)  (modules/DiffEqSolver.py:71-80) ---------------- */

typedef struct odehip_convstack {
  int n_convs;                           /* create_convnet: n_layers + 2 (helpers/utils.py:166-177) */
  int ks;                                /* 3                                                       */
  int channels[ODEHIP_MAX_LAYERS + 1];   /* channels[i] -> channels[i+1]                            */
  const float* w_packed[ODEHIP_MAX_LAYERS];
  const float* w_wino[ODEHIP_MAX_LAYERS];  /* optional Winograd forms (3x3 layers), NULL entries run the direct kernel */
  const void* w_bf16[ODEHIP_MAX_LAYERS];   /* optional bf16 forms: a non-NULL entry runs that layer with bf16 operands and fp32
                                              accumulation (BASELINE.json configs[4]); state and stage combines stay fp32 */
  const void* w_fused;                     /* optional (odehip_pack_convstack_fused_bf16): when every layer is 3x3, 64 -> 64, the
                                              whole stack runs as ONE bf16 launch, one workgroup per sample (fstack_bf16.hip)   */
  const float* bias[ODEHIP_MAX_LAYERS];
  int final_tanh;                        /* final_act=True appends Tanh (helpers/utils.py:179-181)  */
  int act;                               /* hidden activation: 0 = ReLU, 1 = Tanh (create_convnet's nonlinear); a
                                            Tanh head excludes w_fused (the fused kernels take either hidden activation, no head) */
} odehip_convstack;

size_t odehip_convstack_workspace_bytes(const odehip_convstack* f, int batch);

/* y, out: NCHW fp32 (batch, channels[0]|channels[n], 16, 16).  negate != 0 returns -f (backwards=True). */
int odehip_convstack_forward(const odehip_convstack* f, const float* y_nchw, float* out_nchw, int batch,
                             int negate, void* workspace, size_t workspace_bytes, void* stream);

/* ---- odeint, fixed grid: euler / midpoint / rk4(3/8)  (torchdiffeq FixedGridODESolver) ------ */

size_t odehip_odeint_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int method,
                                     int save_for_backward);

/* z0: (B,C,16,16) NCHW; t_host: n_times float64 on the HOST, strictly increasing;
 * out: (n_times,B,C,16,16) NCHW, out[0] = z0.  One step per output interval.
 * negate != 0 integrates dz/dt = -f(z): torchdiffeq's handling of a strictly DEcreasing t is to flip the sign of t
 * and of the dynamics (_impl/odeint.py _check_inputs); the host passes -t here.
 * saved_format_out (required with save_for_backward, else may be NULL) receives how the workspace holds what the backward
 * pass needs: 0 = one fp32 Q4 tensor per evaluation and layer (per-layer / per-evaluation launches), 1 = bf16 "Q4h" tensors
 * written by the whole-trajectory bf16 launch (bf16 fused stack, rk4).  Hand it to odehip_odeint_fixed_backward. */
int odehip_odeint_fixed(const odehip_convstack* f, int method, const float* z0_nchw, const double* t_host,
                        int n_times, int batch, float* out_nchw, int save_for_backward, int negate, void* workspace,
                        size_t workspace_bytes, int* saved_format_out, void* stream);

/* Backward of odehip_odeint_fixed(save_for_backward = 1), on the SAME workspace (untouched in between).
 * This is what `loss.backward()` (train_test.py:204) computes through torchdiffeq's fixed-grid ops: the exact gradient
 * of the discrete solver.  f_dgrad->w_packed[l] = odehip_pack_conv_weight(W_l, transpose_flip = 1) in forward layer
 * order (its bias pointers are ignored).  grad_out (T,B,C,16,16) -> grad_z0 (B,C,16,16), grad_w[l] (OIHW), grad_b[l].
 * Deterministic (no float atomics).  3x3 dynamics with channel counts that are multiples of 64.
 * saved_format: what the forward call reported (0 or 1). */
int odehip_odeint_fixed_backward(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method, const double* t_host,
                                 int n_times, int batch, const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w,
                                 float* const* grad_b, int saved_format, void* workspace, size_t workspace_bytes, void* stream);

/* Adjoint backward: torchdiffeq `odeint_adjoint` semantics (new capability; the reference uses plain autograd).  For
 * i = T-1..1 the augmented state (y, a_y, a_theta) is integrated from t[i] back to t[i-1] with one step of `method`,
 * y is reset to the stored y[i-1], a_y += grad_out[i-1].  y_traj = the forward output (T,B,C,16,16).  Needs no saved
 * activations; workspace size = odehip_odeint_workspace_bytes(..., save_for_backward = 1).  3x3 dynamics, channels % 64 == 0. */
int odehip_odeint_adjoint_backward(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method, const double* t_host,
                                   int n_times, int batch, const float* y_traj_nchw, const float* grad_out_nchw,
                                   float* grad_z0_nchw, float* const* grad_w, float* const* grad_b, void* workspace,
                                   size_t workspace_bytes, void* stream);

/* The adjoint backward on an internal grid (torchdiffeq hands `options` on to every backward interval, so each interval t[i] ->
 * t[i-1] is stepped through a grid of its own).  grid_host: the points of all those grids, joined, in INCREASING time, n_grid of
 * them, grid[0] == t[0], grid[n_grid-1] == t[T-1], every output time among them; out_index[p]: the j with grid[p] == t[j], or -1
 * for a point inside an interval.  Step p+1 -> p integrates the augmented state with one step of `method`; at an output point y is
 * reset to the stored y[j] and a_y += grad_out[j], at an interior point the solver's own y and a_y go on.  A grid without interior
 * points gives odehip_odeint_adjoint_backward's result.  fp32 stacks; n_grid <= 4096 and (n_grid - 1) * stages <= 2048
 * (ODEHIP_EINVAL before any launch otherwise).  Workspace: odehip_odeint_adjoint_grid_workspace_bytes (it grows with n_grid). */
size_t odehip_odeint_adjoint_grid_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int n_grid, int method);
int odehip_odeint_adjoint_backward_on_grid(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method,
                                           const double* t_host, int n_times, const double* grid_host, int n_grid,
                                           const int* out_index, int batch, const float* y_traj_nchw, const float* grad_out_nchw,
                                           float* grad_z0_nchw, float* const* grad_w, float* const* grad_b, void* workspace,
                                           size_t workspace_bytes, void* stream);

/* Adaptive adjoint backward: torchdiffeq `odeint_adjoint(..., method="dopri5", adjoint_options={"norm": "seminorm"})`
 * (BASELINE.json configs[2]; new capability, the reference never calls the adjoint -- modules/DiffEqSolver.py:9).  Each
 * interval t[i] -> t[i-1] is a fresh dopri5 solve of the augmented system with the error norm max(rms_y, rms_a_y); the
 * parameter adjoint does not steer the step size (seminorm) and is accumulated by one weight-gradient launch per layer
 * at the end.  Synchronises `stream` once per attempted step (host-side step control).  `max_accept` bounds the number
 * of accepted steps over the whole backward pass (each keeps its activations); exceeding it returns ODEHIP_EINVAL.
 * stats_host (may be null): {f evaluations of the augmented system, accepted steps, rejected steps}.
 * mixed_norm = 1 is torchdiffeq's DEFAULT adjoint norm: every parameter tensor's RMS error ratio also steers the steps; the
 * parameter block is then integrated step by step (two batched weight-gradient launches per layer and attempt: its error
 * estimate and its increment are both linear in the seven stages). */
size_t odehip_adjoint_dopri5_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int max_accept);
int odehip_odeint_adjoint_dopri5_backward(const odehip_convstack* f, const odehip_convstack* f_dgrad, const double* t_host,
                                          int n_times, int batch, float rtol, float atol, const float* y_traj_nchw,
                                          const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w,
                                          float* const* grad_b, int max_accept, int mixed_norm, int* stats_host, void* workspace,
                                          size_t workspace_bytes, void* stream);

/* ---- ConvGRU cell and the ODE-ConvGRU encoder (modules/ConvGRUCell.py:55-86, modules/ODEConvGRUCell.py:32-78) ---- */

typedef struct odehip_convgru_cell {
  int input, hidden, ks;       /* ConvGRUCell(input_dim, hidden_dim, kernel_size); GroupNorm groups of 32 channels        */
  const float* w_gates;        /* packed conv_gates.0.weight (2*hidden, input+hidden, ks, ks)                              */
  const float* b_gates;        /* conv_gates.0.bias                                                                        */
  const float* gn_gates_w;     /* conv_gates.1.weight (GroupNorm gamma, 2*hidden)                                           */
  const float* gn_gates_b;     /* conv_gates.1.bias                                                                        */
  const float* w_can;          /* packed conv_can.0.weight (hidden, input+hidden, ks, ks)                                   */
  const float* b_can;
  const float* gn_can_w;
  const float* gn_can_b;
  const void* w_gates_bf16;    /* optional: odehip_pack_conv_weight_bf16_ks images; non-NULL = bf16 operands, fp32 accumulation */
  const void* w_can_bf16;      /*           (5x5 cells with input + hidden <= 128 channels)                                   */
  const float* w_gates_wino;   /* optional: odehip_pack_conv_weight_winograd5 forms of the two 5x5 weights; non-NULL = Winograd       */
  const float* w_can_wino;     /*           F(2x2,5x5) in fp32 (36 instead of 100 multiplies per 2x2 outputs; ignored in bf16 mode)  */
} odehip_convgru_cell;
/* The plain cell.  A descriptor whose four gn_* pointers are ALL NULL is the norm-free cell of upstream Vid-ODE
 * (models/base_conv_gru.py:47-72), with upstream's gate order -- the first `hidden` channels of conv_gates are the RESET gate, the
 * second the UPDATE gate (the GroupNorm cell above has the update gate first):
 *   (r, u) = sigmoid(conv_gates(cat(x, h)));  c = tanh(conv_can(cat(x, r h)));  h' = (1 - u) h + u c.
 * Some but not all of the four NULL stays ODEHIP_EINVAL.  Plain cells are taken by odehip_convgru_cell_forward / _backward and their
 * workspace queries, by odehip_odeconvgru_encode, _encode_train, _encode_backward, their _masked forms (same three guarantees for
 * m == 1, m == 0 and fractional m, same exact zeros for an unobserved (frame, sample) in the backward) and the encoder workspace
 * queries.  The gn_* members of odehip_convgru_cell_grads / odehip_encoder_grads are then not written and may be NULL.  Size limits
 * are unchanged (hidden % 32 == 0; multiples of 64 on the training path).  Any ks the convolutions take (upstream: 3).  In bf16
 * compute mode a 3x3 cell runs fp32 in both directions: the bf16 cell kernels are 5x5 only (w_gates_bf16 / w_can_bf16 are ignored
 * for ks != 5).  odehip_convgru_sequence_* refuses plain cells (ODEHIP_EINVAL).  Pure additions: ODEHIP_ABI_VERSION stays. */

size_t odehip_convgru_cell_workspace_bytes(const odehip_convgru_cell* c, int batch);
/* one step: x (B,input,16,16), h (B,hidden,16,16) -> h_next, all NCHW          (ConvGRUCell.forward, seq_len = 1) */
int odehip_convgru_cell_forward(const odehip_convgru_cell* c, const float* x_nchw, const float* h_nchw, float* h_next_nchw,
                                int batch, void* workspace, size_t workspace_bytes, void* stream);

typedef struct odehip_encoder {
  odehip_convstack f_enc;      /* ode_encoder_func.gradient_net                                                            */
  odehip_convgru_cell cell;    /* cgru_cell                                                                                */
  int head_hidden, out_ch;     /* transform_z0: Conv1x1(ch, head_hidden) -> ReLU -> Conv1x1(head_hidden, 2*out_ch)          */
  const float* w_head0;        /* packed 1x1 weights / biases                                                              */
  const float* b_head0;
  const float* w_head1;
  const float* b_head1;
} odehip_encoder;

size_t odehip_encoder_workspace_bytes(const odehip_encoder* e, int n_frames, int batch);
/* inputs (T,B,C,16,16) time-first NCHW, t_host[T] float64 -> mean_z0, std_z0 (B,out_ch,16,16); latent (B,T,C,16,16) or NULL
 * (slot k of a sample = the state after the k-th VISITED frame, as the reference stacks them, ODEConvGRUCell.py:74,76).
 * ODEConvGRUCell.forward / run_ode_conv_gru: run_backwards != 0 visits the frames T-1 .. 0 (what forward() does, :33),
 * 0 visits them 0 .. T-1 with the step sizes the reference's loop then produces (:47,73).  This entry point has no observation
 * mask, as the reference's cell takes one and forgets it (ConvGRUCell.py:55-86): it is odehip_odeconvgru_encode_masked with NULL. */
int odehip_odeconvgru_encode(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames, int batch,
                             int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw, void* workspace,
                             size_t workspace_bytes, void* stream);
/* The same with the observation mask of upstream Vid-ODE (models/base_conv_gru.py:66-70).  mask_tb: (T, B) float32 on the device,
 * mask_tb[i*B + b] = m belongs to FRAME i of sample b whenever that frame is visited (run_backwards changes the visiting order,
 * not the indexing), or NULL = every frame observed = exactly the launches of odehip_odeconvgru_encode.  Per step, with h_ode the
 * Euler-advanced state and h' the cell's result:  m == 1: h', bit for bit what the unmasked call writes;  m == 0: h_ode, copied --
 * nothing the cell computed for that sample is read, so a non-finite unobserved frame stays out of the result;  otherwise
 * m h' + (1 - m) h_ode in fp32.  The step's latent slot receives the blended state.  The mask is read on the device (one scalar per
 * workgroup of the update kernel); the convolutions run for every sample either way.  Workspace: odehip_encoder_workspace_bytes.
 * Arguments are checked before any HIP call (ODEHIP_EINVAL).  Pure additions: ODEHIP_ABI_VERSION stays. */
int odehip_odeconvgru_encode_masked(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames, int batch,
                                    int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw, void* workspace,
                                    size_t workspace_bytes, void* stream, const float* mask_tb);
/* The same with a HOST hint about whole steps.  step_observed_host: n_frames bytes on the HOST, indexed by FRAME like the rows of
 * mask_tb, or NULL = every step runs = exactly odehip_odeconvgru_encode_masked.  A frame whose byte is 0 is computed exactly as if
 * its whole mask_tb row were 0 -- whatever that row holds, and also when mask_tb is NULL -- but without the launches: no cell
 * convolution and no gates / update kernel run for it, the Euler step writes h_ode straight into the next state (the bits the update
 * kernels copy for m == 0), and a wanted latent slot is filled by one small copy kernel.  Nothing of an all-unobserved frame is
 * read, so its contents (non-finite included) cannot reach any output.  cell_steps_run: HOST int or NULL, receives the number of
 * steps for which this call launched the cell.  The hint is read during the call only.  No host synchronisation, no device
 * read-back.  Pure additions: ODEHIP_ABI_VERSION stays. */
int odehip_odeconvgru_encode_steps(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames, int batch,
                                   int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw, void* workspace,
                                   size_t workspace_bytes, void* stream, const float* mask_tb, const unsigned char* step_observed_host,
                                   int* cell_steps_run);

/* Backward of one ConvGRU step (ConvGRUCell.forward with seq_len = 1): grad_h_next -> grad_x, grad_h and the gradients of
 * the cell's eight parameters.  Stateless: the step is recomputed from (x, h) inside the call.  input_dim and hidden_dim
 * must be multiples of 64. */
typedef struct odehip_convgru_cell_bwd {
  const float* w_gates_dx;     /* odehip_pack_conv_weight(conv_gates.0.weight[:, :input], transpose_flip = 1)               */
  const float* w_gates_dh;     /* ... conv_gates.0.weight[:, input:]                                                       */
  const float* w_can_dx;       /* ... conv_can.0.weight[:, :input]                                                         */
  const float* w_can_dh;       /* ... conv_can.0.weight[:, input:]                                                         */
  const void* bf16[4];         /* optional bf16 images of the same four (odehip_pack_conv_weight_bf16_ks, transpose_flip = 1)  */
  const float* wino[4];        /* optional F(2x2,5x5) forms of the same four (odehip_pack_conv_weight_winograd5, transpose_flip = 1) */
} odehip_convgru_cell_bwd;
typedef struct odehip_convgru_cell_grads {
  float *w_gates, *b_gates, *gn_gates_w, *gn_gates_b, *w_can, *b_can, *gn_can_w, *gn_can_b;
} odehip_convgru_cell_grads;
size_t odehip_convgru_cell_backward_workspace_bytes(const odehip_convgru_cell* c, int batch);
int odehip_convgru_cell_backward(const odehip_convgru_cell* c, const odehip_convgru_cell_bwd* cb, const float* x_nchw,
                                 const float* h_nchw, const float* grad_h_next_nchw, float* grad_x_nchw, float* grad_h_nchw,
                                 const odehip_convgru_cell_grads* grads, int batch, void* workspace, size_t workspace_bytes,
                                 void* stream);

/* ---- a whole ConvGRU sequence: ConvGRUCell.forward(input_tensor, h_cur, seq_len) (modules/ConvGRUCell.py:55-86) as the ConvGRU
 * baseline drives it (models/ConvGRU.py:133-149 encoder: frames from a zero state; :225-242 decoder: zero input from a state) ----
 * x_seq (n_steps, batch, input, 16, 16) or NULL = zero input; h0 (batch, hidden, 16, 16) or NULL = zero state; not both NULL.
 * h_seq (n_steps, batch, hidden, 16, 16) is written in place by the step epilogues (slot t = the state after step t; the last
 * state is the view h_seq[n_steps - 1]).  Steps are launches in stream order; enqueue-only, no host synchronisation.
 *   zero input:  the gates and candidate convolutions are ONE-source launches over the state half of the weights (hv->wino[1],
 *                hv->wino[3]; the split-launch choice follows K = hidden * 25); no zero frame is allocated, read or transformed
 *   zero state:  the first step runs over the frame half alone (hv->wino[0], hv->wino[2]) and r * h is not formed
 *   both given:  the two-source launches of odehip_convgru_cell_forward (w_gates_wino / w_can_wino)
 * ks = 5, input % 8 == 0, hidden % 32 == 0 (what the F(2x2,5x5) kernels serve); _train / _backward: both multiples of 64.
 * Arguments are checked before any HIP call (ODEHIP_EINVAL).  Pure additions: no existing struct or signature changes, so
 * ODEHIP_ABI_VERSION stays (as for odehip_frame_metrics).
 * Workspace: odehip_convgru_sequence_workspace_bytes(c, n_steps, batch, has_x, train); forward (train = 0) keeps two states and one
 * step's conv outputs (+ the Q4 frames), train keeps per step h, gates_raw, z, r*h, cand_raw and the backward's gradients of the two
 * conv outputs and the gradient arriving at the step: 10 state-sized Q4 tensors per step (+ 2 frame-sized with has_x), i.e. 40 MiB
 * per step at batch 64, hidden 64.
 * odehip_convgru_sequence_train = _forward that keeps those tensors; the workspace must stay untouched until _backward.
 * odehip_convgru_sequence_backward: back-propagation through time in one call.  grad_h_seq (n_steps, batch, hidden, 16, 16) = the
 * gradient arriving at every h_seq slot (a gradient of the last state is added to slot n_steps - 1 by the caller).  has_x / has_h0
 * as in the train call; grad_x_seq (x_seq's shape) is written iff has_x, grad_h0 iff has_h0 (else pass NULL).  Reverse sweep
 * t = n_steps-1 .. 0 with the cell backward kernels (one-source input-gradient launches without x: no gradient is formed for the
 * zero frame), then per weight half and 64 x 64 channel tile ONE weight-gradient launch over all steps (steps are one more batch
 * axis; slabs summed in a fixed order), GroupNorm affine and bias gradients summed in a fixed order: bitwise reproducible.  Without
 * x the frame half of grads->w_gates / w_can is written as exact zeros (what autograd gives for a zero input). */
typedef struct odehip_convgru_cell_halves {
  /* forward images of the two HALVES of the two 5x5 weights, in the order conv_gates.0.weight[:, :input], conv_gates.0.weight[:, input:],
   * conv_can.0.weight[:, :input], conv_can.0.weight[:, input:] (each slice made contiguous, then packed with transpose_flip = 0): a step
   * with one source runs over its half alone.  Entries a call does not need may be NULL. */
  const float* wino[4];        /* odehip_pack_conv_weight_winograd5 (fp32 mode)                                              */
  const void* bf16[4];         /* odehip_pack_conv_weight_bf16_ks (bf16 mode, i.e. odehip_convgru_cell.w_gates_bf16 != NULL) */
} odehip_convgru_cell_halves;
size_t odehip_convgru_sequence_workspace_bytes(const odehip_convgru_cell* c, int n_steps, int batch, int has_x, int train);
int odehip_convgru_sequence_forward(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv, const float* x_seq_nchw, const float* h0_nchw, int n_steps,
                                    int batch, float* h_seq_nchw, void* workspace, size_t workspace_bytes, void* stream);
int odehip_convgru_sequence_train(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv, const float* x_seq_nchw, const float* h0_nchw, int n_steps, int batch,
                                  float* h_seq_nchw, void* workspace, size_t workspace_bytes, void* stream);
int odehip_convgru_sequence_backward(const odehip_convgru_cell* c, const odehip_convgru_cell_halves* hv, const odehip_convgru_cell_bwd* cb, int has_x, int has_h0,
                                     int n_steps, int batch, const float* grad_h_seq_nchw, float* grad_x_seq_nchw,
                                     float* grad_h0_nchw, const odehip_convgru_cell_grads* grads, void* workspace,
                                     size_t workspace_bytes, void* stream);

/* ---- training path of the encoder: `loss.backward()` through ODEConvGRUCell.forward (train_test.py:204) ---------------- */

typedef struct odehip_encoder_bwd {
  odehip_convstack f_dgrad;    /* encoder dynamics with weights packed transpose_flip = 1 (bias pointers ignored)          */
  const float* w_gates_dx;     /* odehip_pack_conv_weight(conv_gates.0.weight[:, :input],  transpose_flip = 1)              */
  const float* w_gates_dh;     /* ... conv_gates.0.weight[:, input:]                                                       */
  const float* w_can_dx;       /* ... conv_can.0.weight[:, :input]                                                         */
  const float* w_can_dh;       /* ... conv_can.0.weight[:, input:]                                                         */
  const float* w_head0_t;      /* ... transform_z0.0.weight, transform_z0.2.weight                                         */
  const float* w_head1_t;
  const void* bf16[4];         /* optional bf16 images of w_gates_dx, w_gates_dh, w_can_dx, w_can_dh                          */
  const float* wino[4];        /* optional F(2x2,5x5) forms of the same four (ks = 5, fp32 mode)                                */
} odehip_encoder_bwd;

typedef struct odehip_encoder_grads {  /* outputs, each shaped like its parameter (conv weights OIHW) */
  float* f_w[ODEHIP_MAX_LAYERS];
  float* f_b[ODEHIP_MAX_LAYERS];
  float *w_gates, *b_gates, *gn_gates_w, *gn_gates_b, *w_can, *b_can, *gn_can_w, *gn_can_b;
  float *w_head0, *b_head0, *w_head1, *b_head1;
} odehip_encoder_grads;

/* Forward that keeps the conv outputs of every frame in `workspace` (which the caller must leave untouched until the
 * backward call), then the reverse sweep: grad_mean / grad_std (B,out_ch,16,16) -> grad_inputs (T,B,C,16,16) and the
 * gradient of every parameter of the encoder dynamics, the ConvGRU cell (incl. GroupNorm affine) and the 1x1 head.
 * run_backwards as in odehip_odeconvgru_encode (the same value in both calls); latent_nchw (B,T,C,16,16) or NULL receives
 * run_ode_conv_gru's latent_ys, grad_latent_nchw (same shape) or NULL is the gradient that arrives through it.
 * Channel counts must be multiples of 64, encoder dynamics 3x3.  Deterministic (no float atomics). */
size_t odehip_encoder_train_workspace_bytes(const odehip_encoder* e, int n_frames, int batch);
int odehip_odeconvgru_encode_train(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames, int batch,
                                   int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw, void* workspace,
                                   size_t workspace_bytes, void* stream);
int odehip_odeconvgru_encode_backward(const odehip_encoder* e, const odehip_encoder_bwd* eb, const double* t_host, int n_frames,
                                      int batch, int run_backwards, const float* grad_mean_nchw, const float* grad_std_nchw,
                                      const float* grad_latent_nchw, float* grad_inputs_nchw, const odehip_encoder_grads* grads,
                                      void* workspace, size_t workspace_bytes, void* stream);
/* The pair with the observation mask of odehip_odeconvgru_encode_masked (mask_tb (T, B) on the device or NULL; the two calls above
 * are these with NULL).  Nothing of the mask is kept in the workspace (odehip_encoder_train_workspace_bytes as before): the backward
 * call is handed the SAME pointer, whose contents must not have changed.  With g the gradient at the blended state of a step, the
 * cell's chain is fed m g and h_ode additionally receives (1 - m) g: nothing is added for m == 1; for m == 0 the chain is fed exact
 * zeros, stored as such and not as products with what the forward kept.  So with finite frames an unobserved (frame, sample) has
 * an exactly zero grad_inputs slice and contributes exact zeros to every weight, bias and GroupNorm-affine gradient.  A NON-FINITE
 * unobserved frame is contained by the forward only: the weight-gradient products multiply it by those zeros. */
int odehip_odeconvgru_encode_train_masked(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames,
                                          int batch, int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw,
                                          void* workspace, size_t workspace_bytes, void* stream, const float* mask_tb);
int odehip_odeconvgru_encode_backward_masked(const odehip_encoder* e, const odehip_encoder_bwd* eb, const double* t_host, int n_frames,
                                             int batch, int run_backwards, const float* grad_mean_nchw, const float* grad_std_nchw,
                                             const float* grad_latent_nchw, float* grad_inputs_nchw, const odehip_encoder_grads* grads,
                                             void* workspace, size_t workspace_bytes, void* stream, const float* mask_tb);
/* The pair with the host step hint of odehip_odeconvgru_encode_steps (step_observed_host: n_frames bytes on the HOST indexed by
 * frame, or NULL = the two calls above; both calls of a pair are given the same hint).  For a frame whose byte is 0 the forward keeps
 * only what the sweep reads for it (the state in front of the Euler step and the dynamics' hidden activations; the next state IS
 * h_ode), and the sweep launches no gates / update backward kernel and no input-gradient convolution: the state gradient goes
 * unchanged to the Euler step's adjoint, and the frame's grad_inputs slab is zero-filled in stream order.  The cell's weight-gradient
 * tables hold the observed frames only (fewer than n_frames entries: the fixed summation order is that of the shorter table); with no
 * observed frame there is no cell weight-gradient launch and the cell's gradient tensors are exact zeros.  The encoder dynamics,
 * their weight gradients over all n_frames steps and the head are untouched.  odehip_encoder_train_workspace_bytes as before.
 * cell_steps_run: HOST int or NULL, the number of steps whose cell kernels this call launched.  Since nothing multiplies an
 * all-unobserved frame any more, its contents cannot reach any gradient either. */
int odehip_odeconvgru_encode_train_steps(const odehip_encoder* e, const float* inputs_nchw, const double* t_host, int n_frames,
                                         int batch, int run_backwards, float* mean_nchw, float* std_nchw, float* latent_nchw,
                                         void* workspace, size_t workspace_bytes, void* stream, const float* mask_tb,
                                         const unsigned char* step_observed_host, int* cell_steps_run);
int odehip_odeconvgru_encode_backward_steps(const odehip_encoder* e, const odehip_encoder_bwd* eb, const double* t_host, int n_frames,
                                            int batch, int run_backwards, const float* grad_mean_nchw, const float* grad_std_nchw,
                                            const float* grad_latent_nchw, float* grad_inputs_nchw, const odehip_encoder_grads* grads,
                                            void* workspace, size_t workspace_bytes, void* stream, const float* mask_tb,
                                            const unsigned char* step_observed_host, int* cell_steps_run);

/* ---- odeint, adaptive dopri5 (torchdiffeq Dopri5Solver; the reference's default method, configs.yaml:79) ------ */

/* Exact-global step control when the batch is sharded over ranks: torchdiffeq's error norm is one RMS
 * over the WHOLE batch.  With a callback installed, odehip_odeint_dopri5 hands every sum of squares (n <= 4 floats in
 * `scratch_dev`, device memory the caller owns) to `cb`, which must enqueue an in-place SUM all-reduce of scratch_dev[0..n)
 * over the ranks on `stream` (RCCL) and return 0; element counts are multiplied by world_size.  All ranks then take the same
 * accept/reject decisions as one device holding the whole batch (up to summation order).  One collective per attempted step
 * (plus two for the initial step): latency-bound, and the host no longer runs one attempt ahead.  cb = NULL restores
 * per-shard control.
 * odehip_set_norm_allreduce_counted installs the same hook under a wider contract (a pure addition; the call above keeps its own):
 * every adaptive method code runs under it (ODEHIP_BOSH3 too: what is summed -- d0 and d1, d2, one error norm per attempt -- does not
 * depend on the stage count), and the element count the norms divide by is summed through the callback as well, ONE more call with
 * n = 1 at the start of every solve, so the shards need not be equal (world_size is not multiplied in).  Under either hook nothing is
 * saved by a saving forward (the backward pass re-integrates the logged steps) and the asynchronous start is refused. */
typedef int (*odehip_allreduce_fn)(float* scratch_dev, int n, void* stream, void* user);
int odehip_set_norm_allreduce(odehip_allreduce_fn cb, void* user, int world_size, float* scratch_dev);
int odehip_set_norm_allreduce_counted(odehip_allreduce_fn cb, void* user, int world_size, float* scratch_dev);

size_t odehip_dopri5_workspace_bytes(const odehip_convstack* f, int batch, int n_times);

/* Same tensors as odehip_odeint_fixed.  rtol/atol as passed by DiffEqSolver (modules/DiffEqSolver.py:13: 1e-4, 1e-5).
 * Step control runs on the device (global RMS norm over the whole batch, as torchdiffeq); outputs are the quartic
 * dense output at t[i].  The call returns after the controller has reported completion (it polls a pinned host
 * mailbox; it does not synchronise the stream otherwise).  stats_host[4] (may be NULL) = {nfe, n_accept, n_reject,
 * attempts enqueued}.  first_step > 0 is torchdiffeq's options={'first_step': dt} (skips the initial-step heuristic);
 * max_steps <= 0 means unlimited (torchdiffeq max_num_steps = 2^31-1); like torchdiffeq's it bounds the attempted steps (accepted
 * or rejected) spent on ONE output time -- the counter is a local of `_advance(next_t)` and restarts with every output.
 * accepted_host (may be NULL): receives (t0, dt) of the accepted steps, in order, at most accepted_cap pairs -- the
 * input of odehip_odeint_dopri5_backward (stats_host[1] > accepted_cap means the log was cut).
 * Errors: ODEHIP_ENOTCONV (dt underflow / max_steps), ODEHIP_ENAN (non-finite error ratio). */
int odehip_odeint_dopri5(const odehip_convstack* f, const float* z0_nchw, const double* t_host, int n_times, int batch,
                         float rtol, float atol, double first_step, int max_steps, int negate, float* out_nchw,
                         int* stats_host, double* accepted_host, int accepted_cap, void* workspace, size_t workspace_bytes,
                         void* stream);

/* `loss.backward()` through odeint(method="dopri5") -- the reference's default training path (configs.yaml:79,
 * modules/DiffEqSolver.py:9, train_test.py:204): the gradient of the arithmetic of the accepted steps (what autograd
 * through torchdiffeq differentiates; step sizes are constants, as under torchdiffeq's no_grad step-size update).
 * Re-integrates the `n_steps` accepted steps of the forward call from z0 keeping activations (n_steps * ~3.5 state-sized
 * tensors per conv layer), walks them backwards, one weight-gradient launch per layer at the end.  Enqueue-only.  For 64-channel
 * fp32 stacks the re-integration and the whole reverse sweep are ONE launch of the adaptive persistent walk (DESIGN.md section
 * 4.4a).  3x3 dynamics, channels % 64 == 0, increasing t. */
size_t odehip_dopri5_backward_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int n_steps);
int odehip_odeint_dopri5_backward(const odehip_convstack* f, const odehip_convstack* f_dgrad, const double* t_host, int n_times,
                                  int batch, const double* accepted_host, int n_steps, const float* z0_nchw,
                                  const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w, float* const* grad_b,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* The same pair WITHOUT the re-integration: the forward of a training step keeps the stage inputs and hidden activations of every
 * accepted step (an attempt writes them into a slot chosen on the device; a rejected attempt's slot is reused), the backward walks
 * them in reverse.  odehip_odeint_dopri5_saving = odehip_odeint_dopri5 (same arguments; no `negate`) + max_accept slots of
 * workspace (odehip_dopri5_saving_workspace_bytes; ~140 MB per slot at B=64) + *saved_out: 1 if the activations are in the
 * workspace, 0 if nothing was saved (the stack is not a 64-channel fp32 stack, the persistent walk is unavailable, exact-global
 * step control is on, or more than max_accept steps were accepted) -- the caller then uses odehip_odeint_dopri5_backward.
 * odehip_odeint_dopri5_backward_saved takes that workspace (untouched since the forward) with the forward's accepted-step log. */
size_t odehip_dopri5_saving_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int max_accept);
int odehip_odeint_dopri5_saving(const odehip_convstack* f, const float* z0_nchw, const double* t_host, int n_times, int batch,
                                float rtol, float atol, double first_step, int max_steps, float* out_nchw, int* stats_host,
                                double* accepted_host, int accepted_cap, int max_accept, int* saved_out, void* workspace,
                                size_t workspace_bytes, void* stream);
int odehip_odeint_dopri5_backward_saved(const odehip_convstack* f, const odehip_convstack* f_dgrad, const double* t_host, int n_times,
                                        int batch, const double* accepted_host, int n_steps, const float* grad_out_nchw,
                                        float* grad_z0_nchw, float* const* grad_w, float* const* grad_b, int max_accept,
                                        void* saved_workspace, size_t saved_workspace_bytes, void* stream);

/* The ASYNCHRONOUS pair (ABI 8).  odehip_odeint_dopri5 / _saving return only when the device-side controller has reported
 * completion -- the host cannot enqueue the work BEHIND the solver (decoder, loss, the backward pass) meanwhile, and in a whole
 * training step the device then idles while ~600 launches are enqueued.  odehip_odeint_dopri5_start takes _saving's arguments
 * (max_accept = 0: nothing is kept for a backward pass), enqueues `attempts` attempted steps (those queued behind completion
 * return at once) and comes back WITHOUT waiting: no stats, no status.  The caller enqueues its consumers of `out` behind this
 * call, so the attempts enqueued HERE are all the solve ever gets: behind the last one sits a seal kernel which, if the solve is
 * not done or has failed (max_num_steps, dt underflow, non-finite state), fills the frames it has not reached with NaN (ABI 10;
 * before, collect enqueued the missing attempts behind the consumers, which had then read uninitialised frames).  odehip_odeint_dopri5_collect(token) waits for the device (normally long
 * done) and reports what the synchronous call reports -- including ODEHIP_ENOTCONV / ODEHIP_ENAN, i.e. an error surfaces at
 * collect time -- or ODEHIP_ETRUNC for a sealed, unfinished solve (stats_host[3] = the attempts that were enqueued; stats are
 * filled in that case too, so the caller can size its retry).  Everything start was given (workspace, out, z0) must stay
 * untouched until collect; at most 4 solves may be pending; not available under exact-global step control. */
int odehip_odeint_dopri5_start(const odehip_convstack* f, const float* z0_nchw, const double* t_host, int n_times, int batch,
                               float rtol, float atol, double first_step, int max_steps, float* out_nchw, int max_accept,
                               int attempts, int* token_out, void* workspace, size_t workspace_bytes, void* stream);
int odehip_odeint_dopri5_collect(int token, int* stats_host, double* accepted_host, int accepted_cap, int* saved_out);

/* ---- odeint, adaptive, by method code: ODEHIP_DOPRI5 or ODEHIP_BOSH3 (torchdiffeq's Bogacki-Shampine 3(2) pair: four stages, FSAL,
 * three evaluations of f per attempted step, order 3 -- the step-size exponents are 1/3).  One entry point per dopri5 call above, with
 * the same arguments, semantics, statuses and workspace rules, plus `method`; the odehip_*dopri5* functions above ARE these calls
 * with ODEHIP_DOPRI5.  Both methods run the same drivers from their tableau (csrc/dopri5_control.h): the persistent adaptive walk,
 * the device-side controller and the pinned mailbox, the saving slots (method's stage count per slot) and the reverse sweep.  A
 * workspace is laid out for its method: size it, fill it and read it with one and the same code.  Any other method code:
 * ODEHIP_EINVAL (the size functions return 0).  ODEHIP_BOSH3 under exact-global step control is refused with ODEHIP_EINVAL when the
 * hook was installed with odehip_set_norm_allreduce, and runs when it was installed with odehip_set_norm_allreduce_counted.  The adjoint pair below takes the method code too: under the seminorm both methods take the device-steered backward solve where it
 * is available (64-channel fp32 stack, 2 <= n_times <= 256, the adaptive persistent walk, ODEHIP_ADJOINT_DEVICE not 0), else the
 * host-driven one, which also serves the mixed norm.  odehip_last_adjoint_controller(): which of the two steered the last
 * odehip_odeint_adjoint_adaptive_backward call of this process (1 device, 0 host, -1 none yet).  Arguments are checked before any HIP
 * call.  Pure additions: ODEHIP_ABI_VERSION stays. */
size_t odehip_adaptive_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int method);
size_t odehip_adaptive_saving_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int max_accept, int method);
size_t odehip_adaptive_backward_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int n_steps, int method);
int odehip_odeint_adaptive(int method, const odehip_convstack* f, const float* z0_nchw, const double* t_host, int n_times, int batch,
                           float rtol, float atol, double first_step, int max_steps, int negate, float* out_nchw, int* stats_host,
                           double* accepted_host, int accepted_cap, void* workspace, size_t workspace_bytes, void* stream);
int odehip_odeint_adaptive_saving(int method, const odehip_convstack* f, const float* z0_nchw, const double* t_host, int n_times,
                                  int batch, float rtol, float atol, double first_step, int max_steps, float* out_nchw, int* stats_host,
                                  double* accepted_host, int accepted_cap, int max_accept, int* saved_out, void* workspace,
                                  size_t workspace_bytes, void* stream);
int odehip_odeint_adaptive_start(int method, const odehip_convstack* f, const float* z0_nchw, const double* t_host, int n_times,
                                 int batch, float rtol, float atol, double first_step, int max_steps, float* out_nchw, int max_accept,
                                 int attempts, int* token_out, void* workspace, size_t workspace_bytes, void* stream);
size_t odehip_adjoint_adaptive_workspace_bytes(const odehip_convstack* f, int batch, int n_times, int max_accept, int method);
int odehip_odeint_adjoint_adaptive_backward(int method, const odehip_convstack* f, const odehip_convstack* f_dgrad, const double* t_host,
                                            int n_times, int batch, float rtol, float atol, const float* y_traj_nchw,
                                            const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w, float* const* grad_b,
                                            int max_accept, int mixed_norm, int* stats_host, void* workspace, size_t workspace_bytes,
                                            void* stream);
int odehip_last_adjoint_controller(void);
int odehip_odeint_adaptive_collect(int token, int* stats_host, double* accepted_host, int accepted_cap, int* saved_out);
int odehip_odeint_adaptive_backward(int method, const odehip_convstack* f, const odehip_convstack* f_dgrad, const double* t_host,
                                    int n_times, int batch, const double* accepted_host, int n_steps, const float* z0_nchw,
                                    const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w, float* const* grad_b,
                                    void* workspace, size_t workspace_bytes, void* stream);
int odehip_odeint_adaptive_backward_saved(int method, const odehip_convstack* f, const odehip_convstack* f_dgrad, const double* t_host,
                                          int n_times, int batch, const double* accepted_host, int n_steps, const float* grad_out_nchw,
                                          float* grad_z0_nchw, float* const* grad_w, float* const* grad_b, int max_accept,
                                          void* saved_workspace, size_t saved_workspace_bytes, void* stream);

/* ---- optimizer step of the training loop (train_test.py:24,205: optim.Adam(model.parameters(), lr)) ------------------------ */

/* One launch for every parameter tensor: torch.optim.Adam arithmetic (amsgrad off; weight_decay is the L2 form), `step` counts
 * from 1.  Host arrays of n_tensors device pointers / element counts. */
int odehip_adam_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                     const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay,
                     int step, void* stream);

/* Gradient clipping by global L2 norm (train_test.py:187-195: torch.nn.utils.clip_grad_norm_(model.parameters(), opt.clip)) without a
 * host read and without a grid-wide barrier: stream order between plain launches is the barrier.  Pure additions: ODEHIP_ABI_VERSION
 * stays.  Enqueue-only on `stream`, caller-provided memory only, arguments checked before any HIP call (ODEHIP_EINVAL: null pointers,
 * a negative or NaN max_norm, a workspace that is too small).  Host arrays of n_tensors device pointers / element counts as for
 * odehip_adam_step; a tensor of 0 elements may have a null pointer.
 *
 * odehip_grad_norm: ceil(n_tensors / 24) launches write one float64 partial sum of g*g per workgroup to partials_ws (plain stores, no
 * atomics: two calls are bitwise equal), a one-workgroup launch adds them in index order and writes three floats to out3 (device):
 *   out3[0] = total_norm   = (float)sqrt(sum)
 *   out3[1] = coef         = clamp(reciprocal(total_norm + 1e-6f) * max_norm, max = 1), every step rounded to fp32: torch's
 *                            `max_norm / (total_norm + 1e-6)` is that product; a NaN norm gives a NaN coefficient
 *                            (error_if_nonfinite=False), an Inf norm gives 0
 *   out3[2] = clipped_norm = total_norm * coef
 * partials_ws: odehip_grad_norm_workspace_bytes(n_tensors, numel) bytes, 8-byte aligned.
 * odehip_grad_scale: g *= *coef_dev for every tensor (the stand-alone clip_grad_norm_), ceil(n_tensors / 24) launches.
 * odehip_adam_step_clipped: odehip_adam_step on g * *coef_dev; the scaled gradient is also written back to `grads`, so the caller's
 * gradients end as torch's clip_grad_norm_ would leave them.  With *coef_dev == 1 parameters, moments and gradients get
 * odehip_adam_step's bits. */
size_t odehip_grad_norm_workspace_bytes(int n_tensors, const long long* numel);
int odehip_grad_norm(const float* const* grads, const long long* numel, int n_tensors, float max_norm, void* partials_ws, size_t ws_bytes,
                     float* out3, void* stream);
int odehip_grad_scale(float* const* grads, const long long* numel, int n_tensors, const float* coef_dev, void* stream);
int odehip_adam_step_clipped(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_avg_sq,
                             const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay,
                             int step, const float* coef_dev, void* stream);

/* Adamax (optim_step.hip): Vid-ODE's optimizer (Vid-ODE/main.py:187: optim.Adamax(netG.parameters(), lr)) on the tables, the grid and the
 * argument checks of the Adam pair above.  Pure additions: ODEHIP_ABI_VERSION stays.  torch.optim.Adamax arithmetic (single-tensor
 * path, maximize off; weight_decay is the L2 form and is skipped when 0), `step` counts from 1 and lr / (1 - beta1^step) is computed
 * on the host in float64:
 *   g += wd p;  exp_avg = b1 exp_avg + (1 - b1) g;  exp_inf = max(b2 exp_inf, |g| + eps);  p -= lr / (1 - b1^step) * exp_avg / exp_inf
 * exp_inf is torch's bit for bit (every operation a single fp32 rounding), and its maximum propagates NaN as torch.maximum does: a
 * non-finite gradient never becomes a finite update.  ceil(n_tensors / 24) plain launches, no atomics: two calls are bitwise equal.
 * odehip_adamax_step_clipped: the same on g * *coef_dev (out3 + 1 of odehip_grad_norm), rounded on its own and written back to
 * `grads`; with *coef_dev == 1 everything gets odehip_adamax_step's bits.  A tensor of 0 elements may have null pointers there. */
int odehip_adamax_step(float* const* params, const float* const* grads, float* const* exp_avg, float* const* exp_inf,
                       const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay,
                       int step, void* stream);
int odehip_adamax_step_clipped(float* const* params, float* const* grads, float* const* exp_avg, float* const* exp_inf,
                               const long long* numel, int n_tensors, float lr, float beta1, float beta2, float eps, float weight_decay,
                               int step, const float* coef_dev, void* stream);

/* ---- VidODE's warp chain + mask compositing (models/VidODE.py:119-140, get_warped_images :160-186) -------------------------- */

/* pred_outputs (B,T,c+3,H,W) = the flow decoder's output per predicted frame: channels [0:2] optical flow (x, y) in pixels,
 * [2:2+c] the "intermediate" frame, [2+c] the mask logit.  start_image (B,c,H,W) = the last observed frame.  grid_x[W], grid_y[H]
 * = torch.linspace(-1, 1, n) (VidODE.py:122-123; handed over so that they are the caller's torch's values).  For t = 0..T-1:
 *   warped_t = grid_sample(warped_{t-1}, grid + flow_t / ((n-1)/2), bilinear, padding_mode="border", align_corners=False)
 *   masks_t = sigmoid(logit_t);  pred_x_t = masks_t * warped_t + (1 - masks_t) * intermediate_t
 * with warped_{-1} = start_image -- the whole chain in ONE launch (one workgroup per sample, the image stays in LDS).
 * Outputs: pred_x, warped (B,T,c,H,W), masks (B,T,1,H,W).  c <= 4, 2*c*H*W*4 bytes must fit in LDS (160 KiB). */
int odehip_warp_composite(const float* pred_outputs, const float* start_image, const float* grid_x, const float* grid_y, int batch,
                          int n_times, int channels, int height, int width, float* pred_x, float* warped, float* masks,
                          void* stream);
/* Backward of the above: gradients w.r.t. pred_outputs (flow through the bilinear weights -- zero where a coordinate was clamped
 * to the border --, intermediate frames, mask logits) and, if grad_start_image != NULL, the start image.  `warped` is the forward's
 * output; grad_warped / grad_masks may be NULL (no gradient arrives through those outputs).  The scatter into the previous
 * image's gradient uses LDS float atomics: reproducible to rounding, not bitwise. */
int odehip_warp_composite_backward(const float* pred_outputs, const float* start_image, const float* warped, const float* grid_x,
                                   const float* grid_y, const float* grad_pred_x, const float* grad_warped, const float* grad_masks,
                                   int batch, int n_times, int channels, int height, int width, float* grad_pred_outputs,
                                   float* grad_start_image, void* stream);

/* nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False) of VidODE's flow decoder (models/VidODE.py:34, applied per
 * predicted frame by get_flowmaps :143-158) on `planes` = N * C images of (height, width) -> (2 height, 2 width), ATen's arithmetic
 * (source index max(0, (dst + 0.5) / 2 - 0.5), the four-point blend in its order of operations).  HBM-bound data movement: torch's
 * own kernel runs it at 20 GB/s on this stack (4.2 ms per call, 85 % of a VidODE forward at batch 64).  width must be even.
 * Backward: the transpose as a gather (deterministic). */
int odehip_upsample2x_bilinear(const float* in, float* out, long long planes, int height, int width, void* stream);
int odehip_upsample2x_bilinear_backward(const float* grad_out, float* grad_in, long long planes, int height, int width, void* stream);

/* BatchNorm2d -> ReLU (-> that upsampling) of the same decoder (models/VidODE.py:35-36) as one pass over the convolution's output
 * x (batch, channels, height, width) NCHW fp32; width % 4 == 0.  training != 0: the statistics of THIS call (biased variance for the
 * normalisation; running_mean / running_var, if given, updated with `momentum` and the unbiased variance, as nn.BatchNorm2d does);
 * else the running statistics.  weight / bias may be NULL (affine=False).  out = relu(bn(x)), upsampled x2 (-> 2 height x 2 width) when
 * upsample != 0.  mean_out, invstd_out, scale_out, shift_out [channels]: what the backward needs (scale = weight * invstd,
 * shift = bias - mean * scale).  workspace: odehip_bn_workspace_bytes(channels) (forward), + 2 * channels floats (backward).
 * Backward: grad_out has out's shape; g_pre (x's shape) is scratch the caller provides; grad_x, grad_weight, grad_bias are written.
 * Every reduction has a fixed order: bitwise reproducible. */
size_t odehip_bn_workspace_bytes(int channels);
int odehip_bn_relu_up2x_forward(const float* x, int batch, int channels, int height, int width, const float* weight, const float* bias,
                                float* running_mean, float* running_var, int training, float momentum, float eps, int upsample, float* out,
                                float* mean_out, float* invstd_out, float* scale_out, float* shift_out, void* workspace,
                                size_t workspace_bytes, void* stream);
int odehip_bn_relu_up2x_backward(const float* grad_out, const float* x, int batch, int channels, int height, int width, const float* mean,
                                 const float* invstd, const float* scale, const float* shift, int training, int upsample, float* grad_x,
                                 float* grad_weight, float* grad_bias, float* g_pre, void* workspace, size_t workspace_bytes, void* stream);

/* BatchNorm statistics over the ranks of a batch-sharded job: the train-mode pass above cut in two at its per-channel float64 sums, so
 * that the caller can sum them over the ranks in between (ONE collective per pass, on `stream`).  A rank's shard holds at least one
 * sample; shards may be uneven, the element count travels with the sums.
 *   odehip_bn_sync_stats              sums [2 channels + 1] (device) = [sum x | sum x^2 | batch * height * width] of this shard
 *   odehip_bn_sync_relu_up2x_forward  the rest of the forward from the REDUCED sums: mean, biased variance, running statistics with the
 *                                     global count, scale / shift, out.  Keep sums[2 channels] (the global count) for the backward.
 *   odehip_bn_sync_backward_sums      g_pre written once; sums [2 channels] = [sum g_pre | sum g_pre * xhat] of this shard, xhat from the
 *                                     global mean / invstd of the forward; grad_weight, grad_bias = these LOCAL sums (as nn.SyncBatchNorm
 *                                     returns them: the gradient all-reduce adds them up)
 *   odehip_bn_sync_backward_apply     grad_x = scale * (g_pre - m1 - xhat * m2), (m1, m2) = the REDUCED sums / *count (device)
 * workspace: odehip_bn_workspace_bytes(channels) (stats, backward_sums), 2 * channels floats (backward_apply).  With one rank the four
 * calls compute bit for bit what the two calls above do.  Arguments are checked before any HIP call (ODEHIP_EINVAL).  Pure additions:
 * ODEHIP_ABI_VERSION stays. */
int odehip_bn_sync_stats(const float* x, int batch, int channels, int height, int width, double* sums, void* workspace, size_t workspace_bytes,
                         void* stream);
int odehip_bn_sync_relu_up2x_forward(const float* x, int batch, int channels, int height, int width, const double* sums, const float* weight,
                                     const float* bias, float* running_mean, float* running_var, float momentum, float eps, int upsample,
                                     float* out, float* mean_out, float* invstd_out, float* scale_out, float* shift_out, void* stream);
int odehip_bn_sync_backward_sums(const float* grad_out, const float* x, int batch, int channels, int height, int width, const float* mean,
                                 const float* invstd, const float* scale, const float* shift, int upsample, float* g_pre, float* grad_weight,
                                 float* grad_bias, double* sums, void* workspace, size_t workspace_bytes, void* stream);
int odehip_bn_sync_backward_apply(const float* g_pre, const float* x, int batch, int channels, int height, int width, const float* mean,
                                  const float* invstd, const float* scale, const double* sums, const double* count, float* grad_x,
                                  void* workspace, size_t workspace_bytes, void* stream);

/* ---- the conv encoder / decoder either side of the path (models/ODEConvGRU.py:101-118 Encoder, :121-140 Decoder; n_downs = 2) --
 * Each is ONE fused launch: the 32x32 intermediate stays in LDS, the 16 -> out_ch and in_ch -> 32 layers run on the fp32 MFMA.
 * Frames are 64x64, latents 16x16 (the path's fixed map size).  LeakyReLU slope: the reference's 0.2.
 *
 * Encoder: Conv2d(in_ch, 16, 3, 2, 1) -> LeakyReLU -> Conv2d(16, out_ch, 3, 2, 1) -> LeakyReLU.  w1 (16, in_ch, 3, 3), b1 (16),
 * w2 (out_ch, 16, 3, 3), b2 (out_ch) as nn.Conv2d holds them; in_ch 1..4, out_ch 32 / 64 / 128.  `pack` (device,
 * odehip_frame_encoder_pack_floats floats) is refreshed by odehip_pack_frame_encoder whenever the parameters change.
 * frames (B, T, in_ch, 64, 64) -- the reference's inputs.view(b*t, c, h, w) (:63) -- and the result is written TIME-FIRST,
 * (T, B, out_ch, 16, 16) contiguous: what :64-68 produce as a permuted view and odehip_odeconvgru_encode consumes. */
size_t odehip_frame_encoder_pack_floats(int in_ch, int out_ch);
int odehip_pack_frame_encoder(const float* w1, const float* b1, const float* w2, const float* b2, int in_ch, int out_ch, float* pack,
                              void* stream);
int odehip_frame_encode(const float* pack, const float* frames, int batch, int n_frames, int in_ch, int out_ch, float negative_slope,
                        float* out_time_first, void* stream);
/* Decoder: ConvTranspose2d(in_ch, 32, 4, 2, 1) -> LeakyReLU -> ConvTranspose2d(32, out_ch, 4, 2, 1) [-> sigmoid if apply_sigmoid:
 * the F.sigmoid of :85].  w1 (in_ch, 32, 4, 4), b1 (32), w2 (32, out_ch, 4, 4), b2 (out_ch) as nn.ConvTranspose2d holds them;
 * in_ch 32 / 64 / 128, out_ch 1..4.  latents (N, in_ch, 16, 16) -- the solver's (T, B, C, 16, 16) as it lies, N = T*B (:84) --
 * -> out (N, out_ch, 64, 64). */
size_t odehip_frame_decoder_pack_floats(int in_ch, int out_ch);
int odehip_pack_frame_decoder(const float* w1, const float* b1, const float* w2, const float* b2, int in_ch, int out_ch, float* pack,
                              void* stream);
int odehip_frame_decode(const float* pack, const float* latents, int n_images, int in_ch, int out_ch, float negative_slope,
                        int apply_sigmoid, float* out, void* stream);
/* Backward of the two fused launches above (frame_codec_backward.hip) -- what `loss.backward()` needs from the Encoder / Decoder of
 * models/ODEConvGRU.py:101-140 in a training step, for ONE frame channel and 32 / 64 latent channels (other shapes: rc != 0, the
 * caller keeps the library's backward).  The 32x32 intermediates are recomputed in LDS from the forward's inputs; weight gradients
 * are summed in a fixed order (bitwise reproducible).  All gradients are WRITTEN (not accumulated), in the parameters' own layouts.
 * `workspace`: device scratch of odehip_frame_*_backward_workspace_floats floats (0 = unsupported shape).
 *
 * Decoder: pack = the forward's pack, w1 = the first ConvTranspose2d's weight (in_ch, 32, 4, 4) as it lies; latents (N, in_ch, 16,
 * 16) and pred (N, 1, 64, 64) = the forward's input and output, g_out = dL/d pred (sigmoid_applied: pred is after the sigmoid and
 * its derivative pred (1 - pred) is applied here).  Out: g_latents (N, in_ch, 16, 16), dw1 (in_ch, 32, 4, 4), db1 (32), dw2 (32, 1,
 * 4, 4), db2 (1). */
/* odehip_frame_decode_train = odehip_frame_decode that also writes the 32-channel intermediate (after its LeakyReLU) to mid_save
 * (n_images * 32 * 32 * 32 floats, channel quads: [N][8][32][32] x 4; may be NULL): handed to the backward as mid_saved it replaces the
 * recomputation there (mid_saved NULL: recomputed from the latents, nothing but inputs and outputs kept). */
int odehip_frame_decode_train(const float* pack, const float* latents, int n_images, int in_ch, int out_ch, float negative_slope,
                              int apply_sigmoid, float* out, float* mid_save, void* stream);
size_t odehip_frame_decode_backward_workspace_floats(int n_images, int in_ch, int out_ch);
int odehip_frame_decode_backward(const float* pack, const float* w1, const float* latents, const float* mid_saved, const float* pred,
                                 const float* g_out, int n_images, int in_ch, int out_ch, float negative_slope, int sigmoid_applied,
                                 float* g_latents, float* dw1, float* db1, float* dw2, float* db2, float* workspace,
                                 size_t workspace_floats, void* stream);
/* Encoder: pack = the forward's pack, w2 = the second Conv2d's weight (out_ch, 16, 3, 3); frames (B, T, 1, 64, 64),
 * out_time_first = the forward's result (T, B, out_ch, 16, 16), g_out_time_first = dL/d of it in the same layout.  The frames
 * receive no gradient.  Out: dw1 (16, 1, 3, 3), db1 (16), dw2 (out_ch, 16, 3, 3), db2 (out_ch). */
size_t odehip_frame_encode_backward_workspace_floats(int batch, int n_frames, int in_ch, int out_ch);
int odehip_frame_encode_backward(const float* pack, const float* w2, const float* frames, const float* out_time_first,
                                 const float* g_out_time_first, int batch, int n_frames, int in_ch, int out_ch, float negative_slope,
                                 float* dw1, float* db1, float* dw2, float* db2, float* workspace, size_t workspace_floats, void* stream);

/* odehip_odeint_fixed runs a forward-only trajectory of a 64-channel fp32 stack as ONE persistent launch (the four workgroups of a
 * sample hand layers to each other through L2 instead of through launch boundaries).  On by default
 * (environment ODEHIP_PERSISTENT=0 turns it off); this switch is for A/B measurements and tests.  Returns the previous
 * setting.  odehip_persistent_trajectory_launches: how many trajectories have taken that path in this process. */
int odehip_set_persistent_trajectory(int enable);
long long odehip_persistent_trajectory_launches(void);
/* Fixed-grid trajectories of a 64-channel stack whose batch gives every group of four workgroups ONE sample (batch <= 64) walk in
 * row strips: workgroup = (sample, all 64 output channels, 4 rows), one input transform per tile.  Results
 * are bit-identical to the other walks.  On by default (environment ODEHIP_STRIP_WALK=0 turns it off); the switch is for A/B
 * measurements and tests and returns the previous setting.  odehip_strip_walk_launches: launches of that kernel in this process. */
int odehip_set_strip_walk(int enable);
long long odehip_strip_walk_launches(void);
/* Sticky error word of the persistent launches: 0 = none, else the code a capped in-kernel wait left when it gave up (2: a
 * partner workgroup never announced itself, 3: a partner's layer never arrived).  Host-side read of mapped memory, no
 * synchronisation.  clear != 0 resets the word and switches the persistent path off for the process. */
int odehip_persistent_error(int clear);

/* Moving-MNIST-shaped frames rendered on the device (replaces the host generator dataloader.py:47-103 + the normalisation of
 * __getitem__ :217-218).  init: [batch][n_digits][4] doubles = x, y, v_x, v_y in the unit square (drawn by the host as
 * dataloader.py:50-54 does); digit_ids: [batch][n_digits] indices into glyphs [n_glyphs][28][28] (uint8); lut256[v] =
 * float32(v) / 255 - 0.5 evaluated in float32 as numpy does for the reference's float32 frames.  Frames 0..t_in-1 go to out_in (batch, t_in, 1, 64, 64), the rest to out_pred (batch, t_out, 1,
 * 64, 64).  The digit ids are NOT range-checked on the device: the caller guarantees 0 <= id < n_glyphs. */
int odehip_mmnist_render(const double* init, const int* digit_ids, const unsigned char* glyphs, int n_glyphs,
                         const float* lut256, int batch, int n_digits, int t_in, int t_out, float* out_in, float* out_pred,
                         void* stream);

/* The training batches of upstream Vid-ODE assembled from a clip store that stays on the device (vidode_batch.hip; DESIGN.md section
 * 4.18): the frame gather of VideoDataset.__getitem__ (Vid-ODE/dataloader.py), RandomHorizontalFlip, ToTensor(scale=True), Normalize(0.5,
 * 0.5) (video_transforms.py:32-70), the stacking of video_collate_fn, the split of utils.split_and_subsample_batch and the mask
 * multiplies of utils.get_next_batch, as ONE launch.  Enqueue-only on `stream`, caller-provided memory only, no LDS, no atomics,
 * arguments checked before any HIP call (ODEHIP_EINVAL).  Pure addition: ODEHIP_ABI_VERSION stays.
 *   store      uint8 on the device, store_frames frames of (height, width, channels), channel-last and back to back (the clips of a
 *              dataset one after the other); channels 1 or 3
 *   lut256     256 floats on the device: the value of a pixel byte after ToTensor / Normalize, computed by the caller in float32
 *   outs       HOST array of n_outputs (1..3) device pointers, output k = (batch, n_frames[k], channels, height, width) float32,
 *              16-byte aligned; n_frames: HOST array
 *   table      int32 words on the device, table_words of them (checked against the shapes):
 *                [batch]                    flip flag per sample (non-zero: every frame of the sample is mirrored left-right)
 *                per output k, in order:    [batch * n_frames[k]] absolute frame index in the store of slot (b, t), then
 *                                           [batch * n_frames[k]] float32 bit patterns: the factor (mask value) of slot (b, t)
 *   out_k[b][t][c][y][x] = lut256[store[frame][y][flip ? width-1-x : x][c]] * factor      (one fp32 multiply: a masked frame gets the
 *              signed zeros of upstream's `filter_mask * data`)
 * A frame index outside [0, store_frames) is not read; its slot is filled with NaN.  width % 4 == 0 takes the 16-byte path (the
 * store must then be 4-byte aligned); any other width takes guarded per-pixel loads and stores. */
int odehip_vidode_batch(const unsigned char* store, long long store_frames, int height, int width, int channels,
                        const float* lut256, const int* table, long long table_words, int batch, int n_outputs, float* const* outs,
                        const int* n_frames, void* stream);

/* odehip_vidode_batch with upstream's RandomRotation between the flip and ToTensor (vidode_rotate.hip): one
 * angle per sample, every frame of the sample rotated by it as skimage.transform.rotate(frame, angle, preserve_range=True) is stated
 * in DESIGN (bilinear, 0 outside the frame, values clipped from below to the frame's own minimum byte).  A rotated pixel is no byte,
 * so there is no lut256: `input_norm` selects Normalize(0.5, 0.5) after ToTensor(scale=True).  ONE launch, enqueue-only on `stream`,
 * caller-provided memory only, no LDS, no atomics, arguments checked before any HIP call (ODEHIP_EINVAL).  Pure addition:
 * ODEHIP_ABI_VERSION stays.  store, outs, n_frames as for odehip_vidode_batch (no alignment asked of the store: byte loads).
 *   frame_min  uint8 on the device, store_frames entries: the smallest byte of each frame over all its channels
 *   table      int32 words on the device, 8-byte aligned, table_words of them (checked against the shapes):
 *                [4 * batch]                per sample two float64 (bit patterns, 2 words each): cos and sin of the angle
 *                [batch]                    flip flag per sample
 *                per output k, in order:    frames and factors as for odehip_vidode_batch
 *   with cx = width / 2 - 0.5, cy = height / 2 - 0.5, all in float64, one rounding per operation, left to right:
 *     sx = cos * (x - cx) - sin * (y - cy) + cx,  sy = sin * (x - cx) + cos * (y - cy) + cy
 *     x0 = floor(sx), x1 = ceil(sx), dx = sx - x0 (y likewise);  p(yy, xx) = store[frame][yy][flip ? width-1-xx : xx][c], 0 outside
 *     v = (1 - dy) * ((1 - dx) * p(y0, x0) + dx * p(y0, x1)) + dy * ((1 - dx) * p(y1, x0) + dx * p(y1, x1))
 *     v = max(v, frame_min[frame]) unless v == 0            (a non-finite cos or sin gives v = 0)
 *   out_k[b][t][c][y][x] = normalise(float32(v) / 255) * factor, normalise(f) = input_norm ? (f - 0.5) / 0.5 : f, in float32
 * cos = 1, sin = 0 gives what odehip_vidode_batch gives with the lut256 of the same input_norm, bit for bit.  A frame index outside
 * [0, store_frames) is not read; its slot is filled with NaN.  width % 4 == 0 takes 16-byte stores, any other width guarded ones. */
int odehip_vidode_batch_rotated(const unsigned char* store, long long store_frames, int height, int width, int channels,
                                const unsigned char* frame_min, int input_norm, const int* table, long long table_words, int batch,
                                int n_outputs, float* const* outs, const int* n_frames, void* stream);

/* Evaluation metrics of predicted frames against the ground truth (frame_metrics.hip) -- what the reference's test() computes per
 * predicted frame on the host (train_test.py:104-117: F.mse_loss(...).item(), math.log10, utils.get_normalized_ssim), in two launches
 * on `stream` with no host synchronisation.  pred, truth: (batch, n_frames, channels, 64, 64) fp32, contiguous; channels 1 or 3 (any
 * other frame shape: ODEHIP_EINVAL).  data_range R > 0: the value range of the frames (1 for [0, 1], 255 for [0, 255]).  Out, all written:
 *   sse[b][t]    sum over the frame of (pred - truth)^2
 *   ssim[b][t]   scikit-image's structural_similarity(gaussian_weights=True, use_sample_covariance=False, data_range=R) per channel
 *                (sigma 1.5, 11 taps, mean over rows / columns 5..58), averaged over the channels
 *   mse[t]       sum_b sse[b][t] / (batch * channels * 64 * 64)
 *   psnr[t]      10 log10(R^2 / mse[t]); +inf where mse[t] == 0 (the reference divides by zero there and raises)
 *   ssim_t[t]    sum_b ssim[b][t] / batch
 * Every reduction runs in a fixed order (no atomics: two calls are bitwise equal).  A NaN in a frame makes that frame's sse / ssim
 * and the three [t] values NaN and leaves every other frame alone.  Arguments are checked before any HIP call. */
int odehip_frame_metrics(const float* pred, const float* truth, int batch, int n_frames, int channels, int height, int width,
                         float data_range, float* sse, float* ssim, float* mse, float* psnr, float* ssim_t, void* stream);

/* Upstream Vid-ODE's evaluation protocol on the device (png_metrics.hip) -- what Vid-ODE/tester.py:49-78,
 * visualize.save_test_images and evaluate.Evaluation compute through 8-bit PNG files, PIL and scikit-image: per image the squared error
 * of the 8-bit RGB bytes, its MSE on the [0, 1] scale and the Gaussian SSIM (data_range 255) of the 8-bit luma.  One launch (two with
 * `accum`), enqueue-only on `stream`, caller-provided memory only, no atomics (two calls are bitwise equal), arguments checked before
 * any HIP call (ODEHIP_EINVAL).  Pure addition: ODEHIP_ABI_VERSION stays.
 *   pred, truth   (batch, n_frames, channels, size, size) fp32, contiguous, 16-byte aligned; channels 1 or 3; size 32, 64 or 128
 *   denorm        non-zero: upstream's opt.input_norm, v = min(max((x + 1) / 2, 0), 1) first (utils.denorm)
 *   byte          trunc(min(max(v * 255 + 0.5, 0), 255)), every step one fp32 operation (torchvision's save_image); one channel is
 *                 replicated into R, G and B;  luma L = (19595 R + 38470 G + 7471 B + 0x8000) >> 16 (PIL's convert('L'))
 *   sse[b][t]     int64: sum over the 3 * size^2 RGB bytes of (byte_pred - byte_truth)^2, exact
 *   mse[b][t]     float64: sse / (255^2 * 3 * size^2)
 *   ssim[b][t]    float64: scikit-image's structural_similarity(gaussian_weights=True, use_sample_covariance=False, data_range=255)
 *                 of the two luma planes (sigma 1.5, 11 taps, mean over rows / columns 5 .. size-6), moments in float64
 *   pred_bytes, truth_bytes   both NULL, or (batch, n_frames, size, size, 3) uint8, 4-byte aligned: the RGB bytes in PNG pixel order
 *   accum         NULL, or 24 bytes on the device, 8-byte aligned: {float64 sum of ssim, float64 sum of mse, int64 image count}.  A
 *                 second launch adds this call's batch * n_frames values to the running sums one by one in ascending order (so the sums
 *                 do not depend on how a set was split into calls) and the number of images to the count.
 * A NaN in either frame of an image (found by comparing the float with itself) makes that image's ssim and mse NaN, leaves its sse
 * at -1 and writes the NaN pixel's byte as 0; no other image is affected. */
int odehip_png_metrics(const float* pred, const float* truth, int batch, int n_frames, int channels, int size, int denorm,
                       long long* sse, double* mse, double* ssim, unsigned char* pred_bytes, unsigned char* truth_bytes, void* accum,
                       void* stream);

/* z0 ~ N(mean_z0, std_z0) by the reparameterisation trick and its KL term against N(0, 1) (latent_sample.hip): the `opt.z_sample`
 * mode the reference declares in configs.yaml and leaves at a TODO (models/ODEConvGRU.py:72-77; the objective is named in
 * models/ConvGRU.py:285-290).  ONE launch each, enqueue-only on `stream`, caller-provided memory only, arguments checked before any
 * HIP call (ODEHIP_EINVAL).  Pure additions: ODEHIP_ABI_VERSION stays.
 * mean, std: (batch, channels, 16, 16) fp32 NCHW, channels % 4 == 0; n_samples = K >= 1.
 *   z0       (K * batch, channels, 16, 16), sample-major: row k * batch + b = fma(std[b], eps[k][b], mean[b])
 *   kl       NULL or (batch): kl[b] = sum_{c,h,w} 0.5 (mean^2 + std^2 - 1) - log std, i.e. torch.distributions.kl_divergence(
 *            Normal(mean, std), Normal(0, 1)) summed per sample; every term and the sum in float64, rounded to fp32 once, fixed order,
 *            no atomics (two calls are bitwise equal).  No clamp: std == 0 gives +inf, a NaN stays a NaN (in its own sample only).
 *   eps_out  NULL or z0's shape: the noise that was used.
 * Noise.  eps_in != NULL (z0's shape): the caller's noise, the generator is not run.  Otherwise a counter-based stream: the element
 * quad q = ((k * global_batch + batch_offset + b) * channels + c) * 64 + pixel / 4 (pixel = h * 16 + w) of the GLOBAL noise tensor
 * (K, global_batch, channels, 16, 16) is
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (q lo, q hi, offset lo, offset hi), key = (seed lo, seed hi))   [Random123 constants]
 *   u(w)             = ((w >> 9) + 0.5) * 2^-23            in (0, 1), 24 significant bits: exact in fp32
 *   r_i              = sqrt(-2 ln u(w_2i)),  i = 0, 1      at most sqrt(48 ln 2) = 5.77
 *   eps[4 pixels]    = (r_0 cos(2 pi u(w1)), r_0 sin(2 pi u(w1)), r_1 cos(2 pi u(w3)), r_1 sin(2 pi u(w3)))
 * evaluated in fp32 (logf, sqrtf, sincospif of the exact 2 u).  batch_offset = the first global sample of this shard, global_batch
 * the size of the whole batch (batch_offset + batch <= global_batch; one device: 0 and batch).  The draw depends on nothing else --
 * not on the launch geometry, not on the shard: a shard gets the rows of the full draw bit for bit.  `offset` separates the draws of
 * one seed (the Python binding advances it by one per call).
 *
 * odehip_latent_sample_backward: grad_z0 (K * batch, channels, 16, 16); grad_kl NULL (no KL term) or (batch); the forward's mean, std,
 * K and noise arguments (eps is regenerated from the counter: nothing is stored between forward and backward).  Out:
 *   grad_mean[b] = sum_k grad_z0[k][b]             + grad_kl[b] mean[b]
 *   grad_std[b]  = sum_k grad_z0[k][b] eps[k][b]   + grad_kl[b] (std[b] - 1 / std[b])
 * k in ascending order with explicit fmas: the regenerated-noise call and the eps_in = eps_out call are bitwise equal.  The |.| behind
 * std_z0 belongs to the encoder's backward (odehip_odeconvgru_encode_backward: grad_std), not to this call. */
int odehip_latent_sample(const float* mean, const float* std, int batch, int channels, int height, int width, int n_samples,
                         uint64_t seed, uint64_t offset, int batch_offset, int global_batch, const float* eps_in, float* z0, float* kl,
                         float* eps_out, void* stream);
int odehip_latent_sample_backward(const float* grad_z0, const float* grad_kl, const float* mean, const float* std, int batch,
                                  int channels, int height, int width, int n_samples, uint64_t seed, uint64_t offset, int batch_offset,
                                  int global_batch, const float* eps_in, float* grad_mean, float* grad_std, void* stream);

/* The scalar training losses and their backward (frame_loss.hip): what models/ODEConvGRU.py, models/ConvGRU.py and models/VidODE.py
 * compute between the forward and the backward pass, as one call each way instead of a chain of small library kernels (and, for the
 * L1 pair, of host synchronisations).  Enqueue-only on `stream`, caller-provided memory only, arguments checked before any HIP call
 * (ODEHIP_EINVAL: null pointers, counts below 1, misaligned pointers or strides).  Pure additions: ODEHIP_ABI_VERSION stays.
 * Arithmetic, both kinds: every difference, square, absolute value and sum in float64 from the fp32 inputs, rounded to fp32 once; the
 * order of every sum is a function of the sizes alone (thread partials in element order with 16-byte loads, wave xor-shuffles, wave
 * partials in index order, workgroup partials in workgroup order; no atomics): two calls are bitwise equal, on any machine.  A NaN or
 * Inf of an input reaches the loss by plain arithmetic.  Forward: two launches (partials into `workspace`, then a one-workgroup
 * final); backward: one launch.  out: three floats.
 *
 * odehip_loss_mse: pred (n_samples * batch, row_elems) sample-major, truth (batch, row_elems), both contiguous and 16-byte aligned,
 * row_elems % 4 == 0: element i of pred row k * batch + b pairs with element i of truth row b (the truth is not repeated in memory).
 * kl NULL or (batch).  N = n_samples * batch * row_elems.
 *   out[1] = mse     = sum (pred - truth)^2 / N
 *   out[2] = kl_term = kl_scale * sum_b kl[b]           (0 with kl == NULL; the models pass kl_scale = 1 / (batch * latent elements))
 *   out[0] = loss    = mse + kl_weight * kl_term        (mse with kl == NULL)
 * workspace: odehip_loss_mse_workspace_bytes(n_samples, batch, row_elems) bytes, 8-byte aligned.
 * odehip_loss_mse_backward: grad_out = one float ON THE DEVICE (d / d loss; never copied to the host).
 *   grad_pred = fl32(pred - truth) * fl32(2 grad_out / N)       (pred's shape; a non-finite value stays in its own element)
 *   grad_kl[b] = fl32(grad_out * kl_weight * kl_scale)          (grad_kl NULL: not written) */
size_t odehip_loss_mse_workspace_bytes(int n_samples, int batch, long long row_elems);
int odehip_loss_mse(const float* pred, const float* truth, int n_samples, int batch, long long row_elems, const float* kl, double kl_scale,
                    float kl_weight, float* out, void* workspace, size_t workspace_bytes, void* stream);
int odehip_loss_mse_backward(const float* grad_out, const float* pred, const float* truth, int n_samples, int batch, long long row_elems,
                             double kl_scale, float kl_weight, float* grad_pred, float* grad_kl, void* stream);

/* odehip_loss_vidode_l1: the L1 pair of models/VidODE.py's get_loss (reference :211-226).  frame_elems = P, a multiple of 4.
 *   pred   (batch, n_sel, P) contiguous
 *   inter  (batch, n_sel, P) through inter_batch_stride / inter_frame_stride in elements (multiples of 4; P contiguous elements per
 *          frame): the channel slice [:, :, 2:2+c] of the flow decoder's (batch, n_sel, c + 3, H, W) output as it lies
 *   truth  (batch, n_frames, P) contiguous;  init (batch, P) through init_batch_stride: the last observed frame, a view as well
 *   mask   (batch, n_frames), non-zero = selected: float32 (mask_is_byte 0) or uint8 / bool (mask_is_byte 1)
 * s(b, j) = the j-th selected frame of row b (each workgroup scans its mask row; no prefix tensor, no host count; selected frames
 * behind the n_sel-th are ignored).  d(b, t) = truth[b][t] - (t > 0 ? truth[b][t - 1] : init[b]).  N = batch * n_sel * P.
 *   out[1] = l1_pred = sum |pred[b][j] - truth[b][s(b, j)]| / N
 *   out[2] = l1_diff = sum |inter[b][j] - d(b, s(b, j))| / N
 *   out[0] = loss    = l1_pred + l1_diff
 * A row that selects fewer than n_sel frames makes all three NaN; nothing is read for the frames it cannot pair.
 * workspace: odehip_loss_vidode_l1_workspace_bytes(batch, n_sel, frame_elems) bytes, 8-byte aligned.
 * odehip_loss_vidode_l1_backward: grad_out = one float on the device; grad_pred, grad_inter (batch, n_sel, P) contiguous:
 *   grad_pred  = sgn(pred - truth_s) * fl32(grad_out / N),  grad_inter = sgn(inter - d) * fl32(grad_out / N)
 * sgn as the backward of torch.abs has it: 0 at 0 and at NaN, +-1 at +-inf (the sign of the float64 difference).  The frames of a
 * row with too few selected frames get NaN. */
size_t odehip_loss_vidode_l1_workspace_bytes(int batch, int n_sel, int frame_elems);
int odehip_loss_vidode_l1(const float* pred, const float* inter, long long inter_batch_stride, long long inter_frame_stride,
                          const float* truth, const float* init, long long init_batch_stride, const void* mask, int mask_is_byte, int batch,
                          int n_frames, int n_sel, int frame_elems, float* out, void* workspace, size_t workspace_bytes, void* stream);
int odehip_loss_vidode_l1_backward(const float* grad_out, const float* pred, const float* inter, long long inter_batch_stride,
                                   long long inter_frame_stride, const float* truth, const float* init, long long init_batch_stride,
                                   const void* mask, int mask_is_byte, int batch, int n_frames, int n_sel, int frame_elems, float* grad_pred,
                                   float* grad_inter, void* stream);

/* The adversarial step of Vid-ODE (instnorm_act.hip, gan.hip): what runs around the 4x4 convolutions of its two LSGAN discriminators
 * (models/gan.py).  Enqueue-only on `stream`, caller-provided memory only, no atomics, arguments checked before any HIP call
 * (ODEHIP_EINVAL).  Every sum has a fixed order: two calls are bitwise equal.  Pure additions: ODEHIP_ABI_VERSION stays.
 *
 * odehip_instnorm_lrelu_forward: InstanceNorm2d (no affine, biased variance) + LeakyReLU(slope) over contiguous planes x (planes, hw),
 * hw >= 2 (a single element has no variance; torch refuses it too), eps >= 0; slope 0 is ReLU.  One launch.
 *   mean[p] = fl32(sum_64 x / hw),  d = fl32(x - mean_64),  rstd[p] = fl32(1 / sqrt(sum_64 d^2 / hw + eps))       (_64: in float64)
 *   y = xhat > 0 ? xhat : slope * xhat,  xhat = d * rstd           (a constant plane gives exactly 0; never E[x^2] - mean^2)
 * A plane of hw <= 1024 is held in the registers of one wavefront (one read, one write); a larger one is walked three times by one
 * workgroup.  Nothing crosses planes: a NaN or Inf stays in its plane.
 * odehip_instnorm_lrelu_backward: from grad_y and the forward's x, mean, rstd, one launch:
 *   xhat = (x - mean) * rstd,  g' = xhat > 0 ? grad_y : slope * grad_y,  grad_x = rstd * (g' - mean(g') - xhat * mean(g' * xhat))
 * (the two plane means from float64 sums; the comparison is false for NaN, as torch's leaky_relu_backward has it). */
int odehip_instnorm_lrelu_forward(const float* x, int planes, int hw, float eps, float slope, float* y, float* mean, float* rstd,
                                  void* stream);
int odehip_instnorm_lrelu_backward(const float* grad_y, const float* x, const float* mean, const float* rstd, int planes, int hw,
                                   float slope, float* grad_x, void* stream);

/* odehip_gan_seq_assemble: the sequences the sequence discriminator judges.  input_real (batch, t_in, P), frames (batch, t, P), P =
 * frame_elems -> out (t * batch, L, P), all contiguous; row i * batch + n:
 *   interp 0 (extrapolation)  L = max(t, t_in + 1):  [zeros x (L - l_i)] ++ input_real[n, i:] ++ frames[n, :i+1],  l_i = max(0, t_in - i) + i + 1
 *   interp 1 (interpolation)  t_in == t, L = t:      input_real[n] with frame i replaced by frames[n, i]
 * One launch, a gather over `out` (16-byte copies when P % 4 == 0 and the pointers are 16-byte aligned).
 * odehip_gan_seq_assemble_backward: grad_out (t * batch, L, P) -> grad_frames (batch, t, P), one launch, a gather over grad_frames:
 * grad_frames[n, j] = the sum of its copies in the rows i = j .. t-1, added in ascending i in fp32 (interpolation: row j alone).
 * input_real is a constant. */
int odehip_gan_seq_assemble(const float* input_real, const float* frames, int batch, int t_in, int t, long long frame_elems, int interp,
                            float* out, void* stream);
int odehip_gan_seq_assemble_backward(const float* grad_out, int batch, int t_in, int t, long long frame_elems, int interp, float* grad_frames,
                                     void* stream);

/* odehip_loss_lsgan: out[0] = fl32(sum_64 (pred[i] - target)^2 / n), n >= 1 floats, any alignment of 4 bytes.  Two launches
 * (workgroup partials in float64 into `workspace`, odehip_loss_lsgan_workspace_bytes(n) bytes, 8-byte aligned; a one-workgroup
 * final); the order of the sum is a function of n alone.
 * odehip_loss_lsgan_backward: grad[i] = fl32(grad_out * 2 * (pred[i] - target) / n) in float64 until the one rounding; grad_out is
 * one float ON THE DEVICE.  One launch. */
size_t odehip_loss_lsgan_workspace_bytes(long long n);
int odehip_loss_lsgan(const float* pred, long long n, float target, float* out, void* workspace, void* stream);
int odehip_loss_lsgan_backward(const float* grad_out, const float* pred, long long n, float target, float* grad, void* stream);

/* Fixed-grid solvers on an internal grid (grid_interp.hip): torchdiffeq 0.2.1's options={"grid_constructor": fn} / "step_size".  The
 * solver runs on a grid of n_grid points chosen by the caller (odehip_odeint_fixed with the grid as its time array) and the n_times
 * requested times are filled by linear interpolation, as FixedGridODESolver.integrate does:
 *   j = 1;  for n = 0 .. n_grid-2, (t0, t1) = (grid[n], grid[n+1]):  while j < n_times and t1 >= t[j]:  emit j from interval n;  j += 1
 * with every comparison in float64.  Pure additions: ODEHIP_ABI_VERSION stays.
 *
 * odehip_grid_emit_table: HOST ONLY (touches no device).  grid and t strictly increasing with grid[0] == t[0] and grid[n_grid-1] ==
 * t[n_times-1] (else ODEHIP_EINVAL); n_grid >= 2 unless n_times == 1.  Out, host arrays:
 *   first (n_grid)   interval n emits the outputs first[n] <= j < first[n+1]; first[0] = 1, first[n_grid-1] = n_times
 *   exact (n_times)  1 if t[j] == t1 of its interval (solution[j] is that grid state itself, no arithmetic), else 0; exact[0] = 1
 *   slope (n_times)  fl32((t[j] - t0) / (t1 - t0)), the quotient taken in float64; 1 for an exact hit, 0 for j = 0
 *
 * odehip_grid_emit: grid_states (n_grid, state_floats) as the solver wrote them -> out (n_times, state_floats), one launch:
 *   out[0] = Y[0];   out[j] = Y[n+1] for an exact hit, else Y[n] + slope[j] * (Y[n+1] - Y[n])    (n = the interval of j)
 * difference, product and sum rounded one after the other (no contraction): the expression order of torchdiffeq's _linear_interp.
 * odehip_grid_scatter: its backward, grad_out (n_times, state_floats) -> grad_grid (n_grid, state_floats), one launch written as a
 * gather per grid point, so that every sum has a fixed order and nothing is atomic:
 *   grad_grid[n] = [n == 0] grad_out[0] + sum_{j in interval n-1} w1_j grad_out[j] + sum_{j in interval n} w0_j grad_out[j]
 * (w1, w0) = (1, 0) for an exact hit (the w0 term is left out), else (slope, 1 - slope) with 1 - slope taken in fp32; j ascending,
 * explicit fmas.  grad_grid is what odehip_odeint_fixed_backward takes as grad_out on the grid.
 * Both: state_floats a positive multiple of 4, device pointers 16-byte aligned; first / slope / exact are the HOST arrays of
 * odehip_grid_emit_table; table_dev is odehip_grid_table_bytes(n_grid, n_times) bytes of the caller's device memory, into which the
 * table travels in one asynchronous staged upload.  Enqueue-only on `stream`, no hidden allocation; null pointers, a table that does
 * not cover the n_times outputs, n_grid < 2 with n_times > 1 and more than 4096 points either way are refused before anything is
 * enqueued (ODEHIP_EINVAL). */
size_t odehip_grid_table_bytes(int n_grid, int n_times);
int odehip_grid_emit_table(const double* grid, int n_grid, const double* t, int n_times, int* first, float* slope, int* exact);
int odehip_grid_emit(const float* grid_states, float* out, const int* first, const float* slope, const int* exact, int n_grid,
                     int n_times, long long state_floats, void* table_dev, size_t table_bytes, void* stream);
int odehip_grid_scatter(const float* grad_out, float* grad_grid, const int* first, const float* slope, const int* exact, int n_grid,
                        int n_times, long long state_floats, void* table_dev, size_t table_bytes, void* stream);

/* Gradients through NEGATED solves: what torchdiffeq differentiates when t is strictly DEcreasing (it solves dz/ds = -f(z) on
 * s = -t; the host passes -t, increasing, as for negate != 0 above).  A Runge-Kutta step sees the dynamics only as the product
 * h * f, so the negated solve IS the plain solver run with the step sizes -h, and every backward pass below is the existing one with
 * that sign on its step sizes: the same launches, tables and kernels, the sign is data (the forward keeps k_scale = -1 on +h, the
 * reverse sweeps read -h wherever a slope's seed, a weight gradient's weight or a recomputed stage is formed).  fp32 stacks only
 * (no bf16 image: ODEHIP_EINVAL); every other limit, the workspace sizes and the argument checks -- before any HIP call -- are those
 * of the entry named.  The entries above are unchanged, their refusals included.  Pure additions: ODEHIP_ABI_VERSION stays.
 *   odehip_odeint_fixed_negated_saving      odehip_odeint_fixed(save_for_backward = 1, negate = 1); saved format 0
 *   odehip_odeint_fixed_negated_backward    odehip_odeint_fixed_backward on that workspace (it re-uploads the step sizes, signed)
 *   odehip_odeint_adjoint_backward_negated  odehip_odeint_adjoint_backward for a trajectory of the negated solve: interval i runs
 *                                           from -t[i] back to -t[i-1] on the negation of the negated dynamics, plain f
 *   odehip_odeint_adaptive_saving_negated   odehip_odeint_adaptive_saving of the negated dynamics: the attempts, the controller and
 *                                           its accept / reject decisions are odehip_odeint_adaptive(negate = 1)'s
 *   odehip_odeint_adaptive_backward_negated, _backward_saved_negated   the two backward passes of the accepted steps of such a solve
 *                                           (accepted_host: the log as reported, dt > 0 on s) */
int odehip_odeint_fixed_negated_saving(const odehip_convstack* f, int method, const float* z0_nchw, const double* t_host, int n_times,
                                       int batch, float* out_nchw, void* workspace, size_t workspace_bytes, void* stream);
int odehip_odeint_fixed_negated_backward(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method, const double* t_host,
                                         int n_times, int batch, const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w,
                                         float* const* grad_b, void* workspace, size_t workspace_bytes, void* stream);
int odehip_odeint_adjoint_backward_negated(const odehip_convstack* f, const odehip_convstack* f_dgrad, int method, const double* t_host,
                                           int n_times, int batch, const float* y_traj_nchw, const float* grad_out_nchw,
                                           float* grad_z0_nchw, float* const* grad_w, float* const* grad_b, void* workspace,
                                           size_t workspace_bytes, void* stream);
int odehip_odeint_adaptive_saving_negated(int method, const odehip_convstack* f, const float* z0_nchw, const double* t_host, int n_times,
                                          int batch, float rtol, float atol, double first_step, int max_steps, float* out_nchw,
                                          int* stats_host, double* accepted_host, int accepted_cap, int max_accept, int* saved_out,
                                          void* workspace, size_t workspace_bytes, void* stream);
int odehip_odeint_adaptive_backward_negated(int method, const odehip_convstack* f, const odehip_convstack* f_dgrad, const double* t_host,
                                            int n_times, int batch, const double* accepted_host, int n_steps, const float* z0_nchw,
                                            const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w, float* const* grad_b,
                                            void* workspace, size_t workspace_bytes, void* stream);
int odehip_odeint_adaptive_backward_saved_negated(int method, const odehip_convstack* f, const odehip_convstack* f_dgrad,
                                                  const double* t_host, int n_times, int batch, const double* accepted_host, int n_steps,
                                                  const float* grad_out_nchw, float* grad_z0_nchw, float* const* grad_w,
                                                  float* const* grad_b, int max_accept, void* saved_workspace,
                                                  size_t saved_workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ODECGRU_HIP_H */
