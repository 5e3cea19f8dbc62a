#!/bin/bash
# Mutation check of the parity suite ("a deliberately wrong tableau coefficient turns the suite red").
# Builds mutated copies of the library under gpurun_ab/mut/ (git-ignored scratch that travels to the GPU box) -- run with
# `tools/mutation_check.sh build` HERE (hipcc cross-compiles; `patterns` only checks that every pattern still changes one file), then `tools/mutation_check.sh run` on the GPU box: every mutant
# must FAIL the forward parity tests, the unmutated library must pass them.  Summary -> gpurun_out/mutation_check.txt.
set -u
ROOT=$(cd "$(dirname "$0")/.." && pwd)
MUT=$ROOT/gpurun_ab/mut
declare -A SED
# the tableau of the fixed-grid methods (fixed_tableau.h): every driver and both bf16 whole-trajectory kernels read it
SED[rk4_stage3]='s/{-(1.0f \/ 3.0f), 1.0f}/{-0.25f, 1.0f}/'                                   # a[2][0] of the 3/8 rule: x3 = y + h (k2 - k1/3): -1/3 -> -1/4
SED[rk4_weights_classic]='s/{0.125f, 0.375f, 0.375f, 0.125f}/{0.1666667f, 0.3333333f, 0.3333333f, 0.1666667f}/'
SED[midpoint_half]='s/{2, {{}, {0.5f}}, {0.0f, 1.0f}}/{2, {{}, {0.45f}}, {0.0f, 1.0f}}/'
# ... and the three plans derived from it, one mutant each (forward combine, reverse-sweep targets, adjoint targets).  plan_reverse_sign
# alters second-order terms only: the kink-free strict test misses it, test_backward_random_dynamics and test_hip_bf16's comparison
# of the register-resident sweep with the per-launch one catch it;
# plan_adjoint_result_weight needs dynamics with a sizeable Jacobian: test_hip_tanh_dynamics's adjoint parity does (both in TESTS)
SED[plan_forward_own_weight]='s/  p.c\[p.n_prev\] = row\[s\];/  p.c[p.n_prev] = row[s] * 0.9f;/'
SED[plan_reverse_sign]='s/    if (written) p.t\[p.n++\] = FixedTarget{j, j, 1.0f, 0.0f, 0.0f, T.a\[s\]\[j\]};/    if (written) p.t[p.n++] = FixedTarget{j, j, 1.0f, 0.0f, 0.0f, -T.a[s][j]};/'
SED[plan_adjoint_result_weight]='s/  if (T.b\[s\] != 0.0f) p.t\[p.n++\] = FixedTarget{kSlotR, r_src, 1.0f, 0.0f, 0.0f, T.b\[s\]};/  if (T.b[s] != 0.0f) p.t[p.n++] = FixedTarget{kSlotR, r_src, 1.0f, 0.0f, 0.0f, T.b[s] * 0.5f};/'
SED[codec_convt_tap]='s/if (parity == 0) { k = t == 0 ? 1 : 3;/if (parity == 0) { k = t == 0 ? 3 : 1;/'        # frame decoder: kernel rows of the even output rows swapped
SED[codec_enc_slope]='s/v = w2\[((size_t)co \* kEncMid + 4 \* kq + j) \* 9 + tap\];/v = w2[((size_t)co * kEncMid + 4 * kq + j) * 9 + (8 - tap)];/'  # frame encoder: second conv's filter flipped
SED[wino5_bt_coef]='s/out\[0\] = fma2(4.0f, in\[0\], fma2(-5.0f, in\[2\], in\[4\]));/out[0] = fma2(4.0f, in[0], fma2(-4.0f, in[2], in[4]));/'      # F(2x2,5x5): B^T row 0: -5 -> -4
SED[wino5_at_coef]='s/^  return i == 0 ? 0.0f : (i == 1 ? 1.0f : (i == 2 ? -1.0f : (i == 3 ? 2.0f : (i == 4 ? -2.0f : 1.0f))));/  return i == 0 ? 0.0f : (i == 1 ? 1.0f : (i == 2 ? -1.0f : (i == 3 ? 2.0f : (i == 4 ? -1.0f : 1.0f))));/'    # F(2x2,5x5): A^T row 1: -2 -> -1
SED[wgrad_wino_g]='s/const float hs = 0.5f \* (u\[1\]\[j\] + u\[2\]\[j\]), hd = 0.5f \* (u\[1\]\[j\] - u\[2\]\[j\]);/const float hs = 0.5f * (u[1][j] + u[2][j]), hd = 0.4f * (u[1][j] - u[2][j]);/'   # Winograd-domain weight gradient: one G entry 0.5 -> 0.4
SED[wgrad_wino_at]='s/\*(f32x4\*)(wr + (4 \* i + 2) \* kW2Plane) = t\[i\]\[0\] - t\[i\]\[1\];/*(f32x4*)(wr + (4 * i + 2) * kW2Plane) = t[i][0] + t[i][1];/'   # ... and one sign of A dY A^T
# ---- round 3: the adaptive walk, the device-driven adjoint, the saving forward, the 16-workgroup walk
SED[adapt_combine_ccur]='s/      d_cA = m.c1\[np\];/      d_cA = m.c1[np] * 1.01f;/'                                  # adaptive walk: weight of the stage's own k in an order-1 combine
SED[adapt_ew_coef]='s/    const float c1 = (m.c_dev ? ((ConstF\*)m.c_dev)\[j\] : m.c1\[j\]) \* hs;/    const float c1 = (m.c_dev ? ((ConstF*)m.c_dev)[j] : m.c1[j]) * hs * 1.01f;/'   # elementwise rows of the walk
SED[walk16_ew_coef]='s/      s1 = fma4(kv, (m.c_dev ? ((ConstF\*)m.c_dev)\[j\] : m.c1\[j\]) \* hs, s1);/      s1 = fma4(kv, (m.c_dev ? ((ConstF*)m.c_dev)[j] : m.c1[j]) * hs * 1.01f, s1);/'   # ... and their sixteen-workgroup copy (ew_row16)
SED[dopri5_dense_weight]='s/^ODEHIP_HD inline double dense_weight(int s, double x, double b, double m, int last) {$/ODEHIP_HD inline double dense_weight(int s, double x, double b, double m, int last) { x *= 0.97;/'   # dopri5_control.h: dense-output weights evaluated at the wrong point (one function behind the device controller, the host-driven adjoint and the backward sweep)
SED[walk16_out_transform]='s/      val = pk_sub(pk_sub(\*(const f32x4\*)(x + 1024) + bias4, \*(const f32x4\*)(x + 2048)), \*(const f32x4\*)(x + 3072));/      val = pk_sub(pk_sub(*(const f32x4*)(x + 1024) + bias4, *(const f32x4*)(x + 3072)), *(const f32x4*)(x + 2048)) * 1.001f;/'   # 16-workgroup walk: second half of the output transform
# ---- the pieces the walks of conv_wino.hip share: each must turn red a test of EVERY walk that uses it (profiles/mutation_walk_epilogue.txt)
SED[shared_out_transform]='s/    y\[2 \* i + 1\] = pk_sub(pk_sub(S\[i\]\[1\] + bias4, S\[i\]\[2\]), S\[i\]\[3\]);/    y[2 * i + 1] = pk_sub(pk_sub(S[i][1] + bias4, S[i][3]), S[i][2]) * 1.001f;/'   # out_transform (per-launch kernel, co-tile walks, strip walk): odd output columns; blind to the bit-identity tests (all go wrong alike), caught against the oracle: test_hip_odeint.py::test_full_size_against_oracle[rk4] (strip walk, B = 64) and [dopri5] (adaptive co-tile walk)
SED[six_row_transform]='s/    \*(f32x4\*)(v + 1 \* 1024) = T\[1\] + T\[2\];/    *(f32x4*)(v + 1 * 1024) = T[1] - T[2];/'   # SixRowProducer (sixteen-workgroup walk, strip walk): V column 1; tests/test_hip_strip_walk.py and a B <= 16 case of test_persistent_trajectory_is_bit_identical_to_per_layer_launches
SED[saving_slot_offset]='s/  fa.off_y1 = (long long)((tb->stages - 1) \* BL.st);/  fa.off_y1 = (long long)((tb->stages - 2) * BL.st);/'                # saving forward: y1 read from the wrong stage input of the slot
SED[wgrad_wino5_bt]='s/  out\[0\] = w5_fma2(4.0f, in\[0\], w5_fma2(-5.0f, in\[2\], in\[4\]));/  out[0] = w5_fma2(4.0f, in[0], w5_fma2(-4.0f, in[2], in[4]));/'   # Winograd F(2x2,5x5) weight gradient: B^T row 0
SED[codec_bwd_dec_tap]='s/          const int pa = (ky \& 1) ^ 1, ta = ky >> 1, pb = (kx \& 1) ^ 1, tb = kx >> 1;/          const int pa = (ky \& 1) ^ 1, ta = ky >> 1, pb = (kx \& 1), tb = kx >> 1;/'   # decoder backward: column parity of the second layer'"'"'s weights
SED[codec_bwd_enc_dx]='s/        const int dx = kx == 0 ? 1 : 0;/        const int dx = kx == 2 ? 1 : 0;/'   # encoder backward: which odd-column tap reads the next source column
SED[codec_bwd_dw1_centre]='s/        const float\* const bp = gm + ((2 \* iy + ky) \* kMW + 8 \* kq + kx) \* kMPix + nn;/        const float* const bp = gm + ((2 * iy + ky) * kMW + 8 * kq + kx + 1) * kMPix + nn;/'   # decoder backward: dW1 operand shifted by one column
# ---- round 4: the flow decoder's upsampling, the split 5x5 launches, the seal of an asynchronous solve
SED[upsample_src_index]='s/  float s = 0.5f \* ((float)dst + 0.5f) - 0.5f;/  float s = 0.5f * ((float)dst + 0.5f) - 0.45f;/'           # bilinear x2: source index off by 0.05 px
SED[split5_drop_partial]='s/      for (int e = 0; e < 4; ++e) tot\[e\] = k == 0 ? pk\[e\] : tot\[e\] + pk\[e\];/      for (int e = 0; e < 4; ++e) tot[e] = k <= 1 ? pk[e] : tot[e] + pk[e];/'   # split 5x5 conv: the first split'"'"'s partial is dropped
SED[seal_no_nan]='s/  for (long long i = (long long)blockIdx.x \* 256 + threadIdx.x; i < n; i += (long long)gridDim.x \* 256) o\[i\] = nan;/  for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) o[i] = 0.0f;/'   # sealed async solve: unreached frames zero instead of NaN
SED[bn_bwd_mean_term]='s/  m2\[c\] = (float)(b \/ count);/  m2[c] = (float)(a \/ count);/'   # fused BatchNorm backward: the xhat term gets the wrong mean
SED[bn_running_var_biased]='s/    const double unbiased = count > 1.0 ? var \* count \/ (count - 1.0) : var;/    const double unbiased = var;/'   # running_var updated with the biased variance
SED[relu_launders_nan]='s/__device__ __forceinline__ float relu_f(float v) { return v < 0.0f ? 0.0f : v; }/__device__ __forceinline__ float relu_f(float v) { return fmaxf(v, 0.0f); }/'   # the ReLU of every epilogue back to v_max_f32: NaN -> 0
SED[evalwalk_no_nan_fill]='s/      nan_fill_row16(\*(const ConvArgs\*)((ConstArgs\*)table + l), b, cq, rq, pa.reloc, pa.out_nchw);/      (void)0;/'   # sixteen-workgroup walk: a launch whose wait gave up leaves its outputs as they are
SED[dopri5_beta32]='s|{44.0 / 45, -56.0 / 15, 32.0 / 9, 0, 0, 0}|{44.0 / 45, -56.0 / 15, 31.0 / 9, 0, 0, 0}|'   # dopri5_control.h: one beta of the Dormand-Prince tableau
# ---- NaN semantics: a failed asynchronous solve, the ReLU-backward masks
SED[seal_skips_failed_solve]='s|  if (st->done \&\& st->status == 0) return;   // finished: every frame is written|  if (st->done) return;|'   # seal: a solve the controller failed keeps stale frames
SED[act_bwd_launders_nan]='s/    g.x = y.x <= 0.0f ? 0.0f : g.x; g.y = y.y <= 0.0f ? 0.0f : g.y;/    g.x = y.x > 0.0f ? g.x : 0.0f; g.y = y.y > 0.0f ? g.y : 0.0f;/;s/    g.z = y.z <= 0.0f ? 0.0f : g.z; g.w = y.w <= 0.0f ? 0.0f : g.w;/    g.z = y.z > 0.0f ? g.z : 0.0f; g.w = y.w > 0.0f ? g.w : 0.0f;/'   # fp32 ReLU backward: NaN -> 0
SED[bn_bwd_launders_nan]='s/      const float gv = pre <= 0.0f ? 0.0f : grad_at<UP>(g, pl, y, xx, H, W);/      const float gv = pre > 0.0f ? grad_at<UP>(g, pl, y, xx, H, W) : 0.0f;/'   # fused BatchNorm + ReLU backward: NaN -> 0
SED[bf16_mask_launders_nan]='s/          v.x = m.x <= 0.f ? 0.f : v.x; v.y = m.y <= 0.f ? 0.f : v.y; v.z = m.z <= 0.f ? 0.f : v.z; v.w = m.w <= 0.f ? 0.f : v.w;/          v.x = m.x > 0.f ? v.x : 0.f; v.y = m.y > 0.f ? v.y : 0.f; v.z = m.z > 0.f ? v.z : 0.f; v.w = m.w > 0.f ? v.w : 0.f;/'   # bf16 per-evaluation mask: NaN -> 0
SED[btraj_mask_drops_negative_nan]='s/__device__ __forceinline__ bool bf16_relu_pass(unsigned f32_bits) { return !(__uint_as_float(f32_bits) <= 0.0f); }/__device__ __forceinline__ bool bf16_relu_pass(unsigned f32_bits) { return (int)f32_bits > 0; }/'   # bf16 reverse sweep: the old sign-bit test, a NaN with its sign bit set -> 0
# ---- evaluation metrics (frame_metrics.hip): the window, the interior, the constants, the covariance
SED[ssim_sigma]='s/  const double sigma = 1.5;/  const double sigma = 1.4;/'                                   # Gaussian taps of sigma 1.4
SED[ssim_interior_shift]='s/^constexpr int kSsimCrop = kSsimRadius; /constexpr int kSsimCrop = kSsimRadius + 1; /'   # ssim_window.h (frame_metrics.hip and png_metrics.hip share it): S averaged from row and column 6 on
SED[ssim_c2]='s/ssim_constant<float>(0.01, range), ssim_constant<float>(0.03, range), sse, ssim);/ssim_constant<float>(0.01, range), ssim_constant<float>(0.02, range), sse, ssim);/'   # C2 = (0.02 R)^2
SED[ssim_covariance]='s/  const T vxy = uxy - ux \* uy;/  const T vxy = uxy - ux * ux;/'       # vxy = uxy - ux ux
# ---- ConvGRU sequences (convgru_sequence.hip; the step itself is cell_forward_step in convgru.hip): the weight halves, the zero state, the batched weight gradient, the h_seq slots
SED[seq_state_half_from_frame_half]='s/  const int j_gates = x \&\& h ? -1 : (x ? 0 : 1);/  const int j_gates = x \&\& h ? -1 : (x ? 0 : 0);/'   # zero input: the gates conv runs over the FRAME half of its weights
SED[seq_first_step_reads_h0]='s/    const bool has_h = h0 || t > 0;/    const bool has_h = true;/'   # zero state: the first step reads the (unwritten) state slot
SED[seq_wgrad_drops_step]='s/      const int n_eval = half == 0 ? T : n_state, a_ch = half == 0 ? I : H;/      const int n_eval = (half == 0 ? T : n_state) - 1, a_ch = half == 0 ? I : H;/'   # batched weight gradient: the last step is left out
SED[seq_slot_off_by_one]='s/    float\* slot = h_seq + (size_t)t \* batch \* H \* kPix;/    float* slot = h_seq + (size_t)(t > 0 ? t - 1 : 0) * batch * H * kPix;/'   # h_seq[t] written to slot t - 1
# ---- sampled z0 (latent_sample.hip and its binding): the KL term, the sign of the noise in grad_std, the offset of consecutive draws
SED[kl_drops_log_sigma]='s/        acc += 0.5 \* (md \* md + sd \* sd - 1.0) - log(sd);/        acc += 0.5 * (md * md + sd * sd - 1.0);/'   # kl = sum 0.5 (mu^2 + sigma^2 - 1), no - log sigma
SED[grad_std_eps_sign]='s/      gs\[i\] = k ? fmaf(g\[i\], e\[i\], gs\[i\]) : g\[i\] \* e\[i\];/      gs[i] = k ? fmaf(g[i], -e[i], gs[i]) : g[i] * -e[i];/'   # grad_std = - sum_k g eps
# ---- the training losses (frame_loss.hip): the divisor, the pairing of draws and truth rows, the frame differences, the mask row, grad_kl
SED[loss_divisor_forgets_k]='s/static inline double mse_elems(int n_samples, int batch, long long row_elems) { return (double)n_samples \* (double)batch \* (double)row_elems; }/static inline double mse_elems(int n_samples, int batch, long long row_elems) { return (double)batch * (double)row_elems; }/'   # N = B F: the K draws forgotten
SED[loss_truth_row_of_repeated_truth]='s/  const unsigned b = r % batch;/  const unsigned b = r \/ n_samples;/'   # pred row k B + b paired as if the truth lay batch-major under it (row (k B + b) \/ K; the literal "row k B + b" of a truth that is not repeated would read past it)
SED[loss_init_for_every_frame]='s/  r.prev = it.s > 0 ? r.t - fq : (const f32x4l\*)(a.init + it.b \* a.init_bs);/  r.prev = (const f32x4l*)(a.init + it.b * a.init_bs);/'   # d(b, t) = truth[t] - init for every t
SED[loss_mask_row_zero]='s/  const long long row = (long long)b \* a.n_frames;/  const long long row = 0;/'   # s(b, j) from the mask of row 0
SED[loss_grad_kl_drops_weight]='s/    const float gk = (float)(g \* (double)kl_weight \* kl_scale);/    const float gk = (float)(g * kl_scale);/'   # grad_kl = g kl_scale
# ---- internal grids (grid_interp.hip): the two weights of an interpolated output in the backward gather
SED[grid_scatter_weights_swapped]='s/      const float w1 = tb.exact\[j\] ? 1.0f : tb.slope\[j\];/      const float w1 = tb.exact[j] ? 1.0f : 1.0f - tb.slope[j];/;s/      const float w0 = 1.0f - tb.slope\[j\];/      const float w0 = tb.slope[j];/'   # the end state of an interval gets 1 - slope, its start state slope
# ---- the forward convolutions' dispatch by channel shape (test_hip_conv_shapes.py): each one stays inside the buffers of the layer it is given
SED[resident3_as_resident2]='s/        case 3: return launch_resident<3>(a, stream);/        case 3: return launch_resident<2>(a, stream);/'   # 48-channel 3x3: the last 16 input channels dropped
SED[wino3_as_wino2]='s/    case 3: return launch_wino_n<3>(a, stream);/    case 3: return launch_wino_n<2>(a, stream);/'   # ... and on the Winograd kernel
SED[bf16_2_as_bf16_1]='s/    case 2: return launch_bf16_n<2>(a, stream);/    case 2: return launch_bf16_n<1>(a, stream);/'   # 32-channel bf16 3x3: the last 16 input channels dropped
SED[gn_gates_odd_boundary]='s/    if (HAS_H \&\& !is_z) s \*= hp\[q \* kPix\];/    if (HAS_H \&\& !is_z \&\& !((hid_groups \& 1) \&\& hid_groups > 1 \&\& g == hid_groups)) s *= hp[q * kPix];/'   # 3 or 5 groups per gate (hidden 96, 160): the first r group is handled as a z group (no r * h)
# ---- the norm-free ConvGRU cell of upstream Vid-ODE (convgru_plain.hip; tests/test_hip_vidode_upstream.py)
SED[plain_gates_swapped]='s/  const bool is_reset = q < hq;/  const bool is_reset = q >= hq;/;s/  const size_t o = ((size_t)b \* hq + (is_reset ? q : q - hq)) \* kPix + threadIdx.x;/  const size_t o = ((size_t)b * hq + (q < hq ? q : q - hq)) * kPix + threadIdx.x;/'   # the first half of conv_gates taken as the update gate (same addresses)
SED[plain_bwd_drops_bypass]='s/  if (blend) d += (1.0f - m) \* g;  \/\/ the part of the blend that bypasses the cell/  (void)blend;/'   # fractional mask: the (1-m) g term of the state gradient dropped
# ---- upstream Vid-ODE's evaluation protocol (png_metrics.hip; tests/test_hip_png_metrics.py)
SED[png_luma_no_rounding]='s/  return (19595u \* r + 38470u \* g + 7471u \* b + 0x8000u) >> 16;/  return (19595u * r + 38470u * g + 7471u * b) >> 16;/'   # PIL'"'"'s luma truncated instead of rounded
# ---- the solver arithmetic in epilogue() (conv_common.h; tests/test_hip_solver_stacks.py): every pattern matches the copy behind the
# 32x32-accumulator kernels only, not emit_quad()'s; each stays inside the buffers of the layer it is given
SED[epilogue_drops_k_scale]='s/    kc = act_fwd(kc, a.act) \* m.k_scale;   \/\/ (a Tanh head before the sign)/    kc = act_fwd(kc, a.act);/'   # stage combine: the sign of a decreasing t is lost
# (combine 2 multiplies by sc_c + sc_h * h, but every driver sets sc_c = 1, sc_h = 0: dropping `v *= sc;` changes no result the
# library can produce, so the combine-2 mutant drops the activation mask instead)
SED[epilogue_mask_dropped]='s/^        if (w.mask_src) v = act_bwd(v, \*(const f32x4\*)(w.mask_src + off), a.act);$/        (void)0;/'   # combine 2: the gradient passes every hidden unit unmasked
SED[epilogue_target_drops_h]='s/      f32x4 o = gx \* (T.g_c + T.g_h \* hb);/      f32x4 o = gx * T.g_c;/'   # combine 3: the device-side step size of a reverse-sweep target
SED[epilogue_partial_slot]='s/m.err_partials\[part_idx >= 0 ? part_idx : (int)(blockIdx.x + blockIdx.y \* gridDim.x) \* 4 + wave\] = esum;/m.err_partials[part_idx >= 0 ? part_idx : (int)(blockIdx.x + blockIdx.y * gridDim.x) + wave] = esum;/'   # error partials of neighbouring workgroups overwrite each other (lower slots: inside the array)
SED[dopri5_partial_count]='s/  const int n_conv_partials = pps > 16 ? batch \* pps : batch \* (C \/ 32) \* 2 \* 4;/  const int n_conv_partials = pps > 16 ? batch * pps : batch * (C \/ 64) * 2 * 4;/'   # the controller sums half of the partials (none at C = 32); the arrays keep their size of at least 1024 floats
# ---- bosh3 (dopri5_control.h, dopri5.hip): each is rejected by the new files alone -- MUT_TESTS="tests/test_hip_bosh3.py"; the three
# header mutants also by tests/test_adaptive_control_cpu.py, which compiles the header of the tree it runs in
SED[bosh3_keeps_dopri5_exponent]='s|fmax(0.9 / pow((double)ratio, 1.0 / (double)order), dfactor)|fmax(0.9 / pow((double)ratio, 0.2), dfactor)|'   # _optimal_step_size with 1/5 for every method
SED[bosh3_cmid_on_stage_1]='s|^    {0, 1.0 / 2, 0, 0},$|    {1.0 / 2, 0, 0, 0},|'   # c_mid applied to k1 instead of k2
SED[bosh3_fsal_hands_over_k3]='s|      const f32x4 k7 = ((const f32x4\*)a.k\[LAST\])\[i\];|      const f32x4 k7 = ((const f32x4*)a.k[LAST == 3 ? 2 : LAST])[i];|'   # f1 of a bosh3 step = k3 instead of k4
SED[bosh3_initial_step_fifth_root]='s|  else h1 = powf(0.01f / fmaxf(d1, d2), 1.0f / (float)order);|  else h1 = powf(0.01f / fmaxf(d1, d2), 1.0f / 5.0f);|'   # _select_initial_step with dopri5 exponent
# ---- the adjoint's slot geometry (adjoint_layout.h), shared by the host loop and the device-steered path: both go wrong alike, so
# their agreement does not show it; the oracle comparison of tests/test_hip_adjoint_paths.py does -- MUT_TESTS="tests/test_hip_adjoint_paths.py"
SED[adjoint_gp_stride]='s|cap \* NH \* hid + ((size_t)s \* NG + l) \* hid|cap * NH * hid + ((size_t)s * NH + l) * hid|'   # gradient slots of a stage strided by NH, not NG: the seed of stage s is overwritten by stage s + 1 (lower offsets: inside the slot)
# ---- two samples per group and the second pass of the fp32 walks (conv_wino.hip: persist_walk<ADAPT> and persist_walk_v, one file):
# each stays inside the buffers it is given and makes no wait longer (all partners of a group take the same wrong sample)
# -- MUT_TESTS="tests/test_hip_interleaved_walks.py" (profiles/mutation_interleaved_walks.txt)
SED[interleave_second_sample_dropped]='s/    const int n_interleaved = b + n_groups < pa.batch ? 2 : 1;/    const int n_interleaved = 1;/'   # samples 64 .. 127 are never written
SED[interleave_wrong_sample]='s/readfirstlane(b + s \* n_groups)/readfirstlane(b)/'   # sample b is walked twice, b + 64 never
SED[second_pass_skipped]='s/b < pa.batch; b += 2 \* n_groups)/b < pa.batch; b += 4 * n_groups)/'   # samples >= 128 are never written
# ---- odeint_adjoint on internal grids (fixed_grid.hip: adjoint_sweep): both stay inside the workspace.  Rejected by the Tanh cases of
# the new file -- MUT_TESTS="tests/test_hip_grid_adjoint.py" (profiles/mutation_grid_adjoint.txt); the third mutant, the anchoring of the
# backward grids, lives in the binding (PYSED below)
SED[grid_adjoint_resets_interior_y]='s/output_of(p) >= 0 ? L.p(ws, off_traj + (size_t)output_of(p) \* L.st) : L.y(ws, p); };/output_of(p) >= 0 ? L.p(ws, off_traj + (size_t)output_of(p) * L.st) : L.p(ws, off_traj + (size_t)(n_times - 1) * L.st); };/'   # inside an interval y comes from the stored trajectory (its last frame), not from the solver
SED[grid_adjoint_interior_grad_out]='s/      const float\* go = interior ? nullptr : L.go(ws, output_of(n));/      const float* go = L.go(ws, interior ? 0 : output_of(n));/'   # a_y takes a grad_out frame at interior points too
# ---- gradients through negated solves (a decreasing t): the reverse sweep's seeds lose their -1 -- the step sizes of the backward
# passes go unsigned (fixed_grid.hip: fill_step_sizes), the increasing case is untouched -- MUT_TESTS="tests/test_hip_reverse_time.py" (profiles/mutation_reverse_time.txt)
SED[reverse_time_seed_sign]='s/hbuf\[i\] = sign \* (float)(t_host\[i + 1\] - t_host\[i\]);/hbuf[i] = (float)(t_host[i + 1] - t_host[i]);/'
# mutants of the Python binding, "file|sed script": applied to the tree's own file for the run and restored afterwards (run only)
declare -A PYSED
PYSED[grid_adjoint_anchored_low]='ode-rl_amd/hip_ops.py|s/^        pair = torch.stack(\[-th\[i\], -th\[i - 1\]\])$/        pair = torch.stack([th[i - 1], th[i]])/;s/^        points.append(-sub\[1:\])$/        points.append(sub[:-1].flip(0))/'   # the sub-steps of a backward interval anchored at t[i-1]: the constructor sees the unflipped pair
PYSED[z0_offset_stuck]='ode-rl_amd/autograd.py|s/gen.set_offset(at + 4)/gen.set_offset(at)/;s/_explicit_seed\[1\] = offset + 1/_explicit_seed[1] = offset/'   # consecutive sample_z0 calls draw the same noise
# ---- VidODE's whole-model backward (tests/test_hip_vidode_grads.py): each leaves every forward value bitwise as it is
PYSED[vidode_prev_detached]='ode-rl_amd/models/VidODE.py|s/^            prev = sol_out\[:, t, \.\.\.\]$/            prev = sol_out[:, t, ...].detach()/'   # a latent frame reaches the NEXT frame'"'"'s decoder call without a gradient
PYSED[vidode_skip_detached]='ode-rl_amd/models/VidODE.py|s/^        skip = self\.conv_encoder(inputs\[:, -1, \.\.\.\])$/        skip = self.conv_encoder(inputs[:, -1, ...]).detach()/'   # the second encoder pass contributes nothing to the encoder'"'"'s gradients
PYSED[vidode_inter_detached]='ode-rl_amd/models/VidODE.py|s/self\.extra_info\["pred_intermediates"\], self\.batch_dict/self.extra_info["pred_intermediates"].detach(), self.batch_dict/'   # the frame-difference term of the loss reaches nothing
PYSED[bn_conv_bias_eval_grad]='ode-rl_amd/autograd.py|s/else stats\[2\] \* gb$/else gb/'   # eval(): the folded convolution bias gets d beta instead of scale * d beta
TESTS="tests/test_hip_grid_options.py::test_backward_matches_autograd_through_the_restated_loop tests/test_hip_bf16.py::test_whole_trajectory_training_matches_per_evaluation_launches tests/test_hip_tanh_dynamics.py::test_adjoint_matches_oracle_adjoint tests/test_hip_backward.py::test_adjoint_matches_oracle_adjoint tests/test_hip_backward.py::test_backward_random_dynamics tests/test_hip_frame_loss.py tests/test_hip_latent_sample.py tests/test_hip_convgru_sequence.py::test_rollout_forward_against_the_float64_restatement[False-True-10-4-64] tests/test_hip_convgru_sequence.py::test_bptt_against_float64_autograd[False-True-10-4] tests/test_hip_convgru_sequence.py::test_bptt_against_float64_autograd[True-False-10-4] tests/test_hip_convgru_sequence.py::test_a_zero_state_reads_nothing_of_the_state_buffers tests/test_hip_convgru_sequence.py::test_rollout_agrees_with_the_step_by_step_forward[False-True-10-4] tests/test_hip_backward.py::test_backward_strict_on_kink_free_dynamics tests/test_hip_frame_codec.py::test_encoder_matches_reference_fixture tests/test_hip_frame_codec.py::test_decoder_matches_reference_fixture tests/test_hip_conv.py::test_winograd5_conv_matches_torch tests/test_hip_full_size.py::test_cell_and_encoder_full_channels tests/test_hip_odeint.py::test_fixed_grid_on_vigorous_dynamics_matches_reference_fixture tests/test_hip_odeint.py::test_dopri5_on_vigorous_dynamics_matches_reference_fixture tests/test_hip_odeint.py::test_fixed_grid_matches_golden_and_oracle tests/test_hip_odeint.py::test_full_size_against_oracle tests/test_hip_backward.py::test_dopri5_backward_matches_autograd_through_oracle tests/test_hip_backward.py::test_dopri5_adjoint_matches_oracle_adjoint tests/test_hip_backward.py::test_dopri5_saving_forward_equals_reintegration tests/test_hip_reference_configs.py::test_config0_as_stated_b4 tests/test_hip_encoder_backward.py::test_convgru_cell_backward_matches_autograd_through_oracle tests/test_hip_frame_codec.py::test_backward_matches_fp64_autograd tests/test_hip_vidode.py::test_upsample2x_matches_torch tests/test_hip_vidode.py::test_bn_relu_up_matches_torch tests/test_hip_backward.py::test_async_dopri5_forward_matches_the_synchronous_one tests/test_hip_errors.py::test_a_non_finite_state_is_not_laundered tests/test_hip_errors.py::test_a_lost_partner_in_a_single_evaluation_walk_is_loud tests/test_hip_solver_failures.py::test_a_failed_asynchronous_solve_is_sealed_and_reported[max_num_steps-no_grad] tests/test_hip_solver_failures.py::test_a_failed_asynchronous_solve_is_sealed_and_reported[overflow-saving] tests/test_hip_relu_nan_backward.py::test_fixed_grid_backward_passes_the_gradient_of_a_nan_channel[euler-3-per_layer] tests/test_hip_relu_nan_backward.py::test_fixed_grid_backward_passes_the_gradient_of_a_nan_channel[rk4-20-persistent] tests/test_hip_relu_nan_backward.py::test_bf16_backward_passes_the_gradient_of_a_nan_channel tests/test_hip_relu_nan_backward.py::test_bn_relu_up_backward_passes_the_gradient_of_a_nan_activation[shape0-True-True-x] tests/test_hip_relu_nan_backward.py::test_bn_relu_up_backward_passes_the_gradient_of_a_nan_activation[shape0-False-False-gamma] tests/test_hip_frame_metrics.py::test_matches_the_fp64_restatement[3-5-3] tests/test_hip_frame_metrics.py::test_matches_the_fp64_restatement[64-10-1] tests/test_hip_frame_metrics.py::test_evaluate_end_to_end tests/test_hip_conv_shapes.py tests/test_hip_vidode_grads.py tests/test_hip_vidode_upstream.py tests/test_hip_png_metrics.py::test_ssim_matches_the_float64_restatement"
[ -n "${MUT_TESTS:-}" ] && TESTS=$MUT_TESTS   # a subset of the tests (a GPU lease is short): e.g. the files that cover the mutants of MUT_ONLY
# a mutated copy of the sources under $MUT/<mutant>; names the file that differs from the tree's (diff -q) and fails unless exactly one does
mutate() {
  local m=$1 d=$MUT/$1 f changed=0
  rm -rf "$d"; mkdir -p "$d/ode-rl_amd/csrc" "$d/include"
  # sources AND the unmutated build's objects with their timestamps: make then recompiles only what the mutation touches
  cp -p "$ROOT"/ode-rl_amd/csrc/*.hip "$ROOT"/ode-rl_amd/csrc/*.h "$ROOT"/ode-rl_amd/csrc/Makefile "$d/ode-rl_amd/csrc/"
  cp -p "$ROOT"/include/*.h "$d/include/"
  if [ -d "$ROOT/ode-rl_amd/csrc/build" ]; then mkdir -p "$d/ode-rl_amd/csrc/build"; cp -p "$ROOT"/ode-rl_amd/csrc/build/*.o "$d/ode-rl_amd/csrc/build/"; fi
  sed -i "${SED[$m]}" "$d"/ode-rl_amd/csrc/*.hip "$d"/ode-rl_amd/csrc/*.h
  for f in "$d"/ode-rl_amd/csrc/*.hip "$d"/ode-rl_amd/csrc/*.h; do
    diff -q "$f" "$ROOT/ode-rl_amd/csrc/$(basename "$f")" >/dev/null || { echo "mutant $m: ode-rl_amd/csrc/$(basename "$f") differs from the tree's"; changed=$((changed + 1)); }
  done
  if [ $changed -ne 1 ]; then echo "mutant $m: the pattern changed $changed files (expected exactly 1)" >&2; return 1; fi
}
case "${1:-}" in
patterns)   # every pattern still finds its line: the mutated sources only, nothing is built
  bad=0
  for m in "${!SED[@]}"; do
    mutate "$m" || bad=1
    rm -rf "$MUT/$m"
  done
  exit $bad ;;
build)
  for m in "${!SED[@]}"; do
    if [ -n "${MUT_ONLY:-}" ] && [[ ! " $MUT_ONLY " =~ " $m " ]]; then continue; fi
    d=$MUT/$m
    mutate "$m" || exit 1
    make -s -C "$d/ode-rl_amd/csrc" -j8 OUT_DIR="$d/lib" >/dev/null 2>&1 || { echo "mutant $m failed to build" >&2; exit 1; }
    rm -rf "$d/ode-rl_amd/csrc/build"
    echo "built $m"
  done ;;
run)
  # MUT_ONLY="name name ...": only those mutants, appended to the summary (a GPU lease is too short for all nineteen in one go)
  out=$ROOT/gpurun_out/mutation_check.txt
  cd "$ROOT"
  bad=0
  if [ -z "${MUT_ONLY:-}" ]; then
    : > "$out"
    python -m pytest $TESTS -q > gpurun_out/mut_baseline.log 2>&1; rc=$?
    echo "unmutated library: pytest rc=$rc ($(tail -1 gpurun_out/mut_baseline.log))" | tee -a "$out"
    [ $rc -ne 0 ] && bad=1
  fi
  for d in "$MUT"/*/; do
    m=$(basename "$d")
    if [ -n "${MUT_ONLY:-}" ] && [[ ! " $MUT_ONLY " =~ " $m " ]]; then continue; fi
    ODEHIP_LIB=$d/lib/libodecgru_hip.so python -m pytest $TESTS -q > gpurun_out/mut_$m.log 2>&1; rc=$?
    echo "mutant $m: pytest rc=$rc ($(tail -1 gpurun_out/mut_$m.log)) failed: $(grep -c '^FAILED' gpurun_out/mut_$m.log)" | tee -a "$out"
    grep '^FAILED' gpurun_out/mut_$m.log | sed 's/ - .*//' >> "$out"
    [ $rc -eq 0 ] && { echo "  !! mutant $m SURVIVED" | tee -a "$out"; bad=1; }
    # the mutant must fail on PARITY (an assertion of a test), not because it could not be loaded or crashed
    if grep -qE "is missing: build it|reports ABI version|cannot open shared object|undefined symbol|AttributeError: .*odehip_|OSError|Segmentation|core dumped" gpurun_out/mut_$m.log; then
      echo "  !! mutant $m failed for the wrong reason (library not loaded / crash): rebuild the mutants" | tee -a "$out"; bad=1
    fi
  done
  logs=$(dirname "$out")   # the logs go next to the summary
  for m in "${!PYSED[@]}"; do
    if [ -n "${MUT_ONLY:-}" ] && [[ ! " $MUT_ONLY " =~ " $m " ]]; then continue; fi
    f=${PYSED[$m]%%|*}; script=${PYSED[$m]#*|}
    cp -p "$f" "$logs/mut_$m.orig"
    sed -i "$script" "$f"
    if cmp -s "$f" "$logs/mut_$m.orig"; then echo "mutant $m: the pattern changed nothing in $f" | tee -a "$out"; bad=1; continue; fi
    python -m pytest $TESTS -q > $logs/mut_$m.log 2>&1; rc=$?
    cp -p "$logs/mut_$m.orig" "$f"
    echo "mutant $m: pytest rc=$rc ($(tail -1 $logs/mut_$m.log)) failed: $(grep -c '^FAILED' $logs/mut_$m.log)" | tee -a "$out"
    grep '^FAILED' $logs/mut_$m.log | sed 's/ - .*//' >> "$out"
    [ $rc -eq 0 ] && { echo "  !! mutant $m SURVIVED" | tee -a "$out"; bad=1; }
  done
  exit $bad ;;
baseline)   # the unmutated library alone (starts a fresh summary; the mutants then follow with MUT_ONLY=... run, one lease at a time)
  out=$ROOT/gpurun_out/mutation_check.txt
  cd "$ROOT"
  python -m pytest $TESTS -q > gpurun_out/mut_baseline.log 2>&1; rc=$?
  echo "unmutated library: pytest rc=$rc ($(tail -1 gpurun_out/mut_baseline.log))" | tee "$out"
  exit $rc ;;
*) echo "usage: $0 patterns|build|baseline|run" >&2; exit 2 ;;
esac
