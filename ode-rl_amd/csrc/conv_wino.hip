// conv_wino.hip -- 3x3 convolution on 16x16 maps by Winograd F(2x2, 3x3) on exact-fp32 MFMA (gfx950).
//
// Same contract as conv3x3_resident_kernel (conv_q4.hip) -- one nn.Conv2d(cin, cout, 3, 1, 1) of the dynamics f
// (/root/reference/helpers/utils.py:167-177) with the fused epilogues -- but 2.25x fewer multiplies:
//   Y = A^T [ sum_ci (G g G^T) .* (B^T d B) ] A     per 2x2 output tile, 4x4 input patch d, 3x3 filter g.
// The sum over ci for each of the 16 transform positions xi is a GEMM  M_xi[co][tile] = U_xi[co][ci] V_xi[ci][tile].
// The arithmetic is still fp32 throughout (reassociated, not reduced precision); rel-L2 vs direct fp32 conv ~1e-6.
//
// Workgroup = (sample, 32 output channels, 8 output rows = 4x8 tiles of 2x2), 512 threads, ROLE-SPECIALISED waves
// (two per SIMD: one of each role):
//   waves 0-3  CONSUMERS: wave w owns the (16 co x 16 tiles) block (w>>1, w&1) for ALL 16 xi -- 16 accumulators of
//              v_mfma_f32_16x16x4_f32 (64 AGPRs).  Per 16-channel chunk 64 MFMAs, fed by 16 ds_read_b128 (the V fragments) and
//              16 buffer_load_dwordx4 (the U fragments).  The pre-transformed weights U are a packed constant that nothing in
//              the CU produces: a lane's A operand of position xi is 16 contiguous bytes of the packed tensor, so it goes from
//              L2 / the vector L1 straight into VGPRs, kUAhead positions ahead of the MFMAs that use it, across chunk
//              boundaries, and never through LDS; a layer's first kUAhead positions are requested on entry, in front of the
//              first barrier (in a walk: while the producers still wait for the partners).  (The two waves with the same
//              w>>1 load the same addresses.)  Because a lane ends up holding M_xi[4 consecutive co][its tile]
//              for every xi, the output transform A^T M A is register-only and its result is exactly one Q4 channel quad per
//              pixel: no LDS exchange.
//   waves 4-7  PRODUCERS: LDS-DMA of the raw input tile two chunks ahead (4 quads x 10 rows x 18 cols, zero-PADDED BY THE
//              DMA: per-lane source offsets, out-of-image slots get an out-of-range offset and the buffer range check writes
//              zeros), then the input transform V = B^T d B of the next chunk (12 ds_read_b128 + 8 ds_write_b128 + float4 VALU
//              per thread).
// One s_barrier per chunk hands V_c to the consumers and the freed buffers back to the producers.
// LDS: raw[2] 32 KiB + V[2] 64 KiB = 96 KiB.
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "conv_common.h"

namespace odehip {

constexpr int kWU = 32 * 1024;        // U chunk in the packed tensor: 16 xi x [quad 4][co 32][4 ci] (never staged in LDS)
constexpr int kWRaw = 16 * 1024;      // raw chunk: 4 quads x 4 KiB: 10 rows x 20 slots of 16 B (18 padded cols, de-interleaved)
constexpr int kWV = 32 * 1024;        // V chunk: 16 xi x [quad 4][tile 32][4 ci]
constexpr int kWinoLds = 2 * kWRaw + 2 * kWV;  // 96 KiB
constexpr int kUAhead = 8;            // U fragments (positions xi) a consumer wave keeps in flight ahead of its MFMAs: a position is
                                      // 128 matrix cycles, so 8 cover ~1,000 cycles of L2-hit latency under load, in 32 VGPRs (kept
                                      // in flight from one layer into the next as well, the fixed-grid walk spills 68 VGPRs)

__device__ __forceinline__ f32x4 load_u(__amdgpu_buffer_rsrc_t r, int voffset, int soffset) {
  return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, voffset, soffset, 0));
}

// a - b on 4 floats as two v_pk_add_f32 with the negate modifier (hipcc emits four v_sub_f32 otherwise; every VALU
// cycle here is taken from the fp32 MFMAs of the consumer wave on the same SIMD)
__device__ __forceinline__ f32x4 pk_sub(f32x4 a, f32x4 b) {
  typedef float f32x2 __attribute__((ext_vector_type(2)));
  f32x2 lo, hi;
  const f32x2 alo = {a.x, a.y}, ahi = {a.z, a.w}, blo = {b.x, b.y}, bhi = {b.z, b.w};
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(lo) : "v"(alo), "v"(blo));
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(hi) : "v"(ahi), "v"(bhi));
  return f32x4{lo.x, lo.y, hi.x, hi.y};
}

// Hand-off between the rows of the trajectory walks (below): `done` is the sample's flag line, one word per consumer wave of its
// workgroups (16 words, or 64 on the sixteen-workgroup walk); a wave stores the number of rows it has finished (single writer per
// word: no read-modify-write anywhere).  A row's input is complete once the words of the workgroups that wrote it have reached
// `wait_target`.  The sixteen-workgroup walk names the fields it fills and leaves those of the four-workgroup layers (word0, stamps,
// split_wait) at the defaults below.
struct PersistHook {
  unsigned* done = nullptr;
  unsigned target = 0u;  // index of this row in the launch's walk (every launch gets a zeroed flag line)
  int word0 = 0;         // first of this workgroup's four words
  unsigned* abort_ = nullptr;    // device word: some wait of this launch has given up -- nobody waits any more
  unsigned* host_err = nullptr;  // mapped host word: a capped wait gave up (never expected; the kernel then finishes with wrong data)
  bool fence = false;    // the sample's workgroups are NOT on one XCD: agent-scope release / acquire around the hand-off
  float* nchw_base = nullptr;    // base of the NCHW result tensor (the table holds offsets into it, in `dbg`)
  unsigned long long* stamps = nullptr;  // diagnostic (odehip_set_debug_buffer): 8 x 100 MHz timestamps of this layer, or null
  int batch = 0;
  bool first = true;     // layer 0 of the launch: its input was complete before the launch
  bool solo = false;     // the group walks ONE sample: the producers have nothing to prepare while the consumers finish a layer
  bool announce = true;  // false: the first of a workgroup's two passes over a 128-channel layer -- its flags are stored after the second
  bool split_wait = false;  // the input chunks 0/1 and 2/3 come from the two co tiles of a 64 -> 64 layer: wait for them separately
  int sleep6 = 0;        // s_sleep(6) periods (0.18 us each) in front of the first poll (four workgroups: solo only)
  const unsigned long long* reloc = nullptr;  // adaptive walk: base addresses of the relocation classes (rel() below), or null
  unsigned wait_target = 0u;  // what the partners' flags must have reached before this row's input is loaded (target, or target - 1
                              // for a row that does not depend on the row in front of it: ConvArgs::dep_back)
};

// Relocatable pointers of the adaptive walk's tables.  A driver whose buffers are chosen ON THE DEVICE (the slot an adaptive
// solver's accepted step keeps, the state pointers that swap with FSAL) writes such a pointer as  class << 56 | byte offset  and a
// device-side controller keeps reloc[class] = the base address current for the next launch; the walk resolves the field when it
// reads the row (scalar arithmetic on uniform values).  Class 0 = an ordinary pointer.  User-space addresses have their top 16
// bits clear, so the tag cannot collide with one.
template <typename T>
__device__ __forceinline__ T* rel(const unsigned long long* reloc, T* p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned cls = (unsigned)(v >> 56);
  if (cls == 0) return p;
  typedef const __attribute__((address_space(4))) unsigned long long ConstU;
  return (T*)((v & 0x00ffffffffffffffull) + *((ConstU*)reloc + cls));
}
__device__ __forceinline__ void pstamp(const PersistHook& hk, int i, int lane) {
  if (hk.stamps && lane == 0) hk.stamps[i] = __builtin_amdgcn_s_memrealtime();
}

// a pointer the compiler must treat as wave-uniform (else every LDS-DMA on a descriptor built from it is wrapped in a
// waterfall loop: measured 125 ns per DMA instruction instead of a few clocks)
template <typename T>
__device__ __forceinline__ T* uniform_ptr(T* p) {
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return (T*)(((unsigned long long)hi << 32) | lo);
}

// The flag line of a sample: word (2 ct + rh) * 4 + consumer wave.  The input chunks 2 ct', 2 ct' + 1 of the next layer (32 channels)
// are exactly what the two workgroups with ct = ct' wrote: their loads only have to wait for THOSE eight words --
// (word & sel_mask) == sel_val; the default waits for all sixteen.
__device__ __forceinline__ void wait_done(const PersistHook& hk, int sel_mask = 0, int sel_val = 0) {
  int n = 0;
  const int lane = threadIdx.x & 63;
  const bool mine = lane < 16 && (lane & sel_mask) == sel_val;
  while (!__all(!mine || __hip_atomic_load(hk.done + (lane & 15), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= hk.wait_target)) {
    __builtin_amdgcn_s_sleep(1);
    if ((++n & 1023) == 0) {
      if (__hip_atomic_load(hk.abort_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1u) break;
      if (n > (1 << 23)) {  // seconds: partners lost -- report and stop ALL waiting rather than hang the device
        __hip_atomic_store(hk.abort_, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *hk.host_err = 3;
        break;
      }
    }
  }
  if (hk.fence) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// A wave announces its share of row hk.target: its stores are in L2 once they are acknowledged; then -- behind an agent-scope release
// if the group spans XCDs -- it stores target + 1 into its own flag word (unless this is the first of two passes over the layer:
// !hk.announce).  stamp: the diagnostic timestamp 7 is taken between the two.  The four-workgroup elementwise row (ew_row) keeps the
// sequence written out: through this function the adaptive walk spills two more scalar registers than its ceiling allows.
__device__ __forceinline__ void announce(const PersistHook& hk, unsigned* done_word, bool stamp = false) {
  const int lane = threadIdx.x & 63;
  wait_vmcnt<0>();
  if (stamp) pstamp(hk, 7, lane);
  if (hk.fence) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  if (lane == 0 && hk.announce) __hip_atomic_store(done_word, hk.target + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Prologue of a walk, part 1: the GROUP workgroups of a sample (logical ids lid & ~(GROUP - 1) ...) publish the XCD they really run
// on (XCC_ID + 1; the words are zero on entry) and read each other's; returns the uniform `fence` flag: true if they differ, so the
// hand-off needs agent-scope fences.  The wait is capped: a partner that never arrives sets the abort word and the host word.
template <int GROUP>
__device__ __forceinline__ bool xcc_rendezvous(unsigned* xcc_of, int lid, unsigned* abort_word, unsigned* host_err) {
  const unsigned my_xcc = (__builtin_amdgcn_s_getreg((3 << 11) | 20) & 15u) + 1u;  // HW_REG_XCC_ID[3:0]
  if (threadIdx.x == 0) __hip_atomic_store(xcc_of + lid, my_xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  bool fence = false;
  for (int p = 0; p < GROUP; ++p) {
    unsigned v = 0;
    int n = 0;
    while ((v = __hip_atomic_load(xcc_of + (lid & ~(GROUP - 1)) + p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0) {
      __builtin_amdgcn_s_sleep(2);
      if (++n > (1 << 23)) {
        __hip_atomic_store(abort_word, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *host_err = 2;
        break;
      }
    }
    fence |= (v != my_xcc);
  }
  return __builtin_amdgcn_readfirstlane(fence);
}

// Prologue of a walk, part 2 (all of it uniform and constant during the launch): false = nothing to walk -- an adaptive solver that
// finished while this launch was queued (table[0].skip), or a device-side controller that lost its way.  section: null, or the
// device-steered {first row, number of rows} of this launch's walk; table and n_layers then become that section.
__device__ __forceinline__ bool walk_start(const ConvArgs*& table, int& n_layers, const int* section) {
  typedef const __attribute__((address_space(4))) int ConstI;
  const int* skip = table[0].skip;
  if (skip && *(ConstI*)skip) return false;
  if (section) {
    const int row0 = ((ConstI*)section)[0], n_dev = ((ConstI*)section)[1];
    if (row0 < 0 || n_dev <= 0 || row0 + n_dev > n_layers) return false;
    table += row0;
    n_layers = n_dev;
  }
  return true;
}

// The row cursor of a walk.  The table is constant for the whole launch and is read in place (a private copy would live in scratch):
// through address space 4 its fields are fetched with SCALAR loads (as a plain global pointer they become vector loads, each followed
// by vmcnt(0), because the kernel also stores to global memory).  A row that is first touched when it is needed costs a trip to HBM on
// the critical path of every layer, so the next row is pulled into L2 a layer ahead and the producers' two pointers (src, u) are
// fetched a layer ahead.  (The wide walk reads src and u from the current row and keeps its own loop: through this cursor it needs
// 254 VGPRs and scratch.)
struct RowCursor {
  const ConvArgs* table;
  int n_layers;
  const float *src, *u, *src_next, *u_next;
  __device__ __forceinline__ RowCursor(const ConvArgs* t, int n)
      : table(t), n_layers(n), src(t[0].src1), u(t[0].w_wino), src_next(nullptr), u_next(nullptr) {}
  __device__ __forceinline__ const ConvArgs& row(int l) {
    typedef const __attribute__((address_space(4))) ConvArgs ConstArgs;
    const ConvArgs& a = *(const ConvArgs*)((ConstArgs*)table + l);
    src_next = src;
    u_next = u;
    if (l + 1 < n_layers) {
      src_next = table[l + 1].src1;
      u_next = table[l + 1].w_wino;
      if (threadIdx.x < (sizeof(ConvArgs) + 63) / 64) {
        const unsigned v = __builtin_nontemporal_load((const unsigned*)&table[l + 1] + threadIdx.x * 16);
        asm volatile("" ::"v"(v));
      }
    }
    return a;
  }
  __device__ __forceinline__ void next() {
    src = src_next;
    u = u_next;
  }
};

// The epilogue of a fixed-grid walk's layer (PERSIST without ADAPT) on operands fetched at the START of the layer: every scalar the
// epilogue needs AND this lane's own operands of the stage combine (y, earlier k's: written by this very lane at least one layer ago)
// are fetched behind the wait for the first chunk -- after the last MFMA there is only arithmetic and stores left.  (Read from the
// table at that point they cost a scalar-cache miss each, one after the other.)  A lane owns channel quad Q of one 2x2 output tile:
// quad q of the four is pixel (row0 + (q >> 1), 2 otx + (q & 1)).  Shared by wino_layer and wino_strip_layer, which differ only in which
// (Q, tile) a lane owns: emit_quad's plain / stage-combine arithmetic, same expressions, same order.
template <int QOUT>
struct PreEpilogue {
  int combine = 0, act = 0, np = 0;
  float* dst = nullptr;
  float* kout = nullptr;
  float* out1 = nullptr;
  float* out2 = nullptr;
  float* nchw = nullptr;
  bool y = false;
  float h = 1.0f, ks = 1.0f, c1c = 0.0f, c2c = 0.0f, c1[3] = {0.f, 0.f, 0.f}, c2[3] = {0.f, 0.f, 0.f};
  f32x4 yv[4], kv[3][4];

  __device__ __forceinline__ void fetch(const ConvArgs& a, const PersistHook& hk, int b, int Q, int row0, int otx) {
    combine = a.combine;
    act = a.act;
    dst = a.dst;
    // a table whose step size only exists on the device (dopri5: h_by_value == 0) takes the shared epilogue for its
    // stage-combine / reverse layers; ReLU-mask layers of such a table read *h_ptr here
    if (combine == 1 && !a.h_by_value) combine = 3;
    if (combine == 2) {  // ReLU-mask backward layer: dst = scale * acc * (mask > 0); the mask values are fetched now
      const BwdArgs& w = a.bwd;
      typedef const __attribute__((address_space(4))) float ConstF;
      const float hb = a.h_by_value ? a.cmb.atol : (w.h_ptr ? *(ConstF*)w.h_ptr : 0.0f);  // constant during the launch
      ks = w.sc_c + w.sc_h * hb;
      y = w.mask_src != nullptr;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const size_t off = (((size_t)b * QOUT + Q) * kPix + (row0 + (q >> 1)) * 16 + 2 * otx + (q & 1)) * 4;
        if (y) yv[q] = *(const f32x4*)(w.mask_src + off);
      }
    } else if (combine == 1) {
      const CombineArgs& m = a.cmb;
      np = m.n_prev;
      h = m.atol;  // the step size itself: the host resolves *h_ptr into this (otherwise unused) field of a persistent table
      ks = m.k_scale;
      c1c = m.c1[np];
      c2c = m.c2[np];
      kout = m.k_out;
      out1 = m.out1;
      out2 = m.out2;
      nchw = a.dbg ? hk.nchw_base + ((size_t)a.dbg - 1) : nullptr;
      y = m.y != nullptr;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const size_t off = (((size_t)b * QOUT + Q) * kPix + (row0 + (q >> 1)) * 16 + 2 * otx + (q & 1)) * 4;
        if (y) yv[q] = *(const f32x4*)(m.y + off);
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < np) kv[j][q] = *(const f32x4*)(m.k_prev[j] + off);
      }
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        c1[j] = m.c1[j];
        c2[j] = m.c2[j];
      }
    }
  }

  // quad q of the lane's four, pixel P, conv output v (bias included)
  __device__ __forceinline__ void emit(const ConvArgs& a, int b, int Q, int q, int P, f32x4 v, float& esum) const {
    const size_t off = (((size_t)b * QOUT + Q) * kPix + P) * 4;
    if (!combine) {
      *(f32x4*)(dst + off) = act_fwd(v, act);
      return;
    }
    if (combine == 2) {
      v *= ks;
      if (y) v = act_bwd(v, yv[q], act);
      *(f32x4*)(dst + off) = v;
      return;
    }
    if (combine == 3) {  // reverse-sweep targets: the shared epilogue, read from the table
      emit_quad<false>(a, b, Q, P, v, esum);
      return;
    }
    const f32x4 kc = act_fwd(v, act) * ks;   // (a Tanh head before the sign)
    if (kout) *(f32x4*)(kout + off) = kc;
    if (y) {
      // a stage writes EITHER the next stage input (out1) OR the step result (out2, + its NCHW frame): only the sum that is stored is
      // formed (the same expression as before for each)
      if (out1) {
        f32x4 sa = kc * c1c;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < np) sa += kv[j][q] * c1[j];
        *(f32x4*)(out1 + off) = yv[q] + sa * h;
      }
      if (out2 || nchw) {
        f32x4 sb = kc * c2c;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < np) sb += kv[j][q] * c2[j];
        const f32x4 o2 = yv[q] + sb * h;
        if (out2) *(f32x4*)(out2 + off) = o2;
        if (nchw) {
          float* o = nchw + ((size_t)b * (QOUT * 4) + Q * 4) * kPix + P;
          o[0] = o2.x; o[kPix] = o2.y; o[2 * kPix] = o2.z; o[3 * kPix] = o2.w;
        }
      }
    }
  }
};

// One chunk (16 input channels, all 16 positions xi) of a consumer wave's (16 co x 16 tiles) block, shared by wino_layer and
// wino_strip_layer: v = this lane's fragment of position 0 in the chunk's V buffer (positions VSTRIDE bytes apart).  Two xi at a time:
// consecutive MFMAs hit different accumulators (a dependent 16x16x4 issues 8 cycles late); the V fragments of the next pair are read,
// and the U fragments kUAhead positions on requested, while this pair's 8 MFMAs run.  U ring: slot g % kUAhead holds position g of the
// layer (g = 16 c + xi); the caller requests the first kUAhead on entry.  no_u: the ablations without memory traffic keep their constants.
template <int VSTRIDE, int NCHUNK>
__device__ __forceinline__ void chunk_mma(const char* v, int c, __amdgpu_buffer_rsrc_t ru, int u_off, f32x4 (&uw)[kUAhead],
                                          f32x4 (&acc)[16], bool no_u) {
  static_assert(kUAhead % 2 == 0 && kUAhead <= 16, "the U ring is refilled a pair of positions at a time");
  constexpr int kG = 16 * NCHUNK;
  f32x4 x0 = *(const f32x4*)(v), x1 = *(const f32x4*)(v + VSTRIDE);
  f32x4 x0n, x1n;
#pragma unroll
  for (int x = 0; x < 16; x += 2) {
    const int g = c * 16 + x, s0 = g % kUAhead, s1 = (g + 1) % kUAhead;
    const f32x4 w0 = uw[s0], w1 = uw[s1];
    if (x + 2 < 16) {
      x0n = *(const f32x4*)(v + (x + 2) * VSTRIDE);
      x1n = *(const f32x4*)(v + (x + 3) * VSTRIDE);
    }
    if (g + kUAhead < kG && !no_u) {
      uw[s0] = load_u(ru, u_off, (g + kUAhead) * 2048);
      uw[s1] = load_u(ru, u_off, (g + kUAhead + 1) * 2048);
    }
    acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.x, x0.x, acc[x], 0, 0, 0);
    acc[x + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.x, x1.x, acc[x + 1], 0, 0, 0);
    acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.y, x0.y, acc[x], 0, 0, 0);
    acc[x + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.y, x1.y, acc[x + 1], 0, 0, 0);
    acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.z, x0.z, acc[x], 0, 0, 0);
    acc[x + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.z, x1.z, acc[x + 1], 0, 0, 0);
    acc[x] = __builtin_amdgcn_mfma_f32_16x16x4f32(w0.w, x0.w, acc[x], 0, 0, 0);
    acc[x + 1] = __builtin_amdgcn_mfma_f32_16x16x4f32(w1.w, x1.w, acc[x + 1], 0, 0, 0);
    x0 = x0n; x1 = x1n;
    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
    __builtin_amdgcn_sched_group_barrier(0x100, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x020, 2, 0);
    __builtin_amdgcn_sched_group_barrier(0x008, 7, 0);
    __builtin_amdgcn_sched_barrier(0);
  }
}

// The output transform A^T M A in registers: the lane holds M_xi[its co quad][its tile] for all 16 xi (acc[4 row + col]); y[q] is the
// conv output (bias included) of quad q of its 2x2 tile, pixel (q >> 1, q & 1).
__device__ __forceinline__ void out_transform(const f32x4 (&acc)[16], f32x4 bias4, f32x4 (&y)[4]) {
  f32x4 S[2][4];
#pragma unroll
  for (int cI = 0; cI < 4; ++cI) {
    S[0][cI] = acc[0 * 4 + cI] + acc[1 * 4 + cI] + acc[2 * 4 + cI];
    S[1][cI] = pk_sub(pk_sub(acc[1 * 4 + cI], acc[2 * 4 + cI]), acc[3 * 4 + cI]);
  }
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    y[2 * i] = S[i][0] + S[i][1] + S[i][2] + bias4;
    y[2 * i + 1] = pk_sub(pk_sub(S[i][1] + bias4, S[i][2]), S[i][3]);
  }
}

// One 3x3 layer for workgroup (sample b, 32-channel tile ct, image half rh).  PERSIST: called in a loop by
// wino_persist_kernel -- the input tile is loaded past the per-CU cache (sc0 sc1: it was written by other CUs of this launch),
// the first weight chunk is requested BEFORE waiting for the partners, and finished output is announced through hk.done.
// QOUT: output channel quads of the layer as the PERSIST epilogue's prefetched operands are addressed (16 = 64 channels; the
// per-launch kernel goes through emit_quad, which reads a.qout)
// ADAPT (with PERSIST): the walk of the adaptive solver's tables (wino_persist_d_kernel) -- every epilogue's operands are reduced at
// the START of the layer to at most four quads per output pixel (a stage combine of any depth becomes y, the two partial sums over
// the earlier stages and y1; reverse-sweep targets up to two (srcA, srcB) pairs), the step size may live on the device.
template <int NCHUNK, bool DBG, bool PERSIST, int QOUT = 16, bool ADAPT = false>
__device__ __forceinline__ void wino_layer(const float* __restrict__ p_src, const float* __restrict__ p_u, int p_qin, const ConvArgs& a,
                                           int b, int ct, int rh, char* smem, const PersistHook& hk) {
  static_assert(!PERSIST || (NCHUNK % 2 == 0), "the layer-to-layer LDS hand-over assumes an even chunk count");
  constexpr int kRawAux = PERSIST ? 16 : 0;  // sc1 (agent scope): never served from this CU's vector cache
  char* const Rb = smem;
  char* const Vb = smem + 2 * kWRaw;
  Stamps st(a, (DBG && (a.debug & 16)) ? 256 : (DBG ? 0 : -1));  // debug 16: stamps from a producer wave instead of a consumer
  st.take(0);
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r0 = rh * 8;
  constexpr int nchunk = NCHUNK;
  const bool skip = !PERSIST && a.skip && *a.skip;  // adaptive solver finished while this launch was queued (uniform)
  const bool dbg_noprod = DBG && (a.debug & 1), dbg_nomfma = DBG && (a.debug & 2), dbg_notr = DBG && (a.debug & 32),
             dbg_nodma = DBG && (a.debug & 128);  // diagnostic ablations (tools/conv_microbench.py)

  if (wave >= 4) {
    // =========================================== PRODUCERS ===========================================
    const int pw = wave - 4, ptid = tid - 256;
    const __amdgpu_buffer_rsrc_t rx = make_rsrc((const char*)p_src + (size_t)b * p_qin * kQuadBytes, (unsigned)p_qin * kQuadBytes);
    // Raw tile in LDS: row r (image row r0 - 1 + r) = 20 slots of 16 B: [even padded cols 0,2,..,16 | odd padded cols
    // 1,3,..,17 | 2 unused]; padded col pc = image col + 1.  A 4x4 patch reads cols 2tx + j: for a fixed j the 8 tiles of a
    // row hit CONSECUTIVE slots, and the 20-slot row stride puts the 4 tile rows of a ds_read_b128 lane group in
    // different bank quarters: conflict-free (a plain [row][18 cols] layout is 4-way conflicted on these stride-2 reads).
    int vr[4];
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int s = 64 * p + lane;
      const int row = s / 20, w = s - row * 20;
      const int pc = w < 9 ? 2 * w : 2 * (w - 9) + 1;
      const int irow = r0 - 1 + row, col = pc - 1;
      vr[p] = (s < 200 && w < 18 && irow >= 0 && irow < kHW && col >= 0 && col < kHW) ? irow * 256 + col * 16 : kOobOffset;
    }
    auto issue_raw = [&](int c, int buf) {
#pragma unroll
      for (int p = 0; p < 4; ++p)
        __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, ODEHIP_LDS_PTR(Rb + buf * kWRaw + (pw * 4 + p) * 1024), 16, vr[p],
                                                 (c * 4 + pw) * kQuadBytes, 0, kRawAux);
    };
    // input transform task: (half th, quad tq, tile tt) -> V rows 2*th, 2*th+1 of B^T d B.  Each producer wave
    // transforms the quad it DMA'd itself (tq = pw), so raw data needs no cross-wave hand-off: its own vmcnt suffices.
    const int th = lane >> 5, tq = pw, tt = lane & 31;
    (void)ptid;
    const int tty = tt >> 3, ttx = tt & 7;
    // Patch rows p0..p3 (LDS rows 2ty..2ty+3).  B^T d:  T0 = p0 - p2, T1 = p1 + p2, T2 = p2 - p1, T3' = p3 - p1 (= -T3; the
    // sign is folded into the packed U rows of xi = 12..15).  Half 0 loads (p2, p0, p1), half 1 loads (p1, p2, p3): both
    // halves then compute  Ta = d1 - d0,  Tb = d2 + sgn*d0  with sgn = +1 / -1 -- no per-lane selects in the VALU stream.
    const int r_a = th == 0 ? 2 : 1, r_b = th == 0 ? 0 : 2, r_c = th == 0 ? 1 : 3;
    const int raw_base = tq * 4096 + (2 * tty * 20 + ttx) * 16;  // + (j&1)*9*16 + (j>>1)*16 per patch column j
    const int off_a = raw_base + r_a * 320, off_b = raw_base + r_b * 320, off_c = raw_base + r_c * 320;
    const float sgn = th == 0 ? 1.0f : -1.0f;
    const int v_off = tq * 512 + tt * 16;                                  // + xi * 2048
    auto transform = [&](int rbuf, int vbuf) {
      const char* r = Rb + rbuf * kWRaw;
      f32x4 d0[4], d1[4], d2[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (DBG && (a.debug & 512)) {
          d0[j] = d1[j] = d2[j] = f32x4{1.f, 2.f, 3.f, (float)j};
        } else {
          const int cj = ((j & 1) * 9 + (j >> 1)) * 16;
          d0[j] = *(const f32x4*)(r + off_a + cj);
          d1[j] = *(const f32x4*)(r + off_b + cj);
          d2[j] = *(const f32x4*)(r + off_c + cj);
        }
      }
      f32x4 T[2][4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        T[0][j] = pk_sub(d1[j], d0[j]);
        T[1][j] = d2[j] + d0[j] * sgn;
      }
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        char* v = Vb + vbuf * kWV + v_off + (2 * th + i) * 4 * 2048;
        if (DBG && (a.debug & 256)) {
          const f32x4 sum = (T[i][0] - T[i][2]) + (T[i][1] + T[i][2]) + (T[i][2] - T[i][1]) + (T[i][1] - T[i][3]);
          asm volatile("" ::"v"(sum.x), "v"(sum.y), "v"(sum.z), "v"(sum.w));
        } else {
          *(f32x4*)(v + 0 * 2048) = pk_sub(T[i][0], T[i][2]);
          *(f32x4*)(v + 1 * 2048) = T[i][1] + T[i][2];
          *(f32x4*)(v + 2 * 2048) = pk_sub(T[i][2], T[i][1]);
          *(f32x4*)(v + 3 * 2048) = pk_sub(T[i][1], T[i][3]);
        }
      }
    };

    // DMA issue order per wave: raw_0 (4) | raw_1 (4) | then per iteration c: raw_{c+2} (4).
    // Counted waits (vmcnt counts this wave's DMAs in issue order) leave the younger ones in flight.
    if (PERSIST) {
      if (pw == 0) pstamp(hk, 0, lane);
      // chunks 0 and 1 are the channels of co tile 0: only ITS two workgroups must be done before they are loaded; co tile 1's are
      // waited for in front of chunk 2 (same-box A/B over 10 alternations: median 1.4152 -> 1.4076 ms per trajectory; a wait per
      // chunk -- four polls per layer -- costs more than it saves: 1.53 ms)
      if (!hk.first) {
        // One sample per group: the partners cannot be done before this workgroup's own consumers are through their last chunk (~1 us
        // from here): sleep through most of it instead of polling -- a polling wave takes issue slots from the consumer wave of its
        // SIMD.  Sweep on one box (PersistArgs::sleep6 = periods of 0.18 us; median of 3 alternations, ms): headline 0: 1.432,
        // 2: 1.504, 3: 1.435, 4: 1.401, 5: 1.389, 6: 1.409, 8: 1.452; forward + backward 0: 4.75, 4: 4.57, 5: 4.55, 6: 4.54, 8: 4.60;
        // dopri5 forward 0: 0.799, 4: 0.783, 5: 0.777, 8: 0.796; 128-channel-ended stack 0: 1.640, 4: 1.627, 5: 1.638.  A barrier that
        // releases the producers exactly when the consumers' last MFMA has issued is worse than the fixed sleep (it also holds back
        // the next layer's start).
        if (hk.solo && hk.wait_target == hk.target)   // (a row with a relaxed dependency has nothing to sleep for)
          for (int i = 0; i < hk.sleep6; ++i) __builtin_amdgcn_s_sleep(6);
        if (hk.split_wait) wait_done(hk, 0x8, 0x0); else wait_done(hk);
      }
      if (pw == 0) pstamp(hk, 1, lane);
      issue_raw(0, 0);
      issue_raw(1, 1);
      wait_vmcnt<4>();                 // raw_0 landed (raw_1 still in flight)
      if (pw == 0) pstamp(hk, 2, lane);
      transform(0, 0);
      if (pw == 0) pstamp(hk, 3, lane);
    } else if (!skip && !dbg_noprod) {
      issue_raw(0, 0);
      if (nchunk > 1) issue_raw(1, 1);
      if (nchunk > 1) wait_vmcnt<4>(); else wait_vmcnt<0>();   // raw_0 landed (raw_1 still in flight)
      transform(0, 0);
    }
    st.take(2);
#pragma unroll
    for (int c = 0; c < nchunk; ++c) {
      __builtin_amdgcn_s_barrier();  // [c] V_c ready for the consumers; they are done with chunk c-1
      if (!skip && !dbg_noprod && c + 1 < nchunk) {
        if (c + 2 < nchunk) {
          if (PERSIST && c == 0 && !hk.first && hk.split_wait) wait_done(hk, 0x8, 0x8);   // chunks 2 and 3: co tile 1's workgroups
          if (!dbg_nodma) issue_raw(c + 2, c & 1);        // raw buffer consumed by this wave's transform of chunk c
          wait_vmcnt<4>();                                // raw_{c+1} landed (raw_{c+2} still in flight)
        } else {
          wait_vmcnt<0>();                                // raw_{c+1}, the last one
        }
        if (!dbg_notr) transform((c + 1) & 1, (c + 1) & 1);  // V buffer last read by the MFMAs of chunk c-1
      }
      if (c < 4) st.take(3 + c);
    }
    st.flush(a);
    return;
  }

  // ============================================= CONSUMERS =============================================
  const int ch = wave >> 1, thh = wave & 1;
  const int i16 = lane & 15, kq = lane >> 4;
  f32x4 acc[16];
#pragma unroll
  for (int x = 0; x < 16; ++x) acc[x] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int u_off = kq * 512 + (ch * 16 + i16) * 16;  // this lane's 16 bytes of a position's 2 KiB block [quad 4][co 32][4 ci]
  const int v_off = kq * 512 + (thh * 16 + i16) * 16;
  // the U ring's first positions (chunk_mma): buffer loads, the range check keeps every address inside this tile
  const bool dbg_nou = dbg_noprod || dbg_nodma;     // the ablations without memory traffic: U fragments are constants
  const __amdgpu_buffer_rsrc_t ru = make_rsrc((const char*)p_u + (size_t)ct * (NCHUNK * kWU), (unsigned)NCHUNK * kWU);
  f32x4 uw[kUAhead];
#pragma unroll
  for (int g = 0; g < kUAhead; ++g) {
    if (skip || dbg_nou) uw[g] = f32x4{1.f, 1.f, 1.f, 1.f};
    else uw[g] = load_u(ru, u_off, g * 2048);
  }
  const int Q = ct * 8 + ch * 4 + kq;
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (a.bias) bias4 = *(const f32x4*)(a.bias + Q * 4);  // loaded now, used after the last MFMA
  // PERSIST: the epilogue's scalars and this lane's own operands are fetched now, behind the wait for the first chunk (PreEpilogue)
  const int tile = thh * 16 + i16, oty = tile >> 3, otx = tile & 7;
  PreEpilogue<QOUT> ep;
  // ---- ADAPT: the reduced operand set (see the template comment)
  int d_kind = 0;   // 0 plain / ReLU store; 1 stage combine (order 1); 2 ReLU-mask backward; 3 reverse-sweep targets (<= 2, constant
                    // coefficients) held in registers; 5 anything else: the shared epilogue reads the table after the matrix work
  f32x4 d_y[4], d_y1[4], d_sa[4], d_sb[4];
  float d_h = 1.0f, d_ks = 1.0f, d_cA = 0.0f, d_cB = 0.0f, d_rtol = 0.0f, d_atol = 0.0f, d_t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float* d_o[4] = {nullptr, nullptr, nullptr, nullptr};   // kind 1: k_out, out1, out2, nchw frame; kind 3: target outputs 0, 1
  bool d_has_y = false, d_err = false, d_f[4] = {false, false, false, false};
  if constexpr (ADAPT) {
    typedef const __attribute__((address_space(4))) float ConstF;
    const unsigned long long* const rl = hk.reloc;   // relocatable pointers (rel()): every pointer of the reduced paths below is
                                                     // resolved here; rows that fall to the shared epilogue (kind 5) must not carry any
    ep.act = a.act;
    ep.dst = rel(rl, a.dst);
    d_kind = a.combine == 0 ? 0 : 5;
    if (a.combine == 2) {
      const BwdArgs& w = a.bwd;
      const float hb = a.h_by_value ? a.cmb.atol : (w.h_ptr ? *(ConstF*)w.h_ptr : 0.0f);
      d_ks = w.sc_c + w.sc_h * hb;
      d_has_y = w.mask_src != nullptr;
      d_kind = 2;
      const float* const mask = rel(rl, w.mask_src);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const size_t off = (((size_t)b * QOUT + Q) * kPix + (r0 + 2 * oty + (q >> 1)) * 16 + 2 * otx + (q & 1)) * 4;
        if (d_has_y) d_y[q] = *(const f32x4*)(mask + off);
      }
    } else if (a.combine == 3 && a.bwd.n_targets <= 2 && !a.bwd.h_ptr) {
      const BwdArgs& w = a.bwd;
      d_kind = 3;
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        if (t < w.n_targets) {
          const BwdTarget& T = w.tgt[t];
          d_o[t] = rel(rl, T.out);
          d_t[3 * t] = T.g_c; d_t[3 * t + 1] = T.a_c; d_t[3 * t + 2] = T.b_c;
          d_f[2 * t] = T.srcA != nullptr; d_f[2 * t + 1] = T.srcB != nullptr;
          const float* const sA = rel(rl, T.srcA);
          const float* const sB = rel(rl, T.srcB);
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const size_t off = (((size_t)b * QOUT + Q) * kPix + (r0 + 2 * oty + (q >> 1)) * 16 + 2 * otx + (q & 1)) * 4;
            if (t == 0) {
              if (d_f[0]) d_y[q] = *(const f32x4*)(sA + off);
              if (d_f[1]) d_y1[q] = *(const f32x4*)(sB + off);
            } else {
              if (d_f[2]) d_sa[q] = *(const f32x4*)(sA + off);
              if (d_f[3]) d_sb[q] = *(const f32x4*)(sB + off);
            }
          }
        }
      }
    } else if (a.combine == 1 && (a.cmb.order == 1 || !a.cmb.y) && !(a.cmb.err_partials && (a.cmb.out2 || a.cmb.out2_nchw || a.dbg))) {
      const CombineArgs& m = a.cmb;
      d_kind = 1;
      const int np = m.n_prev;
      d_h = a.h_by_value ? m.atol : (m.h_ptr ? *(ConstF*)m.h_ptr : 1.0f);
      d_ks = m.k_scale;
      d_err = m.err_partials != nullptr;
      d_has_y = m.y != nullptr;
      d_cA = m.c1[np];
      d_cB = d_err ? m.ce[np] : m.c2[np];
      d_rtol = m.rtol; d_atol = m.atol;
      d_o[0] = rel(rl, m.k_out); d_o[1] = rel(rl, m.out1); d_o[2] = rel(rl, m.out2);
      d_o[3] = a.dbg ? hk.nchw_base + ((size_t)a.dbg - 1) : m.out2_nchw;
      const bool needB = d_err || d_o[2] || d_o[3];
      const float* const yp = rel(rl, m.y);
      const float* const y1p = rel(rl, m.err_y1);
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        d_sa[q] = d_sb[q] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (d_has_y) {
          const size_t off = (((size_t)b * QOUT + Q) * kPix + (r0 + 2 * oty + (q >> 1)) * 16 + 2 * otx + (q & 1)) * 4;
          d_y[q] = *(const f32x4*)(yp + off);
          if (d_err) d_y1[q] = *(const f32x4*)(y1p + off);
        }
      }
      if (d_has_y) {
        // the sums over the earlier stages, in the order of combine1_prev (conv_common.h).  Fully unrolled with the operands of all
        // stages fetched up front: as a run-time loop every iteration waited for its own scalar loads (pointer, relocation base,
        // coefficients) and then for its vector loads -- ~1.2 us per earlier stage in front of the layer's first barrier
        // (tools/adjoint_stamps.py: the consumers of a stage-7 layer arrived 2.9 us after their producers were ready)
        const float* kp[ODEHIP_MAX_STAGES - 1];
        float cA[ODEHIP_MAX_STAGES - 1], cB[ODEHIP_MAX_STAGES - 1];
#pragma unroll
        for (int j = 0; j < ODEHIP_MAX_STAGES - 1; ++j) {
          kp[j] = j < np ? rel(rl, m.k_prev[j]) : nullptr;
          cA[j] = m.c1[j];
          cB[j] = d_err ? m.ce[j] : m.c2[j];
        }
#pragma unroll
        for (int j = 0; j < ODEHIP_MAX_STAGES - 1; ++j) {
          if (j < np) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              const size_t off = (((size_t)b * QOUT + Q) * kPix + (r0 + 2 * oty + (q >> 1)) * 16 + 2 * otx + (q & 1)) * 4;
              const f32x4 kv = *(const f32x4*)(kp[j] + off);
              d_sa[q] = fma4(kv, cA[j], d_sa[q]);
              if (needB) d_sb[q] = fma4(kv, cB[j], d_sb[q]);
            }
          }
        }
      }
    }
  } else if (PERSIST) {
    ep.fetch(a, hk, b, Q, r0 + 2 * oty, otx);
  }
  st.take(2);
#pragma unroll
  for (int c = 0; c < nchunk; ++c) {
    __builtin_amdgcn_s_barrier();  // [c]
    if (PERSIST && c == 0 && wave == 0) pstamp(hk, 4, lane);
    if (!skip && !dbg_nomfma) chunk_mma<2048, NCHUNK>(Vb + (c & 1) * kWV + v_off, c, ru, u_off, uw, acc, dbg_nou);
    if (st.on && c < 4) {
      asm volatile("" ::"v"(acc[15][0]));
      st.take(3 + c);
    }
  }
  if (skip) return;
  if (PERSIST && wave == 0) pstamp(hk, 5, lane);

  float esum = 0.0f;
  // ADAPT: the same arithmetic as emit_quad's (order 1 for stage combines), on the operands reduced at the start of the layer
  auto emit_adapt = [&](int q, int P, f32x4 v) {
    const size_t off = (((size_t)b * QOUT + Q) * kPix + P) * 4;
    if (d_kind == 0) {
      *(f32x4*)(ep.dst + off) = act_fwd(v, ep.act);
    } else if (d_kind == 2) {
      v *= d_ks;
      if (d_has_y) v = act_bwd(v, d_y[q], ep.act);
      *(f32x4*)(ep.dst + off) = v;
    } else if (d_kind == 1) {
      const f32x4 kc = act_fwd(v, ep.act) * d_ks;   // (a Tanh head before the sign)
      if (d_o[0]) *(f32x4*)(d_o[0] + off) = kc;
      if (d_has_y) {
        if (d_o[1]) *(f32x4*)(d_o[1] + off) = fma4(fma4(kc, d_cA, d_sa[q]), d_h, d_y[q]);
        if (d_err) {
          esum = combine1_err(fma4(kc, d_cB, d_sb[q]), d_h, d_y[q], d_y1[q], d_rtol, d_atol, esum);
        } else if (d_o[2] || d_o[3]) {
          const f32x4 o2 = fma4(fma4(kc, d_cB, d_sb[q]), d_h, d_y[q]);
          if (d_o[2]) *(f32x4*)(d_o[2] + off) = o2;
          if (d_o[3]) {
            float* o = d_o[3] + ((size_t)b * (QOUT * 4) + Q * 4) * kPix + P;
            o[0] = o2.x; o[kPix] = o2.y; o[2 * kPix] = o2.z; o[3 * kPix] = o2.w;
          }
        }
      }
    } else if (d_kind == 3) {
      if (d_o[0]) {
        f32x4 o = v * d_t[0];
        if (d_f[0]) o = fma4(d_y[q], d_t[1], o);
        if (d_f[1]) o = fma4(d_y1[q], d_t[2], o);
        *(f32x4*)(d_o[0] + off) = o;
      }
      if (d_o[1]) {
        f32x4 o = v * d_t[3];
        if (d_f[2]) o = fma4(d_sa[q], d_t[4], o);
        if (d_f[3]) o = fma4(d_sb[q], d_t[5], o);
        *(f32x4*)(d_o[1] + off) = o;
      }
    } else {
      emit_quad(a, b, Q, P, v, esum, a.dbg ? hk.nchw_base + ((size_t)a.dbg - 1) : nullptr);
    }
  };
  f32x4 y[4];   // lane (tile i16 of half thh, row group kq): its 2x2 tile
  out_transform(acc, bias4, y);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int P = (r0 + 2 * oty + (q >> 1)) * 16 + 2 * otx + (q & 1);
    if constexpr (ADAPT) emit_adapt(q, P, y[q]);
    else if (PERSIST) ep.emit(a, b, Q, q, P, y[q], esum);
    else emit_quad(a, b, Q, P, y[q], esum);
  }
  if (PERSIST) {
    if (a.combine == 1 && a.cmb.err_partials) {
      // adaptive error norm: this wave's partial goes to the slot the per-layer launch (grid (4, batch), XCD-remapped ids) would
      // have used for workgroup (b, ct, rh), so the controller adds the same numbers in the same order
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) esum += __shfl_xor(esum, o, 64);
      const int nwg_pl = (QOUT / 4) * hk.batch, lid_pl = b * (QOUT / 4) + ct * 2 + rh;  // per-layer grid: (2 co tiles' worth of halves x QOUT / 8, batch)
      const int bid_pl = (nwg_pl & 7) == 0 ? (lid_pl % (nwg_pl >> 3)) * 8 + lid_pl / (nwg_pl >> 3) : lid_pl;
      if (lane == 0) a.cmb.err_partials[bid_pl * 4 + wave] = esum;
    }
    // this wave's share of the layer is in L2 once its stores are acknowledged; then it counts itself in
    if (wave == 0) pstamp(hk, 6, lane);
    announce(hk, hk.done + hk.word0 + wave, wave == 0);
  } else {
    finish_err(a, esum, wave);
    st.flush(a);
  }
}

template <int NCHUNK, bool DBG>
__global__ __launch_bounds__(512, 1) void conv3x3_wino_kernel(const float* __restrict__ p_src, const float* __restrict__ p_u,
                                                              int p_qin, int p_qout, const ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  (void)p_qout;
  // workgroups are dealt round-robin over the 8 XCDs in dispatch order: remap so that every XCD gets a CONTIGUOUS range of
  // logical ids, i.e. the four workgroups of a sample (two co tiles x two image halves, which read the same input) share an L2
  const int nwg = gridDim.x * gridDim.y;
  int lid = blockIdx.x + gridDim.x * blockIdx.y;
  if ((nwg & 7) == 0) lid = (lid & 7) * (nwg >> 3) + (lid >> 3);
  const int rh = lid & 1, ct = (lid >> 1) % (gridDim.x >> 1), b = (lid >> 1) / (gridDim.x >> 1);
  const PersistHook none;
  wino_layer<NCHUNK, DBG, false>(p_src, p_u, p_qin, a, b, ct, rh, smem, none);
}

// ---- a whole fixed-grid trajectory in ONE launch (64-channel dynamics, forward only) ---------------------------------------
// The ~2 us between dependent launches (and the cold start of every launch) is a fifth of a 10 us layer.  Here the 4
// workgroups of a sample (2 channel tiles x 2 image halves) stay resident and walk the layer table themselves; between layers
// they only wait for EACH OTHER (a per-sample counter), never for the grid.  What makes that cheap: with the XCD-aware id
// mapping the four partners sit on ONE XCD, whose L2 is the coherence point of their stores -- so the hand-off needs no L2
// write-back / invalidate, only (a) stores acknowledged (vmcnt(0)) before the counter is bumped and (b) input loads that skip
// the per-CU cache.  The dispatch order is not an architectural guarantee, so every workgroup publishes the XCD it really
// runs on (XCC_ID) and a group whose members differ falls back to agent-scope fences: slower, still correct.  All waits are
// capped (-> *host_err; the grid is one workgroup per CU and the occupancy is checked before the first launch), so a lost
// partner cannot hang the device.
struct PersistArgs {
  const ConvArgs* table;  // one entry per layer of the whole trajectory, in execution order (library-owned device copy)
  int n_layers, batch;
  unsigned* done;         // [batch] counters, one per 256-byte line (kDoneStride words apart), zero on entry: counters of groups
                          // on different XCDs must not share a cache line -- the line would bounce between the L2s on every bump
  unsigned* xcc_of;       // [gridDim.x], zero on entry: XCC_ID + 1 of each logical workgroup; xcc_of[gridDim.x] = abort word
  unsigned* host_err;
  float* out_nchw;        // base of the (T,B,C,16,16) result: table entries carry offsets into it (in `dbg`)
  unsigned long long* stamps;  // diagnostic: [64 layers][8] timestamps of logical workgroup 0, or null
  int sleep6;             // PersistHook::sleep6
  int sleep6_combine;     // added in front of a layer whose input comes out of a stage-combine epilogue
  const int* n_layers_ptr;  // adaptive walk only: if non-null, {first row, number of rows} of this launch's walk are read from the
                            // device (a device-side controller picks the section of the table); n_layers is then the table's size
  const unsigned long long* reloc;  // adaptive walk only: relocation bases (rel()), or null
  int fault_inject;       // tests only (ODEHIP_FAULT_INJECT=1, sixteen-workgroup walk): logical workgroup 0 leaves in front of row 1, so its
                          // partners' capped waits give up -- the give-up path (abort word, NaN fill, sticky host word) end to end
};

// An elementwise row of the adaptive walk (ConvArgs::combine == 4, odehip_internal.h).  Only the consumer waves work, each lane on
// the four quads the conv epilogues give it (channel quad Q of its 2x2 output tile): whatever it reads was written by this very
// lane (or before the launch), so there is nothing to wait for; the row is then announced like a layer.
template <int QOUT>
__device__ __forceinline__ void ew_row(const ConvArgs& a, int b, int ct, int rh, const PersistHook& hk) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (wave >= 4) return;
  typedef const __attribute__((address_space(4))) float ConstF;
  const CombineArgs& m = a.cmb;
  const unsigned long long* const rl = hk.reloc;
  const float hs = m.h_ptr ? *(ConstF*)m.h_ptr : 1.0f;
  const int ch = wave >> 1, thh = wave & 1, i16 = lane & 15, kq = lane >> 4;
  const int Q = ct * 8 + ch * 4 + kq, tile = thh * 16 + i16, oty = tile >> 3, otx = tile & 7, r0 = rh * 8;
  const float* const yp = rel(rl, m.y);
  if (a.combine == 5) {
    // norm row: this wave's share of sum(((a - b) / (atol + |y| * rtol))^2), a = k_prev[0], b = k_prev[1] (n_prev == 2), into
    // err_partials[(sample * 4 + workgroup of the sample) * 4 + wave] -- the scaled sums of squares of an initial-step search
    // (torchdiffeq _select_initial_step) without a separate reduction launch; the controller adds the partials in a fixed order
    const float* const pa = rel(rl, m.k_prev[0]);
    const float* const pb = m.n_prev > 1 ? rel(rl, m.k_prev[1]) : nullptr;
    float sum = 0.0f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const size_t o = (((size_t)b * QOUT + Q) * kPix + (r0 + 2 * oty + (q >> 1)) * 16 + 2 * otx + (q & 1)) * 4;
      f32x4 d = *(const f32x4*)(pa + o);
      const f32x4 yv = *(const f32x4*)(yp + o);
      if (pb) d -= *(const f32x4*)(pb + o);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float r = d[i] / __builtin_fmaf(fabsf(yv[i]), m.rtol, m.atol);
        sum = __builtin_fmaf(r, r, sum);
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) m.err_partials[(b * 4 + ct * 2 + rh) * 4 + wave] = sum;
    wait_vmcnt<0>();
    if (hk.fence) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
    if (lane == 0) __hip_atomic_store(hk.done + hk.word0 + wave, hk.target + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  float* const o1 = rel(rl, m.out1);
  float* const o2 = rel(rl, m.out2);
  f32x4 s1[4], s2[4];
  size_t off[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    off[q] = (((size_t)b * QOUT + Q) * kPix + (r0 + 2 * oty + (q >> 1)) * 16 + 2 * otx + (q & 1)) * 4;
    s1[q] = f32x4{0.f, 0.f, 0.f, 0.f};
    if (yp) s1[q] = *(const f32x4*)(yp + off[q]);
    s2[q] = s1[q];
  }
  for (int j = 0; j < m.n_prev; ++j) {   // ew_quad's fma sequence (conv_common.h), four quads at a time
    const float* const kp = rel(rl, m.k_prev[j]);
    const float c1 = (m.c_dev ? ((ConstF*)m.c_dev)[j] : m.c1[j]) * hs;
    const float c2 = m.c2[j] * hs;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const f32x4 kv = *(const f32x4*)(kp + off[q]);
      s1[q] = fma4(kv, c1, s1[q]);
      if (o2) s2[q] = fma4(kv, c2, s2[q]);
    }
  }
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    if (o1) *(f32x4*)(o1 + off[q]) = s1[q];
    if (o2) *(f32x4*)(o2 + off[q]) = s2[q];
  }
  wait_vmcnt<0>();
  if (hk.fence) __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
  if (lane == 0) __hip_atomic_store(hk.done + hk.word0 + wave, hk.target + 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool ADAPT>
__device__ __forceinline__ void persist_walk(const PersistArgs& pa, const ConvArgs* table) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nwg = gridDim.x;  // a multiple of 32: every XCD holds whole groups of 4
  const int lid = ((int)blockIdx.x & 7) * (nwg >> 3) + ((int)blockIdx.x >> 3);
  const int rh = lid & 1, ct = (lid >> 1) & 1, group = lid >> 2;
  const bool fence = xcc_rendezvous<4>(pa.xcc_of, lid, pa.xcc_of + nwg, pa.host_err);
  int n_layers = pa.n_layers;
  if (!walk_start(table, n_layers, ADAPT ? pa.n_layers_ptr : nullptr)) return;
  const int n_groups = nwg >> 2;
  // A group walks TWO samples at a time, layer by layer in turn (when the batch gives it more than one): the hand-off latency of
  // one sample's layer (stores acknowledged -> flags seen -> next input tile loaded) is then covered by the other sample's layer.
  for (int b = group; b < pa.batch; b += 2 * n_groups) {
    const int n_interleaved = b + n_groups < pa.batch ? 2 : 1;
    RowCursor cur(table, n_layers);
    int prev_combine = 0;  // the layer whose output this one waits for ended in a Runge-Kutta stage combine (a longer epilogue)
    for (int l = 0; l < n_layers; ++l) {
      const ConvArgs& a = cur.row(l);
#pragma unroll 1
      for (int s = 0; s < n_interleaved; ++s) {
        const int bs = __builtin_amdgcn_readfirstlane(b + s * n_groups);
        const PersistHook hk = {pa.done + (size_t)bs * kDoneStride, (unsigned)l, (lid & 3) * 4, pa.xcc_of + nwg, pa.host_err, fence,
                                pa.out_nchw, (pa.stamps && lid == 0 && bs == group && l < 64) ? pa.stamps + l * 8 : nullptr, pa.batch,
                                l == 0, n_interleaved == 1, true, true, pa.sleep6 + (prev_combine == 1 ? pa.sleep6_combine : 0),
                                ADAPT ? pa.reloc : nullptr,
                                (unsigned)(ADAPT && a.dep_back > 0 && l > 0 ? l - 1 : l)};
        if constexpr (ADAPT) {
          if (a.combine >= 4) ew_row<16>(a, bs, ct, rh, hk);
          else wino_layer<4, false, true, 16, true>(uniform_ptr(rel(pa.reloc, cur.src)), uniform_ptr(cur.u), 16, a, bs, ct, rh, smem, hk);
        } else {
          wino_layer<4, false, true>(uniform_ptr(cur.src), uniform_ptr(cur.u), 16, a, bs, ct, rh, smem, hk);
        }
      }
      prev_combine = a.combine;
      cur.next();
    }
  }
}

__global__ __launch_bounds__(512, 1) void wino_persist_kernel(const PersistArgs pa) { persist_walk<false>(pa, pa.table); }

// The walk of the adaptive solver's tables (dopri5 attempts, the backward passes of dopri5, the adaptive adjoint): stage combines of
// any depth with the step size on the device, elementwise rows, reverse-sweep targets -- a separate kernel so that the fixed-grid
// headline's instantiation above is not touched by any of it.
__global__ __launch_bounds__(512, 1) void wino_persist_d_kernel(const PersistArgs pa) { persist_walk<true>(pa, pa.table); }

// ---- the same walk for stacks with 128-channel ends (VidODE's dynamics 128 -> 64 -> 64 -> 128; helpers/utils.py:158-183 with
// n_inputs = n_outputs = 128, n_units = 64): still four workgroups per sample.  A 128 -> 64 layer is eight input chunks; a
// 64 -> 128 layer has four co tiles, so every workgroup makes TWO passes (co tiles ct and ct + 2) and announces the layer after the
// second; the partners' flags are waited for all at once (the chunk <-> co-tile correspondence of the 64 -> 64 case does not hold).
// A separate kernel: the headline's instantiation above is not touched by these code paths.
__device__ __forceinline__ void persist_walk_v(const PersistArgs& pa, const ConvArgs* table) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nwg = gridDim.x;
  const int lid = ((int)blockIdx.x & 7) * (nwg >> 3) + ((int)blockIdx.x >> 3);
  const int rh = lid & 1, ct = (lid >> 1) & 1, group = lid >> 2;
  const bool fence = xcc_rendezvous<4>(pa.xcc_of, lid, pa.xcc_of + nwg, pa.host_err);
  {  // an adaptive solver that finished while this launch was queued: nothing to do (uniform; constant during the launch)
    typedef const __attribute__((address_space(4))) int ConstI;
    const int* skip = table[0].skip;
    if (skip && *(ConstI*)skip) return;
  }
  const int n_groups = nwg >> 2;
  for (int b = group; b < pa.batch; b += 2 * n_groups) {
    const int n_interleaved = b + n_groups < pa.batch ? 2 : 1;
    int prev_combine = 0;
    for (int l = 0; l < pa.n_layers; ++l) {
      typedef const __attribute__((address_space(4))) ConvArgs ConstArgs;
      const ConvArgs& a = *(const ConvArgs*)((ConstArgs*)table + l);
      if (l + 1 < pa.n_layers && threadIdx.x < (sizeof(ConvArgs) + 63) / 64) {
        const unsigned v = __builtin_nontemporal_load((const unsigned*)&table[l + 1] + threadIdx.x * 16);
        asm volatile("" ::"v"(v));
      }
      const float* src = uniform_ptr(a.src1);
      const float* u = uniform_ptr(a.w_wino);
      const int qin = a.qin, qout = a.qout;
#pragma unroll 1
      for (int s = 0; s < n_interleaved; ++s) {
        const int bs = __builtin_amdgcn_readfirstlane(b + s * n_groups);
        PersistHook hk = {pa.done + (size_t)bs * kDoneStride, (unsigned)l, (lid & 3) * 4, pa.xcc_of + nwg, pa.host_err, fence,
                          pa.out_nchw, nullptr, pa.batch, l == 0, n_interleaved == 1, true, false,
                          pa.sleep6 + (prev_combine == 1 ? pa.sleep6_combine : 0), nullptr, (unsigned)l};
        if (qout == 16) {
          if (qin == 16) wino_layer<4, false, true, 16>(src, u, 16, a, bs, ct, rh, smem, hk);
          else           wino_layer<8, false, true, 16>(src, u, 32, a, bs, ct, rh, smem, hk);
        } else {  // 64 -> 128: co tiles ct and ct + 2; the second pass needs no wait (same input) and announces the layer
          hk.announce = false;
          wino_layer<4, false, true, 32>(src, u, 16, a, bs, ct, rh, smem, hk);
          hk.announce = true;
          hk.first = true;
          wino_layer<4, false, true, 32>(src, u, 16, a, bs, ct + 2, rh, smem, hk);
        }
      }
      prev_combine = a.combine;
    }
  }
}

__global__ __launch_bounds__(512, 1) void wino_persist_v_kernel(const PersistArgs pa) { persist_walk_v(pa, pa.table); }

// one sample per group: the walk in row strips (below, behind the sixteen-workgroup walk whose producers it shares)
__global__ void wino_persist_strip_kernel(const PersistArgs pa);

template <int NCHUNK, bool DBG>
static int launch_wino_nd(const ConvArgs& a, hipStream_t stream) {
  static bool attr_set = false;
  if (!attr_set) {
    ODEHIP_CHECK_HIP(hipFuncSetAttribute((const void*)conv3x3_wino_kernel<NCHUNK, DBG>, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    attr_set = true;
  }
  hipLaunchKernelGGL((conv3x3_wino_kernel<NCHUNK, DBG>), dim3((a.qout / 8) * 2, a.batch), dim3(512), kWinoLds, stream, a.src1, a.w_wino, a.qin, a.qout, a);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
template <int NCHUNK>
static int launch_wino_n(const ConvArgs& a, hipStream_t stream) {
  return a.debug ? launch_wino_nd<NCHUNK, true>(a, stream) : launch_wino_nd<NCHUNK, false>(a, stream);
}

int launch_wino_persist(const ConvArgs* table_dev, int n_layers, int batch, unsigned* done, unsigned* xcc_of, unsigned* host_err_dev,
                        float* out_nchw, int grid, hipStream_t stream, bool wide, bool adaptive, const int* n_layers_ptr,
                        const unsigned long long* reloc, bool strip) {
  static bool attr_set = false;
  ODEHIP_REQUIRE(!(wide && adaptive) && (adaptive || !n_layers_ptr), "wino_persist: no adaptive walk for 128-channel-ended stacks");
  ODEHIP_REQUIRE(!strip || (!wide && !adaptive && batch <= grid / 4), "wino_persist: the strip walk takes fixed-grid 64-channel tables, one sample per group");
  if (!attr_set) {
    ODEHIP_CHECK_HIP(hipFuncSetAttribute((const void*)wino_persist_d_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ODEHIP_CHECK_HIP(hipFuncSetAttribute((const void*)wino_persist_v_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ODEHIP_CHECK_HIP(hipFuncSetAttribute((const void*)wino_persist_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    ODEHIP_CHECK_HIP(hipFuncSetAttribute((const void*)wino_persist_strip_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    // every workgroup must be resident at once: one per CU (96 KiB of LDS each: two do not fit), `grid` <= number of CUs (checked by the caller)
    int per_cu = 0;
    ODEHIP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)wino_persist_kernel, 512, kWinoLds));
    ODEHIP_REQUIRE(per_cu >= 1, "wino_persist: the kernel does not fit a CU");
    ODEHIP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)wino_persist_d_kernel, 512, kWinoLds));
    ODEHIP_REQUIRE(per_cu >= 1, "wino_persist: the adaptive kernel does not fit a CU");
    ODEHIP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)wino_persist_strip_kernel, 512, kWinoLds));
    ODEHIP_REQUIRE(per_cu >= 1, "wino_persist: the strip kernel does not fit a CU");
    attr_set = true;
  }
  PersistArgs pa;
  pa.table = table_dev; pa.n_layers = n_layers; pa.batch = batch; pa.done = done; pa.xcc_of = xcc_of; pa.host_err = host_err_dev;
  pa.out_nchw = out_nchw;
  pa.stamps = g_debug_buf;
  constexpr int kSleep6 = 5;          // 5 x 0.18 us (sweep in wino_layer's comment)
  constexpr int kSleep6Combine = 4;   // sweep: 0: 1.382, 4: 1.367, 6: 1.370, 8: 1.383, 12: 1.404 ms
  // The strip walk's own pair: its producers finish their last transform earlier, so they have longer to sleep.  Sweep at B = 64
  // (profiles/strip_walk.json; median of 3 runs, ms): sleep6 / combine 7/4: 1.233 (one run of three at 1.38), 8/4: 1.198 (one at 1.38),
  // 9/4: 1.213, 10/4: 1.224, 11/4: 1.245, 12/4: 1.274, 14/4: 1.326; 10/0: 1.224, 10/8: 1.240.  Below 9 periods a run can settle in
  // a slow mode (1.38 - 1.51 ms: the producers poll the flag line while the neighbours' consumers still work); 10 keeps two periods
  // of margin to that edge for 1 % of the trajectory.
  constexpr int kStripSleep6 = 10, kStripSleep6Combine = 4;
  pa.sleep6 = strip ? kStripSleep6 : kSleep6;
  pa.sleep6_combine = strip ? kStripSleep6Combine : kSleep6Combine;
  pa.n_layers_ptr = n_layers_ptr;
  pa.reloc = reloc;
  pa.fault_inject = 0;
  // An ordinary launch: the co-residency a cooperative launch would verify is checked above, and a cooperative launch runs on a
  // separate hardware queue (extra cross-queue synchronisation per call; it also crashes rocprofv3's teardown on this stack).
  // (the strip walk needs 48 KiB of LDS and asks for the others' 96: a second workgroup must not share its CU)
  if (strip)         hipLaunchKernelGGL(wino_persist_strip_kernel, dim3(grid), dim3(512), kWinoLds, stream, pa);
  else if (wide)     hipLaunchKernelGGL(wino_persist_v_kernel, dim3(grid), dim3(512), kWinoLds, stream, pa);
  else if (adaptive) hipLaunchKernelGGL(wino_persist_d_kernel, dim3(grid), dim3(512), kWinoLds, stream, pa);
  else               hipLaunchKernelGGL(wino_persist_kernel, dim3(grid), dim3(512), kWinoLds, stream, pa);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

// ================================================================================================================================
// Small batches (B <= 16; the reference trains at batch 4, configs.yaml:7): SIXTEEN workgroups per sample.
// The walk above gives a sample four workgroups; at B = 4 that is 16 of 256 CUs, and a layer still costs its full 7.3 us because
// a consumer wave multiplies a whole (16 co x 16 tiles) block for all 16 transform positions (5.2 us).  Here workgroup
// (sample, 16-channel tile cq, row quarter rq) owns ONE such block and its four consumer waves split the positions by COLUMN of
// the 4x4 transform (wave w: xi = w, 4 + w, 8 + w, 12 + w): 16 MFMAs per 16-channel chunk and wave instead of 64.  The first half of
// the output transform (over the rows of M, S_a[col] -- the expressions of the 4-workgroup kernel) is wave-local; the second half
// needs all four columns, so the waves exchange S through LDS (8 KiB) and wave (a, b) finishes output pixel (a, b) of every 2x2 tile
// in the 4-workgroup kernel's order of operations: results are BIT-IDENTICAL to the other walk.  Producers: each wave DMAs and
// transforms the channel quad it loaded, one V row per lane (64 lanes = 16 tiles x 4 rows).  Hand-off: the sample's flag line has
// 64 words (16 workgroups x 4 consumer waves); a workgroup waits for the twelve workgroups of row quarters rq-1 .. rq+1 (all channels
// of the input rows it reads).  Forward tables (plain / ReLU stores, the prefetched stage combine) and reverse sweeps (mask layers
// prefetched, targets through the shared epilogue); LDS 88 KiB.
constexpr int k16U = 16 * 1024;    // U chunk: 16 xi x [quad 4][co 16][4 ci]
constexpr int k16Raw = 8 * 1024;   // raw chunk: 4 quads x 2 KiB: 6 rows x 20 slots of 16 B
constexpr int k16V = 16 * 1024;    // V chunk: 16 xi x [quad 4][tile 16][4 ci]
constexpr int k16X = 8 * 1024;     // exchange: [a 2][col 4][lane 64] quads
constexpr int kWino16Lds = 2 * k16U + 2 * k16Raw + 2 * k16V + k16X;

__device__ __forceinline__ void wait_done16(const PersistHook& hk, int lo_word, int hi_word) {
  int n = 0;
  const int lane = threadIdx.x & 63;
  const bool mine = lane >= lo_word && lane < hi_word;
  while (!__all(!mine || __hip_atomic_load(hk.done + lane, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= hk.wait_target)) {
    __builtin_amdgcn_s_sleep(1);
    if ((++n & 1023) == 0) {
      if (__hip_atomic_load(hk.abort_, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 1u) break;
      if (n > (1 << 23)) {
        __hip_atomic_store(hk.abort_, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        *hk.host_err = 3;
        break;
      }
    }
  }
  if (hk.fence) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
}

// The producer of the two row-quarter kernels (wino_layer16, wino_strip_layer): the raw tile is image rows r0 - 1 .. r0 + 4 in
// wino_layer's 20-slot rows (conflict-free stride-2 reads), zero-padded by the DMA's range check; every producer wave DMAs one
// channel quad of a chunk and transforms the quad it loaded itself (tq = pw: its own vmcnt suffices), one V row per lane
// (lane = (tile tt, V row vi): 8 ds_read_b128 + 4 ds_write_b128).  The issue order and the counted waits stay with each kernel.
struct SixRowProducer {
  __amdgpu_buffer_rsrc_t rx;
  char *Rb, *Vb;
  int pw, vr[2], off_a, off_b, v_off;
  float sg;
  __device__ __forceinline__ SixRowProducer(const float* p_src, int b, int r0, int pw_, int lane, char* raw, char* v)
      : rx(make_rsrc((const char*)p_src + (size_t)b * 16 * kQuadBytes, 16u * kQuadBytes)), Rb(raw), Vb(v), pw(pw_) {
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      const int s = 64 * p + lane;
      const int row = s / 20, w = s - row * 20;
      const int pc = w < 9 ? 2 * w : 2 * (w - 9) + 1;
      const int irow = r0 - 1 + row, col = pc - 1;
      vr[p] = (s < 120 && w < 18 && irow >= 0 && irow < kHW && col >= 0 && col < kHW) ? irow * 256 + col * 16 : kOobOffset;
    }
    const int tt = lane & 15, vi = lane >> 4, tq = pw;
    const int tty = tt >> 3, ttx = tt & 7;
    // V row vi of B^T d:  0: p0 - p2   1: p1 + p2   2: p2 - p1   3: p3 - p1  (sign of row 3 folded into U): T = a + sg * b
    const int ra = vi;
    const int rb = vi < 2 ? 2 : 1;
    sg = vi == 1 ? 1.0f : -1.0f;
    const int raw_base = tq * 2048 + (2 * tty * 20 + ttx) * 16;
    off_a = raw_base + ra * 320;
    off_b = raw_base + rb * 320;
    v_off = tq * 256 + tt * 16 + vi * 4 * 1024;
  }
  __device__ __forceinline__ void issue_raw(int c, int buf) const {
#pragma unroll
    for (int p = 0; p < 2; ++p)
      __builtin_amdgcn_raw_ptr_buffer_load_lds(rx, ODEHIP_LDS_PTR(Rb + buf * k16Raw + pw * 2048 + p * 1024), 16, vr[p],
                                               (c * 4 + pw) * kQuadBytes, 0, 16);
  }
  __device__ __forceinline__ void transform(int rbuf, int vbuf) const {
    const char* r = Rb + rbuf * k16Raw;
    f32x4 T[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int cj = ((j & 1) * 9 + (j >> 1)) * 16;
      const f32x4 da = *(const f32x4*)(r + off_a + cj);
      const f32x4 db = *(const f32x4*)(r + off_b + cj);
      T[j] = da + db * sg;
    }
    char* v = Vb + vbuf * k16V + v_off;
    *(f32x4*)(v + 0 * 1024) = pk_sub(T[0], T[2]);
    *(f32x4*)(v + 1 * 1024) = T[1] + T[2];
    *(f32x4*)(v + 2 * 1024) = pk_sub(T[2], T[1]);
    *(f32x4*)(v + 3 * 1024) = pk_sub(T[1], T[3]);
  }
};

__device__ __forceinline__ void wino_layer16(const float* __restrict__ p_src, const float* __restrict__ p_u, const ConvArgs& a, int b,
                                             int cq, int rq, char* smem, const PersistHook& hk) {
  char* const Ub = smem;
  char* const Rb = smem + 2 * k16U;
  char* const Vb = smem + 2 * k16U + 2 * k16Raw;
  char* const Xb = smem + 2 * k16U + 2 * k16Raw + 2 * k16V;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r0 = rq * 4;
  constexpr int nchunk = 4;

  if (wave >= 4) {
    // =========================================== PRODUCERS ===========================================
    const int pw = wave - 4;
    const int ct = cq >> 1, half = cq & 1;
    const unsigned u_tile_bytes = (unsigned)nchunk * kWU;   // the 32-channel tile this 16-channel tile is half of
    const __amdgpu_buffer_rsrc_t ru = make_rsrc((const char*)p_u + (size_t)ct * u_tile_bytes, u_tile_bytes);
    const SixRowProducer pr(p_src, b, r0, pw, lane, Rb, Vb);
    // U: the chunk's 64 (xi, quad) pieces of this channel half are 256 B each, 512 B apart: one instruction moves four of them
    const int vu = (lane >> 4) * 512 + half * 256 + (lane & 15) * 16;
    auto issue_u = [&](int c, int buf) {
#pragma unroll
      for (int g = 0; g < 4; ++g) {
        const int p = pw * 4 + g;   // pieces 4p .. 4p + 3
        dma16(ru, Ub + buf * k16U + p * 1024, vu, c * kWU + p * 2048);
      }
    };
    // DMA order per wave: U_0 (4) | raw_0 (2) | raw_1 (2) | then per iteration c: U_{c+1} (4) | raw_{c+2} (2)
    issue_u(0, 0);
    if (!hk.first) {
      if (hk.wait_target == hk.target)   // (a row with a relaxed dependency has nothing to sleep for)
        for (int i = 0; i < hk.sleep6; ++i) __builtin_amdgcn_s_sleep(6);
      const int lo = rq > 0 ? (rq - 1) * 16 : 0, hi = rq < 3 ? (rq + 2) * 16 : 64;
      wait_done16(hk, lo, hi);
    }
    pr.issue_raw(0, 0);
    pr.issue_raw(1, 1);
    wait_vmcnt<2>();   // U_0 and raw_0 landed
    pr.transform(0, 0);
#pragma unroll
    for (int c = 0; c < nchunk; ++c) {
      __builtin_amdgcn_s_barrier();  // [c]
      if (c + 1 < nchunk) {
        issue_u(c + 1, (c + 1) & 1);
        if (c + 2 < nchunk) {
          pr.issue_raw(c + 2, c & 1);
          wait_vmcnt<6>();           // raw_{c+1} landed
        } else {
          wait_vmcnt<4>();
        }
        pr.transform((c + 1) & 1, (c + 1) & 1);
        if (c + 2 < nchunk) wait_vmcnt<2>(); else wait_vmcnt<0>();  // U_{c+1} landed
      }
    }
    __builtin_amdgcn_s_barrier();    // [X] the consumers' exchange
    return;
  }

  // ============================================= CONSUMERS =============================================
  const int i16 = lane & 15, kq = lane >> 4;
  f32x4 acc[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int frag_off = kq * 256 + i16 * 16;       // same offset in a U and in a V position block
  const int Q = cq * 4 + kq;
  const int oa = wave >> 1, ob = wave & 1;        // the output pixel of every 2x2 tile this wave finishes
  const int oty = i16 >> 3, otx = i16 & 7;
  const int P = (r0 + 2 * oty + oa) * 16 + 2 * otx + ob;
  const size_t off = (((size_t)b * 16 + Q) * kPix + P) * 4;
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (a.bias) bias4 = *(const f32x4*)(a.bias + Q * 4);
  // epilogue operands fetched now (this lane's own earlier outputs, as in the 4-workgroup walk)
  const unsigned long long* const rl = hk.reloc;
  typedef const __attribute__((address_space(4))) float ConstF16;
  // an order-1 stage combine (the adaptive solver's tables) is reduced to y, two partial sums and y1 here, a reverse-sweep row with
  // up to two constant-coefficient targets to its (srcA, srcB) pairs -- the adaptive walk's scheme (wino_layer<..., ADAPT>), one quad
  // per lane; pointers may be relocatable
  const bool adapt1 = a.combine == 1 && a.cmb.order == 1 && !(a.cmb.err_partials && (a.cmb.out2 || a.dbg));
  const bool adapt3 = a.combine == 3 && a.bwd.n_targets <= 2 && !a.bwd.h_ptr;
  const int e_combine = adapt1 ? 6 : (adapt3 ? 7 : a.combine);
  const int e_act = a.act;
  float* const e_dst = rel(rl, a.dst);
  f32x4 d_y1 = {0.f, 0.f, 0.f, 0.f}, d_sa = {0.f, 0.f, 0.f, 0.f}, d_sb = {0.f, 0.f, 0.f, 0.f};
  float d_cB = 0.0f, d_rtol = 0.0f, d_atol = 0.0f, d_t[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  float* d_o[2] = {nullptr, nullptr};
  bool d_err = false, d_f[4] = {false, false, false, false};
  float* d_part = nullptr;
  int e_np = 0;
  float* e_kout = nullptr;
  float* e_out1 = nullptr;
  float* e_out2 = nullptr;
  float* e_nchw = nullptr;
  bool e_y = false;
  float e_h = 1.0f, e_ks = 1.0f, e_c1c = 0.0f, e_c2c = 0.0f, e_c1[3] = {0.f, 0.f, 0.f}, e_c2[3] = {0.f, 0.f, 0.f};
  f32x4 e_yv = {0.f, 0.f, 0.f, 0.f}, e_kv[3];
  if (e_combine == 1) {
    const CombineArgs& m = a.cmb;
    e_np = m.n_prev;
    // the step size by value (persistent tables of the fixed-grid drivers), or through its pointer (a single evaluation whose dt
    // only exists on the device: the encoder loop's Euler step)
    e_h = a.h_by_value ? m.atol : (m.h_ptr ? *(ConstF16*)m.h_ptr : 1.0f);
    e_ks = m.k_scale;
    e_c1c = m.c1[e_np];
    e_c2c = m.c2[e_np];
    e_kout = m.k_out;
    e_out1 = m.out1;
    e_out2 = m.out2;
    e_nchw = a.dbg ? hk.nchw_base + ((size_t)a.dbg - 1) : nullptr;
    e_y = m.y != nullptr;
    if (e_y) e_yv = *(const f32x4*)(m.y + off);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      if (j < e_np) e_kv[j] = *(const f32x4*)(m.k_prev[j] + off);
      e_c1[j] = m.c1[j];
      e_c2[j] = m.c2[j];
    }
  } else if (e_combine == 2) {   // ReLU-mask layer of a reverse sweep: the mask value is fetched now
    const BwdArgs& w = a.bwd;
    const float hb = a.h_by_value ? a.cmb.atol : (w.h_ptr ? *(ConstF16*)w.h_ptr : 0.0f);
    e_ks = w.sc_c + w.sc_h * hb;
    e_y = w.mask_src != nullptr;
    if (e_y) e_yv = *(const f32x4*)(rel(rl, w.mask_src) + off);
  } else if (e_combine == 6) {   // order-1 stage combine: the sums over the earlier stages (combine1_prev's fma sequence)
    const CombineArgs& m = a.cmb;
    e_np = m.n_prev;
    e_h = a.h_by_value ? m.atol : (m.h_ptr ? *(ConstF16*)m.h_ptr : 1.0f);
    e_ks = m.k_scale;
    d_err = m.err_partials != nullptr;
    d_part = m.err_partials;
    e_y = m.y != nullptr;
    e_c1c = m.c1[e_np];
    d_cB = d_err ? m.ce[e_np] : m.c2[e_np];
    d_rtol = m.rtol; d_atol = m.atol;
    e_kout = rel(rl, m.k_out);
    e_out1 = rel(rl, m.out1);
    e_out2 = rel(rl, m.out2);
    e_nchw = m.out2_nchw;
    const bool needB = d_err || e_out2 || e_nchw;
    if (e_y) {
      e_yv = *(const f32x4*)(rel(rl, m.y) + off);
      if (d_err) d_y1 = *(const f32x4*)(rel(rl, m.err_y1) + off);
      const float* kp[ODEHIP_MAX_STAGES - 1];
      float cA[ODEHIP_MAX_STAGES - 1], cB[ODEHIP_MAX_STAGES - 1];
#pragma unroll
      for (int j = 0; j < ODEHIP_MAX_STAGES - 1; ++j) {
        kp[j] = j < e_np ? rel(rl, m.k_prev[j]) : nullptr;
        cA[j] = m.c1[j];
        cB[j] = d_err ? m.ce[j] : m.c2[j];
      }
#pragma unroll
      for (int j = 0; j < ODEHIP_MAX_STAGES - 1; ++j)
        if (j < e_np) {
          const f32x4 kv = *(const f32x4*)(kp[j] + off);
          d_sa = fma4(kv, cA[j], d_sa);
          if (needB) d_sb = fma4(kv, cB[j], d_sb);
        }
    }
  } else if (e_combine == 7) {   // reverse-sweep targets held in registers
    const BwdArgs& w = a.bwd;
#pragma unroll
    for (int t = 0; t < 2; ++t)
      if (t < w.n_targets) {
        const BwdTarget& T = w.tgt[t];
        d_o[t] = rel(rl, T.out);
        d_t[3 * t] = T.g_c; d_t[3 * t + 1] = T.a_c; d_t[3 * t + 2] = T.b_c;
        d_f[2 * t] = T.srcA != nullptr; d_f[2 * t + 1] = T.srcB != nullptr;
        if (t == 0) {
          if (d_f[0]) e_yv = *(const f32x4*)(rel(rl, T.srcA) + off);
          if (d_f[1]) d_y1 = *(const f32x4*)(rel(rl, T.srcB) + off);
        } else {
          if (d_f[2]) d_sa = *(const f32x4*)(rel(rl, T.srcA) + off);
          if (d_f[3]) d_sb = *(const f32x4*)(rel(rl, T.srcB) + off);
        }
      }
  }
#pragma unroll
  for (int c = 0; c < nchunk; ++c) {
    __builtin_amdgcn_s_barrier();  // [c]
    const char* u = Ub + (c & 1) * k16U + frag_off;
    const char* v = Vb + (c & 1) * k16V + frag_off;
    f32x4 wf[4], xf[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      wf[i] = *(const f32x4*)(u + (4 * i + wave) * 1024);
      xf[i] = *(const f32x4*)(v + (4 * i + wave) * 1024);
    }
    // per position the chunk's four K-steps in the 4-workgroup kernel's order (.x .y .z .w); the four positions interleaved
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i].x, xf[i].x, acc[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i].y, xf[i].y, acc[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i].z, xf[i].z, acc[i], 0, 0, 0);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[i].w, xf[i].w, acc[i], 0, 0, 0);
  }
  // first half of the output transform, over the rows of M (this wave's column): the 4-workgroup kernel's S[0][col], S[1][col]
  {
    const f32x4 S0 = acc[0] + acc[1] + acc[2];
    const f32x4 S1 = pk_sub(pk_sub(acc[1], acc[2]), acc[3]);
    *(f32x4*)(Xb + (0 * 4 + wave) * 1024 + lane * 16) = S0;
    *(f32x4*)(Xb + (1 * 4 + wave) * 1024 + lane * 16) = S1;
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_s_barrier();    // [X]
  f32x4 val;
  {
    const char* x = Xb + oa * 4 * 1024 + lane * 16;
    if (ob == 0) {
      val = *(const f32x4*)(x) + *(const f32x4*)(x + 1024) + *(const f32x4*)(x + 2048) + bias4;
    } else {
      val = pk_sub(pk_sub(*(const f32x4*)(x + 1024) + bias4, *(const f32x4*)(x + 2048)), *(const f32x4*)(x + 3072));
    }
  }
  if (!e_combine) {
    *(f32x4*)(e_dst + off) = act_fwd(val, e_act);
  } else if (e_combine == 2) {
    val *= e_ks;
    if (e_y) val = act_bwd(val, e_yv, e_act);
    *(f32x4*)(e_dst + off) = val;
  } else if (e_combine == 3) {   // reverse-sweep targets: the shared epilogue, read from the table
    float esum = 0.0f;
    emit_quad<false>(a, b, Q, P, val, esum);
  } else if (e_combine == 6) {
    const f32x4 kc = act_fwd(val, e_act) * e_ks;   // (a Tanh head before the sign)
    if (e_kout) *(f32x4*)(e_kout + off) = kc;
    if (e_y) {
      if (e_out1) *(f32x4*)(e_out1 + off) = fma4(fma4(kc, e_c1c, d_sa), e_h, e_yv);
      if (d_err) {
        // this wave's partial of the error norm: 64 partials per sample here (16 workgroups x 4 waves), added by the controller in a
        // fixed order -- not the per-layer kernels' order, so batches up to 16 agree with one launch per layer to round-off of the
        // NORM only (every stored value is still bit-identical)
        float esum = combine1_err(fma4(kc, d_cB, d_sb), e_h, e_yv, d_y1, d_rtol, d_atol, 0.0f);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) esum += __shfl_xor(esum, o, 64);
        if (lane == 0) d_part[(b * 16 + rq * 4 + cq) * 4 + wave] = esum;
      } else if (e_out2 || e_nchw) {
        const f32x4 o2 = fma4(fma4(kc, d_cB, d_sb), e_h, e_yv);
        if (e_out2) *(f32x4*)(e_out2 + off) = o2;
        if (e_nchw) {
          float* o = e_nchw + ((size_t)b * 64 + Q * 4) * kPix + P;
          o[0] = o2.x; o[kPix] = o2.y; o[2 * kPix] = o2.z; o[3 * kPix] = o2.w;
        }
      }
    }
  } else if (e_combine == 7) {
    if (d_o[0]) {
      f32x4 o = val * d_t[0];
      if (d_f[0]) o = fma4(e_yv, d_t[1], o);
      if (d_f[1]) o = fma4(d_y1, d_t[2], o);
      *(f32x4*)(d_o[0] + off) = o;
    }
    if (d_o[1]) {
      f32x4 o = val * d_t[3];
      if (d_f[2]) o = fma4(d_sa, d_t[4], o);
      if (d_f[3]) o = fma4(d_sb, d_t[5], o);
      *(f32x4*)(d_o[1] + off) = o;
    }
  } else {
    const f32x4 kc = act_fwd(val, e_act) * e_ks;   // (a Tanh head before the sign)
    if (e_kout) *(f32x4*)(e_kout + off) = kc;
    if (e_y) {
      if (e_out1) {
        f32x4 sa = kc * e_c1c;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < e_np) sa += e_kv[j] * e_c1[j];
        *(f32x4*)(e_out1 + off) = e_yv + sa * e_h;
      }
      if (e_out2 || e_nchw) {
        f32x4 sb = kc * e_c2c;
#pragma unroll
        for (int j = 0; j < 3; ++j)
          if (j < e_np) sb += e_kv[j] * e_c2[j];
        const f32x4 o2 = e_yv + sb * e_h;
        if (e_out2) *(f32x4*)(e_out2 + off) = o2;
        if (e_nchw) {
          float* o = e_nchw + ((size_t)b * 64 + Q * 4) * kPix + P;
          o[0] = o2.x; o[kPix] = o2.y; o[2 * kPix] = o2.z; o[3 * kPix] = o2.w;
        }
      }
    }
  }
  announce(hk, hk.done + (rq * 4 + cq) * 4 + wave);
}

// elementwise / norm rows (ConvArgs::combine == 4 / 5) in the sixteen-workgroup layout: a lane's one quad (see ew_row)
__device__ __forceinline__ void ew_row16(const ConvArgs& a, int b, int cq, int rq, const PersistHook& hk) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (wave >= 4) return;
  typedef const __attribute__((address_space(4))) float ConstF;
  const CombineArgs& m = a.cmb;
  const unsigned long long* const rl = hk.reloc;
  const int i16 = lane & 15, kq = lane >> 4;
  const int Q = cq * 4 + kq, oa = wave >> 1, ob = wave & 1, oty = i16 >> 3, otx = i16 & 7;
  const int P = (rq * 4 + 2 * oty + oa) * 16 + 2 * otx + ob;
  const size_t off = (((size_t)b * 16 + Q) * kPix + P) * 4;
  const float* const yp = rel(rl, m.y);
  if (a.combine == 5) {
    f32x4 d = *(const f32x4*)(rel(rl, m.k_prev[0]) + off);
    const f32x4 yv = *(const f32x4*)(yp + off);
    if (m.n_prev > 1) d -= *(const f32x4*)(rel(rl, m.k_prev[1]) + off);
    float sum = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float r = d[i] / __builtin_fmaf(fabsf(yv[i]), m.rtol, m.atol);
      sum = __builtin_fmaf(r, r, sum);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if (lane == 0) m.err_partials[(b * 16 + rq * 4 + cq) * 4 + wave] = sum;
  } else {
    const float hs = m.h_ptr ? *(ConstF*)m.h_ptr : 1.0f;
    float* const o1 = rel(rl, m.out1);
    float* const o2 = rel(rl, m.out2);
    f32x4 s1 = {0.f, 0.f, 0.f, 0.f};
    if (yp) s1 = *(const f32x4*)(yp + off);
    f32x4 s2 = s1;
    for (int j = 0; j < m.n_prev; ++j) {
      const f32x4 kv = *(const f32x4*)(rel(rl, m.k_prev[j]) + off);
      s1 = fma4(kv, (m.c_dev ? ((ConstF*)m.c_dev)[j] : m.c1[j]) * hs, s1);
      if (o2) s2 = fma4(kv, m.c2[j] * hs, s2);
    }
    if (o1) *(f32x4*)(o1 + off) = s1;
    if (o2) *(f32x4*)(o2 + off) = s2;
  }
  announce(hk, hk.done + (rq * 4 + cq) * 4 + wave);
}

// A wait of this launch gave up (abort word set; never expected): whatever the walk wrote cannot be trusted.  Every workgroup that is
// still running NaN-fills ITS share (channel tile x row quarter) of every output of every row of the walk before it leaves, so the
// caller cannot be handed plausible-looking numbers -- in particular the single-evaluation walks (the encoder loop's Euler steps at
// batches up to 16), which have no host-side guard launch behind them.  The sticky host word raises at the next library call as well.
__device__ __forceinline__ void nan_fill_row16(const ConvArgs& a, int b, int cq, int rq, const unsigned long long* rl, float* nchw_base) {
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (wave >= 4) return;
  const int i16 = lane & 15, kq = lane >> 4, oa = wave >> 1, ob = wave & 1, oty = i16 >> 3, otx = i16 & 7;
  const int Q = cq * 4 + kq, P = (rq * 4 + 2 * oty + oa) * 16 + 2 * otx + ob;
  const size_t off = (((size_t)b * 16 + Q) * kPix + P) * 4;
  const float nanv = __builtin_nanf("");
  const f32x4 nan4 = {nanv, nanv, nanv, nanv};
  float* outs[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  float* frame = nullptr;
  if (a.combine == 0 || a.combine == 2) {
    outs[0] = rel(rl, a.dst);
  } else if (a.combine == 1 || a.combine == 4) {
    outs[0] = rel(rl, a.cmb.k_out); outs[1] = rel(rl, a.cmb.out1); outs[2] = rel(rl, a.cmb.out2);
    frame = a.dbg ? nchw_base + ((size_t)a.dbg - 1) : a.cmb.out2_nchw;
  } else if (a.combine == 3) {
    for (int t = 0; t < 4; ++t)
      if (t < a.bwd.n_targets) outs[t] = rel(rl, a.bwd.tgt[t].out);
  }
#pragma unroll
  for (int i = 0; i < 6; ++i)
    if (outs[i]) *(f32x4*)(outs[i] + off) = nan4;
  if (frame) {
    float* o = frame + ((size_t)b * 64 + Q * 4) * kPix + P;
    o[0] = o[kPix] = o[2 * kPix] = o[3 * kPix] = nanv;
  }
  if ((a.combine == 1 || a.combine == 5) && a.cmb.err_partials && lane == 0) a.cmb.err_partials[(b * 16 + rq * 4 + cq) * 4 + wave] = nanv;
}

__global__ __launch_bounds__(512, 1) void wino_persist16_kernel(const PersistArgs pa) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // 256 workgroups, dealt round-robin over the 8 XCDs: XCD x holds logical ids 32 x .. 32 x + 31 = two samples' sixteen workgroups
  // each; sample s lives on XCD s % 8 (batches up to 8 get an XCD -- and its L2 -- per sample)
  const int lid = ((int)blockIdx.x & 7) * 32 + ((int)blockIdx.x >> 3);
  const int xcd = lid >> 5, slot = (lid >> 4) & 1, wg = lid & 15;
  const int b = slot * 8 + xcd;
  const int rq = wg >> 2, cq = wg & 3;
  if (b >= pa.batch) return;
  const bool fence = xcc_rendezvous<16>(pa.xcc_of, lid, pa.xcc_of + gridDim.x, pa.host_err);
  const ConvArgs* table = pa.table;
  int n_layers = pa.n_layers;
  if (!walk_start(table, n_layers, pa.n_layers_ptr)) return;
  RowCursor cur(table, n_layers);
  for (int l = 0; l < n_layers; ++l) {
    const ConvArgs& a = cur.row(l);
    PersistHook hk;
    hk.done = pa.done + (size_t)b * kDoneStride;
    hk.target = (unsigned)l;
    hk.wait_target = (unsigned)(a.dep_back > 0 && l > 0 ? l - 1 : l);
    hk.abort_ = pa.xcc_of + gridDim.x; hk.host_err = pa.host_err;
    hk.fence = fence;
    hk.nchw_base = pa.out_nchw;
    hk.batch = pa.batch;
    hk.first = l == 0;
    hk.solo = true;
    hk.sleep6 = pa.sleep6;
    hk.reloc = pa.reloc;
    if (pa.fault_inject && lid == 0 && l == 1) return;   // (tests: a lost partner)
    if (a.combine >= 4) ew_row16(a, b, cq, rq, hk);
    else wino_layer16(uniform_ptr(rel(pa.reloc, cur.src)), uniform_ptr(cur.u), a, b, cq, rq, smem, hk);
    cur.next();
  }
  if (__hip_atomic_load(pa.xcc_of + gridDim.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u) {   // (uniform) some wait gave up
    for (int l = 0; l < n_layers; ++l) {
      typedef const __attribute__((address_space(4))) ConvArgs ConstArgs;
      nan_fill_row16(*(const ConvArgs*)((ConstArgs*)table + l), b, cq, rq, pa.reloc, pa.out_nchw);
    }
  }
}

int launch_wino_persist16(const ConvArgs* table_dev, int n_layers, int batch, unsigned* done, unsigned* xcc_of, unsigned* host_err_dev,
                          float* out_nchw, hipStream_t stream, const int* n_layers_ptr, const unsigned long long* reloc) {
  static bool attr_set = false;
  ODEHIP_REQUIRE(batch >= 1 && batch <= 16, "wino_persist16: batch %d out of range", batch);
  if (!attr_set) {
    ODEHIP_CHECK_HIP(hipFuncSetAttribute((const void*)wino_persist16_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    int per_cu = 0;
    ODEHIP_CHECK_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, (const void*)wino_persist16_kernel, 512, kWino16Lds));
    ODEHIP_REQUIRE(per_cu >= 1, "wino_persist16: the kernel does not fit a CU");
    attr_set = true;
  }
  PersistArgs pa;
  memset(&pa, 0, sizeof(pa));
  pa.table = table_dev; pa.n_layers = n_layers; pa.batch = batch; pa.done = done; pa.xcc_of = xcc_of; pa.host_err = host_err_dev;
  pa.out_nchw = out_nchw;
  pa.n_layers_ptr = n_layers_ptr;
  pa.reloc = reloc;
  // Periods of 0.18 us the producers sleep in front of their first poll (a polling wave takes issue slots from the consumer wave of
  // its SIMD).  Sweep, forward trajectory B = 4, T = 10, rk4 (ms): 0: 1.07, 1: 0.90, 2: 0.66, 3: 0.605, 4: 0.596, 6: 0.619; B = 12 / 16:
  // 3: 0.88 / 0.80, 4: 0.621 / 0.620, 5: 0.608 / 0.617.
  constexpr int kSleep6Upto8 = 4, kSleep6Above8 = 5;
  pa.sleep6 = batch > 8 ? kSleep6Above8 : kSleep6Upto8;
  {   // tests only: the FIRST launch that sees ODEHIP_FAULT_INJECT=1 loses a workgroup (read per launch: a test flips it in-process)
    static int injected = 0;
    const char* e = getenv("ODEHIP_FAULT_INJECT");
    pa.fault_inject = e && e[0] == '1' && injected++ == 0;
  }
  hipLaunchKernelGGL(wino_persist16_kernel, dim3(256), dim3(512), kWino16Lds, stream, pa);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

// ================================================================================================================================
// One sample per group (batch <= number of groups): FOUR ROW STRIPS per sample instead of two co tiles x two image halves.
// In the walk above the two co-tile workgroups of an image half DMA and transform the same raw tile into the same V: every
// V = B^T d B of the trajectory is computed twice, on the SIMDs whose fp32 datapath the MFMAs use.  Here workgroup (sample, row
// quarter rq) owns ALL 64 output channels of 4 output rows (2 x 8 tiles): consumer wave w multiplies the (16 co = quad block w) x
// (16 tiles) block for all 16 xi -- the same 64 MFMAs per chunk, the same 64 accumulators, the same register-only output transform
// as wino_layer, so every accumulator element sees the same MFMA sequence and the results are BIT-IDENTICAL to the other walks and
// to one launch per layer.  All four waves read the same V fragments and four different U blocks (the packed tensor is
// [ct][chunk][xi][quad][co 32][4 ci]: wave w reads co tile w >> 1, co (w & 1) * 16 + i16).  Producers: the sixteen-workgroup walk's
// (6 raw rows x 20 slots; one V row per lane: 8 ds_read_b128 + 4 ds_write_b128) -- half of wino_layer's producer work per chunk.
// Hand-off: flag word rq * 4 + wave; a strip waits for the 8 or 12 words of strips rq - 1 .. rq + 1 (all channels of the input rows
// it reads).  A strip overwrites rows only its neighbours and itself have read, and has seen all of them finish the layer that read
// them, so the tables' buffer reuse (never closer than two layers) holds as it does for the sixteen-workgroup walk.
// LDS: raw[2] 16 KiB + V[2] 32 KiB = 48 KiB.
constexpr int kStripLds = 2 * k16Raw + 2 * k16V;
static_assert(kStripLds <= kWinoLds, "the strip walk is launched with the other walks' LDS request");

__device__ __forceinline__ void wino_strip_layer(const float* __restrict__ p_src, const float* __restrict__ p_u, const ConvArgs& a, int b,
                                                 int rq, char* smem, const PersistHook& hk) {
  char* const Rb = smem;
  char* const Vb = smem + 2 * k16Raw;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r0 = rq * 4;
  constexpr int nchunk = 4;

  if (wave >= 4) {
    // =========================================== PRODUCERS ===========================================
    const int pw = wave - 4;
    const SixRowProducer pr(p_src, b, r0, pw, lane, Rb, Vb);
    // DMA order per wave: raw_0 (2) | raw_1 (2) | then per iteration c: raw_{c+2} (2); counted waits leave the younger ones in flight
    if (pw == 0) pstamp(hk, 0, lane);
    if (!hk.first) {
      // the neighbours cannot be done before this workgroup's own consumers are through their last chunk: sleep through most of it
      // instead of polling (wino_layer)
      for (int i = 0; i < hk.sleep6; ++i) __builtin_amdgcn_s_sleep(6);
      wait_done16(hk, rq > 0 ? (rq - 1) * 4 : 0, rq < 3 ? (rq + 2) * 4 : 16);
    }
    if (pw == 0) pstamp(hk, 1, lane);
    pr.issue_raw(0, 0);
    pr.issue_raw(1, 1);
    wait_vmcnt<2>();                   // raw_0 landed (raw_1 still in flight)
    if (pw == 0) pstamp(hk, 2, lane);
    pr.transform(0, 0);
    if (pw == 0) pstamp(hk, 3, lane);
#pragma unroll
    for (int c = 0; c < nchunk; ++c) {
      __builtin_amdgcn_s_barrier();  // [c] V_c ready for the consumers; they are done with chunk c-1
      if (c + 1 < nchunk) {
        if (c + 2 < nchunk) {
          pr.issue_raw(c + 2, c & 1);   // raw buffer consumed by this wave's transform of chunk c
          wait_vmcnt<2>();           // raw_{c+1} landed (raw_{c+2} still in flight)
        } else {
          wait_vmcnt<0>();           // raw_{c+1}, the last one
        }
        pr.transform((c + 1) & 1, (c + 1) & 1);  // V buffer last read by the MFMAs of chunk c-1
      }
    }
    return;
  }

  // ============================================= CONSUMERS =============================================
  const int i16 = lane & 15, kq = lane >> 4;
  f32x4 acc[16];
#pragma unroll
  for (int x = 0; x < 16; ++x) acc[x] = f32x4{0.f, 0.f, 0.f, 0.f};
  // this lane's 16 bytes of a position's 2 KiB block [quad 4][co 32][4 ci] of co tile wave >> 1
  const int u_off = (wave >> 1) * (nchunk * kWU) + kq * 512 + ((wave & 1) * 16 + i16) * 16;
  const int v_off = kq * 256 + i16 * 16;
  const __amdgpu_buffer_rsrc_t ru = make_rsrc(p_u, 2u * nchunk * kWU);
  f32x4 uw[kUAhead];
#pragma unroll
  for (int g = 0; g < kUAhead; ++g) uw[g] = load_u(ru, u_off, g * 2048);
  const int Q = wave * 4 + kq;
  f32x4 bias4 = {0.f, 0.f, 0.f, 0.f};
  if (a.bias) bias4 = *(const f32x4*)(a.bias + Q * 4);  // loaded now, used after the last MFMA
  const int oty = i16 >> 3, otx = i16 & 7;
  PreEpilogue<16> ep;
  ep.fetch(a, hk, b, Q, r0 + 2 * oty, otx);
#pragma unroll
  for (int c = 0; c < nchunk; ++c) {
    __builtin_amdgcn_s_barrier();  // [c]
    if (c == 0 && wave == 0) pstamp(hk, 4, lane);
    chunk_mma<1024, nchunk>(Vb + (c & 1) * k16V + v_off, c, ru, u_off, uw, acc, false);
  }
  if (wave == 0) pstamp(hk, 5, lane);

  float esum = 0.0f;
  f32x4 y[4];   // lane (tile i16, row group kq): its 2x2 tile
  out_transform(acc, bias4, y);
#pragma unroll
  for (int q = 0; q < 4; ++q) ep.emit(a, b, Q, q, (r0 + 2 * oty + (q >> 1)) * 16 + 2 * otx + (q & 1), y[q], esum);
  // this wave's share of the layer is in L2 once its stores are acknowledged; then it counts itself in
  if (wave == 0) pstamp(hk, 6, lane);
  announce(hk, hk.done + hk.word0 + wave, wave == 0);
}

__global__ __launch_bounds__(512, 1) void wino_persist_strip_kernel(const PersistArgs pa) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nwg = gridDim.x;  // a multiple of 32: every XCD holds whole groups of 4
  const int lid = ((int)blockIdx.x & 7) * (nwg >> 3) + ((int)blockIdx.x >> 3);
  const int rq = lid & 3, group = lid >> 2;
  const bool fence = xcc_rendezvous<4>(pa.xcc_of, lid, pa.xcc_of + nwg, pa.host_err);
  const ConvArgs* table = pa.table;
  int n_layers = pa.n_layers;
  if (!walk_start(table, n_layers, nullptr)) return;
  const int n_groups = nwg >> 2;
  for (int b = group; b < pa.batch; b += n_groups) {   // (the host selects this walk for batch <= n_groups: one sample per group)
    RowCursor cur(table, n_layers);
    int prev_combine = 0;  // the layer whose output this one waits for ended in a Runge-Kutta stage combine (a longer epilogue)
    for (int l = 0; l < n_layers; ++l) {
      const ConvArgs& a = cur.row(l);
      const PersistHook hk = {pa.done + (size_t)b * kDoneStride, (unsigned)l, rq * 4, pa.xcc_of + nwg, pa.host_err, fence,
                              pa.out_nchw, (pa.stamps && lid == 0 && b == group && l < 64) ? pa.stamps + l * 8 : nullptr, pa.batch,
                              l == 0, true, true, false, pa.sleep6 + (prev_combine == 1 ? pa.sleep6_combine : 0), nullptr, (unsigned)l};
      wino_strip_layer(uniform_ptr(cur.src), uniform_ptr(cur.u), a, b, rq, smem, hk);
      prev_combine = a.combine;
      cur.next();
    }
  }
}

// returns 1 if the shape has no Winograd instantiation (the caller then runs the direct kernel)
int launch_wino(const ConvArgs& a, hipStream_t stream) {
  switch (a.qin / 4) {
    case 1: return launch_wino_n<1>(a, stream);
    case 2: return launch_wino_n<2>(a, stream);
    case 3: return launch_wino_n<3>(a, stream);
    case 4: return launch_wino_n<4>(a, stream);
    case 8: return launch_wino_n<8>(a, stream);
    default: return 1;
  }
}

}  // namespace odehip
