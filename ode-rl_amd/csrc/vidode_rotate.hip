// vidode_rotate.hip -- the batch launch of vidode_batch.hip with upstream Vid-ODE's RandomRotation in it:
// frame gather, RandomHorizontalFlip, skimage.transform.rotate(frame, angle, preserve_range=True) as DESIGN states it (bilinear,
// constant 0 outside, the clip to the frame's own minimum), ToTensor(scale=True), Normalize(0.5, 0.5), collate, split and the mask
// multiplies, from the resident uint8 store in ONE launch.  A rotated pixel is no byte, so the 256-entry table of the unrotated launch
// does not apply: the value chain runs per pixel.  Coordinates and interpolation are float64 with fp contract off, operation for
// operation what NumPy does for the restatement (tests/_rotate_ref.py), so the only float32 roundings are upstream's own (.float(),
// .div(255), (v - 0.5) / 0.5, the mask multiply).
// The decomposition is the unrotated kernel's: grid (slot, 256-thread chunks), a thread owns four consecutive output pixels of one
// row for every channel and writes one 16-byte store per plane (consecutive lanes, consecutive groups: contiguous stores).  Per output
// pixel it gathers four source pixels of C bytes with byte loads; at the angles upstream draws (+-10 degrees) the sources of a wave's
// row lie within a few store rows, so the gather hits lines the neighbouring lanes fetched.  No LDS, no atomics.
#include "odehip_internal.h"

namespace odehip {

typedef float f32x4r __attribute__((ext_vector_type(4)));
constexpr int kMaxRotOutputs = 3;

struct VidodeRotateArgs {
  const unsigned char* store;      // [store_frames][H][W][C]
  const unsigned char* frame_min;  // [store_frames]: the smallest byte of each frame
  const int* table;                // [batch] (cos, sin) float64 pairs, [batch] flip flags, then per output frames and factors
  float* out[kMaxRotOutputs];
  int n_frames[kMaxRotOutputs];
  int slot_begin[kMaxRotOutputs];
  int table_off[kMaxRotOutputs];
  long long store_frames;
  int n_outputs, batch, height, width, groups, input_norm;
};

struct Rotation {
  double ca, sa, cx, cy, lift;  // lift: the frame's minimum byte (the clip's lower bound; 0 leaves every value alone)
  float factor;
  int H, W;
  bool flip, norm;
};

// One output pixel (y, x) of the rotated (and before that mirrored) frame, all channels, through upstream's float32 chain.
template <int C>
__device__ __forceinline__ void rotated_pixel(const unsigned char* __restrict__ frame, const Rotation& r, int y, int x, float* q) {
#pragma clang fp contract(off)
  const double rx = (double)x - r.cx, ry = (double)y - r.cy;
  const double sx = r.ca * rx - r.sa * ry + r.cx;
  const double sy = r.sa * rx + r.ca * ry + r.cy;
  // outside (-1, W) x (-1, H) all four sources are outside the frame: exactly 0 (a non-finite angle lands here too, so nothing below
  // converts a value that does not fit an int)
  const bool near = sx > -1.0 && sx < (double)r.W && sy > -1.0 && sy < (double)r.H;
  const double fx = near ? floor(sx) : 0.0, fy = near ? floor(sy) : 0.0;
  const double dx = near ? sx - fx : 0.0, dy = near ? sy - fy : 0.0;
  const int x0 = (int)fx, y0 = (int)fy;
  const int x1 = near ? (int)ceil(sx) : 0, y1 = near ? (int)ceil(sy) : 0;
  const bool in_x0 = near && x0 >= 0, in_x1 = near && x1 >= 0 && x1 < r.W;   // x0 <= W - 1 and y0 <= H - 1 where `near`
  const bool in_y0 = near && y0 >= 0, in_y1 = near && y1 >= 0 && y1 < r.H;
  const int c0 = r.flip ? r.W - 1 - x0 : x0, c1 = r.flip ? r.W - 1 - x1 : x1;   // the mirror comes before the rotation
  const size_t o00 = ((size_t)(in_y0 ? y0 : 0) * r.W + (in_x0 ? c0 : 0)) * C, o01 = ((size_t)(in_y0 ? y0 : 0) * r.W + (in_x1 ? c1 : 0)) * C;
  const size_t o10 = ((size_t)(in_y1 ? y1 : 0) * r.W + (in_x0 ? c0 : 0)) * C, o11 = ((size_t)(in_y1 ? y1 : 0) * r.W + (in_x1 ? c1 : 0)) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const double p00 = in_y0 && in_x0 ? (double)frame[o00 + c] : 0.0, p01 = in_y0 && in_x1 ? (double)frame[o01 + c] : 0.0;
    const double p10 = in_y1 && in_x0 ? (double)frame[o10 + c] : 0.0, p11 = in_y1 && in_x1 ? (double)frame[o11 + c] : 0.0;
    const double top = (1.0 - dx) * p00 + dx * p01;
    const double bottom = (1.0 - dx) * p10 + dx * p11;
    double v = (1.0 - dy) * top + dy * bottom;
    if (v != 0.0 && v < r.lift) v = r.lift;   // clip=True with cval 0 below the frame's range: exact zeros stay
    float f = (float)v / 255.0f;              // .float().div(255)
    if (r.norm) f = (f - 0.5f) / 0.5f;        // Normalize(0.5, 0.5)
    q[c] = f * r.factor;
  }
}

// kAligned: width % 4 == 0, every group is whole and its stores 16-byte aligned.  Otherwise every group takes guarded scalar stores.
template <int C, bool kAligned>
__global__ __launch_bounds__(256) void vidode_rotate_kernel(const VidodeRotateArgs a) {
  const int slot = blockIdx.x;
  int n_frames = a.n_frames[0], begin = 0, off = a.table_off[0];
  float* out = a.out[0];
#pragma unroll
  for (int i = 1; i < kMaxRotOutputs; ++i)
    if (i < a.n_outputs && slot >= a.slot_begin[i]) { n_frames = a.n_frames[i]; begin = a.slot_begin[i]; off = a.table_off[i]; out = a.out[i]; }
  const int local = slot - begin;  // b * T_k + t
  const int b = local / n_frames;
  const int* tbl = a.table + off;
  const long long frame = tbl[local];
  const double* angles = (const double*)a.table;
  Rotation r;
  r.factor = __int_as_float(tbl[a.batch * n_frames + local]);
  r.ca = angles[2 * b];
  r.sa = angles[2 * b + 1];
  r.flip = a.table[4 * a.batch + b] != 0;
  r.norm = a.input_norm != 0;
  r.H = a.height;
  r.W = a.width;
  r.cx = (double)a.width / 2 - 0.5;
  r.cy = (double)a.height / 2 - 0.5;
  const int item = blockIdx.y * 256 + threadIdx.x;
  if (item >= a.height * a.groups) return;
  const int y = item / a.groups, x0 = (item - y * a.groups) * 4;
  const size_t plane = (size_t)a.height * a.width;
  float* dst = out + (size_t)local * C * plane + (size_t)y * a.width + x0;
  const bool known = frame >= 0 && frame < a.store_frames;  // a frame outside the store is not read: its pixels come out NaN
  const unsigned char* src = a.store + (size_t)(known ? frame : 0) * plane * C;
  r.lift = (double)a.frame_min[known ? frame : 0];
  float q[4][C] = {};
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    if (kAligned || x0 + j < a.width) rotated_pixel<C>(src, r, y, x0 + j, q[j]);   // the partial last group stops at the row's end
#pragma unroll
    for (int c = 0; c < C; ++c) q[j][c] = known ? q[j][c] : __builtin_nanf("");
  }
  if (kAligned) {
#pragma unroll
    for (int c = 0; c < C; ++c) *(f32x4r*)(dst + c * plane) = f32x4r{q[0][c], q[1][c], q[2][c], q[3][c]};
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (x0 + j >= a.width) break;
#pragma unroll
      for (int c = 0; c < C; ++c) dst[c * plane + j] = q[j][c];
    }
  }
}

}  // namespace odehip

using namespace odehip;

extern "C" int odehip_vidode_batch_rotated(const unsigned char* store, long long store_frames, int height, int width, int channels,
                                           const unsigned char* frame_min, int input_norm, const int* table, long long table_words,
                                           int batch, int n_outputs, float* const* outs, const int* n_frames, void* stream) {
  ODEHIP_REQUIRE(store && frame_min && table && outs && n_frames, "vidode_batch_rotated: null pointer argument");
  ODEHIP_REQUIRE(store_frames > 0 && store_frames <= 0x7fffffffLL, "vidode_batch_rotated: the store holds 1..2^31-1 frames (got %lld)", store_frames);
  ODEHIP_REQUIRE(height > 0 && width > 0, "vidode_batch_rotated: bad frame size %d x %d", height, width);
  ODEHIP_REQUIRE(channels == 1 || channels == 3, "vidode_batch_rotated: 1 or 3 channels (got %d)", channels);
  ODEHIP_REQUIRE(batch > 0, "vidode_batch_rotated: batch must be positive");
  ODEHIP_REQUIRE(n_outputs >= 1 && n_outputs <= kMaxRotOutputs, "vidode_batch_rotated: 1..%d outputs (got %d)", kMaxRotOutputs, n_outputs);
  ODEHIP_REQUIRE((size_t)table % 8 == 0, "vidode_batch_rotated: the table must be 8-byte aligned (it starts with float64 pairs)");
  VidodeRotateArgs a;
  a.store = store; a.frame_min = frame_min; a.table = table; a.store_frames = store_frames; a.input_norm = input_norm;
  a.n_outputs = n_outputs; a.batch = batch; a.height = height; a.width = width; a.groups = (width + 3) / 4;
  long long slots = 0, words = 5LL * batch;
  for (int k = 0; k < kMaxRotOutputs; ++k) {
    a.out[k] = nullptr; a.n_frames[k] = 1; a.slot_begin[k] = 0; a.table_off[k] = 0;
    if (k >= n_outputs) continue;
    ODEHIP_REQUIRE(outs[k] && n_frames[k] > 0, "vidode_batch_rotated: output %d is null or has no frames", k);
    ODEHIP_REQUIRE((size_t)outs[k] % 16 == 0, "vidode_batch_rotated: output %d must be 16-byte aligned", k);
    ODEHIP_REQUIRE(slots + (long long)batch * n_frames[k] <= 0x3fffffffLL && words + 2LL * batch * n_frames[k] <= 0x7fffffffLL,
                   "vidode_batch_rotated: too many (sample, time) slots");
    a.out[k] = outs[k]; a.n_frames[k] = n_frames[k]; a.slot_begin[k] = (int)slots; a.table_off[k] = (int)words;
    slots += (long long)batch * n_frames[k];
    words += 2LL * batch * n_frames[k];
  }
  ODEHIP_REQUIRE(table_words == words, "vidode_batch_rotated: the table has %lld words, these shapes need %lld", table_words, words);
  const long long chunks = ((long long)height * a.groups + 255) / 256;
  ODEHIP_REQUIRE(chunks <= 65535, "vidode_batch_rotated: frame of %d x %d is too large", height, width);
  const dim3 grid((unsigned)slots, (unsigned)chunks), block(256);
  hipStream_t s = (hipStream_t)stream;
  const bool aligned = width % 4 == 0;
  if (channels == 1 && aligned) hipLaunchKernelGGL((vidode_rotate_kernel<1, true>), grid, block, 0, s, a);
  else if (channels == 1) hipLaunchKernelGGL((vidode_rotate_kernel<1, false>), grid, block, 0, s, a);
  else if (aligned) hipLaunchKernelGGL((vidode_rotate_kernel<3, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((vidode_rotate_kernel<3, false>), grid, block, 0, s, a);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
