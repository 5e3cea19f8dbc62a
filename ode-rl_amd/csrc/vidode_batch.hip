// vidode_batch.hip -- the training batches of upstream Vid-ODE assembled on the device: what its
// VideoDataset.__getitem__ (frame gather, RandomHorizontalFlip, ToTensor(scale=True), Normalize(0.5, 0.5)), video_collate_fn,
// split_and_subsample_batch and the mask multiplies of utils.get_next_batch produce, from clips that stay resident in HBM as uint8.
// A table-driven gather: the host has done the sampling (which frame of the store each (sample, time) slot shows, with which mask
// value, mirrored or not) and this launch does the bytes: per slot one H x W x C channel-last uint8 frame becomes C float32 planes.
// A thread owns four consecutive pixels of one row for every channel: one 4*C-byte load, 4*C lookups in the 256-entry table of
// ToTensor/Normalize results (float32 values computed on the host with upstream's own operations, so nothing is rounded here but the
// one multiply), C 16-byte stores -- the NHWC -> NCHW transposition happens in registers.  Lanes of a wave cover consecutive
// groups of a row, so both the load (4*C bytes per lane) and each plane's store (16 bytes per lane) are contiguous across the wave.
// No LDS, no atomics, one launch for all outputs.  HBM-bound on the stores: 4 bytes written per byte read.
#include "odehip_internal.h"

namespace odehip {

typedef float f32x4 __attribute__((ext_vector_type(4)));
constexpr int kMaxBatchOutputs = 3;

struct VidodeBatchArgs {
  const unsigned char* store;  // [store_frames][H][W][C]
  const float* lut;            // [256]
  const int* table;            // [batch] flip flags, then per output [batch * T_k] frames and [batch * T_k] float factors
  float* out[kMaxBatchOutputs];
  int n_frames[kMaxBatchOutputs];   // T_k
  int slot_begin[kMaxBatchOutputs]; // first (sample, time) slot of output k in blockIdx.x
  int table_off[kMaxBatchOutputs];  // word offset of output k's frames in `table`
  long long store_frames;
  int n_outputs, batch, height, width, groups;  // groups = ceil(width / 4)
};

// kAligned: width % 4 == 0, so every group of every row is whole and 4*C-byte / 16-byte aligned on either side.  Otherwise rows
// start at any byte (and any float), and every group takes the guarded per-pixel form, the partial last group of a row included.
template <int C, bool kAligned>
__global__ __launch_bounds__(256) void vidode_batch_kernel(const VidodeBatchArgs a) {
  const int slot = blockIdx.x;
  int n_frames = a.n_frames[0], begin = 0, off = a.table_off[0];
  float* out = a.out[0];
#pragma unroll
  for (int i = 1; i < kMaxBatchOutputs; ++i)  // which output the slot belongs to (static indices: the arguments stay in SGPRs)
    if (i < a.n_outputs && slot >= a.slot_begin[i]) { n_frames = a.n_frames[i]; begin = a.slot_begin[i]; off = a.table_off[i]; out = a.out[i]; }
  const int local = slot - begin;  // b * T_k + t: the slot's row in the tables and its frame in the output
  const int b = local / n_frames;
  const int* tbl = a.table + off;
  const long long frame = tbl[local];
  const float factor = __int_as_float(tbl[a.batch * n_frames + local]);
  const bool flip = a.table[b] != 0;
  const int item = blockIdx.y * 256 + threadIdx.x;
  if (item >= a.height * a.groups) return;
  const int r = item / a.groups, x0 = (item - r * a.groups) * 4;
  const size_t plane = (size_t)a.height * a.width;
  float* dst = out + (size_t)local * C * plane + (size_t)r * a.width + x0;
  const bool known = frame >= 0 && frame < a.store_frames;  // a frame outside the store is not read: its pixels come out NaN
  const unsigned char* row = a.store + ((size_t)(known ? frame : 0) * a.height + r) * a.width * C;
  if (kAligned) {
    const int xs = flip ? a.width - 4 - x0 : x0;  // the mirrored group, read forwards and reversed below
    unsigned int w[C];
#pragma unroll
    for (int i = 0; i < C; ++i) w[i] = ((const unsigned int*)(row + (size_t)xs * C))[i];
#pragma unroll
    for (int c = 0; c < C; ++c) {
      float q[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int byte = j * C + c;
        const unsigned int v = (w[byte >> 2] >> ((byte & 3) * 8)) & 0xffu;
        q[j] = known ? a.lut[v] * factor : __builtin_nanf("");
      }
      *(f32x4*)(dst + c * plane) = flip ? f32x4{q[3], q[2], q[1], q[0]} : f32x4{q[0], q[1], q[2], q[3]};
    }
  } else {
    for (int j = 0; j < 4 && x0 + j < a.width; ++j) {
      const int xs = flip ? a.width - 1 - (x0 + j) : x0 + j;
#pragma unroll
      for (int c = 0; c < C; ++c) dst[c * plane + j] = known ? a.lut[row[(size_t)xs * C + c]] * factor : __builtin_nanf("");
    }
  }
}

}  // namespace odehip

using namespace odehip;

extern "C" int odehip_vidode_batch(const unsigned char* store, long long store_frames, int height, int width, int channels,
                                   const float* lut256, const int* table, long long table_words, int batch, int n_outputs,
                                   float* const* outs, const int* n_frames, void* stream) {
  ODEHIP_REQUIRE(store && lut256 && table && outs && n_frames, "vidode_batch: null pointer argument");
  ODEHIP_REQUIRE(store_frames > 0 && store_frames <= 0x7fffffffLL, "vidode_batch: the store holds 1..2^31-1 frames (got %lld)", store_frames);
  ODEHIP_REQUIRE(height > 0 && width > 0, "vidode_batch: bad frame size %d x %d", height, width);
  ODEHIP_REQUIRE(channels == 1 || channels == 3, "vidode_batch: 1 or 3 channels (got %d)", channels);
  ODEHIP_REQUIRE(batch > 0, "vidode_batch: batch must be positive");
  ODEHIP_REQUIRE(n_outputs >= 1 && n_outputs <= kMaxBatchOutputs, "vidode_batch: 1..%d outputs (got %d)", kMaxBatchOutputs, n_outputs);
  ODEHIP_REQUIRE((size_t)table % 4 == 0 && (size_t)lut256 % 4 == 0, "vidode_batch: misaligned table");
  const bool aligned = width % 4 == 0;
  ODEHIP_REQUIRE(!aligned || (size_t)store % 4 == 0, "vidode_batch: the store must be 4-byte aligned");
  VidodeBatchArgs a;
  a.store = store; a.lut = lut256; a.table = table; a.store_frames = store_frames;
  a.n_outputs = n_outputs; a.batch = batch; a.height = height; a.width = width; a.groups = (width + 3) / 4;
  long long slots = 0, words = batch;
  for (int k = 0; k < kMaxBatchOutputs; ++k) {
    a.out[k] = nullptr; a.n_frames[k] = 1; a.slot_begin[k] = 0; a.table_off[k] = 0;
    if (k >= n_outputs) continue;
    ODEHIP_REQUIRE(outs[k] && n_frames[k] > 0, "vidode_batch: output %d is null or has no frames", k);
    ODEHIP_REQUIRE((size_t)outs[k] % 16 == 0, "vidode_batch: output %d must be 16-byte aligned", k);
    ODEHIP_REQUIRE(slots + (long long)batch * n_frames[k] <= 0x3fffffffLL, "vidode_batch: too many (sample, time) slots");
    a.out[k] = outs[k]; a.n_frames[k] = n_frames[k]; a.slot_begin[k] = (int)slots; a.table_off[k] = (int)words;
    slots += (long long)batch * n_frames[k];
    words += 2LL * batch * n_frames[k];
  }
  ODEHIP_REQUIRE(table_words == words, "vidode_batch: the table has %lld words, these shapes need %lld", table_words, words);
  const long long chunks = ((long long)height * a.groups + 255) / 256;
  ODEHIP_REQUIRE(chunks <= 65535, "vidode_batch: frame of %d x %d is too large", height, width);
  const dim3 grid((unsigned)slots, (unsigned)chunks), block(256);
  hipStream_t s = (hipStream_t)stream;
  if (channels == 1 && aligned) hipLaunchKernelGGL((vidode_batch_kernel<1, true>), grid, block, 0, s, a);
  else if (channels == 1) hipLaunchKernelGGL((vidode_batch_kernel<1, false>), grid, block, 0, s, a);
  else if (aligned) hipLaunchKernelGGL((vidode_batch_kernel<3, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((vidode_batch_kernel<3, false>), grid, block, 0, s, a);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
