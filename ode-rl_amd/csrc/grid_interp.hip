// grid_interp.hip -- fixed-grid solvers on an internal grid (torchdiffeq 0.2.1: options={"grid_constructor": fn} / "step_size",
// _impl/solvers.py FixedGridODESolver.integrate): the solver walks a grid of G points of the caller's choosing and the T requested
// times are filled by linear interpolation between the two grid states around them.  The trajectory walks are not touched: they run
// on the grid as on any time array, into a (G, B, C, 16, 16) buffer, and the two launches of this file do the rest.
//
//   emit table (host)   the walk of `integrate` over the grid intervals (t0, t1) = (grid[n], grid[n+1]), in float64:
//                         j = 1;  for n = 0 .. G-2:  first[n] = j;  while j < T and t1 >= t[j]:  emit j from interval n;  j += 1
//                       first[G-1] = T.  Output j of interval n is an exact hit if t[j] == t1 (solution[j] = y1, no arithmetic), else
//                       slope[j] = fl32((t[j] - t0) / (t1 - t0)).  An interval emits no output, one, or several.
//   forward emit        out[0] = Y[0];  out[j] = Y[n+1] (exact hit)  or  Y[n] + slope[j] * (Y[n+1] - Y[n])   (n = interval[j])
//                       difference, product, sum: three roundings, contraction off -- torch's own expression order.
//   backward scatter    written as a gather per grid point, so the order of every sum is fixed and there are no atomics:
//                         g_grid[n] = [n == 0] g_out[0] + sum_{j in interval n-1} w1_j g_out[j] + sum_{j in interval n} w0_j g_out[j]
//                       (w1, w0) = (1, 0) for an exact hit -- the w0 term is then left out, not multiplied by zero --, else
//                       (slope, 1 - slope) with 1 - slope in fp32; j ascending, explicit fmas.
//
// Both launches stream 16 bytes per lane: grid (x, frames), every workgroup strides over the state's quads of one frame.  The table
// ({first[G], interval[T], exact[T]} ints, slope[T] floats, each array padded to 16 bytes) travels in one staged upload into memory
// of the caller.
#include <vector>

#include "persist.h"

namespace odehip {

typedef float f32x4g __attribute__((ext_vector_type(4)));

constexpr int kGridThreads = 256;
constexpr int kGridMaxPoints = 4096;   // the fixed-grid drivers' own limit on the points of a time array

static inline size_t pad4(size_t n) { return (n + 3) / 4 * 4; }

struct GridTable {   // views into the device table
  const int* first;
  const int* interval;
  const int* exact;
  const float* slope;
};

static size_t grid_table_words(int n_grid, int n_times) { return pad4((size_t)n_grid) + 3 * pad4((size_t)n_times); }

// grid (x, n_times)
__global__ __launch_bounds__(kGridThreads) void grid_emit_kernel(const float* __restrict__ states, float* __restrict__ out, GridTable tb,
                                                                 long long quads) {
#pragma clang fp contract(off)
  const int j = blockIdx.y;
  const f32x4g* lo = (const f32x4g*)states;
  bool copy = true;
  float s = 0.0f;
  if (j > 0) {
    const int n = tb.interval[j];
    copy = tb.exact[j] != 0;
    s = tb.slope[j];
    lo += (long long)(copy ? n + 1 : n) * quads;
  }
  const f32x4g* const hi = lo + quads;   // read only when interpolating: interval n has a state n + 1
  f32x4g* const dst = (f32x4g*)out + (long long)j * quads;
  const long long step = (long long)gridDim.x * kGridThreads;
  for (long long q = (long long)blockIdx.x * kGridThreads + threadIdx.x; q < quads; q += step) {
    f32x4g r = lo[q];
    if (!copy) {
      const f32x4g y1 = hi[q];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float d = y1[i] - r[i];
        const float p = s * d;
        r[i] = r[i] + p;
      }
    }
    dst[q] = r;
  }
}

// grid (x, n_grid)
__global__ __launch_bounds__(kGridThreads) void grid_scatter_kernel(const float* __restrict__ grad_out, float* __restrict__ grad_grid,
                                                                    GridTable tb, int n_grid, long long quads) {
#pragma clang fp contract(off)
  const int n = blockIdx.y;
  // outputs of the interval that ENDS at this grid point [a0, a1) and of the one that STARTS here [a1, a2)
  const int a1 = tb.first[n];
  const int a0 = n > 0 ? tb.first[n - 1] : a1;
  const int a2 = n + 1 < n_grid ? tb.first[n + 1] : a1;
  const f32x4g* const g = (const f32x4g*)grad_out;
  f32x4g* const dst = (f32x4g*)grad_grid + (long long)n * quads;
  const long long step = (long long)gridDim.x * kGridThreads;
  for (long long q = (long long)blockIdx.x * kGridThreads + threadIdx.x; q < quads; q += step) {
    f32x4g acc = {0.0f, 0.0f, 0.0f, 0.0f};
    if (n == 0) acc = g[q];
    for (int j = a0; j < a1; ++j) {
      const f32x4g v = g[(long long)j * quads + q];
      const float w1 = tb.exact[j] ? 1.0f : tb.slope[j];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(w1, v[i], acc[i]);
    }
    for (int j = a1; j < a2; ++j) {
      if (tb.exact[j]) continue;   // solution[j] = y1: nothing flows to this interval's start
      const f32x4g v = g[(long long)j * quads + q];
      const float w0 = 1.0f - tb.slope[j];
#pragma unroll
      for (int i = 0; i < 4; ++i) acc[i] = fmaf(w0, v[i], acc[i]);
    }
    dst[q] = acc;
  }
}

// Everything both launches refuse before anything is enqueued; 0 or ODEHIP_EINVAL (message set)
static int check_grid_call(const char* who, const void* src, const void* dst, const int* first, const float* slope, const int* exact,
                           int n_grid, int n_times, long long state_floats, const void* table_dev, size_t table_bytes) {
  ODEHIP_REQUIRE(src && dst && first && slope && exact && table_dev, "%s: null pointer", who);
  ODEHIP_REQUIRE(n_times >= 1 && n_grid >= 1 && n_times <= kGridMaxPoints && n_grid <= kGridMaxPoints,
                 "%s: bad sizes (grid of %d points, %d output times; at most %d each)", who, n_grid, n_times, kGridMaxPoints);
  ODEHIP_REQUIRE(n_grid >= 2 || n_times == 1, "%s: a grid of %d point cannot serve %d output times", who, n_grid, n_times);
  ODEHIP_REQUIRE(state_floats >= 4 && state_floats % 4 == 0, "%s: the state must hold a positive multiple of 4 floats (got %lld)", who,
                 state_floats);
  ODEHIP_REQUIRE(((uintptr_t)src | (uintptr_t)dst | (uintptr_t)table_dev) % 16 == 0, "%s: pointers must be 16-byte aligned", who);
  ODEHIP_REQUIRE(table_bytes >= grid_table_words(n_grid, n_times) * 4, "%s: the table memory holds %zu bytes, %zu are needed", who,
                 table_bytes, grid_table_words(n_grid, n_times) * 4);
  // the table must cover the T outputs: first[0] = 1, non-decreasing, first[G-1] = T, only the last entry reaches T ... in short,
  // every output 1 .. T-1 lies in exactly one of the G-1 intervals
  ODEHIP_REQUIRE(first[0] == 1 && first[n_grid - 1] == n_times, "%s: the emit table does not cover the %d outputs (first[0] = %d, first[%d] = %d)",
                 who, n_times, first[0], n_grid - 1, first[n_grid - 1]);
  for (int n = 1; n < n_grid; ++n)
    ODEHIP_REQUIRE(first[n] >= first[n - 1], "%s: the emit table is not monotone at interval %d", who, n);
  for (int j = 1; j < n_times; ++j)
    ODEHIP_REQUIRE(exact[j] || (slope[j] >= 0.0f && slope[j] <= 1.0f), "%s: slope[%d] = %g lies outside [0, 1]", who, j, (double)slope[j]);
  return ODEHIP_OK;
}

// host image of the device table -> uploaded in one piece; the views into the device copy are returned in `tb`
static int upload_grid_table(const int* first, const float* slope, const int* exact, int n_grid, int n_times, void* table_dev, GridTable* tb,
                             hipStream_t stream) {
  const size_t gp = pad4((size_t)n_grid), tp = pad4((size_t)n_times);
  std::vector<int> host(gp + 3 * tp, 0);
  int* const h_first = host.data();
  int* const h_interval = h_first + gp;
  int* const h_exact = h_interval + tp;
  float* const h_slope = (float*)(h_exact + tp);
  for (int n = 0; n < n_grid; ++n) h_first[n] = first[n];
  for (int n = 0; n + 1 < n_grid; ++n)
    for (int j = first[n]; j < first[n + 1]; ++j) h_interval[j] = n;
  h_exact[0] = 1;
  for (int j = 1; j < n_times; ++j) {
    h_exact[j] = exact[j] ? 1 : 0;
    h_slope[j] = slope[j];
  }
  int* const d = (int*)table_dev;
  tb->first = d;
  tb->interval = d + gp;
  tb->exact = d + gp + tp;
  tb->slope = (const float*)(d + gp + 2 * tp);
  return staged_upload(table_dev, host.data(), host.size() * sizeof(int), stream);
}

// workgroups along x: enough to cover the state once, capped so that the whole launch stays near 4096 workgroups (the rest strides)
static unsigned grid_blocks_x(long long quads, int frames) {
  long long want = (quads + kGridThreads - 1) / kGridThreads;
  long long cap = 4096 / frames;
  if (cap < 1) cap = 1;
  return (unsigned)(want < cap ? want : cap);
}

}  // namespace odehip

using namespace odehip;

extern "C" size_t odehip_grid_table_bytes(int n_grid, int n_times) {
  if (n_grid < 1 || n_times < 1) return 0;
  return grid_table_words(n_grid, n_times) * 4;
}

extern "C" int odehip_grid_emit_table(const double* grid, int n_grid, const double* t, int n_times, int* first, float* slope, int* exact) {
  ODEHIP_REQUIRE(grid && t && first && slope && exact, "grid_emit_table: null pointer");
  ODEHIP_REQUIRE(n_times >= 1 && n_grid >= 1, "grid_emit_table: bad sizes (grid of %d points, %d output times)", n_grid, n_times);
  ODEHIP_REQUIRE(n_grid >= 2 || n_times == 1, "grid_emit_table: a grid of %d point cannot serve %d output times", n_grid, n_times);
  for (int n = 1; n < n_grid; ++n)
    ODEHIP_REQUIRE(grid[n] > grid[n - 1], "grid_emit_table: the grid must be strictly increasing (grid[%d]=%g, grid[%d]=%g)", n - 1,
                   grid[n - 1], n, grid[n]);
  for (int j = 1; j < n_times; ++j)
    ODEHIP_REQUIRE(t[j] > t[j - 1], "grid_emit_table: t must be strictly increasing (t[%d]=%g, t[%d]=%g)", j - 1, t[j - 1], j, t[j]);
  ODEHIP_REQUIRE(grid[0] == t[0] && grid[n_grid - 1] == t[n_times - 1],
                 "grid_emit_table: the grid must start at t[0] and end at t[-1] (grid %g .. %g, t %g .. %g)", grid[0], grid[n_grid - 1], t[0],
                 t[n_times - 1]);
  slope[0] = 0.0f;
  exact[0] = 1;   // solution[0] = y0
  int j = 1;
  for (int n = 0; n + 1 < n_grid; ++n) {
    first[n] = j;
    const double t0 = grid[n], t1 = grid[n + 1];
    while (j < n_times && t1 >= t[j]) {
      exact[j] = t[j] == t1;
      slope[j] = exact[j] ? 1.0f : (float)((t[j] - t0) / (t1 - t0));
      ++j;
    }
  }
  first[n_grid - 1] = j;   // == n_times: the last interval ends at t[-1]
  return ODEHIP_OK;
}

extern "C" int odehip_grid_emit(const float* grid_states, float* out, const int* first, const float* slope, const int* exact, int n_grid,
                                int n_times, long long state_floats, void* table_dev, size_t table_bytes, void* stream) {
  if (int rc = check_grid_call("grid_emit", grid_states, out, first, slope, exact, n_grid, n_times, state_floats, table_dev, table_bytes))
    return rc;
  GridTable tb;
  if (int rc = upload_grid_table(first, slope, exact, n_grid, n_times, table_dev, &tb, (hipStream_t)stream)) return rc;
  const long long quads = state_floats / 4;
  hipLaunchKernelGGL(grid_emit_kernel, dim3(grid_blocks_x(quads, n_times), (unsigned)n_times), dim3(kGridThreads), 0, (hipStream_t)stream,
                     grid_states, out, tb, quads);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}

extern "C" int odehip_grid_scatter(const float* grad_out, float* grad_grid, const int* first, const float* slope, const int* exact,
                                   int n_grid, int n_times, long long state_floats, void* table_dev, size_t table_bytes, void* stream) {
  if (int rc = check_grid_call("grid_scatter", grad_out, grad_grid, first, slope, exact, n_grid, n_times, state_floats, table_dev, table_bytes))
    return rc;
  GridTable tb;
  if (int rc = upload_grid_table(first, slope, exact, n_grid, n_times, table_dev, &tb, (hipStream_t)stream)) return rc;
  const long long quads = state_floats / 4;
  hipLaunchKernelGGL(grid_scatter_kernel, dim3(grid_blocks_x(quads, n_grid), (unsigned)n_grid), dim3(kGridThreads), 0, (hipStream_t)stream,
                     grad_out, grad_grid, tb, n_grid, quads);
  ODEHIP_CHECK_HIP(hipGetLastError());
  return ODEHIP_OK;
}
