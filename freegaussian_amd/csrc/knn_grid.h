// The uniform cell grid over [n,3] fp32 points that knn.hip (K9) and dbscan.hip (DB) share: the strided sample and its
// robust extent, the clamped cell keys, the cell starts and the gather into sorted order as float4 (x, y, z, row number).
// Each unit sizes its own cells (knn: for a mean occupancy; dbscan: by eps) and hands the counts to knn_finish_grid.
// The sort between the keys and the cells launch is fg_sort::sort_pairs<uint32_t> with iota values (radix_sort.h).
#pragma once
#include <algorithm>
#include <cmath>

#include "radix_sort.h"

namespace fg_grid {

constexpr int KNN_BLOCK = 256;
constexpr int KNN_SAMPLE = 4096;
constexpr int KNN_MAX_DIM = 1024;  // cells per axis: keys stay below 2^30

struct KnnGrid {
  float lo[3], inv[3], h[3];  // cell c of axis a spans [lo + c h, lo + (c + 1) h); inv = 1 / h (0 on a one-cell axis)
  int g[3];
  float slack;  // what the rounding of the cell assignment and of the face positions may amount to
};

static __global__ void __launch_bounds__(KNN_BLOCK)
knn_sample_kernel(int64_t n, int count, const float* __restrict__ xyz, float* __restrict__ sample) {
  const int s = blockIdx.x * KNN_BLOCK + threadIdx.x;
  if (s >= count) return;
  const int64_t i = (int64_t)s * n / count;
  sample[3 * s + 0] = xyz[3 * i + 0];
  sample[3 * s + 1] = xyz[3 * i + 1];
  sample[3 * s + 2] = xyz[3 * i + 2];
}

// (fmaxf drops a NaN: whatever the coordinate, the cell is inside the grid)
__device__ __forceinline__ int knn_cell(float x, float lo, float inv, int g) {
  return (int)fminf(fmaxf(floorf((x - lo) * inv), 0.f), (float)(g - 1));
}

static __global__ void __launch_bounds__(KNN_BLOCK)
knn_keys_kernel(int64_t n, KnnGrid gr, const float* __restrict__ xyz, uint32_t* __restrict__ keys) {
  const int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int cx = knn_cell(xyz[3 * i + 0], gr.lo[0], gr.inv[0], gr.g[0]);
  const int cy = knn_cell(xyz[3 * i + 1], gr.lo[1], gr.inv[1], gr.g[1]);
  const int cz = knn_cell(xyz[3 * i + 2], gr.lo[2], gr.inv[2], gr.g[2]);
  keys[i] = (uint32_t)((cz * gr.g[1] + cy) * gr.g[0] + cx);
}

// slot i: writes the start of every cell in (key[i-1], key[i]] (the last slot: of every cell after its own, too) and
// gathers its point
static __global__ void __launch_bounds__(KNN_BLOCK)
knn_cells_kernel(int64_t n, int cells, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ order,
                 const float* __restrict__ xyz, int32_t* __restrict__ cell_start, float4* __restrict__ pts) {
  const int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int key = (int)keys[i];
  const int prev = i ? (int)keys[i - 1] : -1;
  for (int c = prev + 1; c <= key; ++c) cell_start[c] = (int32_t)i;
  if (i == n - 1)
    for (int c = key + 1; c <= cells; ++c) cell_start[c] = (int32_t)n;
  const uint32_t row = order[i];
  pts[i] = make_float4(xyz[3 * (int64_t)row + 0], xyz[3 * (int64_t)row + 1], xyz[3 * (int64_t)row + 2],
                       __int_as_float((int)row));
}

// the robust extent of the sample (host): per axis the 2 % / 98 % quantiles, widened by 5 %, clipped to the sample's own
// range; a non-finite coordinate counts as 0; an axis without extent gets 0
inline void knn_extent(const float* sample, int count, float* v /*[count] scratch*/, double lo[3], double ext[3]) {
  for (int a = 0; a < 3; ++a) {
    for (int s = 0; s < count; ++s) {
      const float x = sample[3 * s + a];
      v[s] = std::isfinite(x) ? x : 0.f;
    }
    std::sort(v, v + count);
    const double q0 = v[(int)(0.02 * (count - 1))], q1 = v[(int)std::ceil(0.98 * (count - 1))];
    const double pad = 0.05 * (q1 - q0);
    lo[a] = std::max(q0 - pad, (double)v[0]);
    ext[a] = std::min(q1 + pad, (double)v[count - 1]) - lo[a];
    if (!(ext[a] > 0.0) || !std::isfinite(ext[a])) ext[a] = 0.0;
  }
}

// gr.g[] is set: the origin, the cell sides and their inverses in fp32 (an axis whose side degenerates becomes one cell)
inline void knn_finish_grid(KnnGrid& gr, const double lo[3], const double ext[3]) {
  double amax = 0.0;
  for (int a = 0; a < 3; ++a) {
    gr.lo[a] = (float)lo[a];
    gr.h[a] = gr.g[a] > 1 ? (float)(ext[a] / gr.g[a]) : 0.f;
    gr.inv[a] = gr.g[a] > 1 ? (float)(gr.g[a] / ext[a]) : 0.f;
    if (!std::isfinite(gr.inv[a]) || !(gr.h[a] > 0.f)) {
      gr.g[a] = 1;
      gr.h[a] = gr.inv[a] = 0.f;
    }
    amax = std::max(amax, std::fabs(lo[a]) + std::fabs(lo[a] + ext[a]) + ext[a]);
  }
  // x - lo, the product with inv, lo + c h and the face distance each round once: a few ulps of the coordinates' size
  gr.slack = (float)(1e-6 * amax);
}

// the launches from the planned grid to the sorted points: keys, sort, cell starts + gather.  `sort_ws` is
// fg_sort::workspace_bytes<uint32_t>(n) bytes; cell_start holds cells + 1 words.
inline int knn_build_cells(int64_t n, const KnnGrid& gr, const float* xyz, uint32_t* keys, uint32_t* order, float4* pts,
                           int32_t* cell_start, void* sort_ws, size_t sort_ws_bytes, hipStream_t s) {
  const int cells = gr.g[0] * gr.g[1] * gr.g[2];
  const int nb = (int)((n + KNN_BLOCK - 1) / KNN_BLOCK);
  hipLaunchKernelGGL(knn_keys_kernel, dim3(nb), dim3(KNN_BLOCK), 0, s, n, gr, xyz, keys);
  FG_RETURN_IF_LAUNCH_FAILED();
  int end_bit = 1;  // (one cell: still one pass, it numbers the rows)
  while (end_bit < 32 && ((int64_t)1 << end_bit) < cells) ++end_bit;
  const int rc = fg_sort::sort_pairs<uint32_t>(n, keys, order, end_bit, sort_ws, sort_ws_bytes, s, nullptr,
                                               /*iota_vals=*/true);
  if (rc != FG_OK) return rc;
  hipLaunchKernelGGL(knn_cells_kernel, dim3(nb), dim3(KNN_BLOCK), 0, s, n, cells, keys, order, xyz, cell_start, pts);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

// the one read-back of a call: `count` = min(n, KNN_SAMPLE) strided rows into host[3 count] (the stream is synchronised)
inline bool knn_read_sample(int64_t n, int count, const float* xyz, float* sample_dev, float* host, hipStream_t s) {
  hipLaunchKernelGGL(knn_sample_kernel, dim3((count + KNN_BLOCK - 1) / KNN_BLOCK), dim3(KNN_BLOCK), 0, s, n, count, xyz,
                     sample_dev);
  return hipGetLastError() == hipSuccess &&
         hipMemcpyAsync(host, sample_dev, (size_t)count * 3 * sizeof(float), hipMemcpyDeviceToHost, s) == hipSuccess &&
         hipStreamSynchronize(s) == hipSuccess;
}

}  // namespace fg_grid
