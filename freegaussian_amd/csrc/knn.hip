// K9: exact k-nearest-neighbour search over [n,3] fp32 points on a uniform cell grid (the initial Gaussian scales:
// mean distance to the three nearest neighbours, reference freegaussian_model.py:158-162).
//
//   sample   : a strided sample of <= 4096 points is read back; the host takes the 2 % / 98 % quantiles per axis
//              (widened by 5 %, clipped to the sample's own range) as the grid's extent -- a handful of far-away points
//              cannot stretch the grid -- and sizes the cells for a mean occupancy of FG_KNN_OCC points
//   keys     : cell key = (cz gy + cy) gx + cx, coordinates CLAMPED into the grid (outliers land in the border cells)
//   sort     : fg_sort::sort_pairs<uint32_t> on the key bits, values = row numbers
//   cells    : cell_start[c] = first sorted slot of cell c; the points are gathered into sorted order as float4
//              (x, y, z, row number) so that neighbouring lanes share cells and a point is one 16-byte load
//   search   : one lane per query in sorted order.  The 3x3x3 block first: for each of its nine (dy, dz) rows the slots
//              a workgroup's 256 queries need are ONE contiguous stretch of the sorted array (the key is linear in x),
//              staged through LDS in chunks, every lane testing its own three cells out of it.  Then, per lane, rings:
//              while the k-th best squared distance is not below the squared distance to the nearest face of the
//              searched block that is NOT on the grid boundary, scan the next shell of cells.  A face on the boundary
//              bounds nothing (clamped points lie beyond it), so it never stops the search; a block that covers the
//              grid has seen every point.  The result is exact.
// Arithmetic (compiled with -ffp-contract=off; tests/knn_restatement.py states it on the CPU, bit for bit):
//   dx = xq - xp (y, z alike), d2 = (dx dx + dy dy) + dz dz, candidates ordered by (d2, row number), the query's own
//   row excluded by number.
#include <cstdlib>

#include "knn_grid.h"

#ifndef FG_KNN_OCC
#define FG_KNN_OCC 4  // mean points per cell: a starting value, not yet picked by measurement (make knn-occ builds others)
#endif

namespace {

using namespace fg_grid;  // the grid, its keys / cells launches and the sample's extent: knn_grid.h, shared with dbscan.hip

constexpr int KNN_CHUNK = 1024;  // float4 slots of the LDS stage (16 KiB)

// the K best (d2, row) pairs of a lane, ascending, in registers: every index below is a compile-time constant
template <int K>
struct KnnBest {
  float d[K];
  int r[K];
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int j = 0; j < K; ++j) {
      d[j] = INFINITY;
      r[j] = 0x7FFFFFFF;
    }
  }
  __device__ __forceinline__ void test(const float4 q, int self, const float4 p) {
    const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
    const float d2 = (dx * dx + dy * dy) + dz * dz;
    const int row = __float_as_int(p.w);
    if (row == self || !(d2 < d[K - 1] || (d2 == d[K - 1] && row < r[K - 1]))) return;
    bool lt[K];
#pragma unroll
    for (int j = 0; j < K; ++j) lt[j] = d2 < d[j] || (d2 == d[j] && row < r[j]);
#pragma unroll
    for (int j = K - 1; j > 0; --j) {
      d[j] = lt[j - 1] ? d[j - 1] : (lt[j] ? d2 : d[j]);
      r[j] = lt[j - 1] ? r[j - 1] : (lt[j] ? row : r[j]);
    }
    d[0] = lt[0] ? d2 : d[0];
    r[0] = lt[0] ? row : r[0];
  }
};

template <int K>
__global__ void __launch_bounds__(KNN_BLOCK)
knn_search_kernel(int n, KnnGrid gr, const uint32_t* __restrict__ keys, const float4* __restrict__ pts,
                  const int32_t* __restrict__ cell_start, float* __restrict__ dist2_out, int32_t* __restrict__ idx_out) {
  __shared__ float4 stage[KNN_CHUNK];
  __shared__ int s_lo, s_hi;
  const int64_t i = (int64_t)blockIdx.x * KNN_BLOCK + threadIdx.x;
  const bool active = i < n;
  const int gx = gr.g[0], gy = gr.g[1], gz = gr.g[2];
  const float4 q = active ? pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int key = active ? (int)keys[i] : 0;
  const int cx = key % gx, cy = (key / gx) % gy, cz = key / (gx * gy);
  const int self = __float_as_int(q.w);
  KnnBest<K> best;
  best.init();

  // the 3x3x3 block, row by row through LDS
#pragma unroll 1
  for (int o = 0; o < 9; ++o) {
    const int y = cy + o % 3 - 1, z = cz + o / 3 - 1;
    int a = 0x7FFFFFFF, b = 0;  // this lane's slots of the row: [a, b)
    if (active && y >= 0 && y < gy && z >= 0 && z < gz) {
      const int row = (z * gy + y) * gx;
      const int a0 = cell_start[row + max(cx - 1, 0)], b0 = cell_start[row + min(cx + 1, gx - 1) + 1];
      if (b0 > a0) {
        a = a0;
        b = b0;
      }
    }
    if (threadIdx.x == 0) {
      s_lo = 0x7FFFFFFF;
      s_hi = 0;
    }
    __syncthreads();
    int wa = a, wb = b;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      wa = min(wa, __shfl_xor(wa, m));
      wb = max(wb, __shfl_xor(wb, m));
    }
    if (fg::lane_id() == 0 && wb > wa) {
      atomicMin(&s_lo, wa);
      atomicMax(&s_hi, wb);
    }
    __syncthreads();
    const int lo = s_lo, hi = s_hi;  // the stretch the workgroup needs (empty: lo > hi)
    for (int c = lo; c < hi; c += KNN_CHUNK) {
      const int cnt = min(KNN_CHUNK, hi - c);
      __syncthreads();  // (the previous chunk has been read; first round: s_lo / s_hi have been read)
      for (int t = threadIdx.x; t < cnt; t += KNN_BLOCK) stage[t] = pts[c + t];
      __syncthreads();
      const int j1 = min(b, c + cnt);
      for (int j = max(a, c); j < j1; ++j) best.test(q, self, stage[j - c]);
    }
    __syncthreads();
  }
  if (!active) return;

  // rings: the searched block is [c - R, c + R] per axis, clipped to the grid
  for (int R = 1;; ++R) {
    // squared distance to the nearest face of the block that is not on the grid boundary (none left: all points seen)
    float bound = INFINITY;
    if (cx - R > 0) bound = fminf(bound, q.x - (gr.lo[0] + (float)(cx - R) * gr.h[0]));
    if (cx + R < gx - 1) bound = fminf(bound, (gr.lo[0] + (float)(cx + R + 1) * gr.h[0]) - q.x);
    if (cy - R > 0) bound = fminf(bound, q.y - (gr.lo[1] + (float)(cy - R) * gr.h[1]));
    if (cy + R < gy - 1) bound = fminf(bound, (gr.lo[1] + (float)(cy + R + 1) * gr.h[1]) - q.y);
    if (cz - R > 0) bound = fminf(bound, q.z - (gr.lo[2] + (float)(cz - R) * gr.h[2]));
    if (cz + R < gz - 1) bound = fminf(bound, (gr.lo[2] + (float)(cz + R + 1) * gr.h[2]) - q.z);
    if (!(bound < INFINITY)) break;  // (also what ends the search of a row whose distances are not numbers)
    bound = fmaxf(bound - gr.slack, 0.f);
    if (best.d[K - 1] < bound * bound) break;
    // the shell R + 1: whole x-runs on the rows of its rim, the two end cells on the rows inside
    const int S = R + 1;
    // (dy, dz clipped to the grid up front: a one-cell axis costs one iteration, not 2 S + 1 skipped ones)
    for (int dz = max(-S, -cz); dz <= min(S, gz - 1 - cz); ++dz) {
      for (int dy = max(-S, -cy); dy <= min(S, gy - 1 - cy); ++dy) {
        const int row = ((cz + dz) * gy + (cy + dy)) * gx;
        if (abs(dy) == S || abs(dz) == S) {
          const int j1 = cell_start[row + min(cx + S, gx - 1) + 1];
          for (int j = cell_start[row + max(cx - S, 0)]; j < j1; ++j) best.test(q, self, pts[j]);
        } else {
          if (cx - S >= 0) {
            const int j1 = cell_start[row + cx - S + 1];
            for (int j = cell_start[row + cx - S]; j < j1; ++j) best.test(q, self, pts[j]);
          }
          if (cx + S < gx) {
            const int j1 = cell_start[row + cx + S + 1];
            for (int j = cell_start[row + cx + S]; j < j1; ++j) best.test(q, self, pts[j]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    dist2_out[(int64_t)self * K + j] = best.d[j];
    if (idx_out) idx_out[(int64_t)self * K + j] = best.r[j];
  }
}

// the grid from the sample (host): robust extent per axis, cells of ~FG_KNN_OCC points, an axis thinner than a cell = one cell
KnnGrid knn_plan_grid(int64_t n, const float* sample, int count, float* v /*[count] scratch*/) {
  double lo[3], ext[3];
  knn_extent(sample, count, v, lo, ext);
  const double target = std::max<double>(1.0, (double)n / FG_KNN_OCC);
  bool on[3] = {ext[0] > 0.0, ext[1] > 0.0, ext[2] > 0.0};
  double h = 0.0;
  for (int round = 0; round < 3; ++round) {
    int m = 0;
    double vol = 1.0;
    for (int a = 0; a < 3; ++a)
      if (on[a]) {
        ++m;
        vol *= ext[a];
      }
    if (!m) break;
    h = std::pow(vol / target, 1.0 / m);
    bool dropped = false;
    for (int a = 0; a < 3; ++a)
      if (on[a] && ext[a] < h) {
        on[a] = false;
        dropped = true;
      }
    if (!dropped) break;
  }
  KnnGrid gr;
  for (int a = 0; a < 3; ++a) {
    int g = 1;
    if (on[a] && h > 0.0) g = (int)std::min<double>(KNN_MAX_DIM, std::max(1.0, std::floor(ext[a] / h)));
    gr.g[a] = g;
  }
  while ((double)gr.g[0] * gr.g[1] * gr.g[2] > target) {  // (floor above: a guard, not the rule)
    int a = gr.g[0] >= gr.g[1] ? (gr.g[0] >= gr.g[2] ? 0 : 2) : (gr.g[1] >= gr.g[2] ? 1 : 2);
    if (gr.g[a] <= 1) break;
    --gr.g[a];
  }
  knn_finish_grid(gr, lo, ext);
  return gr;
}

struct KnnWorkspace {
  size_t sample, keys, order, pts, cell_start, sort, total;
};

KnnWorkspace knn_layout(int64_t n) {
  using fg_sort::align256;
  if (n < 0) n = 0;
  KnnWorkspace w;
  size_t at = 0;
  w.sample = at, at += align256((size_t)KNN_SAMPLE * 3 * sizeof(float));
  w.keys = at, at += align256((size_t)n * 4);
  w.order = at, at += align256((size_t)n * 4);
  w.pts = at, at += align256((size_t)n * 16);
  w.cell_start = at, at += align256(((size_t)n + 2) * 4);  // cells <= max(1, n / FG_KNN_OCC)
  w.sort = at, at += fg_sort::workspace_bytes<uint32_t>(n);
  w.total = at;
  return w;
}

}  // namespace

// Test / measurement hook (not in the public header): the grid fg_knn plans from `count` <= 4096 sampled rows (HOST pointer;
// fg_knn samples rows floor(s n / count)).  out_f[10] = lo[3], h[3], inv[3], slack; out_i[4] = g[3], FG_KNN_OCC.
extern "C" int fg_debug_knn_grid(int64_t n, const float* sample_host, int count, float* out_f, int32_t* out_i) {
  if (n < 1 || !sample_host || count < 1 || count > KNN_SAMPLE || !out_f || !out_i) return FG_ERR_INVALID_ARG;
  float* v = static_cast<float*>(std::malloc((size_t)count * sizeof(float)));
  if (!v) return FG_ERR_LAUNCH;
  const KnnGrid gr = knn_plan_grid(n, sample_host, count, v);
  std::free(v);
  for (int a = 0; a < 3; ++a) {
    out_f[a] = gr.lo[a];
    out_f[3 + a] = gr.h[a];
    out_f[6 + a] = gr.inv[a];
    out_i[a] = gr.g[a];
  }
  out_f[9] = gr.slack;
  out_i[3] = FG_KNN_OCC;
  return FG_OK;
}

extern "C" size_t fg_knn_workspace_bytes(int64_t n) { return knn_layout(n).total; }

extern "C" int fg_knn(int64_t n, const float* xyz, int k, float* dist2_out, int32_t* idx_out, void* workspace,
                      size_t workspace_bytes, fg_stream_t stream) {
  if (n < 0 || k < 1 || k > FG_KNN_MAX_K) return FG_ERR_INVALID_ARG;
  if (n == 0) return FG_OK;
  if (n <= k || n >= ((int64_t)1 << 31)) return FG_ERR_INVALID_ARG;
  if (!xyz || !dist2_out || !workspace) return FG_ERR_INVALID_ARG;
  const KnnWorkspace w = knn_layout(n);
  if (workspace_bytes < w.total) return FG_ERR_INVALID_ARG;
  hipStream_t s = fg_hip_stream(stream);
  char* ws = static_cast<char*>(workspace);
  float* sample = reinterpret_cast<float*>(ws + w.sample);
  uint32_t* keys = reinterpret_cast<uint32_t*>(ws + w.keys);
  uint32_t* order = reinterpret_cast<uint32_t*>(ws + w.order);
  float4* pts = reinterpret_cast<float4*>(ws + w.pts);
  int32_t* cell_start = reinterpret_cast<int32_t*>(ws + w.cell_start);

  // the one read-back of the call: the sample that sizes the grid
  const int count = (int)std::min<int64_t>(n, KNN_SAMPLE);
  // (heap, not 64 KB of the caller's stack: a C host may call from a thread with a small one)
  float* host = static_cast<float*>(std::malloc((size_t)count * 4 * sizeof(float)));
  if (!host) return FG_ERR_LAUNCH;
  const bool read_back = knn_read_sample(n, count, xyz, sample, host, s);
  KnnGrid gr = {};
  if (read_back) gr = knn_plan_grid(n, host, count, host + (size_t)count * 3);
  std::free(host);
  if (!read_back) return FG_ERR_LAUNCH;
  const int nb = (int)((n + KNN_BLOCK - 1) / KNN_BLOCK);
  const int rc = knn_build_cells(n, gr, xyz, keys, order, pts, cell_start, ws + w.sort, workspace_bytes - w.sort, s);
  if (rc != FG_OK) return rc;
#define FG_KNN_SEARCH(KK)                                                                                          \
  case KK:                                                                                                         \
    hipLaunchKernelGGL((knn_search_kernel<KK>), dim3(nb), dim3(KNN_BLOCK), 0, s, (int)n, gr, keys, pts, cell_start, \
                       dist2_out, idx_out);                                                                        \
    break
  switch (k) {
    FG_KNN_SEARCH(1);
    FG_KNN_SEARCH(2);
    FG_KNN_SEARCH(3);
    FG_KNN_SEARCH(4);
    FG_KNN_SEARCH(5);
    FG_KNN_SEARCH(6);
    FG_KNN_SEARCH(7);
    FG_KNN_SEARCH(8);
  }
#undef FG_KNN_SEARCH
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}
