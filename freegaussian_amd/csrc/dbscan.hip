// DB: exact DBSCAN over [n,3] fp32 points (the dynamic Gaussians of stage 2: one mask column per cluster).  The definition
// is stated once, in include/fgraster.h ("DB"); tests/dbscan_restatement.py states it on the CPU.  Compiled with
// -ffp-contract=off: the neighbour predicate d2 <= eps2 is knn.hip's arithmetic, dx = xi - xj, d2 = (dx dx + dy dy) + dz dz.
//
//   grid     : knn_grid.h, shared with knn.hip -- sampled robust extent, CLAMPED cell keys, fg_sort::sort_pairs, cell starts,
//              points gathered in sorted order as float4 (x, y, z, row).  Cell side per axis = max(eps (1 + DB_CELL_SLACK),
//              extent / 1024); while the cell count exceeds max(4 n, 4096) the axis with the most cells loses one (its side
//              grows, it never shrinks below the above).
//   WHY THE 3x3x3 BLOCK IS EXHAUSTIVE.  Per axis the cell of x is clamp(floor(t'(x))), t'(x) = fl(fl(x - lo) inv): every
//              step is monotone in x, so x_i <= x_j gives c_i <= c_j, clamped outliers included.  Two neighbours have
//              fl(dx dx) <= d2 <= eps2 = fl(eps eps) (the sums only add non-negative terms and rounding is monotone), hence a
//              true |x_i - x_j| <= eps (1 + 2^-22) (eps is held to [FG_DBSCAN_MIN_EPS, FG_DBSCAN_MAX_EPS], where eps2 is a
//              normal number).  With t = (x - lo) / h the ideal coordinate, |t' - t| <= 3 * 2^-24 |t| (the subtraction, the
//              product and inv = fl(1 / h) round once each), below 3.7e-4 for |t| <= 2048.  If t_j <= 2048 (and t_i >= -2048):
//              t'_j - t'_i <= eps (1 + 2^-22) / h + 7.4e-4 <= 1 / (1 + DB_CELL_SLACK) + 7.6e-4 < 1, the floors differ by at
//              most 1, and clamping is 1-Lipschitz.  If t_j > 2048 then t_i > 2047 and both clamp to the last cell (g <= 1024);
//              alike at the low end.  So a neighbour lies at most one cell away on every axis.
//   core     : one lane per sorted slot scans the nine three-cell x-runs of its block (each ONE contiguous stretch of the
//              sorted array) and stops counting at min_samples; a wave leaves the loop when all its lanes have.
//   mark     : parent[row] = row; a core row's flag goes into bit 31 of its point's row word (n <= 2^24 leaves it free)
//   union    : one lane per core row, the same scan without the early exit; for every core neighbour with a LOWER row,
//              union(i, j) on parent[]: find both roots (path halving: a non-root's parent only ever moves to a lower row of
//              its own tree), atomicCAS the larger root under the smaller, on failure walk on from what the CAS returned.
//              Lock-free: a failed CAS means another lane's succeeded.  Parents are read and path-halved with relaxed
//              agent-scope atomics (a plain load may be served a stale line while other compute units hook).  Every walk and
//              every retry loop is bounded by n + 1: on excess the lane writes status = 1 and returns.  The final root of a
//              component is its lowest core row; the partition is unique, so the order of the atomics does not matter.
//   roots    : root[row] of every core row (-1 otherwise), in a launch of its own
//   number   : count the roots per 256 rows, exclusive scan of the block counts (one workgroup), number[root] = its rank in
//              row order = the cluster number; K = counts_out[0]
//   label    : core rows take number[root]; a non-core row scans once more for the minimum root among its core neighbours
//              (the lowest root is the lowest cluster number) and takes its number, or -1.
// FG_DBSCAN_STAGED=1 builds the core and union passes with the LDS staging of knn's block phase instead of direct loads (each of
// the nine stretches a workgroup's 256 slots need is staged in chunks, every lane testing its own three cells out of it): a
// measurement build (make dbscan-staged, scripts/dbscan_bench.py).  The product build is the one profiles/dbscan.md decides on.
#include <cstdlib>

#include "knn_grid.h"

#ifndef FG_DBSCAN_STAGED
#define FG_DBSCAN_STAGED 0
#endif

namespace {

using namespace fg_grid;

constexpr double DB_CELL_SLACK = 2e-3;
constexpr int DB_CORE_BIT = (int)0x80000000;
constexpr int DB_ROW_MASK = 0x00FFFFFF;

// the neighbour relation of the definition (a NaN compares false: a non-finite row neighbours nobody, itself included)
__device__ __forceinline__ bool db_near(const float4 q, const float4 p, float eps2) {
  const float dx = q.x - p.x, dy = q.y - p.y, dz = q.z - p.z;
  const float d2 = (dx * dx + dy * dy) + dz * dz;
  return d2 <= eps2;
}

// every point of the 3x3x3 block around the cell `key`, until f returns true
template <class F>
__device__ __forceinline__ void db_scan(const KnnGrid& gr, int key, const int32_t* __restrict__ cell_start,
                                        const float4* __restrict__ pts, F&& f) {
  const int gx = gr.g[0], gy = gr.g[1], gz = gr.g[2];
  const int cx = key % gx, cy = (key / gx) % gy, cz = key / (gx * gy);
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, gx - 1) + 1;
#pragma unroll 1
  for (int o = 0; o < 9; ++o) {
    const int y = cy + o % 3 - 1, z = cz + o / 3 - 1;
    if (y < 0 || y >= gy || z < 0 || z >= gz) continue;
    const int row = (z * gy + y) * gx;
    const int j1 = cell_start[row + x1];
    for (int j = cell_start[row + x0]; j < j1; ++j)
      if (f(pts[j])) return;
  }
}

#if FG_DBSCAN_STAGED
constexpr int DB_CHUNK = 1024;  // float4 slots of the LDS stage (16 KiB)

// db_scan through LDS, as knn's block phase: EVERY thread of the workgroup calls it (`live` false: nothing to visit).  A lane
// whose f returned true visits nothing more but keeps meeting the barriers.
template <class F>
__device__ __forceinline__ void db_scan_staged(const KnnGrid& gr, int key, bool live, const int32_t* __restrict__ cell_start,
                                               const float4* __restrict__ pts, float4* stage, int* s_range, F&& f) {
  const int gx = gr.g[0], gy = gr.g[1], gz = gr.g[2];
  const int cx = key % gx, cy = (key / gx) % gy, cz = key / (gx * gy);
  const int x0 = max(cx - 1, 0), x1 = min(cx + 1, gx - 1) + 1;
#pragma unroll 1
  for (int o = 0; o < 9; ++o) {
    const int y = cy + o % 3 - 1, z = cz + o / 3 - 1;
    int a = 0x7FFFFFFF, b = 0;  // this lane's slots of the row: [a, b)
    if (live && y >= 0 && y < gy && z >= 0 && z < gz) {
      const int row = (z * gy + y) * gx;
      const int a0 = cell_start[row + x0], b0 = cell_start[row + x1];
      if (b0 > a0) {
        a = a0;
        b = b0;
      }
    }
    if (threadIdx.x == 0) {
      s_range[0] = 0x7FFFFFFF;
      s_range[1] = 0;
    }
    __syncthreads();
    int wa = a, wb = b;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      wa = min(wa, __shfl_xor(wa, m));
      wb = max(wb, __shfl_xor(wb, m));
    }
    if (fg::lane_id() == 0 && wb > wa) {
      atomicMin(&s_range[0], wa);
      atomicMax(&s_range[1], wb);
    }
    __syncthreads();
    const int lo = s_range[0], hi = s_range[1];  // the stretch the workgroup needs (empty: lo > hi)
    for (int c = lo; c < hi; c += DB_CHUNK) {
      const int cnt = min(DB_CHUNK, hi - c);
      __syncthreads();  // (the previous chunk has been read; first round: s_range has been read)
      for (int t = threadIdx.x; t < cnt; t += KNN_BLOCK) stage[t] = pts[c + t];
      __syncthreads();
      const int j1 = min(b, c + cnt);
      for (int j = max(a, c); live && j < j1; ++j) live = !f(stage[j - c]);
    }
    __syncthreads();
  }
}
#define DB_SCAN_SHARED            \
  __shared__ float4 stage[DB_CHUNK]; \
  __shared__ int s_range[2]
#define DB_SCAN(live, key, f) db_scan_staged(gr, key, live, cell_start, pts, stage, s_range, f)
#else
#define DB_SCAN_SHARED
#define DB_SCAN(live, key, f) \
  if (live) db_scan(gr, key, cell_start, pts, f)
#endif

__global__ void __launch_bounds__(KNN_BLOCK)
db_core_kernel(int n, KnnGrid gr, float eps2, int min_samples, const uint32_t* __restrict__ keys,
               const float4* __restrict__ pts, const int32_t* __restrict__ cell_start, uint8_t* __restrict__ core_out) {
  DB_SCAN_SHARED;
  const int i = blockIdx.x * KNN_BLOCK + threadIdx.x;
  const bool live = i < n;
  const float4 q = live ? pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  int cnt = 0;
  DB_SCAN(live, live ? (int)keys[i] : 0, [&](const float4 p) {
    cnt += db_near(q, p, eps2) ? 1 : 0;
    return cnt >= min_samples;
  });
  if (live) core_out[__float_as_int(q.w)] = cnt >= min_samples ? 1 : 0;
}

__global__ void __launch_bounds__(KNN_BLOCK)
db_mark_kernel(int n, const uint8_t* __restrict__ core, float4* __restrict__ pts, int32_t* __restrict__ parent) {
  const int i = blockIdx.x * KNN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int row = __float_as_int(pts[i].w);
  parent[row] = row;
  if (core[row]) pts[i].w = __int_as_float(row | DB_CORE_BIT);
}

__device__ __forceinline__ int db_load(const int32_t* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of x's tree, -1 after `bound` steps (status set).  Path halving: parent[x] <- its grandparent.
__device__ int db_find(int32_t* parent, int x, int bound, int32_t* status) {
  for (int it = 0; it < bound; ++it) {
    const int p = db_load(parent + x);
    if (p == x) return x;
    const int gp = db_load(parent + p);
    if (gp != p) __hip_atomic_store(parent + x, gp, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    x = gp;
  }
  *status = 1;
  return -1;
}

// joins the trees of a and b; the common root, or -1 (status set)
__device__ int db_union(int32_t* parent, int a, int b, int bound, int32_t* status) {
  a = db_find(parent, a, bound, status);
  b = db_find(parent, b, bound, status);
  for (int it = 0; it < bound; ++it) {
    if (a < 0 || b < 0) return -1;
    if (a == b) return a;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicCAS(parent + hi, hi, lo);
    if (old == hi) return lo;
    a = db_find(parent, old, bound, status);  // hi was hooked by another lane meanwhile: go on from its new parent
    b = db_find(parent, lo, bound, status);
  }
  *status = 1;
  return -1;
}

__global__ void __launch_bounds__(KNN_BLOCK)
db_union_kernel(int n, KnnGrid gr, float eps2, const uint32_t* __restrict__ keys, const float4* __restrict__ pts,
                const int32_t* __restrict__ cell_start, int32_t* parent, int32_t* status) {
  DB_SCAN_SHARED;
  const int i = blockIdx.x * KNN_BLOCK + threadIdx.x;
  const float4 q = i < n ? pts[i] : make_float4(0.f, 0.f, 0.f, 0.f);
  const int w = __float_as_int(q.w);
  const bool live = i < n && (w & DB_CORE_BIT);
  const int self = w & DB_ROW_MASK;
  int mine = self;  // the last root seen for this row's tree
  DB_SCAN(live, i < n ? (int)keys[i] : 0, [&](const float4 p) {
    const int pw = __float_as_int(p.w);
    const int row = pw & DB_ROW_MASK;
    if (!(pw & DB_CORE_BIT) || row >= self || !db_near(q, p, eps2)) return false;
    if (db_load(parent + row) == mine) return false;  // (already under the same root: the common case in a dense cell)
    mine = db_union(parent, mine, row, n + 1, status);
    return mine < 0;
  });
}

__global__ void __launch_bounds__(KNN_BLOCK)
db_roots_kernel(int n, const uint8_t* __restrict__ core, const int32_t* __restrict__ parent, int32_t* __restrict__ root,
                int32_t* status) {
  const int r = blockIdx.x * KNN_BLOCK + threadIdx.x;
  if (r >= n) return;
  int x = -1;
  if (core[r]) {
    x = r;
    int it = 0;
    for (; it <= n; ++it) {
      const int p = parent[x];
      if (p == x) break;
      x = p;
    }
    if (it > n) {
      *status = 1;
      x = -1;
    }
  }
  root[r] = x;
}

// this thread's rank among the workgroup's flagged threads and (everywhere) their total
__device__ __forceinline__ int db_block_rank(bool flag, int& total) {
  __shared__ int s_wave[KNN_BLOCK / 64];
  const unsigned long long m = __ballot(flag);
  const int lane = fg::lane_id(), wave = threadIdx.x >> 6;
  if (lane == 0) s_wave[wave] = __popcll(m);
  __syncthreads();
  int before = __popcll(m & ((1ull << lane) - 1ull));
  total = 0;
#pragma unroll
  for (int k = 0; k < KNN_BLOCK / 64; ++k) {
    before += k < wave ? s_wave[k] : 0;
    total += s_wave[k];
  }
  return before;
}

__global__ void __launch_bounds__(KNN_BLOCK)
db_count_kernel(int n, const int32_t* __restrict__ root, int32_t* __restrict__ block_sum) {
  const int r = blockIdx.x * KNN_BLOCK + threadIdx.x;
  int total;
  db_block_rank(r < n && root[r] == r, total);
  if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// one workgroup: block_sum[0..nb) -> its exclusive scan in place, the total -> counts_out[0]
__global__ void __launch_bounds__(KNN_BLOCK)
db_scan_kernel(int nb, int32_t* __restrict__ block_sum, int32_t* __restrict__ counts_out) {
  __shared__ int s_tot[KNN_BLOCK];
  const int per = (nb + KNN_BLOCK - 1) / KNN_BLOCK;
  const int b0 = min((int)threadIdx.x * per, nb), b1 = min(b0 + per, nb);
  int sum = 0;
  for (int b = b0; b < b1; ++b) sum += block_sum[b];
  s_tot[threadIdx.x] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    int run = 0;
    for (int t = 0; t < KNN_BLOCK; ++t) {
      const int v = s_tot[t];
      s_tot[t] = run;
      run += v;
    }
    counts_out[0] = run;
  }
  __syncthreads();
  int run = s_tot[threadIdx.x];
  for (int b = b0; b < b1; ++b) {
    const int v = block_sum[b];
    block_sum[b] = run;
    run += v;
  }
}

__global__ void __launch_bounds__(KNN_BLOCK)
db_number_kernel(int n, const int32_t* __restrict__ root, const int32_t* __restrict__ block_sum, int32_t* __restrict__ number) {
  const int r = blockIdx.x * KNN_BLOCK + threadIdx.x;
  const bool is_root = r < n && root[r] == r;
  int total;
  const int rank = db_block_rank(is_root, total);
  if (is_root) number[r] = block_sum[blockIdx.x] + rank;
}

__global__ void __launch_bounds__(KNN_BLOCK)
db_label_kernel(int n, KnnGrid gr, float eps2, const uint32_t* __restrict__ keys, const float4* __restrict__ pts,
                const int32_t* __restrict__ cell_start, const int32_t* __restrict__ root, const int32_t* __restrict__ number,
                int32_t* __restrict__ labels_out) {
  const int i = blockIdx.x * KNN_BLOCK + threadIdx.x;
  if (i >= n) return;
  const float4 q = pts[i];
  const int w = __float_as_int(q.w);
  const int self = w & DB_ROW_MASK;
  int best = 0x7FFFFFFF;
  if (w & DB_CORE_BIT) {
    best = root[self];
  } else {
    db_scan(gr, (int)keys[i], cell_start, pts, [&](const float4 p) {
      const int pw = __float_as_int(p.w);
      if ((pw & DB_CORE_BIT) && db_near(q, p, eps2)) best = min(best, root[pw & DB_ROW_MASK]);
      return false;
    });
  }
  labels_out[self] = best >= 0 && best < n ? number[best] : -1;
}

// the grid from the sample (host): the cells are sized by eps, see the file header
KnnGrid db_plan_grid(int64_t n, float eps, const float* sample, int count, float* v /*[count] scratch*/) {
  double lo[3], ext[3];
  knn_extent(sample, count, v, lo, ext);
  const double side_min = (double)eps * (1.0 + DB_CELL_SLACK);
  KnnGrid gr;
  for (int a = 0; a < 3; ++a) {
    const double side = std::max(side_min, ext[a] / KNN_MAX_DIM);
    gr.g[a] = ext[a] > 0.0 ? (int)std::min<double>(KNN_MAX_DIM, std::max(1.0, std::floor(ext[a] / side))) : 1;
  }
  const double cap = (double)std::max<int64_t>(4 * n, 4096);
  while ((double)gr.g[0] * gr.g[1] * gr.g[2] > cap) {
    int a = gr.g[0] >= gr.g[1] ? (gr.g[0] >= gr.g[2] ? 0 : 2) : (gr.g[1] >= gr.g[2] ? 1 : 2);
    --gr.g[a];  // (the product is above 4096: the largest count is above 1)
  }
  knn_finish_grid(gr, lo, ext);
  return gr;
}

struct DbWorkspace {
  size_t sample, keys, order, pts, cell_start, parent, root, block_sum, sort, total;
};

DbWorkspace db_layout(int64_t n) {
  using fg_sort::align256;
  if (n < 0) n = 0;
  DbWorkspace w;
  size_t at = 0;
  w.sample = at, at += align256((size_t)KNN_SAMPLE * 3 * sizeof(float));
  w.keys = at, at += align256((size_t)n * 4);
  w.order = at, at += align256((size_t)n * 4);  // after the gather: number[]
  w.pts = at, at += align256((size_t)n * 16);
  w.cell_start = at, at += align256(((size_t)std::max<int64_t>(4 * n, 4096) + 2) * 4);
  w.parent = at, at += align256((size_t)n * 4);
  w.root = at, at += align256((size_t)n * 4);
  w.block_sum = at, at += align256(((size_t)(n + KNN_BLOCK - 1) / KNN_BLOCK + 1) * 4);
  w.sort = at, at += fg_sort::workspace_bytes<uint32_t>(n);
  w.total = at;
  return w;
}

}  // namespace

extern "C" size_t fg_dbscan_workspace_bytes(int64_t n) {
  if (n < 1 || n > FG_DBSCAN_MAX_ROWS) return 0;
  return db_layout(n).total;
}

// ev (measurement only): DB_STAGES + 1 events, recorded before the first and after each stage
static int db_run(int64_t n, const float* xyz, float eps, int min_samples, int32_t* labels_out, uint8_t* core_out,
                  int32_t* counts_out, void* workspace, size_t workspace_bytes, fg_stream_t stream, hipEvent_t* ev) {
  if (n < 1 || n > FG_DBSCAN_MAX_ROWS) return FG_ERR_INVALID_ARG;
  if (!(eps > 0.f) || !std::isfinite(eps)) return FG_ERR_INVALID_ARG;
  if (min_samples < 1 || min_samples > FG_DBSCAN_MAX_MIN_SAMPLES) return FG_ERR_INVALID_ARG;
  if (!xyz || !labels_out || !core_out || !counts_out || !workspace) return FG_ERR_INVALID_ARG;
  if (eps < FG_DBSCAN_MIN_EPS || eps > FG_DBSCAN_MAX_EPS) return FG_ERR_UNSUPPORTED;
  const DbWorkspace w = db_layout(n);
  if (workspace_bytes < w.total) return FG_ERR_WORKSPACE;
  hipStream_t s = fg_hip_stream(stream);
  char* ws = static_cast<char*>(workspace);
  float* sample = reinterpret_cast<float*>(ws + w.sample);
  uint32_t* keys = reinterpret_cast<uint32_t*>(ws + w.keys);
  uint32_t* order = reinterpret_cast<uint32_t*>(ws + w.order);
  float4* pts = reinterpret_cast<float4*>(ws + w.pts);
  int32_t* cell_start = reinterpret_cast<int32_t*>(ws + w.cell_start);
  int32_t* parent = reinterpret_cast<int32_t*>(ws + w.parent);
  int32_t* root = reinterpret_cast<int32_t*>(ws + w.root);
  int32_t* block_sum = reinterpret_cast<int32_t*>(ws + w.block_sum);
  int32_t* number = reinterpret_cast<int32_t*>(order);

#define DB_STAGE_DONE(k) \
  if (ev && hipEventRecord(ev[k], s) != hipSuccess) return FG_ERR_LAUNCH
  DB_STAGE_DONE(0);
  // the one read-back of the call: the sample that sizes the grid
  const int count = (int)std::min<int64_t>(n, KNN_SAMPLE);
  float* host = static_cast<float*>(std::malloc((size_t)count * 4 * sizeof(float)));
  if (!host) return FG_ERR_LAUNCH;
  const bool read_back = knn_read_sample(n, count, xyz, sample, host, s);
  KnnGrid gr = {};
  if (read_back) gr = db_plan_grid(n, eps, host, count, host + (size_t)count * 3);
  std::free(host);
  if (!read_back) return FG_ERR_LAUNCH;
  if (hipMemsetAsync(counts_out, 0, 2 * sizeof(int32_t), s) != hipSuccess) return FG_ERR_LAUNCH;
  const int rc = knn_build_cells(n, gr, xyz, keys, order, pts, cell_start, ws + w.sort, workspace_bytes - w.sort, s);
  if (rc != FG_OK) return rc;
  DB_STAGE_DONE(1);

  const int m = (int)n, nb = (m + KNN_BLOCK - 1) / KNN_BLOCK;
  const float eps2 = eps * eps;
  const dim3 grid(nb), block(KNN_BLOCK);
  int32_t* status = counts_out + 1;
  hipLaunchKernelGGL(db_core_kernel, grid, block, 0, s, m, gr, eps2, min_samples, keys, pts, cell_start, core_out);
  FG_RETURN_IF_LAUNCH_FAILED();
  DB_STAGE_DONE(2);
  hipLaunchKernelGGL(db_mark_kernel, grid, block, 0, s, m, core_out, pts, parent);
  FG_RETURN_IF_LAUNCH_FAILED();
  DB_STAGE_DONE(3);
  hipLaunchKernelGGL(db_union_kernel, grid, block, 0, s, m, gr, eps2, keys, pts, cell_start, parent, status);
  FG_RETURN_IF_LAUNCH_FAILED();
  DB_STAGE_DONE(4);
  hipLaunchKernelGGL(db_roots_kernel, grid, block, 0, s, m, core_out, parent, root, status);
  FG_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(db_count_kernel, grid, block, 0, s, m, root, block_sum);
  FG_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(db_scan_kernel, dim3(1), block, 0, s, nb, block_sum, counts_out);
  FG_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(db_number_kernel, grid, block, 0, s, m, root, block_sum, number);
  FG_RETURN_IF_LAUNCH_FAILED();
  DB_STAGE_DONE(5);
  hipLaunchKernelGGL(db_label_kernel, grid, block, 0, s, m, gr, eps2, keys, pts, cell_start, root, number, labels_out);
  FG_RETURN_IF_LAUNCH_FAILED();
  DB_STAGE_DONE(6);
#undef DB_STAGE_DONE
  return FG_OK;
}

extern "C" int fg_dbscan(int64_t n, const float* xyz, float eps, int min_samples, int32_t* labels_out, uint8_t* core_out,
                         int32_t* counts_out, void* workspace, size_t workspace_bytes, fg_stream_t stream) {
  return db_run(n, xyz, eps, min_samples, labels_out, core_out, counts_out, workspace, workspace_bytes, stream, nullptr);
}

// Measurement hook (not in the public header): fg_dbscan with a device event between its stages; the stream is synchronised.
// ms_host[6] = grid (sample, keys, sort, cells), core, mark, union, roots + numbering, labels; staged_out = FG_DBSCAN_STAGED.
extern "C" int fg_debug_dbscan_stages(int64_t n, const float* xyz, float eps, int min_samples, int32_t* labels_out,
                                      uint8_t* core_out, int32_t* counts_out, void* workspace, size_t workspace_bytes,
                                      fg_stream_t stream, float* ms_host, int32_t* staged_out) {
  constexpr int DB_STAGES = 6;
  if (!ms_host || !staged_out) return FG_ERR_INVALID_ARG;
  *staged_out = FG_DBSCAN_STAGED;
  hipEvent_t ev[DB_STAGES + 1];
  int made = 0;
  while (made <= DB_STAGES && hipEventCreate(&ev[made]) == hipSuccess) ++made;
  int rc = made == DB_STAGES + 1 ? FG_OK : FG_ERR_LAUNCH;
  if (rc == FG_OK) rc = db_run(n, xyz, eps, min_samples, labels_out, core_out, counts_out, workspace, workspace_bytes, stream, ev);
  if (rc == FG_OK && hipStreamSynchronize(fg_hip_stream(stream)) != hipSuccess) rc = FG_ERR_LAUNCH;
  for (int k = 0; rc == FG_OK && k < DB_STAGES; ++k)
    if (hipEventElapsedTime(&ms_host[k], ev[k], ev[k + 1]) != hipSuccess) rc = FG_ERR_LAUNCH;
  for (int k = 0; k < made; ++k) (void)hipEventDestroy(ev[k]);
  return rc;
}
