// CT: the stage-2 control stage around the control MLP (freegaussian_amd/model.py FreeGaussianControlModel: the torch
// statement is boolean indexing, a Python loop of masked means, a [n,M] x [M,3] product and three zeros + index_put), on a
// plan the host builds once per mask (ops.control_plan: sel_index, bits, rank, counts).  Nothing here reads anything back.
//
//   attr_mean    d_avg[m] = (sum over the rows with bit m of (a - b)) / counts[m]: the difference in fp32 (what the torch
//                statement subtracts), the sum in float64, rounded once.  Two launches: a workgroup per FG_CONTROL_BLOCK_ROWS
//                rows writes its float64 partial sums, one workgroup adds them in block order.  The partition depends on n
//                alone and nothing is atomic: two runs give the same bits.
//   value_rows   value[i] = (sum of d_avg[m] over the set bits of bits[i], ascending m, fp32) / popcount(bits[i]).
//   scatter_fwd  out_means = means + (rank >= 0 ? d_xyz[rank] : 0), d_rotation / d_scaling = the row or zeros, every element
//                of the three [N,*] outputs written.
//   scatter_bwd  the gather of the upstream gradients' selected rows (the gradient of means is the upstream tensor itself).
//
// One lane per row, rows of 12 and 16 bytes: the 64 lanes of a wave cover 768 / 1024 contiguous bytes between them, so every
// cache line fetched is used whole (heads read in place from mlp_train's [n,10] block use all 40 bytes of a row between the
// three of them).  LDS: the 4 x 24 float64 of attr_mean's cross-wave sum and value_rows' copy of d_avg, nothing else.
// Registers (attr_mean): a lane keeps its 4 rows' differences and bits and walks the attributes in groups of 8 -- 24 float64
// accumulators at a time, not M x 3 = 96.
#include "arg_check.h"
#include "fg_common.h"

namespace {

constexpr int CT_BLOCK = 256;
constexpr int CT_ROWS = FG_CONTROL_BLOCK_ROWS;
constexpr int CT_PER_LANE = CT_ROWS / CT_BLOCK;
constexpr int CT_GROUP = 8;
constexpr int CT_WAVES = CT_BLOCK / FG_WAVE;
constexpr int CT_MAX_M = FG_CONTROL_MAX_ATTRS;
static_assert(CT_ROWS % CT_BLOCK == 0 && CT_MAX_M % CT_GROUP == 0 && CT_MAX_M * 3 <= CT_BLOCK, "control.hip layout");

// the counts travel by value, as a kernel argument: the host has them (it refuses a zero before any launch)
struct ct_counts {
  int32_t c[CT_MAX_M];
};

__device__ __forceinline__ uint32_t attr_mask(int M) { return M >= 32 ? 0xffffffffu : (1u << M) - 1u; }

// every lane gets the same bits: a + b and b + a round alike, so both partners of a step hold one value
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int m = FG_WAVE / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

__global__ void __launch_bounds__(CT_BLOCK)
control_partial_kernel(int64_t n, int M, const float* __restrict__ a, int64_t a_stride, const float* __restrict__ b, int64_t b_stride,
                       const uint32_t* __restrict__ bits, double* __restrict__ partial) {
  __shared__ double red[CT_WAVES][CT_GROUP * 3];
  const int tid = threadIdx.x, lane = tid & (FG_WAVE - 1), wave = tid / FG_WAVE;
  const int64_t base = (int64_t)blockIdx.x * CT_ROWS;
  const uint32_t valid = attr_mask(M);
  float d[CT_PER_LANE][3];
  uint32_t bt[CT_PER_LANE];
#pragma unroll
  for (int k = 0; k < CT_PER_LANE; ++k) {
    const int64_t row = base + k * CT_BLOCK + tid;
    bt[k] = 0, d[k][0] = d[k][1] = d[k][2] = 0.f;
    if (row < n) {
      const float* ar = a + row * a_stride;
      const float* br = b + row * b_stride;
      bt[k] = bits[row] & valid;
#pragma unroll
      for (int c = 0; c < 3; ++c) d[k][c] = ar[c] - br[c];
    }
  }
  double* out = partial + (int64_t)blockIdx.x * (M * 3);
  for (int g0 = 0; g0 < M; g0 += CT_GROUP) {
    const int members = min(CT_GROUP, M - g0);
    double acc[CT_GROUP][3];
#pragma unroll
    for (int j = 0; j < CT_GROUP; ++j) acc[j][0] = acc[j][1] = acc[j][2] = 0.0;
#pragma unroll
    for (int k = 0; k < CT_PER_LANE; ++k) {
      const uint32_t group_bits = bt[k] >> g0;
#pragma unroll
      for (int j = 0; j < CT_GROUP; ++j) {
        const bool on = (group_bits >> j) & 1u;
#pragma unroll
        for (int c = 0; c < 3; ++c) acc[j][c] += on ? (double)d[k][c] : 0.0;
      }
    }
#pragma unroll
    for (int j = 0; j < CT_GROUP; ++j) {
      if (j < members) {  // (uniform)
#pragma unroll
        for (int c = 0; c < 3; ++c) {
          const double s = wave_sum_f64(acc[j][c]);
          if (lane == 0) red[wave][j * 3 + c] = s;
        }
      }
    }
    __syncthreads();
    if (tid < members * 3) {
      double s = red[0][tid];
#pragma unroll
      for (int w = 1; w < CT_WAVES; ++w) s += red[w][tid];
      out[g0 * 3 + tid] = s;
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(CT_BLOCK)
control_final_kernel(int64_t blocks, int M, const double* __restrict__ partial, ct_counts counts, float* __restrict__ d_avg) {
  const int t = threadIdx.x;
  if (t >= M * 3) return;
  double s = 0.0;
  for (int64_t blk = 0; blk < blocks; ++blk) s += partial[blk * (M * 3) + t];
  d_avg[t] = (float)(s / (double)counts.c[t / 3]);
}

__global__ void __launch_bounds__(CT_BLOCK)
control_value_kernel(int64_t n, int M, const uint32_t* __restrict__ bits, const float* __restrict__ d_avg, float* __restrict__ value) {
  __shared__ float avg[CT_MAX_M * 3];
  if ((int)threadIdx.x < M * 3) avg[threadIdx.x] = d_avg[threadIdx.x];
  __syncthreads();
  const int64_t row = (int64_t)blockIdx.x * CT_BLOCK + threadIdx.x;
  if (row >= n) return;
  const uint32_t bt = bits[row] & attr_mask(M);
  float s[3] = {0.f, 0.f, 0.f};
  for (uint32_t left = bt; left; left &= left - 1) {  // ascending m
    const int m = __ffs(left) - 1;
#pragma unroll
    for (int c = 0; c < 3; ++c) s[c] += avg[m * 3 + c];
  }
  const float members = (float)__popc(bt);  // (no bit: 0 / 0, the torch statement's NaN)
#pragma unroll
  for (int c = 0; c < 3; ++c) value[row * 3 + c] = __fdiv_rn(s[c], members);
}

__global__ void __launch_bounds__(CT_BLOCK)
control_scatter_fwd_kernel(int64_t N, int64_t n, const int32_t* __restrict__ rank, const float* __restrict__ means,
                           const float* __restrict__ d_xyz, int64_t xyz_stride, const float* __restrict__ d_rot, int64_t rot_stride,
                           const float* __restrict__ d_scale, int64_t scale_stride, float* __restrict__ out_means,
                           float* __restrict__ d_rotation, float* __restrict__ d_scaling) {
  const int64_t row = (int64_t)blockIdx.x * CT_BLOCK + threadIdx.x;
  if (row >= N) return;
  const int64_t r = rank[row];
  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  float x[3] = {0.f, 0.f, 0.f}, s[3] = {0.f, 0.f, 0.f};
  if (r >= 0 && r < n) {  // (a rank outside the plan's rows reads nothing)
    const float* xr = d_xyz + r * xyz_stride;
    const float* qr = d_rot + r * rot_stride;
    const float* sr = d_scale + r * scale_stride;
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = xr[c], s[c] = sr[c];
    q = make_float4(qr[0], qr[1], qr[2], qr[3]);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) out_means[row * 3 + c] = means[row * 3 + c] + x[c], d_scaling[row * 3 + c] = s[c];  // (+ 0: the torch sum)
  reinterpret_cast<float4*>(d_rotation)[row] = q;
}

__global__ void __launch_bounds__(CT_BLOCK)
control_scatter_bwd_kernel(int64_t n, int64_t N, const int32_t* __restrict__ sel_index, const float* __restrict__ g_means,
                           const float* __restrict__ g_rotation, const float* __restrict__ g_scaling, float* __restrict__ g_xyz,
                           int64_t xyz_stride, float* __restrict__ g_rot, int64_t rot_stride, float* __restrict__ g_scale,
                           int64_t scale_stride) {
  const int64_t i = (int64_t)blockIdx.x * CT_BLOCK + threadIdx.x;
  if (i >= n) return;
  const int64_t src = sel_index[i];
  const bool ok = src >= 0 && src < N;  // (a row outside the full set reads nothing)
  if (g_xyz) {
    float* d = g_xyz + i * xyz_stride;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = ok && g_means ? g_means[src * 3 + c] : 0.f;
  }
  if (g_rot) {
    float* d = g_rot + i * rot_stride;
#pragma unroll
    for (int c = 0; c < 4; ++c) d[c] = ok && g_rotation ? g_rotation[src * 4 + c] : 0.f;
  }
  if (g_scale) {
    float* d = g_scale + i * scale_stride;
#pragma unroll
    for (int c = 0; c < 3; ++c) d[c] = ok && g_scaling ? g_scaling[src * 3 + c] : 0.f;
  }
}

// ---- host: argument checks ------------------------------------------------------------------------------------------------

bool attrs_ok(int M) { return M >= 1 && M <= CT_MAX_M; }
bool rows_ok(int64_t n) { return n >= 1 && n <= FG_CONTROL_MAX_ROWS; }
int64_t partial_blocks(int64_t n) { return (n + CT_ROWS - 1) / CT_ROWS; }
unsigned row_blocks(int64_t rows) { return (unsigned)((rows + CT_BLOCK - 1) / CT_BLOCK); }
using namespace fg_args;  // (arg_check.h: the heads and their gradients may be columns of one block, mlp_train's [n,10])

}  // namespace

extern "C" int fg_control_supported(int M) { return attrs_ok(M) ? 1 : 0; }

extern "C" size_t fg_control_workspace_bytes(int64_t n, int M) {
  if (!attrs_ok(M) || !rows_ok(n)) return 0;
  return (size_t)partial_blocks(n) * (size_t)(M * 3) * sizeof(double);
}

extern "C" int fg_control_attr_mean(int64_t n, int M, const float* a, int64_t a_stride, const float* b, int64_t b_stride,
                                    const uint32_t* bits, const int32_t* counts, void* workspace, size_t workspace_bytes, float* d_avg,
                                    fg_stream_t stream) {
  if (n < 1 || M < 1 || !a || !b || !bits || !counts || !d_avg || a_stride < 3 || b_stride < 3) return FG_ERR_INVALID_ARG;
  if (!attrs_ok(M) || !rows_ok(n) || a_stride > FG_CONTROL_MAX_STRIDE || b_stride > FG_CONTROL_MAX_STRIDE) return FG_ERR_UNSUPPORTED;
  ct_counts by_value;
  for (int m = 0; m < CT_MAX_M; ++m) by_value.c[m] = 1;
  for (int m = 0; m < M; ++m) {
    if (counts[m] < 1 || counts[m] > n) return FG_ERR_INVALID_ARG;  // (an attribute without a row has no mean)
    by_value.c[m] = counts[m];
  }
  if (!workspace || !aligned(workspace, sizeof(double))) return FG_ERR_INVALID_ARG;
  const size_t need = fg_control_workspace_bytes(n, M);
  if (workspace_bytes < need) return FG_ERR_WORKSPACE;
  if (clash({{d_avg, (size_t)M * 3 * sizeof(float)}, {workspace, need}},
            {{a, span_bytes(n, a_stride, 3)}, {b, span_bytes(n, b_stride, 3)}, {bits, (size_t)n * sizeof(uint32_t)}}))
    return FG_ERR_INVALID_ARG;
  hipStream_t s = fg_hip_stream(stream);
  const int64_t blocks = partial_blocks(n);
  double* partial = static_cast<double*>(workspace);
  hipLaunchKernelGGL(control_partial_kernel, dim3((unsigned)blocks), dim3(CT_BLOCK), 0, s, n, M, a, a_stride, b, b_stride, bits, partial);
  FG_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(control_final_kernel, dim3(1), dim3(CT_BLOCK), 0, s, blocks, M, partial, by_value, d_avg);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

extern "C" int fg_control_value_rows(int64_t n, int M, const uint32_t* bits, const float* d_avg, float* value, fg_stream_t stream) {
  if (n < 0 || M < 1 || !bits || !d_avg || !value) return FG_ERR_INVALID_ARG;
  if (n == 0) return attrs_ok(M) ? FG_OK : FG_ERR_UNSUPPORTED;
  if (!attrs_ok(M) || !rows_ok(n)) return FG_ERR_UNSUPPORTED;
  if (clash({{value, span_bytes(n, 3, 3)}}, {{bits, (size_t)n * sizeof(uint32_t)}, {d_avg, (size_t)M * 3 * sizeof(float)}}))
    return FG_ERR_INVALID_ARG;
  hipLaunchKernelGGL(control_value_kernel, dim3(row_blocks(n)), dim3(CT_BLOCK), 0, fg_hip_stream(stream), n, M, bits, d_avg, value);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

extern "C" int fg_control_scatter_fwd(int64_t N, int64_t n, const int32_t* rank, const float* means, const float* d_xyz,
                                      int64_t xyz_stride, const float* d_rot, int64_t rot_stride, const float* d_scale,
                                      int64_t scale_stride, float* out_means, float* d_rotation, float* d_scaling, fg_stream_t stream) {
  const rows in[3] = {{d_xyz, xyz_stride, 3}, {d_rot, rot_stride, 4}, {d_scale, scale_stride, 3}};
  if (N < 0 || n < 0 || n > N || !rank || !means || !d_xyz || !d_rot || !d_scale || !out_means || !d_rotation || !d_scaling)
    return FG_ERR_INVALID_ARG;
  if (stride_invalid(in) || !aligned(d_rotation, sizeof(float4))) return FG_ERR_INVALID_ARG;
  if (N == 0) return FG_OK;
  if (!rows_ok(N) || stride_far(in, FG_CONTROL_MAX_STRIDE)) return FG_ERR_UNSUPPORTED;
  // the outputs have N rows, the heads n: without a selected row no head is read
  span ins[5] = {{rank, (size_t)N * sizeof(int32_t)}, {means, span_bytes(N, 3, 3)}, {nullptr, 0}, {nullptr, 0}, {nullptr, 0}};
  if (n > 0)
    for (int k = 0; k < 3; ++k) ins[2 + k] = rows_span(in[k], n);
  if (clash({{out_means, 3, 3}, {d_rotation, 4, 4}, {d_scaling, 3, 3}}, N, ins)) return FG_ERR_INVALID_ARG;
  hipLaunchKernelGGL(control_scatter_fwd_kernel, dim3(row_blocks(N)), dim3(CT_BLOCK), 0, fg_hip_stream(stream), N, n, rank, means, d_xyz,
                     xyz_stride, d_rot, rot_stride, d_scale, scale_stride, out_means, d_rotation, d_scaling);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

extern "C" int fg_control_scatter_bwd(int64_t n, int64_t N, const int32_t* sel_index, const float* g_means, const float* g_rotation,
                                      const float* g_scaling, float* g_d_xyz, int64_t xyz_stride, float* g_d_rot, int64_t rot_stride,
                                      float* g_d_scale, int64_t scale_stride, fg_stream_t stream) {
  const rows out[3] = {{g_d_xyz, xyz_stride, 3}, {g_d_rot, rot_stride, 4}, {g_d_scale, scale_stride, 3}};
  if (n < 0 || N < 0 || n > N || !sel_index || stride_invalid(out)) return FG_ERR_INVALID_ARG;
  if (n == 0) return FG_OK;
  if (!rows_ok(N) || stride_far(out, FG_CONTROL_MAX_STRIDE)) return FG_ERR_UNSUPPORTED;
  // the outputs have n rows, the upstream gradients N
  if (clash(out, n, {{sel_index, (size_t)n * sizeof(int32_t)}, {g_means, span_bytes(N, 3, 3)}, {g_rotation, span_bytes(N, 4, 4)},
                     {g_scaling, span_bytes(N, 3, 3)}}))
    return FG_ERR_INVALID_ARG;
  if (!g_d_xyz && !g_d_rot && !g_d_scale) return FG_OK;  // nothing asked for
  hipLaunchKernelGGL(control_scatter_bwd_kernel, dim3(row_blocks(n)), dim3(CT_BLOCK), 0, fg_hip_stream(stream), n, N, sel_index, g_means,
                     g_rotation, g_scaling, g_d_xyz, xyz_stride, g_d_rot, rot_stride, g_d_scale, scale_stride);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}
