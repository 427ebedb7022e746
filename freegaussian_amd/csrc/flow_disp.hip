// FD: the 2-D displacement of the projected Gaussian centres between frame 0 and the current frame, forward and backward, as
// one streaming launch each -- the per-Gaussian term mu_{i,t} - mu_{i,0} of the composited Gaussian flow (flow.py; two
// stage-by-stage ops.project passes, a select and two _Project backwards are the torch-level statement of it).
//
//   p_t = R_t m_t + tau_t,  p_0 = R_0 m_0 + tau_0,  Delta = p_t - p_0
//   disp = ( f_x (Delta_x z_0 - x_0 Delta_z),  f_y (Delta_y z_0 - y_0 Delta_z) ) / (z_t z_0)
// which is f (x_t / z_t - x_0 / z_0) with the two quotients never formed: at small motion they agree in all but their last
// bits, and their difference would keep only those.  c_x, c_y never enter the value.  With one camera for both frames
// (viewmat_0 null) Delta = R (m_t - m_0): the translation never enters Delta either, and p_t = p_0 + Delta.
//
//   A row is VALID iff z_t > near, z_0 > near and both projected centres f p / z + c lie in [-margin, width + margin] x
//   [-margin, height + margin] (margin = inf: every finite centre does).  An invalid row writes exact zeros and gets exact zero
//   gradients.
//
//   backward  recomputes everything from the inputs (24 B a row: nothing is saved) and writes the closed form
//             d disp / d p_t = f (1 / z_t, -x_t / z_t^2), d disp / d p_0 = -f (1 / z_0, -x_0 / z_0^2), through R_t^T and R_0^T.  One
//             kernel per set of gradients asked for: a gradient that is not wanted is neither computed nor stored.
//
// One lane per row, registers only: no LDS, no atomics, no workspace; rows are independent, so two runs give the same bits.
// A lane reads its row's three floats with three dword loads -- the 64 lanes of a wave cover 768 contiguous bytes per input,
// every cache line fetched is used whole -- and stores its displacement as one 8-byte word (512 contiguous bytes a wave).
// 24 B in and 8 B out per row make a million rows 32 MB: the launch is short at every size the model has, so a row per lane,
// which gives the most waves at 33 000 rows (516 over 256 compute units), is kept at every size; there is no policy to choose.
// The two camera matrices and K are the same for every lane: 41 floats through the scalar cache.
#include "arg_check.h"
#include "fg_common.h"

// No FMA contraction in this file: which products the compiler fuses depends on the code around them, and the kernel that forms
// one gradient must give the bits of the one that forms both.
#pragma clang fp contract(off)

namespace {

constexpr int FD_BLOCK = 256;

struct Cams {
  float Rt[9], tt[3], R0[9], t0[3];  // rows of the two rotations, the translations (one camera: the same twice)
  float fx, fy, cx, cy;
};

__device__ __forceinline__ Cams load_cams(const float* __restrict__ vt, const float* __restrict__ v0, const float* __restrict__ K) {
  Cams c;
  if (!v0) v0 = vt;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) c.Rt[3 * i + j] = vt[4 * i + j], c.R0[3 * i + j] = v0[4 * i + j];
    c.tt[i] = vt[4 * i + 3], c.t0[i] = v0[4 * i + 3];
  }
  c.fx = K[0], c.cx = K[2], c.fy = K[4], c.cy = K[5];
  return c;
}

struct Row {
  float xt, yt, zt, x0, y0, z0, dx, dy, dz;
  bool valid;
};

__device__ __forceinline__ float rot(const float* R, int i, float a, float b, float c) { return R[3 * i] * a + R[3 * i + 1] * b + R[3 * i + 2] * c; }

// SAME: one camera for both frames
template <bool SAME>
__device__ __forceinline__ Row row_of(const Cams& c, const float* mt, const float* m0, float W, float H, float near, float margin) {
  Row r;
  r.x0 = rot(c.R0, 0, m0[0], m0[1], m0[2]) + c.t0[0];
  r.y0 = rot(c.R0, 1, m0[0], m0[1], m0[2]) + c.t0[1];
  r.z0 = rot(c.R0, 2, m0[0], m0[1], m0[2]) + c.t0[2];
  if (SAME) {
    const float a = mt[0] - m0[0], b = mt[1] - m0[1], e = mt[2] - m0[2];
    r.dx = rot(c.Rt, 0, a, b, e), r.dy = rot(c.Rt, 1, a, b, e), r.dz = rot(c.Rt, 2, a, b, e);
    r.xt = r.x0 + r.dx, r.yt = r.y0 + r.dy, r.zt = r.z0 + r.dz;
  } else {
    r.xt = rot(c.Rt, 0, mt[0], mt[1], mt[2]) + c.tt[0];
    r.yt = rot(c.Rt, 1, mt[0], mt[1], mt[2]) + c.tt[1];
    r.zt = rot(c.Rt, 2, mt[0], mt[1], mt[2]) + c.tt[2];
    r.dx = r.xt - r.x0, r.dy = r.yt - r.y0, r.dz = r.zt - r.z0;
  }
  r.valid = r.zt > near && r.z0 > near;
  if (r.valid) {
    const float ut = c.fx * r.xt / r.zt + c.cx, vt = c.fy * r.yt / r.zt + c.cy;
    const float u0 = c.fx * r.x0 / r.z0 + c.cx, v0 = c.fy * r.y0 / r.z0 + c.cy;
    // (a NaN compares false: such a row is invalid)
    r.valid = ut >= -margin && ut <= W + margin && vt >= -margin && vt <= H + margin && u0 >= -margin && u0 <= W + margin &&
              v0 >= -margin && v0 <= H + margin;
  }
  return r;
}

template <bool SAME>
__global__ void __launch_bounds__(FD_BLOCK)
flow_disp_fwd_kernel(int64_t N, const float* __restrict__ means_t, int64_t mt_stride, const float* __restrict__ means_0, int64_t m0_stride,
                     const float* __restrict__ vt, const float* __restrict__ v0, const float* __restrict__ K, float W, float H, float near,
                     float margin, float2* __restrict__ disp) {
  const int64_t row = (int64_t)blockIdx.x * FD_BLOCK + threadIdx.x;
  if (row >= N) return;
  const Cams c = load_cams(vt, v0, K);
  const float* a = means_t + row * mt_stride;
  const float* b = means_0 + row * m0_stride;
  const float mt[3] = {a[0], a[1], a[2]}, m0[3] = {b[0], b[1], b[2]};
  const Row r = row_of<SAME>(c, mt, m0, W, H, near, margin);
  float2 d = make_float2(0.f, 0.f);
  if (r.valid) {
    const float inv = 1.f / (r.zt * r.z0);
    d.x = c.fx * (r.dx * r.z0 - r.x0 * r.dz) * inv;
    d.y = c.fy * (r.dy * r.z0 - r.y0 * r.dz) * inv;
  }
  disp[row] = d;
}

template <bool SAME, bool WANT_T, bool WANT_0>
__global__ void __launch_bounds__(FD_BLOCK)
flow_disp_bwd_kernel(int64_t N, const float* __restrict__ means_t, int64_t mt_stride, const float* __restrict__ means_0, int64_t m0_stride,
                     const float* __restrict__ vt, const float* __restrict__ v0, const float* __restrict__ K, float W, float H, float near,
                     float margin, const float2* __restrict__ g_disp, float* __restrict__ g_means_t, float* __restrict__ g_means_0) {
  const int64_t row = (int64_t)blockIdx.x * FD_BLOCK + threadIdx.x;
  if (row >= N) return;
  const Cams c = load_cams(vt, v0, K);
  const float* a = means_t + row * mt_stride;
  const float* b = means_0 + row * m0_stride;
  const float mt[3] = {a[0], a[1], a[2]}, m0[3] = {b[0], b[1], b[2]};
  const Row r = row_of<SAME>(c, mt, m0, W, H, near, margin);
  const float2 g = g_disp[row];
  if (WANT_T) {
    float o[3] = {0.f, 0.f, 0.f};
    if (r.valid) {
      const float iz = 1.f / r.zt;
      const float px = g.x * c.fx * iz, py = g.y * c.fy * iz;
      const float pz = -(px * r.xt + py * r.yt) * iz;
#pragma unroll
      for (int j = 0; j < 3; ++j) o[j] = c.Rt[j] * px + c.Rt[3 + j] * py + c.Rt[6 + j] * pz;  // R_t^T
    }
    float* d = g_means_t + row * 3;
    d[0] = o[0], d[1] = o[1], d[2] = o[2];
  }
  if (WANT_0) {
    float o[3] = {0.f, 0.f, 0.f};
    if (r.valid) {
      const float iz = 1.f / r.z0;
      const float px = -(g.x * c.fx * iz), py = -(g.y * c.fy * iz);
      const float pz = -(px * r.x0 + py * r.y0) * iz;
#pragma unroll
      for (int j = 0; j < 3; ++j) o[j] = c.R0[j] * px + c.R0[3 + j] * py + c.R0[6 + j] * pz;  // R_0^T
    }
    float* d = g_means_0 + row * 3;
    d[0] = o[0], d[1] = o[1], d[2] = o[2];
  }
}

using namespace fg_args;

constexpr int64_t FD_MAX_ROWS = FG_FLOW_DISP_MAX_ROWS;
constexpr int64_t FD_MAX_STRIDE = FG_FLOW_DISP_MAX_STRIDE;
constexpr size_t MAT = 16 * sizeof(float), KMAT = 9 * sizeof(float);

// what both entry points ask of the arguments they share: FG_OK, or why not.  (NaN fails every comparison below.)
int shared_args(int64_t N, const rows (&in)[2], const float* viewmat_t, const float* K, int width, int height, float near, float margin) {
  if (N < 0 || !in[0].p || !in[1].p || !viewmat_t || !K || stride_invalid(in)) return FG_ERR_INVALID_ARG;
  if (width <= 0 || height <= 0 || !(near >= 0.f) || !(near < INFINITY) || !(margin >= 0.f)) return FG_ERR_INVALID_ARG;
  return FG_OK;
}

template <bool SAME, bool T, bool Z>
void launch_bwd(int64_t N, const float* mt, int64_t mts, const float* m0, int64_t m0s, const float* vt, const float* v0, const float* K,
                int width, int height, float near, float margin, const float* g_disp, float* g_t, float* g_0, hipStream_t s) {
  const unsigned blocks = (unsigned)((N + FD_BLOCK - 1) / FD_BLOCK);
  hipLaunchKernelGGL((flow_disp_bwd_kernel<SAME, T, Z>), dim3(blocks), dim3(FD_BLOCK), 0, s, N, mt, mts, m0, m0s, vt, v0, K, (float)width,
                     (float)height, near, margin, reinterpret_cast<const float2*>(g_disp), g_t, g_0);
}

}  // namespace

extern "C" int fg_flow_disp_fwd(int64_t N, const float* means_t, int64_t mt_stride, const float* means_0, int64_t m0_stride,
                                const float* viewmat_t, const float* viewmat_0, const float* K, int width, int height, float near,
                                float margin, float* disp, fg_stream_t stream) {
  const rows in[2] = {{means_t, mt_stride, 3}, {means_0, m0_stride, 3}};
  if (const int e = shared_args(N, in, viewmat_t, K, width, height, near, margin)) return e;
  if (!disp || !aligned(disp, 8)) return FG_ERR_INVALID_ARG;
  if (N == 0) return FG_OK;
  if (N > FD_MAX_ROWS || stride_far(in, FD_MAX_STRIDE)) return FG_ERR_UNSUPPORTED;
  if (clash({{disp, span_bytes(N, 2, 2)}},
            {rows_span(in[0], N), rows_span(in[1], N), {viewmat_t, MAT}, {viewmat_0, viewmat_0 ? MAT : 0}, {K, KMAT}}))
    return FG_ERR_INVALID_ARG;
  const unsigned blocks = (unsigned)((N + FD_BLOCK - 1) / FD_BLOCK);
  hipStream_t s = fg_hip_stream(stream);
  float2* out = reinterpret_cast<float2*>(disp);
  if (viewmat_0)
    hipLaunchKernelGGL(flow_disp_fwd_kernel<false>, dim3(blocks), dim3(FD_BLOCK), 0, s, N, means_t, mt_stride, means_0, m0_stride,
                       viewmat_t, viewmat_0, K, (float)width, (float)height, near, margin, out);
  else
    hipLaunchKernelGGL(flow_disp_fwd_kernel<true>, dim3(blocks), dim3(FD_BLOCK), 0, s, N, means_t, mt_stride, means_0, m0_stride,
                       viewmat_t, viewmat_0, K, (float)width, (float)height, near, margin, out);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

extern "C" int fg_flow_disp_bwd(int64_t N, const float* means_t, int64_t mt_stride, const float* means_0, int64_t m0_stride,
                                const float* viewmat_t, const float* viewmat_0, const float* K, int width, int height, float near,
                                float margin, const float* g_disp, float* g_means_t, float* g_means_0, fg_stream_t stream) {
  const rows in[2] = {{means_t, mt_stride, 3}, {means_0, m0_stride, 3}};
  if (const int e = shared_args(N, in, viewmat_t, K, width, height, near, margin)) return e;
  if (!g_disp || !aligned(g_disp, 8)) return FG_ERR_INVALID_ARG;
  if (N == 0) return FG_OK;
  if (N > FD_MAX_ROWS || stride_far(in, FD_MAX_STRIDE)) return FG_ERR_UNSUPPORTED;
  const size_t rows3 = span_bytes(N, 3, 3);
  if (clash({{g_means_t, g_means_t ? rows3 : 0}, {g_means_0, g_means_0 ? rows3 : 0}},
            {rows_span(in[0], N), rows_span(in[1], N), {viewmat_t, MAT}, {viewmat_0, viewmat_0 ? MAT : 0}, {K, KMAT},
             {g_disp, span_bytes(N, 2, 2)}}))
    return FG_ERR_INVALID_ARG;
  if (!g_means_t && !g_means_0) return FG_OK;  // nothing asked for
  hipStream_t s = fg_hip_stream(stream);
#define FD_BWD(SAME, T, Z) \
  launch_bwd<SAME, T, Z>(N, means_t, mt_stride, means_0, m0_stride, viewmat_t, viewmat_0, K, width, height, near, margin, g_disp, g_means_t, g_means_0, s)
  switch ((viewmat_0 ? 0 : 4) | (g_means_t ? 2 : 0) | (g_means_0 ? 1 : 0)) {
    case 1: FD_BWD(false, false, true); break;
    case 2: FD_BWD(false, true, false); break;
    case 3: FD_BWD(false, true, true); break;
    case 5: FD_BWD(true, false, true); break;
    case 6: FD_BWD(true, true, false); break;
    default: FD_BWD(true, true, true); break;
  }
#undef FD_BWD
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}
