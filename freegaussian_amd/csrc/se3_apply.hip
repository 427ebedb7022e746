// SE: the SE(3) exponential of the deformation net's (w, v) heads applied to the Gaussian means, forward and backward, as one
// streaming launch each (freegaussian_amd/deform.py _se3 + utils.exp_se3 + utils.transform_points are the torch statement:
// about 40 elementwise / reduce / cat launches forward, an [N,4,4] array and several [N,3,3,3] intermediates kept for
// autograd's backward).
//
//   forward   out = R x + G vs per row (se3_math.h: FG_SE3_EXP, the statements the fused MLP forward's epilogue runs);
//             nothing but out is written.
//   backward  recomputes everything from w, v, x (36 B a row: what the host saves) and forms the exact derivative in forms
//             that do not cancel at small |w| (se3_math.h: fg_se3_row_bwd).  One kernel per set of gradients asked for: a
//             gradient that is not wanted is neither computed nor stored.
//
// One lane per row, registers only: no LDS, no atomics, no workspace.  Rows are independent, so a row with w = 0 (theta = 0:
// non-finite, as in the torch ops) stays in its own row, and two runs give the same bits.  A lane reads its row's three
// floats with three dword loads: the 64 lanes of a wave cover 768 contiguous bytes between them (contiguous [N,3] inputs), so
// every cache line fetched is used whole; w and v read in place from the [N,13] head block use 24 of each row's 52 bytes.
#include "arg_check.h"
#include "fg_common.h"
#include "se3_math.h"

namespace {

constexpr int SE3_BLOCK = 256;

__global__ void __launch_bounds__(SE3_BLOCK)
se3_fwd_kernel(int64_t N, const float* __restrict__ wp, int64_t w_stride, const float* __restrict__ vp, int64_t v_stride,
               const float* __restrict__ pts, float* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * SE3_BLOCK + threadIdx.x;
  if (row >= N) return;
  const float* wr = wp + row * w_stride;
  const float* vr = vp + row * v_stride;
  const float hd[6] = {wr[0], wr[1], wr[2], vr[0], vr[1], vr[2]};
  const float x[3] = {pts[row * 3], pts[row * 3 + 1], pts[row * 3 + 2]};
  FG_SE3_EXP(hd, T)
  for (int i = 0; i < 3; ++i) out[row * 3 + i] = FG_SE3_POINT(T, x, i);
}

template <bool WANT_W, bool WANT_V, bool WANT_X>
__global__ void __launch_bounds__(SE3_BLOCK)
se3_bwd_kernel(int64_t N, const float* __restrict__ wp, int64_t w_stride, const float* __restrict__ vp, int64_t v_stride,
               const float* __restrict__ pts, const float* __restrict__ g_out, float* __restrict__ g_w, int64_t gw_stride,
               float* __restrict__ g_v, int64_t gv_stride, float* __restrict__ g_pts) {
  const int64_t row = (int64_t)blockIdx.x * SE3_BLOCK + threadIdx.x;
  if (row >= N) return;
  const float* wr = wp + row * w_stride;
  const float* vr = vp + row * v_stride;
  const fg_vec3 w = {wr[0], wr[1], wr[2]}, v = {vr[0], vr[1], vr[2]};
  const fg_vec3 x = {pts[row * 3], pts[row * 3 + 1], pts[row * 3 + 2]};
  const fg_vec3 g = {g_out[row * 3], g_out[row * 3 + 1], g_out[row * 3 + 2]};
  fg_vec3 gw, gv, gx;
  fg_se3_row_bwd<WANT_W, WANT_V, WANT_X>(w, v, x, g, gw, gv, gx);
  if (WANT_W) {
    float* d = g_w + row * gw_stride;
    d[0] = gw.x, d[1] = gw.y, d[2] = gw.z;
  }
  if (WANT_V) {
    float* d = g_v + row * gv_stride;
    d[0] = gv.x, d[1] = gv.y, d[2] = gv.z;
  }
  if (WANT_X) {
    float* d = g_pts + row * 3;
    d[0] = gx.x, d[1] = gx.y, d[2] = gx.z;
  }
}

using namespace fg_args;

// FG_SE3_MAX_ROWS / FG_SE3_MAX_STRIDE: 2^30 workgroups at the most, and every span far below 2^63 bytes
constexpr int64_t SE3_MAX_ROWS = FG_SE3_MAX_ROWS;
constexpr int64_t SE3_MAX_STRIDE = FG_SE3_MAX_STRIDE;

template <bool W, bool V, bool X>
void launch_bwd(int64_t N, const float* w, int64_t w_stride, const float* v, int64_t v_stride, const float* pts, const float* g_out,
                float* g_w, int64_t gw_stride, float* g_v, int64_t gv_stride, float* g_pts, hipStream_t s) {
  const unsigned blocks = (unsigned)((N + SE3_BLOCK - 1) / SE3_BLOCK);
  hipLaunchKernelGGL((se3_bwd_kernel<W, V, X>), dim3(blocks), dim3(SE3_BLOCK), 0, s, N, w, w_stride, v, v_stride, pts, g_out, g_w,
                     gw_stride, g_v, gv_stride, g_pts);
}

}  // namespace

extern "C" int fg_se3_apply_fwd(int64_t N, const float* w, int64_t w_stride, const float* v, int64_t v_stride, const float* pts,
                                float* out, fg_stream_t stream) {
  const rows in[2] = {{w, w_stride, 3}, {v, v_stride, 3}};
  if (N < 0 || !w || !v || !pts || !out || stride_invalid(in)) return FG_ERR_INVALID_ARG;
  if (N == 0) return FG_OK;
  if (N > SE3_MAX_ROWS || stride_far(in, SE3_MAX_STRIDE)) return FG_ERR_UNSUPPORTED;
  if (clash({{out, 3, 3}}, N, {rows_span(in[0], N), rows_span(in[1], N), {pts, span_bytes(N, 3, 3)}})) return FG_ERR_INVALID_ARG;
  const unsigned blocks = (unsigned)((N + SE3_BLOCK - 1) / SE3_BLOCK);
  hipLaunchKernelGGL(se3_fwd_kernel, dim3(blocks), dim3(SE3_BLOCK), 0, fg_hip_stream(stream), N, w, w_stride, v, v_stride, pts, out);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

extern "C" int fg_se3_apply_bwd(int64_t N, const float* w, int64_t w_stride, const float* v, int64_t v_stride, const float* pts,
                                const float* g_out, float* g_w, int64_t gw_stride, float* g_v, int64_t gv_stride, float* g_pts,
                                fg_stream_t stream) {
  const rows in[2] = {{w, w_stride, 3}, {v, v_stride, 3}};
  const rows outs[3] = {{g_w, gw_stride, 3}, {g_v, gv_stride, 3}, {g_pts, 3, 3}};  // (a null output's stride is not looked at)
  if (N < 0 || !w || !v || !pts || !g_out || stride_invalid(in) || stride_invalid(outs)) return FG_ERR_INVALID_ARG;
  if (N == 0) return FG_OK;
  if (N > SE3_MAX_ROWS || stride_far(in, SE3_MAX_STRIDE) || stride_far(outs, SE3_MAX_STRIDE)) return FG_ERR_UNSUPPORTED;
  // g_w and g_v may be columns of one row block (interleaved rows, as w and v are)
  const size_t rows3 = span_bytes(N, 3, 3);
  if (clash(outs, N, {rows_span(in[0], N), rows_span(in[1], N), {pts, rows3}, {g_out, rows3}})) return FG_ERR_INVALID_ARG;
  if (!g_w && !g_v && !g_pts) return FG_OK;  // nothing asked for
  hipStream_t s = fg_hip_stream(stream);
#define SE3_BWD(W, V, X) launch_bwd<W, V, X>(N, w, w_stride, v, v_stride, pts, g_out, g_w, gw_stride, g_v, gv_stride, g_pts, s)
  switch ((g_w ? 4 : 0) | (g_v ? 2 : 0) | (g_pts ? 1 : 0)) {
    case 1: SE3_BWD(false, false, true); break;
    case 2: SE3_BWD(false, true, false); break;
    case 3: SE3_BWD(false, true, true); break;
    case 4: SE3_BWD(true, false, false); break;
    case 5: SE3_BWD(true, false, true); break;
    case 6: SE3_BWD(true, true, false); break;
    default: SE3_BWD(true, true, true); break;
  }
#undef SE3_BWD
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}
