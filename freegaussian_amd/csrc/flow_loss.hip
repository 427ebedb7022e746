// FL: the masked L1 between the composited Gaussian flow -- two channels of the render, read where they lie -- and the batch's
// flow array at FULL resolution.  No target tensor exists anywhere: the target pixel and its weight are formed in registers.
//
//   per render pixel (y, x), downscale d (include/fgraster.h has the contract):
//     t     = the mean of the d x d source block at (y d, x d), DIVIDED BY d: a flow measured in full-resolution pixels shrinks
//             with the image
//     w     = 0 if any of the block's 2 d^2 source values is not finite, else the same box mean of the mask (1 without one)
//     loss  = sum w (|pred_x - t_x| + |pred_y - t_y|) / (2 max(sum w, FG_FLOW_L1_TINY))
//     d loss / d pred = w sign(pred - t) / (2 max(sum w, tiny)), sign(0) = 0; exactly 0 where w = 0
//
// The partial-sum scheme is target_loss.hip's: every 256-thread workgroup leaves its two sums in the workspace, a second launch
// of one workgroup adds them in a fixed order.  Here the sums are DOUBLES from the pixel on, rounded once at the end.  No
// atomics: two runs are bit for bit equal.  The two totals stay in the workspace's first 16 bytes for the backward, which
// recomputes target and weight from the source: nothing is read back by the host.
//
// Loads: neighbouring lanes take neighbouring render pixels of a row, so a lane's d source pixels of a block row (8 d bytes)
// follow its neighbour's: every row of the blocks is one contiguous stretch per wave.  A source pixel is one 64-bit load.
#include "arg_check.h"
#include "fg_common.h"

namespace {

constexpr int FL_BLOCK = 256;
constexpr int MAX_SIDE = 1 << 15;  // of the source: every pixel index stays far inside 64 bits, H W inside 2^30

struct Src {
  const float2* flows;
  const void* mask;  // null: weight 1 wherever the block is finite
  int W0, d, mask_f32;
  double inv_dd, inv_ddd;  // 1 / d^2, 1 / d^3: powers of two, exact
};

__device__ __forceinline__ bool finite2(float2 v) { return fabsf(v.x) < INFINITY && fabsf(v.y) < INFINITY; }

// the target pixel and its weight: see the head of the file
__device__ __forceinline__ void target_pixel(const Src& s, int y, int x, float& tx, float& ty, float& w) {
  const int d = s.d;
  const size_t first = (size_t)y * d * s.W0 + (size_t)x * d;  // the block's first source pixel
  double ax = 0.0, ay = 0.0;  // (up to 64 floats add up exactly in double: the mean is rounded once)
  bool fin = true;
  for (int dy = 0; dy < d; ++dy)
    for (int dx = 0; dx < d; ++dx) {
      const float2 v = s.flows[first + (size_t)dy * s.W0 + dx];
      fin = fin && finite2(v);
      ax += (double)v.x;
      ay += (double)v.y;
    }
  float m = 1.f;
  if (s.mask) {
    double am = 0.0;
    if (s.mask_f32) {
      const float* q = static_cast<const float*>(s.mask);
      for (int dy = 0; dy < d; ++dy)
        for (int dx = 0; dx < d; ++dx) am += (double)q[first + (size_t)dy * s.W0 + dx];
    } else {
      const unsigned char* q = static_cast<const unsigned char*>(s.mask);
      unsigned im = 0;
      for (int dy = 0; dy < d; ++dy)
        for (int dx = 0; dx < d; ++dx) im += q[first + (size_t)dy * s.W0 + dx];  // (a bool is the byte 0 or 1)
      am = (double)im;
    }
    m = (float)(am * s.inv_dd);
  }
  tx = fin ? (float)(ax * s.inv_ddd) : 0.f;
  ty = fin ? (float)(ay * s.inv_ddd) : 0.f;
  w = fin ? m : 0.f;
}

// sums of two doubles over the 256 threads of a workgroup (fixed order)
__device__ __forceinline__ double2 block_sum2_256(double a, double b, double2* scratch) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    a += __shfl_xor(a, m);
    b += __shfl_xor(b, m);
  }
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = make_double2(a, b);
  __syncthreads();
  return make_double2((scratch[0].x + scratch[1].x) + (scratch[2].x + scratch[3].x),
                      (scratch[0].y + scratch[1].y) + (scratch[2].y + scratch[3].y));
}

// one render pixel per thread; px, rw: the floats between two pixels and two rows of pred
__global__ void __launch_bounds__(FL_BLOCK)
flow_l1_fwd_kernel(int H, int W, Src s, const float* __restrict__ pred, int64_t px, int64_t rw, double2* __restrict__ partials) {
  __shared__ double2 red[4];
  const int64_t i = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
  double a = 0.0, b = 0.0;
  if (i < (int64_t)H * W) {
    const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
    float tx, ty, w;
    target_pixel(s, y, x, tx, ty, w);
    if (w != 0.f) {  // (a pixel without weight: its prediction does not enter, whatever it holds)
      const float* p = pred + y * rw + x * px;
      a = (double)w * (fabs((double)p[0] - (double)tx) + fabs((double)p[1] - (double)ty));
      b = (double)w;
    }
  }
  const double2 sums = block_sum2_256(a, b, red);
  if (threadIdx.x == 0) partials[blockIdx.x] = sums;
}

// fixed-order reduction of the per-workgroup partial sums -> totals[0] = {sum w (|dx| + |dy|), sum w}, out[0] = the loss
__global__ void __launch_bounds__(1024)
flow_l1_reduce_kernel(int nb, const double2* __restrict__ partials, double2* __restrict__ totals, float* __restrict__ out) {
  __shared__ double2 red[16];
  double a = 0.0, b = 0.0;
  for (int i = threadIdx.x; i < nb; i += 1024) {
    const double2 v = partials[i];
    a += v.x;
    b += v.y;
  }
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    a += __shfl_xor(a, m);
    b += __shfl_xor(b, m);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_double2(a, b);
  __syncthreads();
  if (threadIdx.x == 0) {
    double ta = 0.0, tb = 0.0;
    for (int w = 0; w < 16; ++w) ta += red[w].x, tb += red[w].y;
    totals[0] = make_double2(ta, tb);
    out[0] = (float)(ta / (2.0 * fmax(tb, FG_FLOW_L1_TINY)));
  }
}

__global__ void __launch_bounds__(FL_BLOCK)
flow_l1_bwd_kernel(int H, int W, Src s, const float* __restrict__ pred, int64_t px, int64_t rw, const double2* __restrict__ totals,
                   const float* __restrict__ v_out, float2* __restrict__ g_pred) {
  const int64_t i = (int64_t)blockIdx.x * FL_BLOCK + threadIdx.x;
  if (i >= (int64_t)H * W) return;
  const int y = (int)(i / W), x = (int)(i - (int64_t)y * W);
  float tx, ty, w;
  target_pixel(s, y, x, tx, ty, w);
  float2 g = make_float2(0.f, 0.f);
  if (w != 0.f) {
    const double scale = (double)v_out[0] * (double)w / (2.0 * fmax(totals[0].y, FG_FLOW_L1_TINY));
    const float* p = pred + y * rw + x * px;
    const float a = p[0], b = p[1];
    g.x = a > tx ? (float)scale : (a < tx ? (float)-scale : 0.f);
    g.y = b > ty ? (float)scale : (b < ty ? (float)-scale : 0.f);
  }
  g_pred[i] = g;
}

struct Shape {
  int H, W;  // the render's
  size_t flow_bytes, mask_bytes;
  unsigned blocks;
};

// FG_OK and the shape, or why not: INVALID_ARG for sizes that make no sense, UNSUPPORTED for those outside the range
int shape_of(int H0, int W0, int d, Shape* out) {
  if (H0 <= 0 || W0 <= 0) return FG_ERR_INVALID_ARG;
  if (d != 1 && d != 2 && d != 4 && d != 8) return FG_ERR_UNSUPPORTED;
  if (H0 > MAX_SIDE || W0 > MAX_SIDE) return FG_ERR_UNSUPPORTED;
  Shape s;
  s.H = H0 / d, s.W = W0 / d;
  if (s.H < 1 || s.W < 1) return FG_ERR_UNSUPPORTED;
  s.flow_bytes = (size_t)H0 * W0 * 2 * sizeof(float);
  s.mask_bytes = 0;
  s.blocks = (unsigned)(((size_t)s.H * s.W + FL_BLOCK - 1) / FL_BLOCK);
  *out = s;
  return FG_OK;
}

size_t workspace_of(const Shape& s) { return sizeof(double2) * (1 + (size_t)s.blocks); }

// what both entry points ask of the arguments they share; fills in the mask's bytes and pred's span
int shared_args(int H, int W, const float* pred, int64_t px, int64_t rw, int H0, int W0, int d, const float* flows, const void* mask,
                int mask_dtype, Shape* sh, size_t* pred_bytes) {
  if (const int e = shape_of(H0, W0, d, sh)) return e;
  if (H != sh->H || W != sh->W) return FG_ERR_INVALID_ARG;
  if (!pred || !flows || !fg_args::aligned(pred, 4) || !fg_args::aligned(flows, 8)) return FG_ERR_INVALID_ARG;
  // pixels of two floats that do not meet, rows that do not interleave
  if (px < 2) return FG_ERR_INVALID_ARG;
  if (px > FG_FLOW_L1_MAX_STRIDE) return FG_ERR_UNSUPPORTED;  // (before the product below: it stays inside 64 bits)
  if (rw < (int64_t)(W - 1) * px + 2) return FG_ERR_INVALID_ARG;
  if (rw > (int64_t)FG_FLOW_L1_MAX_STRIDE * MAX_SIDE) return FG_ERR_UNSUPPORTED;
  if (mask) {
    if (mask_dtype != FG_TARGET_U8 && mask_dtype != FG_TARGET_F32) return FG_ERR_UNSUPPORTED;
    if (mask_dtype == FG_TARGET_F32 && !fg_args::aligned(mask, 4)) return FG_ERR_INVALID_ARG;
    sh->mask_bytes = (size_t)H0 * W0 * (mask_dtype == FG_TARGET_F32 ? sizeof(float) : 1);
  }
  *pred_bytes = ((size_t)(H - 1) * (size_t)rw + (size_t)(W - 1) * (size_t)px + 2) * sizeof(float);
  return FG_OK;
}

Src source_of(const float* flows, const void* mask, int mask_dtype, int W0, int d) {
  Src r;
  r.flows = reinterpret_cast<const float2*>(flows), r.mask = mask;
  r.W0 = W0, r.d = d, r.mask_f32 = mask_dtype == FG_TARGET_F32 ? 1 : 0;
  r.inv_dd = 1.0 / (double)(d * d), r.inv_ddd = 1.0 / (double)(d * d * d);
  return r;
}

using fg_args::clash;

}  // namespace

extern "C" size_t fg_flow_l1_workspace_bytes(int H0, int W0, int downscale) {
  Shape s;
  if (shape_of(H0, W0, downscale, &s) != FG_OK) return 0;
  return workspace_of(s);
}

extern "C" int fg_flow_l1_fwd(int H, int W, const float* pred, int64_t pixel_stride, int64_t row_stride, int H0, int W0, int downscale,
                              const float* flows, const void* mask, int mask_dtype, void* workspace, size_t workspace_bytes, float* out,
                              fg_stream_t stream) {
  Shape sh;
  size_t pred_bytes;
  if (const int e = shared_args(H, W, pred, pixel_stride, row_stride, H0, W0, downscale, flows, mask, mask_dtype, &sh, &pred_bytes)) return e;
  if (!workspace || !out || !fg_args::aligned(workspace, 16) || !fg_args::aligned(out, 4)) return FG_ERR_INVALID_ARG;
  const size_t need = workspace_of(sh);
  if (clash({{workspace, need}, {out, sizeof(float)}}, {{pred, pred_bytes}, {flows, sh.flow_bytes}, {mask, sh.mask_bytes}}))
    return FG_ERR_INVALID_ARG;
  if (workspace_bytes < need) return FG_ERR_WORKSPACE;
  const Src s = source_of(flows, mask, mask_dtype, W0, downscale);
  hipStream_t st = fg_hip_stream(stream);
  double2* totals = static_cast<double2*>(workspace);
  hipLaunchKernelGGL(flow_l1_fwd_kernel, dim3(sh.blocks), dim3(FL_BLOCK), 0, st, H, W, s, pred, pixel_stride, row_stride, totals + 1);
  hipLaunchKernelGGL(flow_l1_reduce_kernel, dim3(1), dim3(1024), 0, st, (int)sh.blocks, (const double2*)(totals + 1), totals, out);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

extern "C" int fg_flow_l1_bwd(int H, int W, const float* pred, int64_t pixel_stride, int64_t row_stride, int H0, int W0, int downscale,
                              const float* flows, const void* mask, int mask_dtype, const void* workspace, const float* v_out,
                              float* g_pred, fg_stream_t stream) {
  Shape sh;
  size_t pred_bytes;
  if (const int e = shared_args(H, W, pred, pixel_stride, row_stride, H0, W0, downscale, flows, mask, mask_dtype, &sh, &pred_bytes)) return e;
  if (!workspace || !v_out || !g_pred || !fg_args::aligned(workspace, 16) || !fg_args::aligned(g_pred, 8)) return FG_ERR_INVALID_ARG;
  if (clash({{g_pred, (size_t)H * W * 2 * sizeof(float)}}, {{pred, pred_bytes}, {flows, sh.flow_bytes}, {mask, sh.mask_bytes},
                                                             {workspace, sizeof(double2)}, {v_out, sizeof(float)}}))
    return FG_ERR_INVALID_ARG;
  const Src s = source_of(flows, mask, mask_dtype, W0, downscale);
  hipLaunchKernelGGL(flow_l1_bwd_kernel, dim3(sh.blocks), dim3(FL_BLOCK), 0, fg_hip_stream(stream), H, W, s, pred, pixel_stride, row_stride,
                     static_cast<const double2*>(workspace), v_out, reinterpret_cast<float2*>(g_pred));
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}
