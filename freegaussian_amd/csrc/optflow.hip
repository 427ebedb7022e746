// OF: dense optical flow between two frames -- pyramidal, patch-based, inverse-compositional Lucas-Kanade with a
// forward-backward check.  The definition is stated once, in include/fgraster.h ("OF"); tests/optical_flow_restatement.py
// states it on the CPU in float64 and in fp32, operation by operation in the order used here.
//
//   pyramid  : level 0 = grey of the image (read where it lies: uint8 or float, 1 or 3 channels), one thread per pixel;
//              level l+1 = the 5 x 5 binomial of level l at even coordinates, one thread per output pixel, 25 clamped loads
//              (rows of neighbouring lanes are contiguous up to the stride of 2).
//   level    : THE HOT PATH.  One 256-thread workgroup per 32 x 8 pixel tile, one pixel per thread; all `iters` updates of
//              the level in ONE launch (a pixel's update depends on nothing but its own u).
//              A, Ix, Iy of the tile plus a halo of `radius`, at the CLAMPED coordinates the windows ask for, sit in LDS
//              (3 x 46 x 22 floats at radius 7, 12 KiB; 6.2 KiB at the default radius 3): every window of the tile reads
//              exactly these entries.  A row of the tile is 32 consecutive lanes = one ds_read_b32 lane group reading 32
//              consecutive dwords: conflict-free at any row stride, so the rows are not padded.
//              G (three sums) and its determinant stay in registers across the iterations.
//              B is sampled at per-pixel real offsets: four taps per window entry.  Two builds, the same bits:
//                FG_OPTFLOW_STAGED=1 (the product build): per iteration the tile's range of floor(u) sizes a region of B that
//                is staged in LDS (up to 64 x 40 floats, 10 KiB); a tap outside the region -- a tile whose flows spread
//                further than that -- falls back to a global load.
//                FG_OPTFLOW_STAGED=0: every tap is a load through the caches.  make optflow-direct builds it for
//                scripts/optical_flow_bench.py.  Measured on an MI355X (profiles/optical_flow.md): staging is level at
//                480 x 270 and wins at 960 x 540 (0.84 x) and 1920 x 1080 (0.65 x).
//              LDS per workgroup 22 KiB (12 KiB direct): by LDS 7 workgroups = 28 waves fit a compute unit's 160 KiB (61
//              VGPRs would allow 8); the direct build (41 VGPRs) is bounded by the 8 workgroups = 32 waves alone.
//   validity : one thread per pixel: the smaller eigenvalue the level-0 launch left, the target inside the image, and, with
//              both directions, u_ba sampled at x + u_ab.
// No atomics; every sum is in a fixed order: two runs are bit for bit equal.  Nothing is read back, nothing is allocated.
#include "arg_check.h"
#include "fg_common.h"

#ifndef FG_OPTFLOW_STAGED
#define FG_OPTFLOW_STAGED 1
#endif

namespace {

constexpr int OF_TW = 32, OF_TH = 8, OF_BLOCK = OF_TW * OF_TH;
constexpr int OF_MAX_R = FG_OPTFLOW_MAX_RADIUS;
constexpr int OF_RW = OF_TW + 2 * OF_MAX_R, OF_RH = OF_TH + 2 * OF_MAX_R;  // the tile with its halo, at most
#if FG_OPTFLOW_STAGED
constexpr int OF_SW = 64, OF_SH = 40;  // the staged region of B, at most
#endif
constexpr float OF_LAMBDA = 1e-6f;
constexpr float OF_U_CLAMP = 32768.f;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

// floor and fraction of u, u clamped to +-32768 first (a NaN takes the lower end: fmaxf returns the other operand)
__device__ __forceinline__ void split(float u, int& i, float& f) {
  const float c = fminf(fmaxf(u, -OF_U_CLAMP), OF_U_CLAMP);
  const float fl = floorf(c);
  i = (int)fl;
  f = c - fl;
}

// the sample rule of the definition on one axis: an index below 0 becomes 0, one at or beyond n - 1 becomes n - 1, both with
// fraction 0; i1 is the second tap (inside the image whatever the fraction)
__device__ __forceinline__ void tap(int n, int& i, float& f, int& i1) {
  if (i < 0) i = 0, f = 0.f;
  else if (i >= n - 1) i = n - 1, f = 0.f;
  i1 = min(i + 1, n - 1);
}

__device__ __forceinline__ float lerp2(float v00, float v01, float v10, float v11, float fx, float fy) {
  const float t = v00 + fx * (v01 - v00);
  const float b = v10 + fx * (v11 - v10);
  return t + fy * (b - t);
}

// a float2 image [h,w] at the integer (ix, iy) + fractions, per component
__device__ __forceinline__ float2 bilinear2(const float2* __restrict__ img, int h, int w, int ix, int iy, float fx, float fy) {
  int ix1, iy1;
  tap(w, ix, fx, ix1);
  tap(h, iy, fy, iy1);
  const float2* r0 = img + (size_t)iy * w;
  const float2* r1 = img + (size_t)iy1 * w;
  const float2 a = r0[ix], b = r0[ix1], c = r1[ix], d = r1[ix1];
  return make_float2(lerp2(a.x, b.x, c.x, d.x, fx, fy), lerp2(a.y, b.y, c.y, d.y, fx, fy));
}

// ---- pyramid ---------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
of_grey_kernel(int n, const void* __restrict__ img, int channels, int is_u8, float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  float v[3];
  for (int c = 0; c < channels; ++c) {
    const size_t at = (size_t)i * channels + c;
    v[c] = is_u8 ? (float)static_cast<const unsigned char*>(img)[at] / 255.f : static_cast<const float*>(img)[at];
  }
  out[i] = channels == 1 ? v[0] : (0.299f * v[0] + 0.587f * v[1]) + 0.114f * v[2];
}

__device__ __forceinline__ float five(float p0, float p1, float p2, float p3, float p4) {
  return ((p0 + p4) + 4.f * (p1 + p3)) + 6.f * p2;
}

__global__ void __launch_bounds__(256)
of_down_kernel(int h, int w, const float* __restrict__ src, int h2, int w2, float* __restrict__ dst) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= h2 * w2) return;
  const int y = i / w2, x = i - y * w2;
  int cx[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) cx[d] = clampi(2 * x + d - 2, 0, w - 1);
  float rows[5];
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    const float* r = src + (size_t)clampi(2 * y + d - 2, 0, h - 1) * w;
    rows[d] = five(r[cx[0]], r[cx[1]], r[cx[2]], r[cx[3]], r[cx[4]]);
  }
  dst[i] = five(rows[0], rows[1], rows[2], rows[3], rows[4]) * (1.f / 256.f);
}

// ---- one level ---------------------------------------------------------------------------------------------------------------

struct Level {
  int h, w;            // this level
  int hc, wc;          // the coarser level (u_coarse), if any
  int radius, iters;
  int init_step, W0;   // init: the pixel (y step, x step) of the [H0,W0,2] array, divided by step
  const float* A;
  const float* B;
  const float2* u_coarse;  // null on the coarsest level
  const float2* init;      // null: start at 0 (looked at on the coarsest level only)
  float2* u_out;
  float* eig_out;  // null: not wanted (level 0 of the a -> b direction leaves the smaller eigenvalue of G / (2r+1)^2 here)
};

__global__ void __launch_bounds__(OF_BLOCK)
of_level_kernel(Level L) {
  __shared__ float sA[OF_RW * OF_RH], sIx[OF_RW * OF_RH], sIy[OF_RW * OF_RH];
#if FG_OPTFLOW_STAGED
  __shared__ float sB[OF_SW * OF_SH];
  __shared__ int s_red[4][4];
#endif
  const int h = L.h, w = L.w, r = L.radius;
  const int tx0 = blockIdx.x * OF_TW, ty0 = blockIdx.y * OF_TH;
  const int rw = OF_TW + 2 * r, rh = OF_TH + 2 * r;  // <= OF_RW, OF_RH: the host holds radius to OF_MAX_R
  for (int idx = threadIdx.x; idx < rw * rh; idx += OF_BLOCK) {
    const int j = idx / rw, i = idx - j * rw;
    const int cx = clampi(tx0 - r + i, 0, w - 1), cy = clampi(ty0 - r + j, 0, h - 1);
    const float* row = L.A + (size_t)cy * w;
    sA[idx] = row[cx];
    sIx[idx] = (row[min(cx + 1, w - 1)] - row[max(cx - 1, 0)]) * 0.5f;
    sIy[idx] = (L.A[(size_t)min(cy + 1, h - 1) * w + cx] - L.A[(size_t)max(cy - 1, 0) * w + cx]) * 0.5f;
  }
  const int lx = threadIdx.x & (OF_TW - 1), ly = threadIdx.x / OF_TW;
  const int x = tx0 + lx, y = ty0 + ly;
  const bool live = x < w && y < h;
  // the start
  float ux = 0.f, uy = 0.f;
  if (live) {
    if (L.u_coarse) {
      const float2 c = bilinear2(L.u_coarse, L.hc, L.wc, x >> 1, y >> 1, 0.5f * (float)(x & 1), 0.5f * (float)(y & 1));
      ux = 2.f * c.x, uy = 2.f * c.y;
    } else if (L.init) {
      const float2 c = L.init[(size_t)(y * L.init_step) * L.W0 + (size_t)x * L.init_step];
      const float s = 1.f / (float)L.init_step;
      ux = c.x * s, uy = c.y * s;
    }
  }
  __syncthreads();
  // G: the window's sums, row by row
  float gxx = 0.f, gxy = 0.f, gyy = 0.f;
  const int base = (ly + r) * rw + (lx + r);  // the pixel itself
  if (live) {
    for (int qy = -r; qy <= r; ++qy)
      for (int qx = -r; qx <= r; ++qx) {
        const float gx = sIx[base + qy * rw + qx], gy = sIy[base + qy * rw + qx];
        gxx = gxx + gx * gx;
        gxy = gxy + gx * gy;
        gyy = gyy + gy * gy;
      }
  }
  gxx += OF_LAMBDA, gyy += OF_LAMBDA;
  const float det = gxx * gyy - gxy * gxy;
#pragma unroll 1
  for (int it = 0; it < L.iters; ++it) {
    int x0, y0;
    float fx, fy;
    split(ux, x0, fx);
    split(uy, y0, fy);
#if FG_OPTFLOW_STAGED
    // the tile's range of floor(u) -> the region of B its taps fall in
    int lo_x = live ? x0 : 0x7FFFFFFF, lo_y = live ? y0 : 0x7FFFFFFF, hi_x = live ? x0 : -0x7FFFFFFF, hi_y = live ? y0 : -0x7FFFFFFF;
#pragma unroll
    for (int m = 32; m > 0; m >>= 1) {
      lo_x = min(lo_x, __shfl_xor(lo_x, m)), lo_y = min(lo_y, __shfl_xor(lo_y, m));
      hi_x = max(hi_x, __shfl_xor(hi_x, m)), hi_y = max(hi_y, __shfl_xor(hi_y, m));
    }
    __syncthreads();  // the previous iteration's reads of sB and s_red are done
    if ((threadIdx.x & 63) == 0) {
      int* o = s_red[threadIdx.x >> 6];
      o[0] = lo_x, o[1] = lo_y, o[2] = hi_x, o[3] = hi_y;
    }
    __syncthreads();
    lo_x = min(min(s_red[0][0], s_red[1][0]), min(s_red[2][0], s_red[3][0]));
    lo_y = min(min(s_red[0][1], s_red[1][1]), min(s_red[2][1], s_red[3][1]));
    hi_x = max(max(s_red[0][2], s_red[1][2]), max(s_red[2][2], s_red[3][2]));
    hi_y = max(max(s_red[0][3], s_red[1][3]), max(s_red[2][3], s_red[3][3]));
    // image columns [sx0, sx0 + nw) and rows [sy0, sy0 + nh): what fits of the range's taps (|lo|, |hi| <= 32768: no overflow)
    const int sx0 = clampi(tx0 - r + lo_x, 0, w - 1), sy0 = clampi(ty0 - r + lo_y, 0, h - 1);
    const int nw = clampi(min(tx0 + OF_TW + r + hi_x + 1, w) - sx0, 0, OF_SW);
    const int nh = clampi(min(ty0 + OF_TH + r + hi_y + 1, h) - sy0, 0, OF_SH);
    for (int idx = threadIdx.x; idx < nw * nh; idx += OF_BLOCK) {
      const int j = idx / nw, i = idx - j * nw;
      sB[j * OF_SW + i] = L.B[(size_t)(sy0 + j) * w + (sx0 + i)];  // (sx0 + i < w, sy0 + j < h by nw, nh)
    }
    __syncthreads();
#endif
    if (live) {
      float bx = 0.f, by = 0.f;
      for (int qy = -r; qy <= r; ++qy) {
        int iy = clampi(y + qy, 0, h - 1) + y0, iy1;
        float fyq = fy;
        tap(h, iy, fyq, iy1);
        for (int qx = -r; qx <= r; ++qx) {
          int ix = clampi(x + qx, 0, w - 1) + x0, ix1;
          float fxq = fx;
          tap(w, ix, fxq, ix1);
#if FG_OPTFLOW_STAGED
          const bool in = ix >= sx0 && ix1 < sx0 + nw && iy >= sy0 && iy1 < sy0 + nh;
          float v00, v01, v10, v11;
          if (in) {
            const float* s0 = sB + (iy - sy0) * OF_SW - sx0;
            const float* s1 = sB + (iy1 - sy0) * OF_SW - sx0;
            v00 = s0[ix], v01 = s0[ix1], v10 = s1[ix], v11 = s1[ix1];
          } else {
            const float* r0 = L.B + (size_t)iy * w;
            const float* r1 = L.B + (size_t)iy1 * w;
            v00 = r0[ix], v01 = r0[ix1], v10 = r1[ix], v11 = r1[ix1];
          }
#else
          const float* r0 = L.B + (size_t)iy * w;
          const float* r1 = L.B + (size_t)iy1 * w;
          const float v00 = r0[ix], v01 = r0[ix1], v10 = r1[ix], v11 = r1[ix1];
#endif
          const int at = base + qy * rw + qx;
          const float dt = lerp2(v00, v01, v10, v11, fxq, fyq) - sA[at];
          bx = bx + dt * sIx[at];
          by = by + dt * sIy[at];
        }
      }
      ux = ux - (gyy * bx - gxy * by) / det;
      uy = uy - (gxx * by - gxy * bx) / det;
    }
  }
  if (live) {
    const size_t at = (size_t)y * w + x;
    L.u_out[at] = make_float2(ux, uy);
    if (L.eig_out) {
      const float d = gxx - gyy;
      L.eig_out[at] = ((gxx + gyy) - sqrtf(d * d + 4.f * (gxy * gxy))) * (0.5f / (float)((2 * r + 1) * (2 * r + 1)));
    }
  }
}

// ---- validity ----------------------------------------------------------------------------------------------------------------

__global__ void __launch_bounds__(256)
of_valid_kernel(int H, int W, const float2* __restrict__ u_ab, const float* __restrict__ eig, const float2* __restrict__ u_ba,
                float min_eig, float consistency, unsigned char* __restrict__ valid) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= H * W) return;
  const int y = i / W, x = i - y * W;
  const float2 u = u_ab[i];
  const float px = (float)x + u.x, py = (float)y + u.y;
  bool ok = eig[i] >= min_eig && px >= 0.f && px <= (float)(W - 1) && py >= 0.f && py <= (float)(H - 1);  // (a NaN: false)
  if (ok && u_ba) {
    int x0, y0;
    float fx, fy;
    split(u.x, x0, fx);
    split(u.y, y0, fy);
    const float2 back = bilinear2(u_ba, H, W, x + x0, y + y0, fx, fy);
    const float rx = u.x + back.x, ry = u.y + back.y;
    ok = sqrtf(rx * rx + ry * ry) <= consistency;
  }
  valid[i] = ok ? 1 : 0;
}

// ---- host --------------------------------------------------------------------------------------------------------------------

size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

struct Plan {
  int levels;
  int h[FG_OPTFLOW_MAX_LEVELS], w[FG_OPTFLOW_MAX_LEVELS];
  size_t pyr[FG_OPTFLOW_MAX_LEVELS];  // byte offset of a level inside one pyramid
  size_t pyr_bytes;                   // one pyramid
  size_t eig, u_ab[FG_OPTFLOW_MAX_LEVELS], u_ba[FG_OPTFLOW_MAX_LEVELS];  // offsets in the workspace (u_ab[0] unused: the output)
  size_t bytes;
};

// FG_OK and the plan, or why not
int plan_of(int H, int W, int levels, int both, Plan* out) {
  if (H <= 0 || W <= 0 || levels <= 0) return FG_ERR_INVALID_ARG;
  if (H < FG_OPTFLOW_MIN_SIDE || W < FG_OPTFLOW_MIN_SIDE || H > FG_OPTFLOW_MAX_SIDE || W > FG_OPTFLOW_MAX_SIDE) return FG_ERR_UNSUPPORTED;
  if (levels > FG_OPTFLOW_MAX_LEVELS) return FG_ERR_UNSUPPORTED;
  Plan p;
  p.levels = levels;
  size_t at = 0;
  for (int l = 0; l < levels; ++l) {
    p.h[l] = l ? (p.h[l - 1] + 1) / 2 : H, p.w[l] = l ? (p.w[l - 1] + 1) / 2 : W;
    p.pyr[l] = at;
    at += align256((size_t)p.h[l] * p.w[l] * sizeof(float));
  }
  if (std::min(p.h[levels - 1], p.w[levels - 1]) < FG_OPTFLOW_MIN_COARSEST) return FG_ERR_UNSUPPORTED;
  p.pyr_bytes = at;
  at = 2 * p.pyr_bytes;
  p.eig = at;
  at += align256((size_t)H * W * sizeof(float));
  for (int l = 0; l < levels; ++l) {
    const size_t u = align256((size_t)p.h[l] * p.w[l] * 2 * sizeof(float));
    p.u_ab[l] = at;
    if (l) at += u;
    p.u_ba[l] = at;
    if (both) at += u;
  }
  p.bytes = at;
  *out = p;
  return FG_OK;
}

int image_args(int channels, int dtype, const void* img) {
  if (channels != 1 && channels != 3) return FG_ERR_INVALID_ARG;
  if (dtype != FG_TARGET_U8 && dtype != FG_TARGET_F32) return FG_ERR_INVALID_ARG;
  if (dtype == FG_TARGET_U8 && channels == 1) return FG_ERR_UNSUPPORTED;
  if (!img || (dtype == FG_TARGET_F32 && !fg_args::aligned(img, 4))) return FG_ERR_INVALID_ARG;
  return FG_OK;
}

size_t image_bytes(int H, int W, int channels, int dtype) { return (size_t)H * W * channels * (dtype == FG_TARGET_F32 ? sizeof(float) : 1); }

void launch_pyramid(const Plan& p, int channels, int dtype, const void* img, char* pyr, hipStream_t st) {
  const int n = p.h[0] * p.w[0];
  hipLaunchKernelGGL(of_grey_kernel, dim3((n + 255) / 256), dim3(256), 0, st, n, img, channels, dtype == FG_TARGET_U8 ? 1 : 0,
                     reinterpret_cast<float*>(pyr));
  for (int l = 1; l < p.levels; ++l) {
    const int m = p.h[l] * p.w[l];
    hipLaunchKernelGGL(of_down_kernel, dim3((m + 255) / 256), dim3(256), 0, st, p.h[l - 1], p.w[l - 1],
                       reinterpret_cast<const float*>(pyr + p.pyr[l - 1]), p.h[l], p.w[l], reinterpret_cast<float*>(pyr + p.pyr[l]));
  }
}

// coarse to fine from the pyramid at `pa` to the one at `pb`; u[l]: where level l's flow goes
void launch_direction(const Plan& p, const char* pa, const char* pb, int radius, int iters, const float* init, float2* const* u, float* eig,
                      hipStream_t st) {
  for (int l = p.levels - 1; l >= 0; --l) {
    Level L;
    L.h = p.h[l], L.w = p.w[l];
    const bool top = l == p.levels - 1;
    L.hc = top ? 0 : p.h[l + 1], L.wc = top ? 0 : p.w[l + 1];
    L.radius = radius, L.iters = iters;
    L.init_step = 1 << (p.levels - 1), L.W0 = p.w[0];
    L.A = reinterpret_cast<const float*>(pa + p.pyr[l]), L.B = reinterpret_cast<const float*>(pb + p.pyr[l]);
    L.u_coarse = top ? nullptr : u[l + 1];
    L.init = top ? reinterpret_cast<const float2*>(init) : nullptr;
    L.u_out = u[l];
    L.eig_out = l == 0 ? eig : nullptr;
    hipLaunchKernelGGL(of_level_kernel, dim3((L.w + OF_TW - 1) / OF_TW, (L.h + OF_TH - 1) / OF_TH), dim3(OF_BLOCK), 0, st, L);
  }
}

using fg_args::aligned;
using fg_args::clash;

}  // namespace

extern "C" int fg_optflow_supported(int H, int W, int levels, int radius, int iters) {
  Plan p;
  return plan_of(H, W, levels, 0, &p) == FG_OK && radius >= 1 && radius <= FG_OPTFLOW_MAX_RADIUS && iters >= 1 &&
                 iters <= FG_OPTFLOW_MAX_ITERS
             ? 1
             : 0;
}

extern "C" size_t fg_optflow_workspace_bytes(int H, int W, int levels, int both_directions) {
  Plan p;
  if (plan_of(H, W, levels, both_directions != 0, &p) != FG_OK) return 0;
  return p.bytes;
}

extern "C" int fg_optflow_pyramid(int H, int W, int channels, int dtype, const void* img, int levels, void* workspace,
                                  size_t workspace_bytes, fg_stream_t stream) {
  Plan p;
  if (const int e = plan_of(H, W, levels, 0, &p)) return e;
  if (const int e = image_args(channels, dtype, img)) return e;
  if (!workspace || !aligned(workspace, 256)) return FG_ERR_INVALID_ARG;
  if (clash({{workspace, p.pyr_bytes}}, {{img, image_bytes(H, W, channels, dtype)}})) return FG_ERR_INVALID_ARG;
  if (workspace_bytes < p.pyr_bytes) return FG_ERR_WORKSPACE;
  launch_pyramid(p, channels, dtype, img, static_cast<char*>(workspace), fg_hip_stream(stream));
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

extern "C" int fg_optflow(int H, int W, int channels, int dtype, const void* a, const void* b, int levels, int iters, int radius,
                          float min_eig, int both_directions, float consistency, const float* init, float* flow, uint8_t* valid,
                          void* workspace, size_t workspace_bytes, fg_stream_t stream) {
  Plan p;
  const bool both = both_directions != 0;
  if (both_directions != 0 && both_directions != 1) return FG_ERR_INVALID_ARG;
  if (const int e = plan_of(H, W, levels, both, &p)) return e;
  if (radius <= 0 || iters <= 0) return FG_ERR_INVALID_ARG;
  if (radius > FG_OPTFLOW_MAX_RADIUS || iters > FG_OPTFLOW_MAX_ITERS) return FG_ERR_UNSUPPORTED;
  if (!(min_eig >= 0.f) || !(min_eig < INFINITY)) return FG_ERR_INVALID_ARG;
  if (both && (!(consistency >= 0.f) || !(consistency < INFINITY))) return FG_ERR_INVALID_ARG;
  if (const int e = image_args(channels, dtype, a)) return e;
  if (const int e = image_args(channels, dtype, b)) return e;
  if (!flow || !valid || !workspace || !aligned(flow, 8) || !aligned(init, 8) || !aligned(workspace, 256)) return FG_ERR_INVALID_ARG;
  const size_t img = image_bytes(H, W, channels, dtype), uv = (size_t)H * W * 2 * sizeof(float);
  if (clash({{flow, uv}, {valid, (size_t)H * W}, {workspace, p.bytes}}, {{a, img}, {b, img}, {init, init ? uv : 0}})) return FG_ERR_INVALID_ARG;
  if (workspace_bytes < p.bytes) return FG_ERR_WORKSPACE;
  hipStream_t st = fg_hip_stream(stream);
  char* ws = static_cast<char*>(workspace);
  char* pa = ws;
  char* pb = ws + p.pyr_bytes;
  launch_pyramid(p, channels, dtype, a, pa, st);
  launch_pyramid(p, channels, dtype, b, pb, st);
  float2* u_ab[FG_OPTFLOW_MAX_LEVELS];
  float2* u_ba[FG_OPTFLOW_MAX_LEVELS];
  for (int l = 0; l < p.levels; ++l) {
    u_ab[l] = l ? reinterpret_cast<float2*>(ws + p.u_ab[l]) : reinterpret_cast<float2*>(flow);
    u_ba[l] = reinterpret_cast<float2*>(ws + p.u_ba[l]);
  }
  float* eig = reinterpret_cast<float*>(ws + p.eig);
  launch_direction(p, pa, pb, radius, iters, init, u_ab, eig, st);
  if (both) launch_direction(p, pb, pa, radius, iters, nullptr, u_ba, nullptr, st);
  hipLaunchKernelGGL(of_valid_kernel, dim3(((size_t)H * W + 255) / 256), dim3(256), 0, st, H, W, reinterpret_cast<const float2*>(flow),
                     (const float*)eig, both ? (const float2*)u_ba[0] : nullptr, min_eig, consistency, valid);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}
