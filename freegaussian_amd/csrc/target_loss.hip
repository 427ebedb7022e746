// TL: the image loss of the training step taken straight from the RAW batch image: the target of csrc/loss.hip's loss --
// the batch image as floats, box-downscaled, composited over the step's background, masked -- is formed per pixel in
// registers while the loss kernels fill their LDS windows.  No target tensor exists anywhere.
//
//   per output pixel (y, x), channel c, downscale d (include/fgraster.h has the contract):
//     t_k   = mean of source channel k (uint8: v / 255; float32: as is) over the d x d source block at (y d, x d)
//     gt_c  = t_c (3 channels)  or  t_3 t_c + (1 - t_3) bg_c (4 channels: the composite AFTER the downscale)
//     m     = the same box mean of the mask (1 without one)
//     out   = { mean |gt m - pred m|, mean SSIM(pred m, gt m), mean (pred - gt)^2 }      (the last one UNMASKED: the PSNR's)
//     d/d pred = m (v_l1 L1 term + v_ssim SSIM term); out[2] carries no gradient
//
// The tiling, the two 11-tap passes, the SSIM pixel formula, the fixed-order reduction and the backward's structure are those
// of loss.hip, restated here so that loss.hip's kernels stay bit for bit what they are: only the LOADER differs (and a third
// sum rides along).  One 256-thread workgroup per 32 x 16 tile and channel; windows of 42 x 26 in LDS.
//
// Loads: neighbouring lanes take neighbouring output pixels of one row, so a lane's d-wide run of source pixels follows its
// neighbour's: every row of the d x d blocks is one contiguous stretch per wave.  A 4-channel uint8 pixel is one 32-bit load,
// a 4-channel float32 pixel one 128-bit load.
#include "arg_check.h"
#include "fg_common.h"

namespace {

constexpr int TW = 32, TH = 16;   // tile: 32 columns x 16 rows of pixels per 256-thread workgroup (two rows per thread)
constexpr int WIN = 11;           // taps
constexpr int HALO = WIN - 1;     // 10
constexpr int INW = TW + HALO;    // 42 input columns a tile needs
constexpr int INH = TH + HALO;    // 26 input rows
constexpr int INWP = INW + 1;     // padded LDS rows
constexpr int TWP = TW + 1;
constexpr float SSIM_C1 = 0.01f * 0.01f, SSIM_C2 = 0.03f * 0.03f;  // data_range = 1
constexpr int MAX_SIDE = 1 << 15;  // of the source: every pixel index stays far inside 64 bits, every grid inside 65535 rows

struct Window {
  float g[WIN];
};

Window gaussian_window() {
  Window w;
  double s = 0.0, v[WIN];
  for (int i = 0; i < WIN; ++i) {
    const double d = (double)(i - WIN / 2);
    v[i] = exp(-(d * d) / (2.0 * 1.5 * 1.5));
    s += v[i];
  }
  for (int i = 0; i < WIN; ++i) w.g[i] = (float)(v[i] / s);
  return w;
}

// what the kernels need of the descriptor
struct Source {
  const void* src;
  const void* mask;  // null: m = 1
  const float* bg;   // [3]; null with 3 channels
  int W0, d, mask_f32;
  float dd;  // d * d
};

// the target pixel and its mask value: see the head of the file.  F32: float32 source, else uint8; CH: its channels
template <bool F32, int CH>
__device__ __forceinline__ void target_pixel(const Source& s, int y, int x, int c, float& gt, float& m) {
  const int d = s.d;
  const size_t first = (size_t)y * d * s.W0 + (size_t)x * d;  // the block's first source pixel
  float tc, ta = 1.f;
  if constexpr (F32) {
    // (the sums in double: up to 64 floats add up exactly, so the mean is rounded once -- a flat block gives its own value back,
    //  which a running fp32 sum does not: 3 x 0.2f is not a float)
    const float* p = static_cast<const float*>(s.src);
    double ac = 0.0, aa = 0.0;
    for (int dy = 0; dy < d; ++dy)
      for (int dx = 0; dx < d; ++dx) {
        const size_t px = first + (size_t)dy * s.W0 + dx;
        if constexpr (CH == 4) {
          const float4 v = reinterpret_cast<const float4*>(p)[px];
          ac += (double)(c == 0 ? v.x : (c == 1 ? v.y : v.z));
          aa += (double)v.w;
        } else {
          ac += (double)p[px * 3 + c];
        }
      }
    tc = (float)(ac / (double)s.dd);
    ta = (float)(aa / (double)s.dd);
  } else {
    const unsigned char* p = static_cast<const unsigned char*>(s.src);
    unsigned ic = 0, ia = 0;  // (at most 64 x 255: exact)
    for (int dy = 0; dy < d; ++dy)
      for (int dx = 0; dx < d; ++dx) {
        const size_t px = first + (size_t)dy * s.W0 + dx;
        if constexpr (CH == 4) {
          const unsigned v = reinterpret_cast<const unsigned*>(p)[px];
          ic += (v >> (8 * c)) & 255u;
          ia += v >> 24;
        } else {
          ic += p[px * 3 + c];
        }
      }
    const float den = 255.f * s.dd;
    tc = (float)ic / den;
    ta = (float)ia / den;
  }
  gt = CH == 4 ? ta * tc + (1.f - ta) * s.bg[c] : tc;
  m = 1.f;
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
    m = (float)(am / (double)s.dd);
  }
}

// sums of three values over the 256 threads of a workgroup (fixed order)
__device__ __forceinline__ float3 block_sum3_256(float a, float b, float c, float3* scratch) {
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    a += __shfl_xor(a, m);
    b += __shfl_xor(b, m);
    c += __shfl_xor(c, m);
  }
  if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = make_float3(a, b, c);
  __syncthreads();
  return make_float3((scratch[0].x + scratch[1].x) + (scratch[2].x + scratch[3].x),
                     (scratch[0].y + scratch[1].y) + (scratch[2].y + scratch[3].y),
                     (scratch[0].z + scratch[1].z) + (scratch[2].z + scratch[3].z));
}

// H, W: the output (= pred) size; three channels.  maps null: the values alone (a pred that needs no gradient)
template <bool F32, int CH>
__global__ void __launch_bounds__(256)
target_loss_fwd_kernel(int H, int W, Window win, Source s, const float* __restrict__ pred, float* __restrict__ maps,
                       float4* __restrict__ partials) {
  constexpr int C = 3;
  __shared__ float sx[INH][INWP], sy[INH][INWP];
  __shared__ float hm[5][INH][TWP];
  __shared__ float3 red[4];
  const int c = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int Hm = H - HALO, Wm = W - HALO;
  // input window (zero outside the image: those taps only feed map pixels outside the map); the squared error of the tile's
  // own pixels is taken here, where the unmasked pair is in registers
  float mse = 0.f;
  for (int i = threadIdx.x; i < INH * INW; i += 256) {
    const int r = i / INW, q = i - r * INW;
    const int y = y0 + r, x = x0 + q;
    float a = 0.f, b = 0.f;
    if (y < H && x < W) {
      float gt, m;
      target_pixel<F32, CH>(s, y, x, c, gt, m);
      const float p = pred[((size_t)y * W + x) * C + c];
      if (r < TH && q < TW) mse += (p - gt) * (p - gt);
      a = p * m;
      b = gt * m;
    }
    sx[r][q] = a;
    sy[r][q] = b;
  }
  __syncthreads();
  // a thread's two pixels: column tx, rows 2 ty and 2 ty + 1 of the tile
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float l1 = 0.f;
#pragma unroll
  for (int o = 0; o < 2; ++o)
    if (y0 + 2 * ty + o < H && x0 + tx < W) l1 += fabsf(sy[2 * ty + o][tx] - sx[2 * ty + o][tx]);
  // horizontal pass: 26 rows x 32 columns x five moments; a thread takes FOUR neighbouring columns of a row
  if (threadIdx.x < INH * (TW / 4)) {
    const int r = threadIdx.x >> 3, q = (threadIdx.x & 7) * 4;
    float m[4][5];
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int v = 0; v < 5; ++v) m[o][v] = 0.f;
#pragma unroll
    for (int j = 0; j < WIN + 3; ++j) {
      const float a = sx[r][q + j], b = sy[r][q + j];
      const float aa = a * a, bb = b * b, ab = a * b;
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int k = j - o;
        if (k >= 0 && k < WIN) {
          const float g = win.g[k];
          m[o][0] = fmaf(g, a, m[o][0]);
          m[o][1] = fmaf(g, b, m[o][1]);
          m[o][2] = fmaf(g, aa, m[o][2]);
          m[o][3] = fmaf(g, bb, m[o][3]);
          m[o][4] = fmaf(g, ab, m[o][4]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int v = 0; v < 5; ++v) hm[v][r][q + o] = m[o][v];
  }
  __syncthreads();
  // vertical pass: the map pixels (y0 + 2 ty + {0, 1}, x0 + tx): twelve rows read once for the two
  float acc[2][5];
#pragma unroll
  for (int o = 0; o < 2; ++o)
#pragma unroll
    for (int v = 0; v < 5; ++v) acc[o][v] = 0.f;
#pragma unroll
  for (int j = 0; j < WIN + 1; ++j) {
    float h[5];
#pragma unroll
    for (int v = 0; v < 5; ++v) h[v] = hm[v][2 * ty + j][tx];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int k = j - o;
      if (k >= 0 && k < WIN) {
#pragma unroll
        for (int v = 0; v < 5; ++v) acc[o][v] = fmaf(win.g[k], h[v], acc[o][v]);
      }
    }
  }
  float ssim_sum = 0.f;
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    const int my = y0 + 2 * ty + o, mx = x0 + tx;
    if (my < Hm && mx < Wm) {
      const float mu1 = acc[o][0], mu2 = acc[o][1], exx = acc[o][2], eyy = acc[o][3], exy = acc[o][4];
      const float s1 = exx - mu1 * mu1, s2 = eyy - mu2 * mu2, s12 = exy - mu1 * mu2;
      const float A1 = 2.f * mu1 * mu2 + SSIM_C1, A2 = 2.f * s12 + SSIM_C2;
      const float B1 = mu1 * mu1 + mu2 * mu2 + SSIM_C1, B2 = s1 + s2 + SSIM_C2;
      const float iB1 = 1.f / B1, iB2 = 1.f / B2;
      const float ssim = (A1 * iB1) * (A2 * iB2);
      if (maps) {
        // partial derivatives of the map value: with respect to E[xx], E[xy] and mu_x -- the last one total (loss.hip)
        const float d_xx = -ssim * iB2;
        const float d_xy = 2.f * (A1 * iB1) * iB2;
        const float d_mu = 2.f * mu2 * (A2 * iB2) * iB1 - 2.f * mu1 * ssim * iB1 - 2.f * mu1 * d_xx - mu2 * d_xy;
        const size_t plane = (size_t)Hm * Wm, idx = (size_t)c * plane + (size_t)my * Wm + mx;
        maps[idx] = d_mu;
        maps[(size_t)C * plane + idx] = d_xx;
        maps[2 * (size_t)C * plane + idx] = d_xy;
      }
      ssim_sum += ssim;
    }
  }
  const float3 sums = block_sum3_256(l1, ssim_sum, mse, red);
  if (threadIdx.x == 0) {
    const int b = (blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    partials[b] = make_float4(sums.x, sums.y, sums.z, 0.f);
  }
}

// fixed-order reduction of the per-workgroup partial sums ({|x - y|, SSIM, (pred - gt)^2, unused} per workgroup) ->
// out[0] = mean |x - y|, out[1] = mean SSIM, out[2] = mean squared error
__global__ void __launch_bounds__(1024)
target_loss_reduce_kernel(int nb, const float4* __restrict__ partials, float inv_px, float inv_ssim, float* __restrict__ out) {
  __shared__ float3 red[16];
  float a[4] = {0.f, 0.f, 0.f, 0.f}, b[4] = {0.f, 0.f, 0.f, 0.f}, e[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = threadIdx.x; i < nb; i += 4096) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = i + u * 1024;
      const float4 v = j < nb ? partials[j] : make_float4(0.f, 0.f, 0.f, 0.f);
      a[u] += v.x;
      b[u] += v.y;
      e[u] += v.z;
    }
  }
  float sa = (a[0] + a[1]) + (a[2] + a[3]), sb = (b[0] + b[1]) + (b[2] + b[3]), se = (e[0] + e[1]) + (e[2] + e[3]);
#pragma unroll
  for (int m = 1; m < 64; m <<= 1) {
    sa += __shfl_xor(sa, m);
    sb += __shfl_xor(sb, m);
    se += __shfl_xor(se, m);
  }
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = make_float3(sa, sb, se);
  __syncthreads();
  if (threadIdx.x == 0) {
    float ta = 0.f, tb = 0.f, te = 0.f;
    for (int w = 0; w < 16; ++w) {
      ta += red[w].x;
      tb += red[w].y;
      te += red[w].z;
    }
    out[0] = ta * inv_px;
    out[1] = tb * inv_ssim;
    out[2] = te * inv_px;
  }
}

template <bool F32, int CH>
__global__ void __launch_bounds__(256)
target_loss_bwd_kernel(int H, int W, Window win, Source s, const float* __restrict__ pred, const float* __restrict__ maps,
                       const float* __restrict__ v_out, float inv_l1, float inv_ssim, float* __restrict__ v_pred) {
  constexpr int C = 3;
  __shared__ float sm[3][INH][INWP];
  __shared__ float hm[3][INH][TWP];
  const int c = blockIdx.z, x0 = blockIdx.x * TW, y0 = blockIdx.y * TH;
  const int Hm = H - HALO, Wm = W - HALO;
  const size_t plane = (size_t)Hm * Wm;
  // map window: the map pixels q in [p - 10, p] of the tile's pixels p (zero outside the map: 'full' borders)
  for (int i = threadIdx.x; i < INH * INW; i += 256) {
    const int r = i / INW, q = i - r * INW;
    const int y = y0 - HALO + r, x = x0 - HALO + q;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f;
    if (y >= 0 && y < Hm && x >= 0 && x < Wm) {
      const size_t o = (size_t)c * plane + (size_t)y * Wm + x;
      d0 = maps[o];
      d1 = maps[(size_t)C * plane + o];
      d2 = maps[2 * (size_t)C * plane + o];
    }
    sm[0][r][q] = d0;
    sm[1][r][q] = d1;
    sm[2][r][q] = d2;
  }
  __syncthreads();
  // (loss.hip: the three maps convolved with the symmetric window, four neighbouring columns per thread)
  if (threadIdx.x < INH * (TW / 4)) {
    const int r = threadIdx.x >> 3, q = (threadIdx.x & 7) * 4;
    float m[4][3];
#pragma unroll
    for (int o = 0; o < 4; ++o) m[o][0] = m[o][1] = m[o][2] = 0.f;
#pragma unroll
    for (int j = 0; j < WIN + 3; ++j) {
      const float d0 = sm[0][r][q + j], d1 = sm[1][r][q + j], d2 = sm[2][r][q + j];
#pragma unroll
      for (int o = 0; o < 4; ++o) {
        const int k = j - o;
        if (k >= 0 && k < WIN) {
          const float g = win.g[k];
          m[o][0] = fmaf(g, d0, m[o][0]);
          m[o][1] = fmaf(g, d1, m[o][1]);
          m[o][2] = fmaf(g, d2, m[o][2]);
        }
      }
    }
#pragma unroll
    for (int o = 0; o < 4; ++o)
#pragma unroll
      for (int v = 0; v < 3; ++v) hm[v][r][q + o] = m[o][v];
  }
  __syncthreads();
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  float acc[2][3] = {{0.f, 0.f, 0.f}, {0.f, 0.f, 0.f}};
#pragma unroll
  for (int j = 0; j < WIN + 1; ++j) {
    const float h0 = hm[0][2 * ty + j][tx], h1 = hm[1][2 * ty + j][tx], h2 = hm[2][2 * ty + j][tx];
#pragma unroll
    for (int o = 0; o < 2; ++o) {
      const int k = j - o;
      if (k >= 0 && k < WIN) {
        const float g = win.g[k];
        acc[o][0] = fmaf(g, h0, acc[o][0]);
        acc[o][1] = fmaf(g, h1, acc[o][1]);
        acc[o][2] = fmaf(g, h2, acc[o][2]);
      }
    }
  }
  const float v_l1 = v_out[0] * inv_l1, v_ssim = v_out[1] * inv_ssim;
#pragma unroll
  for (int o = 0; o < 2; ++o) {
    const int y = y0 + 2 * ty + o, x = x0 + tx;
    if (y < H && x < W) {
      const size_t idx = ((size_t)y * W + x) * C + c;
      // the pair the forward held in LDS, recomputed from the source: a = pred m, b = gt m
      float gt, m;
      target_pixel<F32, CH>(s, y, x, c, gt, m);
      const float a = pred[idx] * m, b = gt * m;
      const float sgn = a > b ? 1.f : (a < b ? -1.f : 0.f);  // d|b - a| / da
      const float g = v_l1 * sgn + v_ssim * (acc[o][0] + 2.f * a * acc[o][1] + b * acc[o][2]);
      v_pred[idx] = m == 0.f ? 0.f : m * g;  // (a pixel the mask blacks out: exactly zero, whatever the maps hold)
    }
  }
}

struct Shape {
  int H, W;          // the output's
  size_t src_bytes, mask_bytes;
  bool f32, mask_f32;
};

// FG_OK and the shape, or why not: INVALID_ARG for a descriptor that is malformed, UNSUPPORTED for one outside the range
int shape_of(const fg_target_desc* t, Shape* out) {
  if (!t || t->size != (int32_t)sizeof(fg_target_desc)) return FG_ERR_INVALID_ARG;
  if (t->src_dtype != FG_TARGET_U8 && t->src_dtype != FG_TARGET_F32) return FG_ERR_UNSUPPORTED;
  if (t->mask && t->mask_dtype != FG_TARGET_U8 && t->mask_dtype != FG_TARGET_F32) return FG_ERR_UNSUPPORTED;
  if (t->channels != 3 && t->channels != 4) return FG_ERR_UNSUPPORTED;
  const int d = t->downscale;
  if (d != 1 && d != 2 && d != 4 && d != 8) return FG_ERR_UNSUPPORTED;
  if (t->height <= 0 || t->width <= 0) return FG_ERR_INVALID_ARG;
  if (t->height > MAX_SIDE || t->width > MAX_SIDE) return FG_ERR_UNSUPPORTED;
  Shape s;
  s.H = t->height / d, s.W = t->width / d;
  if (s.H <= HALO || s.W <= HALO) return FG_ERR_UNSUPPORTED;
  s.f32 = t->src_dtype == FG_TARGET_F32, s.mask_f32 = t->mask_dtype == FG_TARGET_F32;
  const size_t px = (size_t)t->height * t->width;
  s.src_bytes = px * t->channels * (s.f32 ? sizeof(float) : 1);
  s.mask_bytes = t->mask ? px * (s.mask_f32 ? sizeof(float) : 1) : 0;
  *out = s;
  return FG_OK;
}

// the pointers of a descriptor whose shape is good
int pointers_ok(const fg_target_desc* t, const Shape& s) {
  if (!t->src) return FG_ERR_INVALID_ARG;
  if (t->channels == 4 && !t->background) return FG_ERR_INVALID_ARG;
  // whole pixels are loaded: a 4-channel pixel as one 32-bit (uint8) or 128-bit (float32) word
  const size_t unit = s.f32 ? (t->channels == 4 ? 16 : 4) : (t->channels == 4 ? 4 : 1);
  if (!fg_args::aligned(t->src, unit)) return FG_ERR_INVALID_ARG;
  if (t->mask && s.mask_f32 && !fg_args::aligned(t->mask, 4)) return FG_ERR_INVALID_ARG;
  if (t->background && !fg_args::aligned(t->background, 4)) return FG_ERR_INVALID_ARG;
  return FG_OK;
}

Source source_of(const fg_target_desc* t, const Shape& s) {
  Source r;
  r.src = t->src, r.mask = t->mask, r.bg = t->background;
  r.W0 = t->width, r.d = t->downscale, r.mask_f32 = s.mask_f32 ? 1 : 0;
  r.dd = (float)(t->downscale * t->downscale);
  return r;
}

size_t blocks_of(const Shape& s) { return (size_t)((s.W + TW - 1) / TW) * ((s.H + TH - 1) / TH) * 3; }

using fg_args::clash;

}  // namespace

extern "C" int fg_target_loss_supported(const fg_target_desc* target) {
  Shape s;
  return shape_of(target, &s) == FG_OK ? 1 : 0;
}

extern "C" size_t fg_target_loss_workspace_floats(const fg_target_desc* target) {
  Shape s;
  if (shape_of(target, &s) != FG_OK) return 0;
  return 4 * blocks_of(s);
}

extern "C" int fg_target_loss_fwd(const fg_target_desc* target, const float* pred, float* maps, float* workspace,
                                  size_t workspace_floats, float* out, fg_stream_t stream) {
  Shape sh;
  if (const int e = shape_of(target, &sh)) return e;
  if (const int e = pointers_ok(target, sh)) return e;
  if (!pred || !workspace || !out || !fg_args::aligned(workspace, 16)) return FG_ERR_INVALID_ARG;
  const size_t need = 4 * blocks_of(sh);
  const size_t image = (size_t)sh.H * sh.W * 3 * sizeof(float), map_bytes = (size_t)9 * (sh.H - HALO) * (sh.W - HALO) * sizeof(float);
  if (clash({{maps, map_bytes}, {workspace, need * sizeof(float)}, {out, 3 * sizeof(float)}},
            {{pred, image}, {target->src, sh.src_bytes}, {target->mask, sh.mask_bytes}, {target->background, 3 * sizeof(float)}}))
    return FG_ERR_INVALID_ARG;
  if (workspace_floats < need) return FG_ERR_WORKSPACE;
  static const Window win = gaussian_window();
  const dim3 grid((sh.W + TW - 1) / TW, (sh.H + TH - 1) / TH, 3);
  const int nb = (int)(grid.x * grid.y * grid.z);
  const Source s = source_of(target, sh);
  hipStream_t st = fg_hip_stream(stream);
  float4* partials = reinterpret_cast<float4*>(workspace);
#define FG_TL_FWD(F32, CH) \
  hipLaunchKernelGGL((target_loss_fwd_kernel<F32, CH>), grid, dim3(256), 0, st, sh.H, sh.W, win, s, pred, maps, partials)
  if (sh.f32) {
    if (target->channels == 4) FG_TL_FWD(true, 4);
    else FG_TL_FWD(true, 3);
  } else {
    if (target->channels == 4) FG_TL_FWD(false, 4);
    else FG_TL_FWD(false, 3);
  }
#undef FG_TL_FWD
  const float inv_px = (float)(1.0 / ((double)sh.H * sh.W * 3));
  const float inv_ssim = (float)(1.0 / ((double)(sh.H - HALO) * (sh.W - HALO) * 3));
  hipLaunchKernelGGL(target_loss_reduce_kernel, dim3(1), dim3(1024), 0, st, nb, (const float4*)partials, inv_px, inv_ssim, out);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

extern "C" int fg_target_loss_bwd(const fg_target_desc* target, const float* pred, const float* maps, const float* v_out,
                                  float* v_pred, fg_stream_t stream) {
  Shape sh;
  if (const int e = shape_of(target, &sh)) return e;
  if (const int e = pointers_ok(target, sh)) return e;
  if (!pred || !maps || !v_out || !v_pred) return FG_ERR_INVALID_ARG;
  const size_t image = (size_t)sh.H * sh.W * 3 * sizeof(float), map_bytes = (size_t)9 * (sh.H - HALO) * (sh.W - HALO) * sizeof(float);
  if (clash({{v_pred, image}}, {{pred, image}, {maps, map_bytes}, {v_out, 2 * sizeof(float)}, {target->src, sh.src_bytes},
                                {target->mask, sh.mask_bytes}, {target->background, 3 * sizeof(float)}}))
    return FG_ERR_INVALID_ARG;
  static const Window win = gaussian_window();
  const dim3 grid((sh.W + TW - 1) / TW, (sh.H + TH - 1) / TH, 3);
  const Source s = source_of(target, sh);
  const float inv_l1 = (float)(1.0 / ((double)sh.H * sh.W * 3));
  const float inv_ssim = (float)(1.0 / ((double)(sh.H - HALO) * (sh.W - HALO) * 3));
#define FG_TL_BWD(F32, CH)                                                                                                 \
  hipLaunchKernelGGL((target_loss_bwd_kernel<F32, CH>), grid, dim3(256), 0, fg_hip_stream(stream), sh.H, sh.W, win, s, pred, maps, \
                     v_out, inv_l1, inv_ssim, v_pred)
  if (sh.f32) {
    if (target->channels == 4) FG_TL_BWD(true, 4);
    else FG_TL_BWD(true, 3);
  } else {
    if (target->channels == 4) FG_TL_BWD(false, 4);
    else FG_TL_BWD(false, 3);
  }
#undef FG_TL_BWD
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}
