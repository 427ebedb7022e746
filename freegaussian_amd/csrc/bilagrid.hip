// BG: the bilateral-grid colour correction of a rendered training image, fused (freegaussian_amd/bilagrid.py
// apply_to_render; reference freegaussian_model.py:879-882).
//
//   out[p] = A(p)[:, :3] rgb[p] + A(p)[:, 3],   A(p) = trilinear slice of one camera's grid [12, GL, GY, GX] at
//            (fx, fy, fz) = (px / (W-1) (GX-1), py / (H-1) (GY-1), luma(rgb[p]) (GL-1)), border-clamped
//
// As torch operators this is an image-sized 3-D grid_sample that writes a [1,12,1,H,W] tensor of matrices (100 MB at
// 1920 x 1080, kept for the backward), a permute and a broadcast multiply; its backward scatters 8 x 12 float atomic
// adds per pixel into the 24 576 floats of the grid.  Here:
//
//   forward / v_rgb   one 256-thread workgroup per 256-pixel segment of an image row.  A row has ONE fy: the workgroup
//             blends the two grid rows it lies between once, for the few x nodes its segment touches, into LDS
//             ([x node][z][12], at most 48 KB), and a pixel then reads the four (x, z) corners of its cell: twelve
//             ds_read_b128.  The per-pixel matrices live in registers only.  The backward recomputes them.
//   v_grid    a GATHER, no atomics.  The pixel -> cell map is separable and monotone, so the pixels of the cell
//             (cy, cx) between four (y, x) nodes form a rectangle known in closed form (first_px below).  One workgroup
//             per cell and per chunk of FG_BILAGRID_CHUNK_PIXELS of its pixels (row-major inside the rectangle): a
//             lane keeps its four pixels in registers and walks the GL levels; per level it adds its pixels, in order,
//             into 4 corners x 12 sums, the wave adds its lanes (fg::wave_reduce_rows_lds: a fixed order; a level none
//             of the wave's pixels touches is skipped, its sums are 0), the workgroup its four waves in wave order
//             -> partials[chunk][z][corner, k][cell] in the caller's workspace.  A second
//             launch forms every element of v_grid as the sum over its (up to) four cells, in the order
//             (y-1, x-1), (y-1, x), (y, x-1), (y, x), and per cell over the chunks in ascending order.  Every sum has one
//             order: two runs are bit for bit equal, and a node no pixel reaches is exactly 0.
//
// Cells.  Along an axis with n nodes and S pixels a pixel p lies in cell c = min(floor(p (n-1) / (S-1)), n-2), in
// INTEGER arithmetic, with t = f - c in [0, 1] (f the correctly rounded fp32 quotient).  The last pixel sits on node
// n-1: cell n-2 with t = 1, which is torch's (i0 = i1 = n-1, t = 0) with the same weights.  first_px(c) =
// ceil(c (S-1) / (n-1)) is the same map inverted, so the gather and the slice agree on every pixel by construction.
#include <algorithm>

#include "arg_check.h"
#include "fg_common.h"

namespace {

constexpr int SEG = 256;                            // pixels of a row per workgroup of the slice kernels
constexpr int PPL = 4;                              // pixels per lane of the gather
constexpr int CHUNK = FG_BILAGRID_CHUNK_PIXELS;     // 256 lanes x PPL
static_assert(CHUNK == 256 * PPL, "a chunk is what one workgroup holds in registers");
constexpr int MAX_XY = 64, MAX_L = 16, MAX_IMAGE = 16384;
constexpr float LW_R = 0.299f, LW_G = 0.587f, LW_B = 0.114f;

__host__ __device__ __forceinline__ int first_px(int c, int S, int n) { return (c * (S - 1) + n - 2) / (n - 1); }
__host__ __device__ __forceinline__ int cell_of(int p, int S, int n) {
  const int c = p * (n - 1) / (S - 1);
  return c < n - 2 ? c : n - 2;
}
// one past the last pixel of cell c
__host__ __device__ __forceinline__ int end_px(int c, int S, int n) { return c == n - 2 ? S : first_px(c + 1, S, n); }

__device__ __forceinline__ float frac_of(int p, int S, int n, int c) {
  return __fdiv_rn((float)(p * (n - 1)), (float)(S - 1)) - (float)c;
}

// A pixel's own cell and fraction from that ONE quotient (no integer division per pixel).  f = p (n-1) / (S-1) <= 63 with
// S-1 < 16384: a quotient below an integer c is below it by at least 1 / (S-1) > 6e-5, sixteen times the rounding of f
// (2^-24 x 64 = 3.8e-6), so the correctly rounded f never reaches c from below and floor(f) IS cell_of's integer quotient.
__device__ __forceinline__ void cell_frac(int p, int S, int n, int& c, float& t) {
  const float f = __fdiv_rn((float)(p * (n - 1)), (float)(S - 1));
  c = min((int)f, n - 2);
  t = f - (float)c;
}

// guidance coordinate: level cell z0 in [0, GL-2], tz in [0, 1]; inside = torch's border rule for the gradient through fz
__device__ __forceinline__ void level_of(float r, float g, float b, int GL, int& z0, float& tz, bool& inside) {
  const float top = (float)(GL - 1);
  const float fz = (LW_R * r + LW_G * g + LW_B * b) * top;
  inside = fz > 0.f && fz < top;
  const float fc = fminf(fmaxf(fz, 0.f), top);
  z0 = min((int)floorf(fc), GL - 2);
  tz = fc - (float)z0;
}

// BWD = false: out = A rgb;  BWD = true: io = v_out, out = v_rgb
template <bool BWD>
__global__ void __launch_bounds__(SEG)
slice_kernel(int H, int W, int GX, int GY, int GL, const float* __restrict__ grid, const float* __restrict__ rgb,
             const float* __restrict__ v_out, float* __restrict__ out) {
  extern __shared__ float4 sg[];  // [x node][z][12] floats: the two grid rows around this image row, blended
  const int py = blockIdx.y, x0 = blockIdx.x * SEG, x1 = min(x0 + SEG, W);
  const int cy = cell_of(py, H, GY);
  const float ty = frac_of(py, H, GY, cy);
  const int cx_lo = cell_of(x0, W, GX), nodes = cell_of(x1 - 1, W, GX) - cx_lo + 2;
  {
    float* s = reinterpret_cast<float*>(sg);
    const int per_node = GL * 12, n = nodes * per_node;
    const size_t plane = (size_t)GY * GX;
    for (int e = threadIdx.x; e < n; e += SEG) {
      const int xn = e / per_node, rem = e - xn * per_node, z = rem / 12, k = rem - z * 12;
      const float* g = grid + ((size_t)k * GL + z) * plane + (size_t)cy * GX + (cx_lo + xn);
      s[e] = (1.f - ty) * g[0] + ty * g[GX];
    }
  }
  __syncthreads();
  const int px = x0 + threadIdx.x;
  if (px >= W) return;
  const size_t p = ((size_t)py * W + px) * 3;
  const float r = rgb[p], g = rgb[p + 1], b = rgb[p + 2];
  int cx, z0;
  float tx, tz;
  cell_frac(px, W, GX, cx, tx);
  bool inside;
  level_of(r, g, b, GL, z0, tz, inside);
  const float4* c00 = sg + ((cx - cx_lo) * GL + z0) * 3;  // (x, z), (x, z+1), (x+1, z), (x+1, z+1)
  const float4* c10 = c00 + GL * 3;
  float lo[12], hi[12];
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    const float4 a0 = c00[q], a1 = c00[3 + q], b0 = c10[q], b1 = c10[3 + q];
    const float ux = 1.f - tx;
    lo[4 * q + 0] = ux * a0.x + tx * b0.x, lo[4 * q + 1] = ux * a0.y + tx * b0.y;
    lo[4 * q + 2] = ux * a0.z + tx * b0.z, lo[4 * q + 3] = ux * a0.w + tx * b0.w;
    hi[4 * q + 0] = ux * a1.x + tx * b1.x, hi[4 * q + 1] = ux * a1.y + tx * b1.y;
    hi[4 * q + 2] = ux * a1.z + tx * b1.z, hi[4 * q + 3] = ux * a1.w + tx * b1.w;
  }
  float A[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) A[k] = (1.f - tz) * lo[k] + tz * hi[k];
  if (!BWD) {
#pragma unroll
    for (int j = 0; j < 3; ++j) out[p + j] = A[4 * j] * r + A[4 * j + 1] * g + A[4 * j + 2] * b + A[4 * j + 3];
  } else {
    const float v0 = v_out[p], v1 = v_out[p + 1], v2 = v_out[p + 2];
    float slope = 0.f;  // sum_k dA/dz[k] v[k / 4] (r, g, b, 1)[k % 4]
    if (inside) {
      const float v[3] = {v0, v1, v2};
#pragma unroll
      for (int j = 0; j < 3; ++j)
        slope += v[j] * ((hi[4 * j] - lo[4 * j]) * r + (hi[4 * j + 1] - lo[4 * j + 1]) * g + (hi[4 * j + 2] - lo[4 * j + 2]) * b +
                         (hi[4 * j + 3] - lo[4 * j + 3]));
      slope *= (float)(GL - 1);
    }
    out[p + 0] = A[0] * v0 + A[4] * v1 + A[8] * v2 + LW_R * slope;
    out[p + 1] = A[1] * v0 + A[5] * v1 + A[9] * v2 + LW_G * slope;
    out[p + 2] = A[2] * v0 + A[6] * v1 + A[10] * v2 + LW_B * slope;
  }
}

// partials[((chunk * GL + z) * 48 + corner * 12 + k) * ncells + cell], corner = 2 (y node is cy + 1) + (x node is cx + 1).
// A workgroup whose chunk starts beyond its cell's pixels writes nothing: the sum pass knows each cell's chunk count.
__global__ void __launch_bounds__(256)
grid_partials_kernel(int H, int W, int GX, int GY, int GL, const float* __restrict__ rgb, const float* __restrict__ v_out,
                     float* __restrict__ partials) {
  __shared__ float red[2][4][48];
  __shared__ __attribute__((aligned(16))) float rows[4][16 * fg::FG_RED_STRIDE];
  const int cell = blockIdx.x, ncells = gridDim.x, cx = cell % (GX - 1), cy = cell / (GX - 1);
  const int xa = first_px(cx, W, GX), nx = end_px(cx, W, GX) - xa;
  const int ya = first_px(cy, H, GY), ny = end_px(cy, H, GY) - ya;
  const int npx = nx * ny, base = blockIdx.y * CHUNK;
  if (base >= npx) return;  // (uniform)
  float r[PPL], g[PPL], b[PPL], v0[PPL], v1[PPL], v2[PPL], tx[PPL], ty[PPL], tz[PPL];
  int z0[PPL];
#pragma unroll
  for (int j = 0; j < PPL; ++j) {
    const int i = base + j * 256 + (int)threadIdx.x;
    r[j] = g[j] = b[j] = v0[j] = v1[j] = v2[j] = tx[j] = ty[j] = tz[j] = 0.f;
    z0[j] = -2;  // no level takes it
    if (i < npx) {
      const int row = i / nx, px = xa + (i - row * nx), py = ya + row;
      const size_t p = ((size_t)py * W + px) * 3;
      r[j] = rgb[p], g[j] = rgb[p + 1], b[j] = rgb[p + 2];
      v0[j] = v_out[p], v1[j] = v_out[p + 1], v2[j] = v_out[p + 2];
      tx[j] = frac_of(px, W, GX, cx), ty[j] = frac_of(py, H, GY, cy);
      bool inside;
      level_of(r[j], g[j], b[j], GL, z0[j], tz[j], inside);
    }
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int z = 0; z < GL; ++z) {
    float* mine = red[z & 1][wave];
    bool touched = false;
#pragma unroll
    for (int j = 0; j < PPL; ++j) touched |= z == z0[j] || z == z0[j] + 1;
    if (__any(touched)) {  // (wave-uniform: rendered images are coherent in luma, most levels see none of a wave's pixels)
      float acc[3][16];    // sum (corner, k) at [(12 corner + k) / 16][(12 corner + k) % 16]
#pragma unroll
      for (int i = 0; i < 48; ++i) acc[i >> 4][i & 15] = 0.f;
#pragma unroll
      for (int j = 0; j < PPL; ++j) {
        const float wz = z == z0[j] ? 1.f - tz[j] : (z == z0[j] + 1 ? tz[j] : 0.f);
        const float wc[4] = {wz * ((1.f - ty[j]) * (1.f - tx[j])), wz * ((1.f - ty[j]) * tx[j]), wz * (ty[j] * (1.f - tx[j])),
                             wz * (ty[j] * tx[j])};
        const float v[3] = {v0[j], v1[j], v2[j]};
        float u[12];
#pragma unroll
        for (int q = 0; q < 3; ++q) u[4 * q] = v[q] * r[j], u[4 * q + 1] = v[q] * g[j], u[4 * q + 2] = v[q] * b[j], u[4 * q + 3] = v[q];
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
          for (int k = 0; k < 12; ++k) acc[(c * 12 + k) >> 4][(c * 12 + k) & 15] = fmaf(wc[c], u[k], acc[(c * 12 + k) >> 4][(c * 12 + k) & 15]);
      }
      // the wave's 64 lanes per sum, through the wave's own LDS rows (fg::wave_reduce_rows_lds: a fixed order): sixteen sums
      // a pass, lane 4 q holds sum q
#pragma unroll
      for (int part = 0; part < 3; ++part) {
        const float s = fg::wave_reduce_rows_lds<16>(acc[part], rows[wave], lane);
        if ((lane & 3) == 0) mine[part * 16 + (lane >> 2)] = s;
      }
    } else if (lane < 48) {
      mine[lane] = 0.f;
    }
    __syncthreads();  // (one barrier per level: the buffers alternate, and the barrier of level z + 1 orders these reads
                      //  before level z + 2 writes the same buffer again)
    if (threadIdx.x < 48) {
      const float(*w)[48] = red[z & 1];
      const int i = threadIdx.x;
      partials[(((size_t)blockIdx.y * GL + z) * 48 + i) * ncells + cell] = (w[0][i] + w[1][i]) + (w[2][i] + w[3][i]);
    }
  }
}

__global__ void __launch_bounds__(256)
grid_sum_kernel(int H, int W, int GX, int GY, int GL, const float* __restrict__ partials, float* __restrict__ v_grid) {
  const int e = blockIdx.x * 256 + threadIdx.x, total = 12 * GL * GY * GX;
  if (e >= total) return;
  const int x = e % GX, y = (e / GX) % GY, z = (e / (GX * GY)) % GL, k = e / (GX * GY * GL);
  const int ncells = (GX - 1) * (GY - 1);
  float sum = 0.f;
#pragma unroll
  for (int dy = 1; dy >= 0; --dy)
#pragma unroll
    for (int dx = 1; dx >= 0; --dx) {
      const int cy = y - dy, cx = x - dx;
      if (cy < 0 || cy > GY - 2 || cx < 0 || cx > GX - 2) continue;
      const int npx = (end_px(cx, W, GX) - first_px(cx, W, GX)) * (end_px(cy, H, GY) - first_px(cy, H, GY));
      const int chunks = (npx + CHUNK - 1) / CHUNK, cell = cy * (GX - 1) + cx;
      const float* src = partials + ((size_t)z * 48 + (dy * 2 + dx) * 12 + k) * ncells + cell;
      for (int c = 0; c < chunks; ++c) sum += src[(size_t)c * GL * 48 * ncells];
    }
  v_grid[e] = sum;
}

bool grid_ok(int GX, int GY, int GL) { return GX >= 2 && GX <= MAX_XY && GY >= 2 && GY <= MAX_XY && GL >= 2 && GL <= MAX_L; }

int longest_cell(int S, int n) {
  int m = 0;
  for (int c = 0; c < n - 1; ++c) m = std::max(m, end_px(c, S, n) - first_px(c, S, n));
  return m;
}

int chunks_of(int H, int W, int GX, int GY) { return (longest_cell(W, GX) * longest_cell(H, GY) + CHUNK - 1) / CHUNK; }

size_t slice_lds_bytes(int W, int GX, int GL) {
  int nodes = 0;
  for (int x0 = 0; x0 < W; x0 += SEG) nodes = std::max(nodes, cell_of(std::min(x0 + SEG, W) - 1, W, GX) - cell_of(x0, W, GX) + 2);
  return (size_t)nodes * GL * 12 * sizeof(float);
}

using fg_args::clash;

}  // namespace

extern "C" int fg_bilagrid_supported(int GX, int GY, int GL) { return grid_ok(GX, GY, GL) ? 1 : 0; }

extern "C" size_t fg_bilagrid_bwd_workspace_bytes(int H, int W, int GX, int GY, int GL) {
  if (!grid_ok(GX, GY, GL) || H < 2 || W < 2 || H > MAX_IMAGE || W > MAX_IMAGE) return 0;
  return (size_t)chunks_of(H, W, GX, GY) * GL * 48 * (GX - 1) * (GY - 1) * sizeof(float);
}

extern "C" int fg_bilagrid_slice_fwd(int H, int W, int GX, int GY, int GL, const float* grid, const float* rgb, float* out,
                                     fg_stream_t stream) {
  if (H < 2 || W < 2 || !grid || !rgb || !out) return FG_ERR_INVALID_ARG;
  if (!grid_ok(GX, GY, GL) || H > MAX_IMAGE || W > MAX_IMAGE) return FG_ERR_UNSUPPORTED;
  const size_t image = (size_t)H * W * 3 * sizeof(float), table = (size_t)12 * GL * GY * GX * sizeof(float);
  if (clash({{out, image}}, {{rgb, image}, {grid, table}})) return FG_ERR_INVALID_ARG;
  const dim3 blocks((W + SEG - 1) / SEG, H);
  hipLaunchKernelGGL(slice_kernel<false>, blocks, dim3(SEG), slice_lds_bytes(W, GX, GL), fg_hip_stream(stream), H, W, GX, GY, GL,
                     grid, rgb, (const float*)nullptr, out);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

extern "C" int fg_bilagrid_slice_bwd(int H, int W, int GX, int GY, int GL, const float* grid, const float* rgb, const float* v_out,
                                     float* v_rgb, float* v_grid, void* workspace, size_t workspace_bytes, fg_stream_t stream) {
  if (H < 2 || W < 2 || !grid || !rgb || !v_out) return FG_ERR_INVALID_ARG;
  if (!grid_ok(GX, GY, GL) || H > MAX_IMAGE || W > MAX_IMAGE) return FG_ERR_UNSUPPORTED;
  const size_t image = (size_t)H * W * 3 * sizeof(float), table = (size_t)12 * GL * GY * GX * sizeof(float);
  const size_t need = fg_bilagrid_bwd_workspace_bytes(H, W, GX, GY, GL);
  if (clash({{v_rgb, image}, {v_grid, table}}, {{rgb, image}, {v_out, image}, {grid, table}})) return FG_ERR_INVALID_ARG;
  if (v_grid) {
    if (!workspace || !fg_args::aligned(workspace, 16)) return FG_ERR_INVALID_ARG;
    if (workspace_bytes < need) return FG_ERR_WORKSPACE;
    if (clash({{workspace, need}}, {{v_grid, table}, {rgb, image}, {v_out, image}, {v_rgb, image}, {grid, table}})) return FG_ERR_INVALID_ARG;
  }
  if (!v_rgb && !v_grid) return FG_OK;  // nothing asked for
  hipStream_t s = fg_hip_stream(stream);
  if (v_rgb) {
    const dim3 blocks((W + SEG - 1) / SEG, H);
    hipLaunchKernelGGL(slice_kernel<true>, blocks, dim3(SEG), slice_lds_bytes(W, GX, GL), s, H, W, GX, GY, GL, grid, rgb, v_out,
                       v_rgb);
  }
  if (v_grid) {
    float* partials = static_cast<float*>(workspace);
    const dim3 blocks((GX - 1) * (GY - 1), chunks_of(H, W, GX, GY));
    hipLaunchKernelGGL(grid_partials_kernel, blocks, dim3(256), 0, s, H, W, GX, GY, GL, rgb, v_out, partials);
    const int total = 12 * GL * GY * GX;
    hipLaunchKernelGGL(grid_sum_kernel, dim3((total + 255) / 256), dim3(256), 0, s, H, W, GX, GY, GL, (const float*)partials, v_grid);
  }
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}
