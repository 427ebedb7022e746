// CC: the metric-side colour correction (freegaussian_amd/bilagrid.py color_correct; reference freegaussian_model.py:935-937,
// :1024-1045), fused: the iterated per-channel quadratic fit of `img` to `ref` without a host round trip.
//
// As torch operators every one of the num_iters x 3 fits builds a [P,10] feature matrix, masks it, widens it to float64,
// copies it to the host and factors it there.  Here the fit is its normal equations: per channel c and iteration k
//
//   G_c = sum_m a a^T (10 x 10),  r_c = sum_m a ref_c     over the pixels m that are unclipped in img, x_k and ref
//
// summed in float64 by the float64 matrix instruction, and a 10 x 10 solve (color_correct_solve.h).
//
//   gram     one 256-thread workgroup per chunk of pixels (chunk_pixels below: a pure function of P).  A thread loads a
//            pixel, recomputes x_k from img through the k warps already solved (cc_chain: the ONE statement of that
//            arithmetic, shared with the last pass) and leaves (x_k, 1) and (ref, mask bits) in LDS.  A wave then feeds its
//            64 pixels, four at a time, to v_mfma_f64_16x16x4_f64: lane (j, i) = (lane >> 4, lane & 15) holds element i of
//            pixel j's row f = m ? [a(10), ref_c, 0 x 5] : 0 as BOTH operands, so one instruction adds f f^T of four
//            pixels: the 11 x 11 corner of the accumulator is G_c, r_c and ref^T ref.  Three accumulators (one per
//            channel) of 4 doubles per lane.  The workgroup adds its four waves in wave order and writes 3 x 121 doubles.
//   solve    one workgroup per channel: four groups of threads add every fourth partial block in ascending order, the
//            four sums are added as (0 + 1) + (2 + 3), and its first wave runs fg_cc_solve (64 lanes as the solver's: five disjoint
//            Jacobi rotations a round, no workgroup barrier).  The weights go to the workspace as
//            float32 (the torch path's w.to(x)), and to `warps` / `rank` where the caller asked.
//   apply    the last pass: out = x_{num_iters}, every pixel.
//
// No atomics and one order for every sum: two runs are bit for bit equal.  No intermediate image is written: pass k reads
// img and ref only.  num_iters + 1 streaming passes and num_iters solve launches, all asynchronous on the stream.
#include <algorithm>

#include "arg_check.h"
#include "color_correct_solve.h"
#include "fg_common.h"

namespace {

constexpr int BLOCK = 256;
constexpr int CHUNK = FG_COLOR_CORRECT_CHUNK_PIXELS;
constexpr int MAX_CHUNKS = FG_COLOR_CORRECT_MAX_CHUNKS;
constexpr int MAX_ITERS = FG_COLOR_CORRECT_MAX_ITERS;
constexpr int64_t MAX_P = (int64_t)16384 * 16384;
constexpr int ENTRIES = 121, ENTRY_STRIDE = 128;  // an 11 x 11 block per channel, padded
constexpr size_t HEAD_BYTES = 2048;               // warps [MAX_ITERS,10,3] float at 0, rank [MAX_ITERS,3] int32 at 1024
constexpr size_t RANK_AT = 1024;
static_assert(CHUNK % BLOCK == 0, "a chunk is whole rounds of the workgroup");
static_assert(MAX_ITERS * 30 * sizeof(float) <= RANK_AT && RANK_AT + MAX_ITERS * 3 * sizeof(int32_t) <= HEAD_BYTES, "head layout");

typedef double double4_t __attribute__((ext_vector_type(4)));

// pixels of one workgroup's chunk: FG_COLOR_CORRECT_CHUNK_PIXELS up to FG_COLOR_CORRECT_MAX_CHUNKS chunks, beyond that the
// least multiple of 256 that keeps the chunk count at or below it
__host__ __device__ inline int64_t chunk_pixels(int64_t P) {
  if (P <= (int64_t)CHUNK * MAX_CHUNKS) return CHUNK;
  const int64_t per = (P + MAX_CHUNKS - 1) / MAX_CHUNKS;
  return (per + BLOCK - 1) / BLOCK * BLOCK;
}
inline int64_t chunks_of(int64_t P) { return (P + chunk_pixels(P) - 1) / chunk_pixels(P); }

bool in_range(int64_t P, int num_iters, double eps) { return P >= 1 && P <= MAX_P && num_iters >= 1 && num_iters <= MAX_ITERS && eps > 0.0 && eps < 0.5; }

__device__ __forceinline__ bool unclipped(float z, float lo, float hi) { return z >= lo && z <= hi; }
__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }  // (a NaN stays a NaN, as torch.clamp)

// x_k from x_0 = img through the first k warps [k][10][3]: fp32 feature products, fp32 accumulation in feature order
__device__ __forceinline__ void cc_chain(float& x0, float& x1, float& x2, const float* __restrict__ warps, int k) {
  for (int it = 0; it < k; ++it) {
    const float* w = warps + it * 30;
    const float a[10] = {__fmul_rn(x0, x0), __fmul_rn(x0, x1), __fmul_rn(x0, x2), __fmul_rn(x1, x1), __fmul_rn(x1, x2),
                         __fmul_rn(x2, x2), x0, x1, x2, 1.f};
    float y0 = 0.f, y1 = 0.f, y2 = 0.f;
#pragma unroll
    for (int i = 0; i < 10; ++i) y0 = fmaf(a[i], w[3 * i], y0), y1 = fmaf(a[i], w[3 * i + 1], y1), y2 = fmaf(a[i], w[3 * i + 2], y2);
    x0 = clamp01(y0), x1 = clamp01(y1), x2 = clamp01(y2);
  }
}

// feature i = s[P_SEL[i]] * s[Q_SEL[i]] of s = (x0, x1, x2, 1): the products with 1 are exact
__device__ __forceinline__ int p_sel(int i) { return i < 3 ? 0 : (i < 5 ? 1 : (i == 5 ? 2 : (i < 9 ? i - 6 : 3))); }
__device__ __forceinline__ int q_sel(int i) { return i < 3 ? i : (i < 5 ? i - 2 : (i == 5 ? 2 : 3)); }

__global__ void __launch_bounds__(BLOCK)
gram_kernel(int64_t P, int64_t per_chunk, const float* __restrict__ img, const float* __restrict__ ref, int k, float lo, float hi,
            const float* __restrict__ warps, double* __restrict__ partials) {
  __shared__ float sx[BLOCK * 4];  // (x0, x1, x2, 1) of x_k
  __shared__ float sr[BLOCK * 4];  // (ref0, ref1, ref2, mask bits)
  __shared__ double red[4][3][256];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, i = lane & 15, j = lane >> 4;
  const int ps = i < 10 ? p_sel(i) : 3, qs = i < 10 ? q_sel(i) : 3;
  const int64_t base = (int64_t)blockIdx.x * per_chunk;
  double4_t acc[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) acc[c] = double4_t{0.0, 0.0, 0.0, 0.0};
  for (int64_t off = 0; off < per_chunk; off += BLOCK) {  // (uniform bounds: every thread reaches every barrier)
    const int64_t p = base + off + tid;
    float x0 = 0.f, x1 = 0.f, x2 = 0.f, r0 = 0.f, r1 = 0.f, r2 = 0.f;
    uint32_t m = 0;  // a pixel beyond P contributes zero rows
    if (p < P) {
      const size_t at = (size_t)p * 3;
      x0 = img[at], x1 = img[at + 1], x2 = img[at + 2];
      r0 = ref[at], r1 = ref[at + 1], r2 = ref[at + 2];
      m = (unclipped(x0, lo, hi) && unclipped(r0, lo, hi) ? 1u : 0u) | (unclipped(x1, lo, hi) && unclipped(r1, lo, hi) ? 2u : 0u) |
          (unclipped(x2, lo, hi) && unclipped(r2, lo, hi) ? 4u : 0u);
      cc_chain(x0, x1, x2, warps, k);
      m &= (unclipped(x0, lo, hi) ? 1u : 0u) | (unclipped(x1, lo, hi) ? 2u : 0u) | (unclipped(x2, lo, hi) ? 4u : 0u);
    }
    __syncthreads();  // the last round's reads are over
    sx[tid * 4] = x0, sx[tid * 4 + 1] = x1, sx[tid * 4 + 2] = x2, sx[tid * 4 + 3] = 1.f;
    sr[tid * 4] = r0, sr[tid * 4 + 1] = r1, sr[tid * 4 + 2] = r2, sr[tid * 4 + 3] = __uint_as_float(m);
    __syncthreads();
#pragma unroll 4
    for (int q = 0; q < 16; ++q) {
      const int pix = wave * 64 + q * 4 + j;
      const float feat = __fmul_rn(sx[pix * 4 + ps], sx[pix * 4 + qs]);
      const uint32_t mm = __float_as_uint(sr[pix * 4 + 3]);
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float v = i < 10 ? feat : (i == 10 ? sr[pix * 4 + c] : 0.f);
        const double f = (mm >> c) & 1u ? (double)v : 0.0;
        acc[c] = __builtin_amdgcn_mfma_f64_16x16x4f64(f, f, acc[c], 0, 0, 0);
      }
    }
  }
  // result element (row, col) = ((lane >> 4) + 4 reg, lane & 15)
#pragma unroll
  for (int c = 0; c < 3; ++c)
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) red[wave][c][(j + 4 * reg) * 16 + i] = acc[c][reg];
  __syncthreads();
  for (int e = tid; e < 3 * ENTRIES; e += BLOCK) {
    const int c = e / ENTRIES, rc = e - c * ENTRIES, row = rc / 11, col = rc - row * 11, at = row * 16 + col;
    partials[((size_t)blockIdx.x * 3 + c) * ENTRY_STRIDE + rc] = (red[0][c][at] + red[1][c][at]) + (red[2][c][at] + red[3][c][at]);
  }
}

// the solver's barrier for ONE wave: a wave's LDS operations complete in order, so the fence (the compiler waits for the
// outstanding ones and moves none across) is all its lanes need to see each other's writes
struct wave_sync {
  __device__ void operator()() const {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
  }
};

__global__ void __launch_bounds__(512)
solve_kernel(int chunks, int k, const double* __restrict__ partials, float* __restrict__ ws_warps, int32_t* __restrict__ ws_rank,
             float* __restrict__ warps_out, int32_t* __restrict__ rank_out) {
  __shared__ double part[4][ENTRY_STRIDE];
  __shared__ double G[100], r[10], w[10], work[FG_CC_WORK];
  const int c = blockIdx.x, tid = threadIdx.x, e = tid & 127, g = tid >> 7;
  double sum = 0.0;
  if (e < ENTRIES)
    for (int ch = g; ch < chunks; ch += 4) sum += partials[((size_t)ch * 3 + c) * ENTRY_STRIDE + e];
  part[g][e] = sum;
  __syncthreads();
  if (tid < ENTRIES) {
    const double v = (part[0][tid] + part[1][tid]) + (part[2][tid] + part[3][tid]);
    const int row = tid / 11, col = tid - row * 11;
    if (row < 10 && col < 10) G[row * 10 + col] = v;
    if (row < 10 && col == 10) r[row] = v;
  }
  __syncthreads();
  if (tid >= 64) return;  // (no barrier below: the first wave solves alone, its 64 lanes as the solver's)
  int rank = fg_cc_solve(G, r, w, work, tid, 64, wave_sync());
  for (int a = 0; a < 10; ++a)
    if (!isfinite((float)w[a])) rank = -1;
  if (tid < 10) {
    const float wf = (float)w[tid];
    ws_warps[(k * 10 + tid) * 3 + c] = wf;
    if (warps_out) warps_out[(k * 10 + tid) * 3 + c] = wf;
  }
  if (tid == 0) {
    ws_rank[k * 3 + c] = rank;
    if (rank_out) rank_out[k * 3 + c] = rank;
  }
}

__global__ void __launch_bounds__(BLOCK)
apply_kernel(int64_t P, const float* __restrict__ img, int num_iters, const float* __restrict__ warps, float* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
  if (p >= P) return;
  const size_t at = (size_t)p * 3;
  float x0 = img[at], x1 = img[at + 1], x2 = img[at + 2];
  cc_chain(x0, x1, x2, warps, num_iters);
  out[at] = x0, out[at + 1] = x1, out[at + 2] = x2;
}

using fg_args::clash;

}  // namespace

extern "C" size_t fg_color_correct_workspace_bytes(int64_t P, int num_iters) {
  if (!in_range(P, num_iters, 0.25)) return 0;
  // (room for min(ceil(P / CHUNK), MAX_CHUNKS) blocks: monotone in P, and never below the chunks_of(P) that are written)
  const int64_t blocks = std::min<int64_t>((P + CHUNK - 1) / CHUNK, MAX_CHUNKS);
  return HEAD_BYTES + (size_t)blocks * 3 * ENTRY_STRIDE * sizeof(double);
}

extern "C" int fg_color_correct(int64_t P, const float* img, const float* ref, int num_iters, double eps, float* out, float* warps,
                                int32_t* rank, void* workspace, size_t workspace_bytes, fg_stream_t stream) {
  if (!img || !ref || !out) return FG_ERR_INVALID_ARG;
  if (!in_range(P, num_iters, eps)) return FG_ERR_UNSUPPORTED;
  const size_t image = (size_t)P * 3 * sizeof(float), need = fg_color_correct_workspace_bytes(P, num_iters);
  const size_t n_warps = (size_t)num_iters * 30 * sizeof(float), n_rank = (size_t)num_iters * 3 * sizeof(int32_t);
  if (clash({{out, image}}, {{img, image}, {ref, image}})) return FG_ERR_INVALID_ARG;
  if (!workspace || !fg_args::aligned(workspace, 16)) return FG_ERR_INVALID_ARG;
  if (workspace_bytes < need) return FG_ERR_WORKSPACE;
  if (clash({{workspace, need}}, {{out, image}, {img, image}, {ref, image}})) return FG_ERR_INVALID_ARG;
  if (clash({{warps, n_warps}, {rank, n_rank}}, {{img, image}, {ref, image}, {out, image}, {workspace, need}})) return FG_ERR_INVALID_ARG;
  const float lo = (float)eps, hi = (float)(1.0 - eps);
  hipStream_t s = fg_hip_stream(stream);
  char* ws = static_cast<char*>(workspace);
  float* ws_warps = reinterpret_cast<float*>(ws);
  int32_t* ws_rank = reinterpret_cast<int32_t*>(ws + RANK_AT);
  double* partials = reinterpret_cast<double*>(ws + HEAD_BYTES);
  const int64_t per = chunk_pixels(P);
  const int chunks = (int)chunks_of(P);
  for (int k = 0; k < num_iters; ++k) {
    hipLaunchKernelGGL(gram_kernel, dim3(chunks), dim3(BLOCK), 0, s, P, per, img, ref, k, lo, hi, (const float*)ws_warps, partials);
    hipLaunchKernelGGL(solve_kernel, dim3(3), dim3(512), 0, s, chunks, k, (const double*)partials, ws_warps, ws_rank, warps, rank);
  }
  hipLaunchKernelGGL(apply_kernel, dim3((unsigned)((P + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, P, img, num_iters, (const float*)ws_warps, out);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

// test hook (bound in _lib._EXTRA, not in the header): fg_cc_solve on the HOST.  G [10,10], r [10] -> w [10], rank [1].
extern "C" int fg_debug_color_correct_solve(const double* G, const double* r, double* w, int32_t* rank) {
  if (!G || !r || !w || !rank) return FG_ERR_INVALID_ARG;
  *rank = fg_cc_solve_serial(G, r, w);
  return FG_OK;
}
