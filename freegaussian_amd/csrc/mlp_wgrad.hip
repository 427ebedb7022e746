// K10 parameter gradients (fg_mlp_param_grads): the [out, N] x [N, in] products of the fused MLP training path, from the
// arrays its other calls leave behind -- enc [N, enc_w], acts [8, N, 256] (h_l), g_pre [8, N, 256] (P_l), g_heads.
//
//   gW_l = P_l^T in_l   (in_0 = enc[:, :in_ch], in_5 = [enc[:, :in_ch], h_4], else h_{l-1}),   gb_l = sum of P_l over the rows,
//   gW_head = g_heads^T h_7,   gb_head = sum of g_heads over the rows.
//
// One call, two launches, no atomics:
//   slabs    : the rows are cut into n slabs of S rows (wg_cut: a function of N alone -- S <= 4096, a multiple of 64, the slabs
//              as equal as that allows; below 131 072 rows up to 32 shorter slabs, so that a small N still spreads over
//              the machine; 4096 and not the library path's 8192: at 240 000 rows the longer slabs left 1080 workgroups for
//              768 places, a quarter of the call spent in a half-empty second round -- profiles/mlp_wgrad.md).  A workgroup takes one job of one slab and stores its partial result into that slab's block
//              of the workspace with plain stores.
//   jobs     : a 128 x 128 tile of one product (28 tiles of the seven hidden products, 4 of the two 256 x in_ch input
//              products) or a 16 x 64 tile of the head product (4 per slab); jobs whose outputs are not asked for do
//              not exist.  The list is dealt to the 8 XCDs in contiguous runs (mlp_wgrad_kernel), so the tiles that share
//              operand rows share an L2.
//   tile     : four waves, each a 2 x 2 block of v_mfma_f32_32x32x2_f32 (exact fp32, 64 accumulator registers).  The A lane
//              (i, k) wants P[row k][col i], the B lane (k, j) wants in[row k][col j]: both operands are read along the
//              rows as they are stored -- 32 rows x 128 columns of each go to LDS per step (row stride 160 floats: the two
//              lane halves read rows k and k + 1, 32 banks apart), the next step's rows are fetched into registers before
//              the 64 MFMAs of the current one.  Nothing is transposed.  An output element is ONE fmaf chain over the
//              slab's rows in row order: at most 4096 terms.
//   bias     : the column sums of a P tile are taken from the LDS copy of the job with column tile 0 (two 16-row partial
//              sums per step, added in a fixed order): g_pre is read for them no second time.  A bias whose weight is
//              not asked for gets a job that stages P alone.
//   heads    : v_mfma_f32_16x16x4_f32: A lane (i, k) = g_heads[row k][i] (zero from rows_total on), B lane (k, j) = h_7[row k][col j],
//              one 16-column block per wave, 32 rows' operands in flight per step; the head bias from the A operands of
//              wave 0 of the first tile.
//   reduce   : one lane per element of the slab block adds the n partials in slab order and writes the output element
//              in nn.Linear's layout with a scalar store (the rows of weight[0] / weight[5] have odd strides); the pad
//              columns k >= in_ch of the input products, and elements of outputs not asked for, are not looked at.
// Rows beyond a slab's end (so beyond N) are never read: both operand tiles hold zeros there.  Columns k >= in_ch of enc
// are replaced by zeros as they are read.  Two runs on the same inputs are bit for bit equal, whatever else the device does.
// fg_mlp_param_grads_p / fg_mlp_train_bwd_p take a precision word for the hidden and input products: FG_MLP_FP32 is all of the
// above (the old entry points pass it); FG_MLP_BF16X3 runs the tile jobs as split-bf16 products in a kernel of their own
// (mlp_wgrad_split_kernel, further down), everything else unchanged.
#include "fg_common.h"
#include "mlp_internal.h"

namespace {

constexpr int WG_W = 256, WG_D = 8, WG_SKIP = 4, WG_XCH = 63;
constexpr int WG_BLOCK = 256;
constexpr int WG_T = 128;            // output tile
constexpr int WG_K = 32;             // rows per step
constexpr int WG_STRIDE = WG_T + 32;  // LDS row stride: rows k and k + 1 land 32 banks apart
constexpr int WG_MAX_SLAB = FG_MLP_WGRAD_MAX_SLAB, WG_MIN_SPLIT = FG_MLP_WGRAD_MIN_SPLIT, WG_MIN_SLABS = 32;

// one slab's block of the workspace (floats)
constexpr size_t WG_OFF_IN = (size_t)(WG_D - 1) * WG_W * WG_W;  // hidden products of layers 1..7 in front
constexpr size_t WG_OFF_BIAS = WG_OFF_IN + 2 * (size_t)WG_W * WG_T;  // input products of layers 0 and 5: [256][128]
constexpr size_t WG_OFF_HW = WG_OFF_BIAS + (size_t)WG_D * WG_W;
constexpr size_t WG_OFF_HB = WG_OFF_HW + 16 * (size_t)WG_W;
constexpr size_t WG_SLAB_FLOATS = WG_OFF_HB + 16;

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

inline int64_t wg_ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

// the most slabs any N' <= N is cut into: what the workspace is sized for (monotone in N)
inline int64_t wg_slab_bound(int64_t N) {
  const int64_t small = wg_ceil_div(N, WG_MIN_SPLIT), big = wg_ceil_div(N, WG_MAX_SLAB);
  const int64_t few = small < WG_MIN_SLABS ? small : WG_MIN_SLABS;
  return big > few ? big : few;
}

// the cut of N rows: slab length (a multiple of 64, <= 4096) and the number of slabs; nothing but N goes in
inline void wg_cut(int64_t N, int* rows, int64_t* slabs) {
  const int64_t want = wg_slab_bound(N);
  const int64_t S = wg_ceil_div(wg_ceil_div(N, want), 64) * 64;
  *rows = (int)S;
  *slabs = wg_ceil_div(N, S);
}

enum : uint32_t { WG_JOB_TILE = 0, WG_JOB_HEAD = 1 };
// a job in one word: type | layer << 4 | row tile << 8 | column tile << 12 | flags << 16
enum : uint32_t { WG_F_GEMM = 1, WG_F_BIAS = 2, WG_F_ENC = 4 };
constexpr int WG_MAX_JOBS = 40;

struct WgArgs {
  const float* enc;
  const float* acts;
  const float* g_pre;
  const float* g_heads;
  float* ws;
  // the launch takes n_slabs slabs from slab0 on (the partial blocks sit at the slabs' own indices); g_pre has pre_rows rows
  // to a layer and starts at row pre_row0 of the other arrays (fg_mlp_param_grads: 0, n_slabs = all, pre_rows = N)
  int64_t N, n_slabs, slab0, pre_rows, pre_row0;
  int slab_rows, n_jobs;
  int in_ch, enc_w, rows_total;
  uint32_t jobs[WG_MAX_JOBS];
};

struct WgOut {
  float* weight[WG_D];
  float* bias[WG_D];
  float* head_weight[FG_MLP_MAX_HEADS];
  float* head_bias[FG_MLP_MAX_HEADS];
  int head_rows[FG_MLP_MAX_HEADS];
  int n_heads, in_ch;
};

// 32 rows x 128 columns of a row-major array (row stride ld floats, 16-byte aligned rows) into registers: thread t takes
// the four floats at column 4 (t & 31) of rows (t >> 5) + 8 q.  Rows from `end` on, and columns from `cols_ld` (how many the
// row has in memory, a multiple of 4) on, are zeros and are not read.  Nothing here looks at the loaded values, so the loads
// stay in flight across the step's MFMAs; wg_stage is where they are waited for.
__device__ __forceinline__ void wg_fetch(f32x4 (&v)[4], const float* __restrict__ src, int64_t ld, int64_t row0, int64_t end,
                                         int col0, int cols_ld, int tid) {
  const int c = 4 * (tid & 31);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int64_t row = row0 + (tid >> 5) + 8 * q;
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (row < end && c < cols_ld) r = *reinterpret_cast<const f32x4*>(src + row * ld + col0 + c);
    v[q] = r;
  }
}

// ... and to LDS; columns from `cols` on (the pad of enc) are replaced by zeros on the way
__device__ __forceinline__ void wg_stage(float* tile, const f32x4 (&v)[4], int cols, int tid) {
  const int c = 4 * (tid & 31);
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    f32x4 r = v[q];
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (c + e >= cols) r[e] = 0.f;
    *reinterpret_cast<f32x4*>(tile + ((tid >> 5) + 8 * q) * WG_STRIDE + c) = r;
  }
}

__device__ __forceinline__ void wg_tile_job(const WgArgs& p, uint32_t job, int64_t r0, int64_t r1, float* __restrict__ ws,
                                            float* As, float* Bs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l = (job >> 4) & 15, it = (job >> 8) & 15, jt = (job >> 12) & 15;
  const uint32_t flags = job >> 16;
  const bool gemm = flags & WG_F_GEMM, bias = flags & WG_F_BIAS, from_enc = flags & WG_F_ENC;

  const float* a_src = p.g_pre + (int64_t)l * p.pre_rows * WG_W;
  const int64_t a_r0 = r0 - p.pre_row0, a_r1 = r1 - p.pre_row0;  // the slab's rows as g_pre counts them
  const float* b_src = from_enc ? p.enc : p.acts + (int64_t)(l > 0 ? l - 1 : 0) * p.N * WG_W;
  const int64_t b_ld = from_enc ? p.enc_w : WG_W;
  const int b_col0 = from_enc ? 0 : jt * WG_T;
  const int b_cols = from_enc ? p.in_ch : WG_T, b_cols_ld = from_enc ? p.enc_w : WG_T;  // columns kept / in memory

  f32x16 acc[2][2];
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
  float bsum = 0.f;

  const int li = lane & 31, lh = lane >> 5;
  const float* a_rd = As + lh * WG_STRIDE + (wave >> 1) * 64 + li;
  const float* b_rd = Bs + lh * WG_STRIDE + (wave & 1) * 64 + li;
  const float* s_rd = As + (tid >> 7) * 16 * WG_STRIDE + (tid & 127);

  f32x4 va[4], vb[4];
  wg_fetch(va, a_src, WG_W, a_r0, a_r1, it * WG_T, WG_T, tid);
  if (gemm) wg_fetch(vb, b_src, b_ld, r0, r1, b_col0, b_cols_ld, tid);
  for (int64_t row = r0; row < r1; row += WG_K) {
    wg_stage(As, va, WG_T, tid);
    if (gemm) wg_stage(Bs, vb, b_cols, tid);
    __syncthreads();
    if (row + WG_K < r1) {
      wg_fetch(va, a_src, WG_W, row + WG_K - p.pre_row0, a_r1, it * WG_T, WG_T, tid);
      if (gemm) wg_fetch(vb, b_src, b_ld, row + WG_K, r1, b_col0, b_cols_ld, tid);
    }
    if (bias) {
      // this thread's column of P over 16 of the step's rows, in row order
      float s = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) s += s_rd[k * WG_STRIDE];
      bsum += s;
    }
    if (gemm) {
      // the operands of row pair kk + 1 are read before the four MFMAs of pair kk
      float a0 = a_rd[0], a1 = a_rd[32], b0 = b_rd[0], b1 = b_rd[32];
#pragma unroll 4
      for (int kk = 0; kk < WG_K / 2; ++kk) {
        const int nx = ((kk + 1) & (WG_K / 2 - 1)) * 2 * WG_STRIDE;  // (the last pair reads the first again: not used)
        const float na0 = a_rd[nx], na1 = a_rd[nx + 32], nb0 = b_rd[nx], nb1 = b_rd[nx + 32];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        a0 = na0, a1 = na1, b0 = nb0, b1 = nb1;
      }
    }
    __syncthreads();
  }

  if (gemm) {
    // C/D map of the 32x32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    float* out = from_enc ? ws + WG_OFF_IN + (size_t)(l == 0 ? 0 : 1) * WG_W * WG_T : ws + (size_t)(l - 1) * WG_W * WG_W;
    const int ld = from_enc ? WG_T : WG_W;
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = it * WG_T + (wave >> 1) * 64 + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * lh;
          const int j = b_col0 + (wave & 1) * 64 + 32 * b + li;
          out[(size_t)i * ld + j] = acc[a][b][e];
        }
  }
  if (bias) {
    // rows 0..15 of every step, then rows 16..31: the two halves meet through LDS (free after the loop's last barrier)
    if (tid >= 128) As[tid & 127] = bsum;
    __syncthreads();
    if (tid < 128) ws[WG_OFF_BIAS + (size_t)l * WG_W + it * WG_T + tid] = bsum + As[tid];
  }
}

// a 16 x 64 tile of g_heads^T h_7 (column tile ct); tile 0 also sums g_heads over the rows
__device__ __forceinline__ void wg_head_job(const WgArgs& p, uint32_t job, int64_t r0, int64_t r1, float* __restrict__ ws,
                                            float* red) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int ct = (job >> 12) & 15;
  const uint32_t flags = job >> 16;
  const bool gemm = flags & WG_F_GEMM, bias = (flags & WG_F_BIAS) && wave == 0;
  const int hi = lane & 15, hq = lane >> 4;
  const int col = ct * 64 + wave * 16 + hi;
  const float* h7 = p.acts + (int64_t)(WG_D - 1) * p.N * WG_W;
  const bool a_live = hi < p.rows_total;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  float bsum = 0.f;
  for (int64_t row = r0; row < r1; row += WG_K) {
    float a[8], b[8];
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      const int64_t r = row + 4 * s + hq;
      a[s] = (r < r1 && a_live) ? p.g_heads[r * p.rows_total + hi] : 0.f;
      b[s] = (r < r1 && gemm) ? h7[r * WG_W + col] : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 8; ++s) {
      if (gemm) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[s], b[s], acc, 0, 0, 0);
      if (bias) bsum += a[s];
    }
  }
  // C/D map of the 16x16 MFMA: column = lane & 15, row = 4 (lane >> 4) + e
  if (gemm)
    for (int e = 0; e < 4; ++e) ws[WG_OFF_HW + (size_t)(4 * hq + e) * WG_W + col] = acc[e];
  if (flags & WG_F_BIAS) {
    if (wave == 0) red[lane] = bsum;
    __syncthreads();
    if (tid < 16) ws[WG_OFF_HB + tid] = ((red[tid] + red[16 + tid]) + red[32 + tid]) + red[48 + tid];
  }
}

__global__ void __launch_bounds__(WG_BLOCK) mlp_wgrad_kernel(WgArgs p) {
  __shared__ __attribute__((aligned(16))) float As[WG_K * WG_STRIDE];
  __shared__ __attribute__((aligned(16))) float Bs[WG_K * WG_STRIDE];
  // Workgroup ids go round the chip's 8 XCDs in turn, each with an L2 of its own.  The (slab, job) list is dealt out in
  // eight contiguous runs, one per XCD, so that the four tiles of one product over one slab -- which read every operand
  // row twice between them -- start side by side behind one L2.  A pure renumbering: what a job computes does not change.
  const int64_t total = p.n_slabs * p.n_jobs, run = (total + 7) / 8;
  const int64_t id = (int64_t)(blockIdx.x & 7) * run + (blockIdx.x >> 3);
  if (id >= total) return;
  const int64_t slab = p.slab0 + id / p.n_jobs;
  const uint32_t job = p.jobs[id % p.n_jobs];
  const int64_t r0 = slab * p.slab_rows;
  const int64_t r1 = r0 + p.slab_rows < p.N ? r0 + p.slab_rows : p.N;
  float* ws = p.ws + (size_t)slab * WG_SLAB_FLOATS;
  if ((job & 15) == WG_JOB_HEAD)
    wg_head_job(p, job, r0, r1, ws, As);
  else
    wg_tile_job(p, job, r0, r1, ws, As, Bs);
}

// one lane per element of a slab block: where it belongs in the outputs (null: nowhere), then the partials in slab order
__global__ void __launch_bounds__(WG_BLOCK) mlp_wgrad_reduce_kernel(const float* __restrict__ ws, int64_t n_slabs, WgOut o) {
  const size_t at = (size_t)blockIdx.x * WG_BLOCK + threadIdx.x;
  if (at >= WG_SLAB_FLOATS) return;
  float* dst = nullptr;
  if (at < WG_OFF_IN) {
    const int l = 1 + (int)(at / (WG_W * WG_W)), i = (int)(at / WG_W) % WG_W, j = (int)(at % WG_W);
    if (o.weight[l]) dst = l == WG_SKIP + 1 ? o.weight[l] + (size_t)i * (o.in_ch + WG_W) + o.in_ch + j : o.weight[l] + (size_t)i * WG_W + j;
  } else if (at < WG_OFF_BIAS) {
    const size_t rel = at - WG_OFF_IN;
    const int l = rel < (size_t)WG_W * WG_T ? 0 : WG_SKIP + 1, i = (int)(rel / WG_T) % WG_W, j = (int)(rel % WG_T);
    if (o.weight[l] && j < o.in_ch) dst = o.weight[l] + (size_t)i * (l == 0 ? o.in_ch : o.in_ch + WG_W) + j;
  } else if (at < WG_OFF_HW) {
    const size_t rel = at - WG_OFF_BIAS;
    if (o.bias[rel / WG_W]) dst = o.bias[rel / WG_W] + rel % WG_W;
  } else {
    const bool is_w = at < WG_OFF_HB;
    const int row = is_w ? (int)((at - WG_OFF_HW) / WG_W) : (int)(at - WG_OFF_HB), k = is_w ? (int)((at - WG_OFF_HW) % WG_W) : 0;
    int v = 0;
    for (int h = 0; h < o.n_heads; ++h) {
      if (row >= v && row < v + o.head_rows[h]) {
        if (is_w && o.head_weight[h]) dst = o.head_weight[h] + (size_t)(row - v) * WG_W + k;
        if (!is_w && o.head_bias[h]) dst = o.head_bias[h] + (row - v);
      }
      v += o.head_rows[h];
    }
  }
  if (!dst) return;
  const float* src = ws + at;
  float s = src[0];
  for (int64_t b = 1; b < n_slabs; ++b) s += src[(size_t)b * WG_SLAB_FLOATS];
  *dst = s;
}

// ---- wgrad_precision = FG_MLP_BF16X3: the same jobs, slabs, partial blocks and reduction; the 128 x 128 tile job on
// v_mfma_f32_32x32x16_bf16, every operand as hi + lo (the contract: include/fgraster.h).  The head jobs are wg_head_job above.
//   k order  : the contraction runs over the ROWS, so a bf16 fragment wants 8 consecutive rows of one column in one lane: the A
//              lane (i, h) holds P[rows 16 s + 8 h + j][col i], the B lane (h, j') in[rows 16 s + 8 h + j][col j'], j = 0..7.
//   step     : 64 rows.  Thread t fetches rows 8 (t & 7) .. + 7 of the four columns 4 (t >> 3) .. + 3 of each operand -- eight
//              16-byte loads an operand, a wave's load covers 8 rows x 128 bytes (whole cache lines), the next step's issued
//              before the current step's MFMAs -- splits the 32 values in registers (once per value and job) and writes each column's 8 hi
//              and 8 lo as one 16-byte LDS store each: the transpose happens in the registers.
//   LDS      : [128 columns][hi 64 | lo 64 | pad 8] bf16 per operand, 34 816 bytes, 69 632 together: two workgroups a CU.
//              The column stride is 68 dwords = 4 mod 64.  Stores (bank = dword mod 32, groups of 8 consecutive lanes): the 8
//              lanes of a group hold the 8 row groups of one column, 16 bytes apart: 32 distinct banks.  Reads (16 bytes, bank =
//              dword mod 64, the 16-lane groups of ds_read_b128): 16 columns of one lane half, 4 banks apart: 64 distinct banks.
//   products : per 16-row step s an accumulator takes P_hi.in_hi, then P_hi.in_lo, then P_lo.in_hi; the steps ascend.
//   bias     : the fp32 column sums come from the fetched registers, before the split: per step a thread adds its 8 rows of
//              a column in row order and that to its running sum (one per row group r = 0..7 of the 64-row steps); at the end
//              the 8 running sums of a column are added in the order r = 0..7.
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int WGS_K = 64;                  // rows per step: four k-steps of the instruction
constexpr int WGS_LO = WGS_K;              // where a column's lo values start
constexpr int WGS_STRIDE = 2 * WGS_K + 8;  // bf16 of a column of the image: 68 dwords
static_assert(2 * WG_T * WGS_STRIDE * sizeof(__bf16) <= 80 * 1024, "two workgroups share a CU's LDS");
static_assert(8 * WG_T * sizeof(float) <= WG_T * WGS_STRIDE * sizeof(__bf16), "the bias sums meet in the A image");

// 64 rows x 128 columns into registers: thread t takes the four floats at column 4 (t >> 3) of rows 8 (t & 7) + q.  Rows
// from `end` on and columns from `cols_ld` on are zeros and are not read (wg_fetch's rules).
__device__ __forceinline__ void wgs_fetch(f32x4 (&v)[8], const float* __restrict__ src, int64_t ld, int64_t row0, int64_t end,
                                          int col0, int cols_ld, int tid) {
  const int c = 4 * (tid >> 3);
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const int64_t row = row0 + 8 * (tid & 7) + q;
    f32x4 r = {0.f, 0.f, 0.f, 0.f};
    if (row < end && c < cols_ld) r = *reinterpret_cast<const f32x4*>(src + row * ld + col0 + c);
    v[q] = r;
  }
}

// ... split, and to the image: a column's 8 rows are one 16-byte store of hi and one of lo; columns from `cols` on (the pad
// of enc) are zeros
__device__ __forceinline__ void wgs_stage(__bf16* img, const f32x4 (&v)[8], int cols, int tid) {
  const int c = 4 * (tid >> 3);
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    bf16x8 hi, lo;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const __bf16 h = (__bf16)v[q][e];
      hi[q] = h;
      lo[q] = (__bf16)(v[q][e] - (float)h);
    }
    if (cols < WG_T && c + e >= cols)
      for (int q = 0; q < 8; ++q) hi[q] = lo[q] = (__bf16)0.f;
    __bf16* dst = img + (c + e) * WGS_STRIDE + 8 * (tid & 7);
    *reinterpret_cast<bf16x8*>(dst) = hi;
    *reinterpret_cast<bf16x8*>(dst + WGS_LO) = lo;
  }
}

__device__ __forceinline__ void wgs_tile_job(const WgArgs& p, uint32_t job, int64_t r0, int64_t r1, float* __restrict__ ws,
                                             __bf16* As, __bf16* Bs) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l = (job >> 4) & 15, it = (job >> 8) & 15, jt = (job >> 12) & 15;
  const uint32_t flags = job >> 16;
  const bool gemm = flags & WG_F_GEMM, bias = flags & WG_F_BIAS, from_enc = flags & WG_F_ENC;

  const float* a_src = p.g_pre + (int64_t)l * p.pre_rows * WG_W;
  const int64_t a_r1 = r1 - p.pre_row0;  // the slab's end as g_pre counts the rows
  const float* b_src = from_enc ? p.enc : p.acts + (int64_t)(l > 0 ? l - 1 : 0) * p.N * WG_W;
  const int64_t b_ld = from_enc ? p.enc_w : WG_W;
  const int b_col0 = from_enc ? 0 : jt * WG_T;
  const int b_cols = from_enc ? p.in_ch : WG_T, b_cols_ld = from_enc ? p.enc_w : WG_T;  // columns kept / in memory

  f32x16 acc[2][2];
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int e = 0; e < 16; ++e) acc[a][b][e] = 0.f;
  float bsum[4] = {0.f, 0.f, 0.f, 0.f};

  const int li = lane & 31, lh = lane >> 5;
  const __bf16* a_rd = As + ((wave >> 1) * 64 + li) * WGS_STRIDE + 8 * lh;
  const __bf16* b_rd = Bs + ((wave & 1) * 64 + li) * WGS_STRIDE + 8 * lh;

  f32x4 va[8], vb[8];
  wgs_fetch(va, a_src, WG_W, r0 - p.pre_row0, a_r1, it * WG_T, WG_T, tid);
  if (gemm) wgs_fetch(vb, b_src, b_ld, r0, r1, b_col0, b_cols_ld, tid);
  for (int64_t row = r0; row < r1; row += WGS_K) {
    if (bias) {
      // this thread's 8 rows of its four columns of P, in row order, before anything is rounded
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        float s = va[0][e];
#pragma unroll
        for (int q = 1; q < 8; ++q) s += va[q][e];
        bsum[e] += s;
      }
    }
    if (gemm) {
      wgs_stage(As, va, WG_T, tid);
      wgs_stage(Bs, vb, b_cols, tid);
      __syncthreads();
    }
    if (row + WGS_K < r1) {
      wgs_fetch(va, a_src, WG_W, row + WGS_K - p.pre_row0, a_r1, it * WG_T, WG_T, tid);
      if (gemm) wgs_fetch(vb, b_src, b_ld, row + WGS_K, r1, b_col0, b_cols_ld, tid);
    }
    if (gemm) {
      // the fragments of step s + 1 are read before the twelve MFMAs of step s
      bf16x8 ah[2], al[2], bh[2], bl[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        ah[x] = *reinterpret_cast<const bf16x8*>(a_rd + 32 * x * WGS_STRIDE);
        al[x] = *reinterpret_cast<const bf16x8*>(a_rd + 32 * x * WGS_STRIDE + WGS_LO);
        bh[x] = *reinterpret_cast<const bf16x8*>(b_rd + 32 * x * WGS_STRIDE);
        bl[x] = *reinterpret_cast<const bf16x8*>(b_rd + 32 * x * WGS_STRIDE + WGS_LO);
      }
#pragma unroll
      for (int s = 0; s < WGS_K / 16; ++s) {
        bf16x8 nah[2], nal[2], nbh[2], nbl[2];
        if (s + 1 < WGS_K / 16) {
#pragma unroll
          for (int x = 0; x < 2; ++x) {
            nah[x] = *reinterpret_cast<const bf16x8*>(a_rd + 16 * (s + 1) + 32 * x * WGS_STRIDE);
            nal[x] = *reinterpret_cast<const bf16x8*>(a_rd + 16 * (s + 1) + 32 * x * WGS_STRIDE + WGS_LO);
            nbh[x] = *reinterpret_cast<const bf16x8*>(b_rd + 16 * (s + 1) + 32 * x * WGS_STRIDE);
            nbl[x] = *reinterpret_cast<const bf16x8*>(b_rd + 16 * (s + 1) + 32 * x * WGS_STRIDE + WGS_LO);
          }
        }
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh[b], acc[a][b], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl[b], acc[a][b], 0, 0, 0);
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
          for (int b = 0; b < 2; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh[b], acc[a][b], 0, 0, 0);
        if (s + 1 < WGS_K / 16) {
#pragma unroll
          for (int x = 0; x < 2; ++x) ah[x] = nah[x], al[x] = nal[x], bh[x] = nbh[x], bl[x] = nbl[x];
        }
      }
      __syncthreads();
    }
  }

  if (gemm) {
    // C/D map of the 32x32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    float* out = from_enc ? ws + WG_OFF_IN + (size_t)(l == 0 ? 0 : 1) * WG_W * WG_T : ws + (size_t)(l - 1) * WG_W * WG_W;
    const int ld = from_enc ? WG_T : WG_W;
    for (int a = 0; a < 2; ++a)
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int i = it * WG_T + (wave >> 1) * 64 + 32 * a + (e & 3) + 8 * (e >> 2) + 4 * lh;
          const int j = b_col0 + (wave & 1) * 64 + 32 * b + li;
          out[(size_t)i * ld + j] = acc[a][b][e];
        }
  }
  if (bias) {
    // the 8 row groups of a column meet through LDS (free after the loop's last barrier) and are added in group order
    float* red = reinterpret_cast<float*>(As);
#pragma unroll
    for (int e = 0; e < 4; ++e) red[(tid & 7) * WG_T + 4 * (tid >> 3) + e] = bsum[e];
    __syncthreads();
    if (tid < WG_T) {
      float s = red[tid];
#pragma unroll
      for (int r = 1; r < 8; ++r) s += red[r * WG_T + tid];
      ws[WG_OFF_BIAS + (size_t)l * WG_W + it * WG_T + tid] = s;
    }
  }
}

// mlp_wgrad_kernel's deal of the (slab, job) list; two workgroups a CU, so that one's split hides under the other's MFMAs
__global__ void __launch_bounds__(WG_BLOCK, 2) mlp_wgrad_split_kernel(WgArgs p) {
  __shared__ __attribute__((aligned(16))) __bf16 As[WG_T * WGS_STRIDE];
  __shared__ __attribute__((aligned(16))) __bf16 Bs[WG_T * WGS_STRIDE];
  const int64_t total = p.n_slabs * p.n_jobs, run = (total + 7) / 8;
  const int64_t id = (int64_t)(blockIdx.x & 7) * run + (blockIdx.x >> 3);
  if (id >= total) return;
  const int64_t slab = p.slab0 + id / p.n_jobs;
  const uint32_t job = p.jobs[id % p.n_jobs];
  const int64_t r0 = slab * p.slab_rows;
  const int64_t r1 = r0 + p.slab_rows < p.N ? r0 + p.slab_rows : p.N;
  float* ws = p.ws + (size_t)slab * WG_SLAB_FLOATS;
  if ((job & 15) == WG_JOB_HEAD)
    wg_head_job(p, job, r0, r1, ws, reinterpret_cast<float*>(As));
  else
    wgs_tile_job(p, job, r0, r1, ws, As, Bs);
}

}  // namespace

extern "C" size_t fg_mlp_param_grads_workspace_bytes(int64_t N) {
  return N <= 0 ? 0 : (size_t)wg_slab_bound(N) * WG_SLAB_FLOATS * sizeof(float);
}

extern "C" int fg_mlp_param_grads_slab_rows(int64_t N) {
  if (N <= 0) return 0;
  int rows;
  int64_t slabs;
  wg_cut(N, &rows, &slabs);
  return rows;
}

namespace {

// The shape checks of the descriptor and `out`, then the jobs of one slab into p and the outputs into o; which inputs the
// jobs read comes back in need_* (need_pre: g_pre).  p.n_jobs == 0: nothing is asked for.
int wg_plan(const fg_mlp_desc* d, const fg_mlp_grads* out, WgArgs& p, WgOut& o, bool& need_enc, bool& need_acts, bool& need_pre,
            bool& need_heads) {
  if (!d || d->size != (int32_t)sizeof(fg_mlp_desc)) return FG_ERR_INVALID_ARG;
  if (d->aux_width < 1 || d->aux_width > 64 || d->mode != FG_MLP_PLAIN) return FG_ERR_INVALID_ARG;
  if (d->n_heads < 1 || d->n_heads > FG_MLP_MAX_HEADS) return FG_ERR_INVALID_ARG;
  int rows_total = 0;
  for (int h = 0; h < d->n_heads; ++h) {
    if (d->head_rows[h] < 1 || d->head_rows[h] > 16) return FG_ERR_INVALID_ARG;
    rows_total += d->head_rows[h];
  }
  if (rows_total > 16) return FG_ERR_INVALID_ARG;
  if (d->depth != WG_D || d->width != WG_W || d->multires != 10) return FG_ERR_UNSUPPORTED;
  if (!out || out->size != (int32_t)sizeof(fg_mlp_grads)) return FG_ERR_INVALID_ARG;

  need_enc = need_acts = need_pre = need_heads = false;
  auto push = [&](uint32_t type, int l, int it, int jt, uint32_t flags) {
    p.jobs[p.n_jobs++] = type | (uint32_t)l << 4 | (uint32_t)it << 8 | (uint32_t)jt << 12 | flags << 16;
  };
  for (int l = 0; l < WG_D; ++l) {
    o.weight[l] = out->weight[l], o.bias[l] = out->bias[l];
    const uint32_t b = out->bias[l] ? WG_F_BIAS : 0;
    if (!out->weight[l] && !b) continue;
    need_pre = true;
    for (int it = 0; it < 2; ++it) {
      if (!out->weight[l]) {
        push(WG_JOB_TILE, l, it, 0, b);
        continue;
      }
      if (l == 0 || l == WG_SKIP + 1) push(WG_JOB_TILE, l, it, 0, WG_F_GEMM | WG_F_ENC | (l == 0 ? b : 0)), need_enc = true;
      if (l > 0) {
        push(WG_JOB_TILE, l, it, 0, WG_F_GEMM | b);
        push(WG_JOB_TILE, l, it, 1, WG_F_GEMM);
        need_acts = true;
      }
    }
  }
  bool head_w = false, head_b = false;
  for (int h = 0; h < d->n_heads; ++h) {
    o.head_weight[h] = out->head_weight[h], o.head_bias[h] = out->head_bias[h], o.head_rows[h] = d->head_rows[h];
    head_w |= out->head_weight[h] != nullptr, head_b |= out->head_bias[h] != nullptr;
  }
  if (head_w)
    for (int ct = 0; ct < 4; ++ct) push(WG_JOB_HEAD, 0, 0, ct, WG_F_GEMM | (ct == 0 && head_b ? WG_F_BIAS : 0));
  else if (head_b)
    push(WG_JOB_HEAD, 0, 0, 0, WG_F_BIAS);
  need_heads = head_w || head_b, need_acts |= head_w;
  p.in_ch = WG_XCH + d->aux_width, p.enc_w = FG_MLP_ENC_WIDTH(d->aux_width), p.rows_total = rows_total;
  o.n_heads = d->n_heads, o.in_ch = p.in_ch;
  return FG_OK;
}

// the jobs of p over the slabs [slab0, slab0 + n_slabs), g_pre as p describes it; `split`: the tile jobs as split-bf16 products
int wg_launch_slabs(WgArgs p, int64_t slab0, int64_t n_slabs, bool split, fg_stream_t stream) {
  p.slab0 = slab0, p.n_slabs = n_slabs;
  hipLaunchKernelGGL(split ? mlp_wgrad_split_kernel : mlp_wgrad_kernel, dim3((unsigned)((n_slabs * p.n_jobs + 7) / 8 * 8)), dim3(WG_BLOCK), 0,
                     fg_hip_stream(stream), p);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

// the partial blocks of all n_slabs slabs, added in slab order, to the outputs
int wg_launch_reduce(const float* ws, int64_t n_slabs, const WgOut& o, fg_stream_t stream) {
  hipLaunchKernelGGL(mlp_wgrad_reduce_kernel, dim3((unsigned)((WG_SLAB_FLOATS + WG_BLOCK - 1) / WG_BLOCK)), dim3(WG_BLOCK), 0,
                     fg_hip_stream(stream), ws, n_slabs, o);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

inline bool wg_precision_ok(int32_t precision) { return precision == FG_MLP_FP32 || precision == FG_MLP_BF16X3; }

}  // namespace

extern "C" int fg_mlp_wgrad_precision_supported(int32_t precision) { return wg_precision_ok(precision); }

extern "C" int fg_mlp_param_grads_p(int64_t N, const fg_mlp_desc* d, const float* enc, const float* acts, const float* g_pre,
                                    const float* g_heads, const fg_mlp_grads* out, int32_t wgrad_precision, void* workspace,
                                    size_t workspace_bytes, fg_stream_t stream) {
  if (!wg_precision_ok(wgrad_precision)) return FG_ERR_INVALID_ARG;
  if (N < 0) return FG_ERR_INVALID_ARG;
  if (N == 0) return FG_OK;
  WgArgs p = {};
  WgOut o = {};
  bool need_enc, need_acts, need_pre, need_heads;
  if (int rc = wg_plan(d, out, p, o, need_enc, need_acts, need_pre, need_heads)) return rc;
  if (p.n_jobs == 0) return FG_OK;
  if ((need_enc && !enc) || (need_acts && !acts) || (need_pre && !g_pre) || (need_heads && !g_heads)) return FG_ERR_INVALID_ARG;
  // (the operand tiles are fetched 16 bytes at a time)
  if (reinterpret_cast<uintptr_t>(enc) % 16 || reinterpret_cast<uintptr_t>(acts) % 16 || reinterpret_cast<uintptr_t>(g_pre) % 16)
    return FG_ERR_INVALID_ARG;

  int slab_rows;
  int64_t n_slabs;
  wg_cut(N, &slab_rows, &n_slabs);
  if (!workspace || n_slabs * p.n_jobs >= ((int64_t)1 << 31)) return FG_ERR_INVALID_ARG;
  if (workspace_bytes < fg_mlp_param_grads_workspace_bytes(N)) return FG_ERR_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return FG_ERR_INVALID_ARG;

  p.enc = enc, p.acts = acts, p.g_pre = g_pre, p.g_heads = g_heads, p.ws = static_cast<float*>(workspace);
  p.N = N, p.slab_rows = slab_rows, p.pre_rows = N, p.pre_row0 = 0;
  if (int rc = wg_launch_slabs(p, 0, n_slabs, wgrad_precision == FG_MLP_BF16X3, stream)) return rc;
  return wg_launch_reduce(p.ws, n_slabs, o, stream);
}

extern "C" int fg_mlp_param_grads(int64_t N, const fg_mlp_desc* d, const float* enc, const float* acts, const float* g_pre,
                                  const float* g_heads, const fg_mlp_grads* out, void* workspace, size_t workspace_bytes,
                                  fg_stream_t stream) {
  return fg_mlp_param_grads_p(N, d, enc, acts, g_pre, g_heads, out, FG_MLP_FP32, workspace, workspace_bytes, stream);
}

// ---- fg_mlp_train_bwd: the chain (mlp.hip) and the slab jobs above, one chunk of slabs at a time, so that g_pre is a
// chunk-sized array of the workspace.  Workspace: [the chain's packed weights, padded to 4 KB][g_pre chunk: 8 x chunk_rows x 256]
// [one partial block per slab of the bound].
namespace {

inline int64_t tb_chunk_slabs(int64_t n_slabs, int32_t chunk_slabs) {
  const int64_t want = chunk_slabs > 0 ? chunk_slabs : FG_MLP_TRAIN_BWD_CHUNK_SLABS;
  return want < n_slabs ? want : n_slabs;
}

// the chain's packed weights, rounded up so that the chunk array behind them starts on a 4 KB boundary of the workspace: its
// rows are read and written 128 bytes a wave at a time, and at the 64-byte offset the bare size leaves every such access
// straddles two cache lines (measured: 3 % of the call, profiles/mlp_chunked_bwd.md)
inline size_t tb_pack_bytes(int64_t N, bool inputs) {
  const size_t b = inputs ? fg_mlp_bwd_inputs_workspace_bytes(N) : fg_mlp_train_workspace_bytes(N);
  return (b + FG_MLP_TRAIN_BWD_ALIGN - 1) / FG_MLP_TRAIN_BWD_ALIGN * FG_MLP_TRAIN_BWD_ALIGN;
}

}  // namespace

extern "C" int64_t fg_mlp_train_bwd_chunk_rows(int64_t N, int32_t chunk_slabs) {
  if (N <= 0 || chunk_slabs < 0) return 0;
  int rows;
  int64_t slabs;
  wg_cut(N, &rows, &slabs);
  return tb_chunk_slabs(slabs, chunk_slabs) * rows;
}

extern "C" size_t fg_mlp_train_bwd_workspace_bytes(int64_t N, int32_t chunk_slabs, int32_t want_g_enc) {
  if (N <= 0 || chunk_slabs < 0) return 0;
  return tb_pack_bytes(N, want_g_enc != 0) + (size_t)WG_D * (size_t)fg_mlp_train_bwd_chunk_rows(N, chunk_slabs) * WG_W * sizeof(float) +
         fg_mlp_param_grads_workspace_bytes(N);
}

extern "C" int fg_mlp_train_bwd_p(int64_t N, const fg_mlp_desc* d, const float* g_heads, const float* enc, const float* acts,
                                  float* g_enc, const fg_mlp_grads* out, int32_t chunk_slabs, int32_t wgrad_precision,
                                  void* workspace, size_t workspace_bytes, fg_stream_t stream) {
  if (!wg_precision_ok(wgrad_precision)) return FG_ERR_INVALID_ARG;
  if (N < 0) return FG_ERR_INVALID_ARG;
  if (N == 0) return FG_OK;
  if (chunk_slabs < 0) return FG_ERR_INVALID_ARG;
  if (int rc = fg_mlp_detail::bwd_check(N, d, nullptr, 0, 0)) return rc;
  WgArgs p = {};
  WgOut o = {};
  bool need_enc, need_acts, need_pre, need_heads;
  if (int rc = wg_plan(d, out, p, o, need_enc, need_acts, need_pre, need_heads)) return rc;
  if (p.n_jobs == 0 && !g_enc) return FG_OK;
  // (the chain reads g_heads and acts whatever is asked for; the operand tiles are fetched 16 bytes at a time)
  if (!g_heads || !acts || (need_enc && !enc)) return FG_ERR_INVALID_ARG;
  if (reinterpret_cast<uintptr_t>(enc) % 16 || reinterpret_cast<uintptr_t>(acts) % 16) return FG_ERR_INVALID_ARG;

  int slab_rows;
  int64_t n_slabs;
  wg_cut(N, &slab_rows, &n_slabs);
  if (n_slabs * (p.n_jobs > 0 ? p.n_jobs : 1) >= ((int64_t)1 << 31)) return FG_ERR_INVALID_ARG;
  const bool inputs = g_enc != nullptr;
  if (int rc = fg_mlp_detail::bwd_check(N, d, workspace, workspace_bytes, fg_mlp_train_bwd_workspace_bytes(N, chunk_slabs, inputs)))
    return rc;

  const int64_t per_chunk = tb_chunk_slabs(n_slabs, chunk_slabs), chunk_rows = per_chunk * slab_rows;
  float* g_pre = reinterpret_cast<float*>(static_cast<char*>(workspace) + tb_pack_bytes(N, inputs));
  p.enc = enc, p.acts = acts, p.g_pre = g_pre, p.g_heads = g_heads, p.ws = g_pre + (size_t)WG_D * chunk_rows * WG_W;
  p.N = N, p.slab_rows = slab_rows, p.pre_rows = chunk_rows;
  if (int rc = fg_mlp_detail::bwd_launch_pack(d, inputs, workspace, stream)) return rc;
  for (int64_t s0 = 0; s0 < n_slabs; s0 += per_chunk) {
    const int64_t s1 = s0 + per_chunk < n_slabs ? s0 + per_chunk : n_slabs;
    const int64_t r0 = s0 * slab_rows, r1 = s1 * slab_rows < N ? s1 * slab_rows : N;
    if (int rc = fg_mlp_detail::bwd_launch_rows(N, d, r0, r1, g_heads, acts, g_pre, chunk_rows, g_enc, workspace, stream)) return rc;
    p.pre_row0 = r0;
    if (p.n_jobs > 0)
      if (int rc = wg_launch_slabs(p, s0, s1 - s0, wgrad_precision == FG_MLP_BF16X3, stream)) return rc;
  }
  return p.n_jobs > 0 ? wg_launch_reduce(p.ws, n_slabs, o, stream) : FG_OK;
}

extern "C" int fg_mlp_train_bwd(int64_t N, const fg_mlp_desc* d, const float* g_heads, const float* enc, const float* acts,
                                float* g_enc, const fg_mlp_grads* out, int32_t chunk_slabs, void* workspace, size_t workspace_bytes,
                                fg_stream_t stream) {
  return fg_mlp_train_bwd_p(N, d, g_heads, enc, acts, g_enc, out, chunk_slabs, FG_MLP_FP32, workspace, workspace_bytes, stream);
}
