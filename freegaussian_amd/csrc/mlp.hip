// K10: fused fp32 forward of the deformation / control MLP (freegaussian_amd/deform.py) for inference: one call, two launches --
// the weights re-ordered (pack), then the network, where a workgroup takes a
// tile of FG_MLP_ROW_TILE rows from the positions to the rigid transforms (or the plain head outputs); no [N,256]
// activation ever reaches global memory.
//
//   pack     : a small launch copies the trunk weights into the caller's workspace in the order the tiles read them
//              (below) and the head weights / biases into one zero-padded [16,256] / [16] block.  ~2 MB read and written
//              per call (measured: profiles/mlp_forward.md); nothing is kept between calls (the library has no state, and the weights of a
//              module in training change every step).
//   input    : row = [posenc(x, 10) (63), aux (A), 0 ...] written to LDS, K padded to a multiple of 8; sincosf is the
//              accurate one (arguments reach 512 x), and x 2^k is exact, so the arguments are utils.positional_encoding's
//   trunk    : 8 linears of 256 + ReLU, activations in place in LDS ([64][260] floats: the row stride of 4 mod 64 dwords
//              makes the 16-byte operand reads conflict free).  Four waves, each owning 64 of the 256 output columns as
//              2 x 2 tiles of v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain starting from the bias).  The
//              layer after the skip first runs over the input row (kept in LDS), then over h: cat([inp, h]).
//   k order  : K is walked in groups of 8; lane half h of a wave holds k = 8 g + 4 h + s in element s of one 16-byte read,
//              for A (LDS) and for B (packed weights) alike, so a chain adds k = 8g, 8g+4, 8g+1, 8g+5, ... -- a fixed
//              order per output element that depends on nothing but the element's own row: rows are independent, bit
//              for bit, whatever tile or lane they land in.
//   packed B : Wp[g][j][e] = W[j][8 g + e] (j = output column, zero beyond the layer's K): the 64 lanes of one B read
//              fetch 1 KB contiguous.
//   heads    : <= 16 output rows over the final h, v_mfma_f32_16x16x4_f32, one 16-row block per wave
//   epilogue : one lane per row: exp_se3 + the transform of x (SE(3) mode) or plain stores
// Plain C++ stores only; no atomics; the result is deterministic.
//
// Training (fg_mlp_train_fwd / fg_mlp_bwd) is the same tile twice more:
//   forward  : mlp_fwd_kernel<true> -- the code above, which also stores the encoded input row, each layer's post-ReLU
//              tile (from the accumulators, as it goes to LDS) and the raw heads.  Same k order, same chains.
//   backward : mlp_bwd_kernel -- the data chain g(h_7) = g_heads W_h, P_l = g(h_l) where h_l > 0, g(h_{l-1}) = P_l W_l[:, hidden],
//              l = 7 .. 0, through the same mlp_gemm_part: the gradient tile sits in LDS where the activations sat, the mask
//              comes from the saved activations, and every P_l tile is stored once.  The reduction runs over a layer's OUTPUT
//              index, so the weights are packed a second way: Tp[g][k][e] = W[8 g + e][first hidden column + k].
//              Nothing flows to the input row (layer 0, the input columns of layer 5): the inputs want no gradient.
//   backward with input-row gradients (fg_mlp_bwd_inputs): mlp_bwd_kernel<true> -- the same chain, and two products more per
//              tile: g_enc = P_5 W_5[:, :in_ch] + P_0 W_0, a [64, <= 128] tile, wave w owning columns 32 w .. 32 w + 31 as a
//              2 x 1 block of the 32x32x2 MFMA (a wave whose block lies beyond the row's padded width skips it).  The layer-5
//              part is taken while P_5 sits in LDS and waits in g_enc (stored and read back by the same lane) until l = 0, where
//              P_0 goes to the same LDS tile for the second part: no third tile, two workgroups per CU as before.  Third packing:
//              Tin[{0,5}][g][k][e] = W_l[8 g + e][k], k < 128, zero from in_ch on.
//              The weight gradients are [256, N] x [N, 256] products over all tiles: the caller's.
// fg_mlp_desc::precision = FG_MLP_BF16X3 (opt-in) runs the same tiles through kernels of their own further down
// (mlp_fwd_split_kernel, mlp_bwd_split_kernel and their pack kernels): every operand as two bf16, three products for one.  The
// kernels above that point are the FG_MLP_FP32 ones and know nothing of it.
#include <cmath>

#include "fg_common.h"
#include "mlp_internal.h"
#include "se3_math.h"

namespace {

constexpr int MLP_M = FG_MLP_ROW_TILE;  // rows per workgroup
constexpr int MLP_W = 256;              // hidden width
constexpr int MLP_D = 8;                // trunk depth
constexpr int MLP_SKIP = 4;             // the layer AFTER this index also takes the input row
constexpr int MLP_FREQS = 10;
constexpr int MLP_XCH = 3 * (1 + 2 * MLP_FREQS);  // 63
constexpr int MLP_ACT_STRIDE = MLP_W + 4;         // 260: 4 mod 64 dwords
constexpr int MLP_IN_STRIDE = 128 + 4;            // input row: <= 63 + 64 channels, padded to 128
constexpr int MLP_HEAD_COL = 4;                   // head results land in columns 4..19 of the (then dead) input rows
constexpr int MLP_BLOCK = 256;
constexpr int MLP_GROUP_FLOATS = MLP_W * 8;  // one k-group of a packed layer

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// packed workspace (floats): the trunk layers one after the other, then the heads
struct MlpLayout {
  int g0;               // k-groups of the input row
  size_t layer[MLP_D];  // float offset of each packed layer
  int groups[MLP_D];
  size_t head_w, head_b, total;  // [16][256], [16]; total in floats
};

inline MlpLayout mlp_layout(int A) {
  MlpLayout L;
  L.g0 = (MLP_XCH + A + 7) / 8;
  size_t at = 0;
  for (int l = 0; l < MLP_D; ++l) {
    L.groups[l] = l == 0 ? L.g0 : (l == MLP_SKIP + 1 ? L.g0 + MLP_W / 8 : MLP_W / 8);
    L.layer[l] = at;
    at += (size_t)L.groups[l] * MLP_GROUP_FLOATS;
  }
  L.head_w = at;
  at += 16 * MLP_W;
  L.head_b = at;
  at += 16;
  L.total = at;
  return L;
}

// the backward's packed workspace: the hidden columns of layers 1..7, then the heads as two k-groups ([16 head rows] x 256)
constexpr int MLP_T_LAYER_FLOATS = (MLP_W / 8) * MLP_GROUP_FLOATS;
constexpr size_t MLP_T_HEAD = (size_t)(MLP_D - 1) * MLP_T_LAYER_FLOATS;
constexpr size_t MLP_T_TOTAL = MLP_T_HEAD + 2 * MLP_GROUP_FLOATS;
constexpr int MLP_GH_STRIDE = 16 + 4;  // the head cotangents of a tile in LDS
// the input-row backward's third block, behind the two above: the input columns of layers 0 and 5, [2][32 groups][128][8]
constexpr int MLP_IN_COLS = 128;
constexpr int MLP_TIN_GROUP_FLOATS = MLP_IN_COLS * 8;
constexpr int MLP_TIN_LAYER_FLOATS = (MLP_W / 8) * MLP_TIN_GROUP_FLOATS;
constexpr size_t MLP_TIN_TOTAL = 2 * (size_t)MLP_TIN_LAYER_FLOATS;

struct MlpArgs {
  const float* x;
  const float* aux;
  int64_t aux_stride;
  const float* W[MLP_D];
  const float* b[MLP_D];
  const float* head_W[FG_MLP_MAX_HEADS];
  const float* head_b[FG_MLP_MAX_HEADS];
  int head_rows[FG_MLP_MAX_HEADS];
  float* out[FG_MLP_MAX_HEADS];
  int n_heads, A, mode;
};

__global__ void __launch_bounds__(MLP_BLOCK)
mlp_pack_kernel(MlpArgs p, MlpLayout L, float* __restrict__ ws) {
  const size_t at = (size_t)blockIdx.x * MLP_BLOCK + threadIdx.x;
  if (at >= L.total) return;
  const int in_ch = MLP_XCH + p.A;
  if (at >= L.head_b) {
    int o = (int)(at - L.head_b), v = 0;
    float r = 0.f;
    for (int h = 0; h < p.n_heads; ++h) {
      if (o >= v && o < v + p.head_rows[h]) r = p.head_b[h][o - v];
      v += p.head_rows[h];
    }
    ws[at] = r;
    return;
  }
  if (at >= L.head_w) {
    const int o = (int)(at - L.head_w) / MLP_W, k = (int)(at - L.head_w) % MLP_W;
    int v = 0;
    float r = 0.f;
    for (int h = 0; h < p.n_heads; ++h) {
      if (o >= v && o < v + p.head_rows[h]) r = p.head_W[h][(o - v) * MLP_W + k];
      v += p.head_rows[h];
    }
    ws[at] = r;
    return;
  }
  int l = 0;
  while (l + 1 < MLP_D && at >= L.layer[l + 1]) ++l;
  const size_t rel = at - L.layer[l];
  const int g = (int)(rel / MLP_GROUP_FLOATS), j = (int)(rel % MLP_GROUP_FLOATS) / 8, e = (int)(rel % 8);
  const float* W = p.W[l];
  float r = 0.f;
  if (l == 0) {
    const int k = 8 * g + e;
    if (k < in_ch) r = W[(size_t)j * in_ch + k];
  } else if (l == MLP_SKIP + 1) {
    const int ld = in_ch + MLP_W;
    if (g < L.g0) {
      const int k = 8 * g + e;
      if (k < in_ch) r = W[(size_t)j * ld + k];
    } else {
      r = W[(size_t)j * ld + in_ch + 8 * (g - L.g0) + e];
    }
  } else {
    r = W[(size_t)j * MLP_W + 8 * g + e];
  }
  ws[at] = r;
}

// the backward's weights: Tp[l - 1][g][k][e] = W_l[8 g + e][off_l + k] (off_5 = in_ch, else 0), heads: Tp[g][k][e] = W_h[8 g + e][k]
__global__ void __launch_bounds__(MLP_BLOCK)
mlp_pack_t_kernel(MlpArgs p, float* __restrict__ ws) {
  const size_t at = (size_t)blockIdx.x * MLP_BLOCK + threadIdx.x;
  if (at >= MLP_T_TOTAL) return;
  const int in_ch = MLP_XCH + p.A;
  const size_t rel = at < MLP_T_HEAD ? at % MLP_T_LAYER_FLOATS : at - MLP_T_HEAD;
  const int j = 8 * (int)(rel / MLP_GROUP_FLOATS) + (int)(rel % 8), k = (int)(rel % MLP_GROUP_FLOATS) / 8;
  float r = 0.f;
  if (at < MLP_T_HEAD) {
    const int l = 1 + (int)(at / MLP_T_LAYER_FLOATS);
    r = l == MLP_SKIP + 1 ? p.W[l][(size_t)j * (in_ch + MLP_W) + in_ch + k] : p.W[l][(size_t)j * MLP_W + k];
  } else {
    int v = 0;
    for (int h = 0; h < p.n_heads; ++h) {
      if (j >= v && j < v + p.head_rows[h]) r = p.head_W[h][(j - v) * MLP_W + k];
      v += p.head_rows[h];
    }
  }
  ws[at] = r;
}

// the input-row backward's weights: Tin[i][g][k][e] = W_l[8 g + e][k] for l = (0, 5)[i] and k < in_ch, zero up to k = 127
__global__ void __launch_bounds__(MLP_BLOCK)
mlp_pack_tin_kernel(MlpArgs p, float* __restrict__ tin) {
  const size_t at = (size_t)blockIdx.x * MLP_BLOCK + threadIdx.x;
  if (at >= MLP_TIN_TOTAL) return;
  const int in_ch = MLP_XCH + p.A;
  const int l = at < MLP_TIN_LAYER_FLOATS ? 0 : MLP_SKIP + 1;
  const int rel = (int)(at % MLP_TIN_LAYER_FLOATS);
  const int j = 8 * (rel / MLP_TIN_GROUP_FLOATS) + rel % 8, k = rel % MLP_TIN_GROUP_FLOATS / 8;
  tin[at] = k < in_ch ? p.W[l][(size_t)j * (l == 0 ? in_ch : in_ch + MLP_W) + k] : 0.f;
}

// acc += src[rows][8 groups ...] x Wp: `a` points at this lane's row of the LDS source (+ 4 h), `b` at this lane's column
// of the packed layer (+ 4 h).  The next group's operands are fetched before the current group's 16 MFMAs.
__device__ __forceinline__ void mlp_gemm_part(f32x16 (&acc)[2][2], const float* a, int stride, int groups,
                                              const float* __restrict__ b) {
  f32x4 a0 = *reinterpret_cast<const f32x4*>(a), a1 = *reinterpret_cast<const f32x4*>(a + 32 * stride);
  f32x4 b0 = *reinterpret_cast<const f32x4*>(b), b1 = *reinterpret_cast<const f32x4*>(b + 32 * 8);
  for (int g = 0; g < groups; ++g) {
    f32x4 na0 = a0, na1 = a1, nb0 = b0, nb1 = b1;
    if (g + 1 < groups) {
      const float* an = a + 8 * (g + 1);
      const float* bn = b + (size_t)(g + 1) * MLP_GROUP_FLOATS;
      na0 = *reinterpret_cast<const f32x4*>(an);
      na1 = *reinterpret_cast<const f32x4*>(an + 32 * stride);
      nb0 = *reinterpret_cast<const f32x4*>(bn);
      nb1 = *reinterpret_cast<const f32x4*>(bn + 32 * 8);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b0[s], acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b1[s], acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b0[s], acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b1[s], acc[1][1], 0, 0, 0);
    }
    a0 = na0, a1 = na1, b0 = nb0, b1 = nb1;
  }
}

// mlp_gemm_part for a 2 x 1 block over the 128-column packing Tin: the same operand reads, k order and prefetch
__device__ __forceinline__ void mlp_gemm_in(f32x16 (&acc)[2], const float* a, int stride, int groups, const float* __restrict__ b) {
  f32x4 a0 = *reinterpret_cast<const f32x4*>(a), a1 = *reinterpret_cast<const f32x4*>(a + 32 * stride);
  f32x4 b0 = *reinterpret_cast<const f32x4*>(b);
  for (int g = 0; g < groups; ++g) {
    f32x4 na0 = a0, na1 = a1, nb0 = b0;
    if (g + 1 < groups) {
      const float* an = a + 8 * (g + 1);
      na0 = *reinterpret_cast<const f32x4*>(an);
      na1 = *reinterpret_cast<const f32x4*>(an + 32 * stride);
      nb0 = *reinterpret_cast<const f32x4*>(b + (size_t)(g + 1) * MLP_TIN_GROUP_FLOATS);
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[s], b0[s], acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[s], b0[s], acc[1], 0, 0, 0);
    }
    a0 = na0, a1 = na1, b0 = nb0;
  }
}

// exp_se3 of (w / |w| + 1e-5, v / |w| + 1e-5; |w|) and the transform of x (se3_math.h: the arithmetic of utils.exp_se3)
__device__ __forceinline__ void mlp_se3_row(const float* hd, const float* x, int64_t row, const MlpArgs& p) {
  FG_SE3_EXP(hd, T)
  if (float* d = p.out[0]) {
    d += row * 16;
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 4; ++j) d[4 * i + j] = T[i][j];
    d[12] = 0.f, d[13] = 0.f, d[14] = 0.f, d[15] = 1.f;
  }
  if (float* d = p.out[1])
    for (int j = 0; j < 4; ++j) d[row * 4 + j] = hd[6 + j];
  if (float* d = p.out[2])
    for (int j = 0; j < 3; ++j) d[row * 3 + j] = hd[10 + j];
  if (float* d = p.out[3])
    for (int i = 0; i < 3; ++i) d[row * 3 + i] = FG_SE3_POINT(T, x, i);
}

// what the training forward stores besides (fg_mlp_train_fwd)
struct MlpSaved {
  float* heads;  // [N, rows_total]
  float* enc;    // [N, 8 g0]
  float* acts;   // [8, N, 256]
  int rows_total;
};

template <bool TRAIN>
__global__ void __launch_bounds__(MLP_BLOCK)
mlp_fwd_kernel(int64_t N, MlpArgs p, MlpLayout L, const float* __restrict__ ws, MlpSaved sv) {
  __shared__ __attribute__((aligned(16))) float act[MLP_M * MLP_ACT_STRIDE];
  __shared__ __attribute__((aligned(16))) float inp[MLP_M * MLP_IN_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * MLP_M;

  // ---- the input rows: four lanes per row
  {
    const int r = tid >> 2, q = tid & 3;
    const int64_t row = row0 + r;
    const bool live = row < N;
    float* dst = inp + r * MLP_IN_STRIDE;
    float x[3] = {0.f, 0.f, 0.f};
    if (live)
      for (int c = 0; c < 3; ++c) x[c] = p.x[row * 3 + c];
    if (q == 3)
      for (int c = 0; c < 3; ++c) dst[c] = x[c];
    for (int k = q; k < MLP_FREQS; k += 4) {
      const float f = (float)(1 << k);
      for (int c = 0; c < 3; ++c) {
        float s, co;
        sincosf(x[c] * f, &s, &co);
        dst[3 + 6 * k + c] = s;
        dst[3 + 6 * k + 3 + c] = co;
      }
    }
    const float* aux = p.aux + row * p.aux_stride;
    for (int a = q; a < p.A; a += 4) dst[MLP_XCH + a] = live ? aux[a] : 0.f;
    for (int k = MLP_XCH + p.A + q; k < 8 * L.g0; k += 4) dst[k] = 0.f;
  }
  __syncthreads();
  if (TRAIN) {  // the encoded rows, zero pad included: consecutive lanes, consecutive floats
    const int w = 8 * L.g0;
    for (int i = tid; i < MLP_M * w; i += MLP_BLOCK) {
      const int r = i / w, k = i % w;
      if (row0 + r < N) sv.enc[(row0 + r) * w + k] = inp[r * MLP_IN_STRIDE + k];
    }
  }

  // ---- trunk
  const int li = lane & 31, lh = lane >> 5;
  const float* a_inp = inp + li * MLP_IN_STRIDE + 4 * lh;
  const float* a_act = act + li * MLP_ACT_STRIDE + 4 * lh;
  const size_t b_lane = (size_t)(wave * 64 + li) * 8 + 4 * lh;
  for (int l = 0; l < MLP_D; ++l) {
    f32x16 acc[2][2];
    const float* bias = p.b[l] + wave * 64 + li;
    for (int cb = 0; cb < 2; ++cb) {
      const float bv = bias[32 * cb];
      for (int e = 0; e < 16; ++e) acc[0][cb][e] = bv, acc[1][cb][e] = bv;
    }
    const float* wp = ws + L.layer[l] + b_lane;
    if (l == 0) {
      mlp_gemm_part(acc, a_inp, MLP_IN_STRIDE, L.g0, wp);
    } else if (l == MLP_SKIP + 1) {
      mlp_gemm_part(acc, a_inp, MLP_IN_STRIDE, L.g0, wp);
      mlp_gemm_part(acc, a_act, MLP_ACT_STRIDE, MLP_W / 8, wp + (size_t)L.g0 * MLP_GROUP_FLOATS);
    } else {
      mlp_gemm_part(acc, a_act, MLP_ACT_STRIDE, MLP_W / 8, wp);
    }
    __syncthreads();  // every wave has read the whole of the previous layer
    // C/D map of the 32x32 MFMA: column = lane & 31, row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5)
    for (int rb = 0; rb < 2; ++rb)
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = 32 * rb + (e & 3) + 8 * (e >> 2) + 4 * lh;
          const float h = fmaxf(acc[rb][cb][e], 0.f);
          act[r * MLP_ACT_STRIDE + wave * 64 + 32 * cb + li] = h;
          if (TRAIN && row0 + r < N) sv.acts[((int64_t)l * N + row0 + r) * MLP_W + wave * 64 + 32 * cb + li] = h;
        }
    __syncthreads();
  }

  // ---- heads: wave w takes rows 16 w .. 16 w + 15; A[row = lane & 15][k = lane >> 4], four k per MFMA
  {
    const int hi = lane & 15, hq = lane >> 4;
    const float* a = act + (wave * 16 + hi) * MLP_ACT_STRIDE + 4 * hq;
    const float* b = ws + L.head_w + hi * MLP_W + 4 * hq;
    const float bv = ws[L.head_b + hi];
    f32x4 acc = {bv, bv, bv, bv};
    for (int g = 0; g < MLP_W / 16; ++g) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(a + 16 * g);
      const f32x4 bw = *reinterpret_cast<const f32x4*>(b + 16 * g);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bw[s], acc, 0, 0, 0);
    }
    // C/D map of the 16x16 MFMA: column = lane & 15, row = 4 (lane >> 4) + e
    for (int e = 0; e < 4; ++e) inp[(wave * 16 + 4 * hq + e) * MLP_IN_STRIDE + MLP_HEAD_COL + hi] = acc[e];
  }
  __syncthreads();

  // ---- epilogue: one lane per row
  if (tid < MLP_M && row0 + tid < N) {
    const int64_t row = row0 + tid;
    const float* src = inp + tid * MLP_IN_STRIDE;
    float hd[16];
    for (int o = 0; o < 16; ++o) hd[o] = src[MLP_HEAD_COL + o];
    if (TRAIN) {
      for (int o = 0; o < sv.rows_total; ++o) sv.heads[row * sv.rows_total + o] = hd[o];
    } else if (p.mode == FG_MLP_SE3) {
      const float x[3] = {src[0], src[1], src[2]};
      mlp_se3_row(hd, x, row, p);
    } else {
      int v = 0;
      for (int h = 0; h < p.n_heads; ++h) {
        const int rows = p.head_rows[h];
        if (float* d = p.out[h])
          for (int j = 0; j < rows; ++j) d[row * rows + j] = hd[v + j];
        v += rows;
      }
    }
  }
}

// INPUTS: also g_enc [N, enc_w] = P_5 W_5[:, :in_ch] + P_0 W_0 from `tin` (fg_mlp_bwd_inputs); false: neither is looked at.
// A launch takes the rows from tile tile_begin up to row N (the END of its rows, not of the arrays; acts_rows = the rows of a
// layer of acts): g_heads, acts and g_enc are addressed by the row itself, g_pre by the row less the launch's first with
// pre_rows rows to a layer -- fg_mlp_train_bwd's chunk array; the whole-array calls pass tile_begin = 0 and acts_rows =
// pre_rows = N.  (The first tile as a 32-bit argument: the kernel sits at the scalar-register limit, and a 64-bit first row
// cost <true> two vector registers over its 224 -- profiles/mlp_chunked_bwd.md.)
template <bool INPUTS>
__global__ void __launch_bounds__(MLP_BLOCK) __attribute__((amdgpu_waves_per_eu(INPUTS ? 2 : 1)))
mlp_bwd_kernel(int64_t N, int tile_begin, int64_t acts_rows, int64_t pre_rows, int rows_total, const float* __restrict__ g_heads,
               const float* __restrict__ acts, float* __restrict__ g_pre, const float* __restrict__ ws,
               const float* __restrict__ tin, float* __restrict__ g_enc, int in_ch, int enc_w) {
  __shared__ __attribute__((aligned(16))) float grad[MLP_M * MLP_ACT_STRIDE];
  __shared__ __attribute__((aligned(16))) float gh[MLP_M * MLP_GH_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row_begin = (int64_t)tile_begin * MLP_M, row0 = row_begin + (int64_t)blockIdx.x * MLP_M;

  // ---- the head cotangents: [64][16], zero beyond rows_total and beyond N
  for (int i = tid; i < MLP_M * 16; i += MLP_BLOCK) {
    const int r = i >> 4, o = i & 15;
    gh[r * MLP_GH_STRIDE + o] = (row0 + r < N && o < rows_total) ? g_heads[(row0 + r) * rows_total + o] : 0.f;
  }
  __syncthreads();

  const int li = lane & 31, lh = lane >> 5;
  const float* a_grad = grad + li * MLP_ACT_STRIDE + 4 * lh;
  const size_t b_lane = (size_t)(wave * 64 + li) * 8 + 4 * lh;
  f32x16 acc[2][2];
  for (int rb = 0; rb < 2; ++rb)
    for (int cb = 0; cb < 2; ++cb)
      for (int e = 0; e < 16; ++e) acc[rb][cb][e] = 0.f;
  // (INPUTS) whether any of this wave's 64 x 32 block of g_enc lies inside the row, and its column of the packed weights
  const bool in_block = INPUTS && 32 * wave < enc_w;
  const float* b_in = tin + (size_t)(wave * 32 + li) * 8 + 4 * lh;
  mlp_gemm_part(acc, gh + li * MLP_GH_STRIDE + 4 * lh, MLP_GH_STRIDE, 2, ws + MLP_T_HEAD + b_lane);  // g(h_7)
  for (int l = MLP_D - 1; l >= 0; --l) {
    // P_l = g(h_l) where h_l > 0: to g_pre and, for the next product, in place of the previous tile
    const float* h = acts + (int64_t)l * acts_rows * MLP_W;
    // (row_begin taken off the layer's base, a scalar: the row offsets below are the ones acts is read with)
    float* out = g_pre + ((int64_t)l * pre_rows - row_begin) * MLP_W;
    for (int rb = 0; rb < 2; ++rb)
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = 32 * rb + (e & 3) + 8 * (e >> 2) + 4 * lh, c = wave * 64 + 32 * cb + li;
          const bool live = row0 + r < N;
          const float v = live && h[(row0 + r) * MLP_W + c] > 0.f ? acc[rb][cb][e] : 0.f;
          if (live) out[(row0 + r) * MLP_W + c] = v;
          acc[rb][cb][e] = v;
        }
    if (l == 0 && !INPUTS) break;
    __syncthreads();  // every wave has read the whole of the tile behind (l = 7: nothing to wait for, one barrier)
    for (int rb = 0; rb < 2; ++rb)
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = 32 * rb + (e & 3) + 8 * (e >> 2) + 4 * lh;
          grad[r * MLP_ACT_STRIDE + wave * 64 + 32 * cb + li] = acc[rb][cb][e];
          acc[rb][cb][e] = 0.f;
        }
    __syncthreads();
    if (INPUTS && in_block && (l == MLP_SKIP + 1 || l == 0)) {
      // the chain of a g_enc element: from 0, layer 5's 256 terms, then layer 0's.  The partial sum waits in g_enc itself,
      // written and read back by the same lane, so no register is held across the layers between (rows >= N: zeros in
      // the tile, nothing stored)
      const int c = wave * 32 + li;
      f32x16 gin[2];
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = 32 * rb + (e & 3) + 8 * (e >> 2) + 4 * lh;
          gin[rb][e] = l == 0 && row0 + r < N && c < enc_w ? g_enc[(row0 + r) * enc_w + c] : 0.f;
        }
      mlp_gemm_in(gin, a_grad, MLP_ACT_STRIDE, MLP_W / 8, b_in + (l == 0 ? 0 : MLP_TIN_LAYER_FLOATS));
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = 32 * rb + (e & 3) + 8 * (e >> 2) + 4 * lh;
          if (row0 + r < N && c < enc_w) g_enc[(row0 + r) * enc_w + c] = c < in_ch ? gin[rb][e] : 0.f;
        }
    }
    if (INPUTS && l == 0) break;
    mlp_gemm_part(acc, a_grad, MLP_ACT_STRIDE, MLP_W / 8, ws + (size_t)(l - 1) * MLP_T_LAYER_FLOATS + b_lane);  // g(h_{l-1})
  }
}

// ---- FG_MLP_BF16X3: the same tiles on the bf16 matrix instruction, every operand as hi + lo (the contract: include/fgraster.h).
//   split    : hi = bf16(v) (round to nearest even), lo = bf16(v - float(hi)); done ONCE per value, by the lane that holds the
//              accumulator (layer epilogue), by the pack launches (weights), by the loaders (input row, head cotangents)
//   LDS      : a row holds its hi values, then its lo values, then 8 bf16 of padding: [64][2 x 256 + 8] bf16 is byte for byte the
//              fp32 tile ([64][260] floats), and the row stride is the same 4 mod 64 dwords, so the 16-byte operand reads fall on
//              the banks they fell on.  Input row [64][2 x 128 + 8], head cotangents [64][2 x 16 + 8]: the fp32 arrays' bytes too.
//   k order  : K is walked in steps of 16; lane half h of a wave holds k = 16 s + 8 h + j, j = 0..7, in one 16-byte read, for A
//              (LDS) and B (packed weights) alike.  Per step an output element takes A_hi B_hi, then A_hi B_lo, then A_lo B_hi
//              (v_mfma_f32_32x32x16_bf16, fp32 accumulation, A_lo B_lo dropped); steps in ascending order; the accumulator
//              starts where the fp32 chain's does.  Nothing but the element's own row enters: rows stay independent.
//   packed B : per layer [step][plane: hi, lo][column][16] bf16 -- 16 KB a step, what two k-groups of the fp32 packing take, so
//              every workspace size holds (an odd number of k-groups of the input row rounds up to a step of zeros: still within
//              the documented size, which is that of the widest input row, 16 groups)
//   heads    : the forward's 16-row head product stays on v_mfma_f32_16x16x4_f32: the last layer's epilogue leaves h_7 in LDS as
//              fp32 (the tile has the bytes), and the head code is the fp32 kernel's
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
constexpr int MLPS_ACT_STRIDE = 2 * MLP_W + 8, MLPS_ACT_LO = MLP_W;                 // 520 bf16 = 260 dwords
constexpr int MLPS_IN_STRIDE = 2 * MLP_IN_COLS + 8, MLPS_IN_LO = MLP_IN_COLS;       // 264 bf16 = 132 dwords
constexpr int MLPS_GH_STRIDE = 2 * 16 + 8, MLPS_GH_LO = 16;                         // 40 bf16 = 20 dwords
constexpr int MLPS_PLANE = MLP_W * 16;        // bf16 of one plane of one k-step of a 256-column packing
constexpr int MLPS_TIN_PLANE = MLP_IN_COLS * 16;
static_assert(MLPS_ACT_STRIDE * 2 == MLP_ACT_STRIDE * 4 && MLPS_IN_STRIDE * 2 == MLP_IN_STRIDE * 4 && MLPS_GH_STRIDE * 2 == MLP_GH_STRIDE * 4,
              "the split tiles take the fp32 tiles' bytes");

// the forward's packed workspace under FG_MLP_BF16X3: offsets in floats (one float = the hi and the lo of one weight), heads fp32
struct MlpSplitLayout {
  int s0;               // k-steps of the input row
  size_t layer[MLP_D];  // float offset of each packed layer
  int steps[MLP_D];
  size_t head_w, head_b, total;
};

inline MlpSplitLayout mlp_split_layout(int A) {
  MlpSplitLayout L;
  L.s0 = (MLP_XCH + A + 15) / 16;
  size_t at = 0;
  for (int l = 0; l < MLP_D; ++l) {
    L.steps[l] = l == 0 ? L.s0 : (l == MLP_SKIP + 1 ? L.s0 + MLP_W / 16 : MLP_W / 16);
    L.layer[l] = at;
    at += (size_t)L.steps[l] * MLPS_PLANE;
  }
  L.head_w = at;
  at += 16 * MLP_W;
  L.head_b = at;
  at += 16;
  L.total = at;
  return L;
}

__device__ __forceinline__ void mlp_split(float v, __bf16& hi, __bf16& lo) {
  hi = (__bf16)v;
  lo = (__bf16)(v - (float)hi);
}

// one weight to its two planes: `rel` = its index in the layer's [step][column][16] order, `plane` the bf16 of one plane of a step
__device__ __forceinline__ void mlp_split_store(__bf16* layer, size_t rel, int plane, float v) {
  __bf16 hi, lo;
  mlp_split(v, hi, lo);
  __bf16* dst = layer + rel / plane * (2 * (size_t)plane) + rel % plane;
  dst[0] = hi;
  dst[plane] = lo;
}

__global__ void __launch_bounds__(MLP_BLOCK)
mlp_pack_split_kernel(MlpArgs p, MlpSplitLayout L, float* __restrict__ ws) {
  const size_t at = (size_t)blockIdx.x * MLP_BLOCK + threadIdx.x;
  if (at >= L.total) return;
  const int in_ch = MLP_XCH + p.A;
  if (at >= L.head_w) {  // the heads as the fp32 pack leaves them: [16][256], then [16]
    const bool is_b = at >= L.head_b;
    const int o = is_b ? (int)(at - L.head_b) : (int)(at - L.head_w) / MLP_W, k = is_b ? 0 : (int)(at - L.head_w) % MLP_W;
    int v = 0;
    float r = 0.f;
    for (int h = 0; h < p.n_heads; ++h) {
      if (o >= v && o < v + p.head_rows[h]) r = is_b ? p.head_b[h][o - v] : p.head_W[h][(o - v) * MLP_W + k];
      v += p.head_rows[h];
    }
    ws[at] = r;
    return;
  }
  int l = 0;
  while (l + 1 < MLP_D && at >= L.layer[l + 1]) ++l;
  const size_t rel = at - L.layer[l];
  const int s = (int)(rel / MLPS_PLANE), j = (int)(rel % MLPS_PLANE) / 16, k = 16 * s + (int)(rel % 16);
  const float* W = p.W[l];
  float r = 0.f;
  if (l == 0) {
    if (k < in_ch) r = W[(size_t)j * in_ch + k];
  } else if (l == MLP_SKIP + 1) {
    const int ld = in_ch + MLP_W;
    if (s < L.s0) {
      if (k < in_ch) r = W[(size_t)j * ld + k];
    } else {
      r = W[(size_t)j * ld + in_ch + k - 16 * L.s0];
    }
  } else {
    r = W[(size_t)j * MLP_W + k];
  }
  mlp_split_store(reinterpret_cast<__bf16*>(ws + L.layer[l]), rel, MLPS_PLANE, r);
}

// the backward's weights, split: per layer [16 steps][hi, lo][k][16] of W_l[16 s + e][off_l + k]; the heads are one step
__global__ void __launch_bounds__(MLP_BLOCK)
mlp_pack_t_split_kernel(MlpArgs p, float* __restrict__ ws) {
  const size_t at = (size_t)blockIdx.x * MLP_BLOCK + threadIdx.x;
  if (at >= MLP_T_TOTAL) return;
  const int in_ch = MLP_XCH + p.A;
  const size_t rel = at < MLP_T_HEAD ? at % MLP_T_LAYER_FLOATS : at - MLP_T_HEAD;
  const int j = 16 * (int)(rel / MLPS_PLANE) + (int)(rel % 16), k = (int)(rel % MLPS_PLANE) / 16;
  float r = 0.f;
  if (at < MLP_T_HEAD) {
    const int l = 1 + (int)(at / MLP_T_LAYER_FLOATS);
    r = l == MLP_SKIP + 1 ? p.W[l][(size_t)j * (in_ch + MLP_W) + in_ch + k] : p.W[l][(size_t)j * MLP_W + k];
  } else {
    int v = 0;
    for (int h = 0; h < p.n_heads; ++h) {
      if (j >= v && j < v + p.head_rows[h]) r = p.head_W[h][(j - v) * MLP_W + k];
      v += p.head_rows[h];
    }
  }
  mlp_split_store(reinterpret_cast<__bf16*>(ws + (at - rel)), rel, MLPS_PLANE, r);
}

// the input-row backward's weights, split: Tin[{0,5}][16 steps][hi, lo][k < 128][16] of W_l[16 s + e][k], zero from in_ch on
__global__ void __launch_bounds__(MLP_BLOCK)
mlp_pack_tin_split_kernel(MlpArgs p, float* __restrict__ tin) {
  const size_t at = (size_t)blockIdx.x * MLP_BLOCK + threadIdx.x;
  if (at >= MLP_TIN_TOTAL) return;
  const int in_ch = MLP_XCH + p.A;
  const int l = at < MLP_TIN_LAYER_FLOATS ? 0 : MLP_SKIP + 1;
  const int rel = (int)(at % MLP_TIN_LAYER_FLOATS);
  const int j = 16 * (rel / MLPS_TIN_PLANE) + rel % 16, k = rel % MLPS_TIN_PLANE / 16;
  const float r = k < in_ch ? p.W[l][(size_t)j * (l == 0 ? in_ch : in_ch + MLP_W) + k] : 0.f;
  mlp_split_store(reinterpret_cast<__bf16*>(tin + (at - rel)), (size_t)rel, MLPS_TIN_PLANE, r);
}

// acc += src x packed weights, three products a step: `a` points at this lane's row of the LDS source (+ 8 h; the lo values
// a_lo further on), `b` at this lane's column of the packed layer's hi plane (+ 8 h; the lo plane `plane` further on), NB column
// blocks of 32.  The next step's operands are fetched before the current step's MFMAs; the four (two) accumulators take a
// term in turn, so no instruction waits on the one before it.
template <int NB>
__device__ __forceinline__ void mlp_gemm_split(f32x16 (&acc)[2][NB], const __bf16* a, int stride, int a_lo, int steps,
                                               const __bf16* __restrict__ b, int plane) {
  bf16x8 ah[2], al[2], bh[NB], bl[NB];
  for (int rb = 0; rb < 2; ++rb) {
    ah[rb] = *reinterpret_cast<const bf16x8*>(a + 32 * rb * stride);
    al[rb] = *reinterpret_cast<const bf16x8*>(a + 32 * rb * stride + a_lo);
  }
  for (int cb = 0; cb < NB; ++cb) {
    bh[cb] = *reinterpret_cast<const bf16x8*>(b + 32 * 16 * cb);
    bl[cb] = *reinterpret_cast<const bf16x8*>(b + 32 * 16 * cb + plane);
  }
  for (int s = 0; s < steps; ++s) {
    bf16x8 nah[2], nal[2], nbh[NB], nbl[NB];
    for (int rb = 0; rb < 2; ++rb) nah[rb] = ah[rb], nal[rb] = al[rb];
    for (int cb = 0; cb < NB; ++cb) nbh[cb] = bh[cb], nbl[cb] = bl[cb];
    if (s + 1 < steps) {
      const __bf16* an = a + 16 * (s + 1);
      const __bf16* bn = b + (size_t)(s + 1) * (2 * plane);
      for (int rb = 0; rb < 2; ++rb) {
        nah[rb] = *reinterpret_cast<const bf16x8*>(an + 32 * rb * stride);
        nal[rb] = *reinterpret_cast<const bf16x8*>(an + 32 * rb * stride + a_lo);
      }
      for (int cb = 0; cb < NB; ++cb) {
        nbh[cb] = *reinterpret_cast<const bf16x8*>(bn + 32 * 16 * cb);
        nbl[cb] = *reinterpret_cast<const bf16x8*>(bn + 32 * 16 * cb + plane);
      }
    }
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) acc[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rb], bh[cb], acc[rb][cb], 0, 0, 0);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) acc[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[rb], bl[cb], acc[rb][cb], 0, 0, 0);
#pragma unroll
    for (int rb = 0; rb < 2; ++rb)
#pragma unroll
      for (int cb = 0; cb < NB; ++cb) acc[rb][cb] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[rb], bh[cb], acc[rb][cb], 0, 0, 0);
    for (int rb = 0; rb < 2; ++rb) ah[rb] = nah[rb], al[rb] = nal[rb];
    for (int cb = 0; cb < NB; ++cb) bh[cb] = nbh[cb], bl[cb] = nbl[cb];
  }
}

// mlp_fwd_kernel under FG_MLP_BF16X3: the same phases, the same stores (all from fp32 values)
template <bool TRAIN>
__global__ void __launch_bounds__(MLP_BLOCK)
mlp_fwd_split_kernel(int64_t N, MlpArgs p, MlpSplitLayout L, const float* __restrict__ ws, MlpSaved sv) {
  __shared__ __attribute__((aligned(16))) __bf16 act[MLP_M * MLPS_ACT_STRIDE];
  __shared__ __attribute__((aligned(16))) __bf16 inp[MLP_M * MLPS_IN_STRIDE];
  float* actf = reinterpret_cast<float*>(act);  // [64][260] floats: the fp32 input rows first, h_7 for the heads last
  float* inpf = reinterpret_cast<float*>(inp);  // [64][132] floats: the head results, once the input rows are dead
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row0 = (int64_t)blockIdx.x * MLP_M;
  const int enc_w = FG_MLP_ENC_WIDTH(p.A);

  // ---- the input rows in fp32, as the fp32 kernel forms them (into the activation tile, which nothing uses yet)
  {
    const int r = tid >> 2, q = tid & 3;
    const int64_t row = row0 + r;
    const bool live = row < N;
    float* dst = actf + r * MLP_IN_STRIDE;
    float x[3] = {0.f, 0.f, 0.f};
    if (live)
      for (int c = 0; c < 3; ++c) x[c] = p.x[row * 3 + c];
    if (q == 3)
      for (int c = 0; c < 3; ++c) dst[c] = x[c];
    for (int k = q; k < MLP_FREQS; k += 4) {
      const float f = (float)(1 << k);
      for (int c = 0; c < 3; ++c) {
        float s, co;
        sincosf(x[c] * f, &s, &co);
        dst[3 + 6 * k + c] = s;
        dst[3 + 6 * k + 3 + c] = co;
      }
    }
    const float* aux = p.aux + row * p.aux_stride;
    for (int a = q; a < p.A; a += 4) dst[MLP_XCH + a] = live ? aux[a] : 0.f;
    for (int k = MLP_XCH + p.A + q; k < enc_w; k += 4) dst[k] = 0.f;
  }
  __syncthreads();
  if (TRAIN) {
    for (int i = tid; i < MLP_M * enc_w; i += MLP_BLOCK) {
      const int r = i / enc_w, k = i % enc_w;
      if (row0 + r < N) sv.enc[(row0 + r) * enc_w + k] = actf[r * MLP_IN_STRIDE + k];
    }
  }
  // split once, zero up to the last k-step's end
  {
    const int w = 16 * L.s0;
    for (int i = tid; i < MLP_M * w; i += MLP_BLOCK) {
      const int r = i / w, k = i % w;
      __bf16 hi, lo;
      mlp_split(k < enc_w ? actf[r * MLP_IN_STRIDE + k] : 0.f, hi, lo);
      inp[r * MLPS_IN_STRIDE + k] = hi;
      inp[r * MLPS_IN_STRIDE + MLPS_IN_LO + k] = lo;
    }
  }
  __syncthreads();

  // ---- trunk
  const int li = lane & 31, lh = lane >> 5;
  const __bf16* a_inp = inp + li * MLPS_IN_STRIDE + 8 * lh;
  const __bf16* a_act = act + li * MLPS_ACT_STRIDE + 8 * lh;
  const size_t b_lane = (size_t)(wave * 64 + li) * 16 + 8 * lh;
  for (int l = 0; l < MLP_D; ++l) {
    f32x16 acc[2][2];
    const float* bias = p.b[l] + wave * 64 + li;
    for (int cb = 0; cb < 2; ++cb) {
      const float bv = bias[32 * cb];
      for (int e = 0; e < 16; ++e) acc[0][cb][e] = bv, acc[1][cb][e] = bv;
    }
    const __bf16* wp = reinterpret_cast<const __bf16*>(ws + L.layer[l]) + b_lane;
    if (l == 0) {
      mlp_gemm_split<2>(acc, a_inp, MLPS_IN_STRIDE, MLPS_IN_LO, L.s0, wp, MLPS_PLANE);
    } else if (l == MLP_SKIP + 1) {
      mlp_gemm_split<2>(acc, a_inp, MLPS_IN_STRIDE, MLPS_IN_LO, L.s0, wp, MLPS_PLANE);
      mlp_gemm_split<2>(acc, a_act, MLPS_ACT_STRIDE, MLPS_ACT_LO, MLP_W / 16, wp + (size_t)L.s0 * (2 * MLPS_PLANE), MLPS_PLANE);
    } else {
      mlp_gemm_split<2>(acc, a_act, MLPS_ACT_STRIDE, MLPS_ACT_LO, MLP_W / 16, wp, MLPS_PLANE);
    }
    __syncthreads();  // every wave has read the whole of the previous layer
    for (int rb = 0; rb < 2; ++rb)
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = 32 * rb + (e & 3) + 8 * (e >> 2) + 4 * lh, c = wave * 64 + 32 * cb + li;
          const float h = fmaxf(acc[rb][cb][e], 0.f);
          if (l == MLP_D - 1) {
            actf[r * MLP_ACT_STRIDE + c] = h;
          } else {
            __bf16 hi, lo;
            mlp_split(h, hi, lo);
            act[r * MLPS_ACT_STRIDE + c] = hi;
            act[r * MLPS_ACT_STRIDE + MLPS_ACT_LO + c] = lo;
          }
          if (TRAIN && row0 + r < N) sv.acts[((int64_t)l * N + row0 + r) * MLP_W + c] = h;
        }
    __syncthreads();
  }

  // ---- heads: the fp32 kernel's, over the fp32 h_7
  {
    const int hi = lane & 15, hq = lane >> 4;
    const float* a = actf + (wave * 16 + hi) * MLP_ACT_STRIDE + 4 * hq;
    const float* b = ws + L.head_w + hi * MLP_W + 4 * hq;
    const float bv = ws[L.head_b + hi];
    f32x4 acc = {bv, bv, bv, bv};
    for (int g = 0; g < MLP_W / 16; ++g) {
      const f32x4 av = *reinterpret_cast<const f32x4*>(a + 16 * g);
      const f32x4 bw = *reinterpret_cast<const f32x4*>(b + 16 * g);
#pragma unroll
      for (int s = 0; s < 4; ++s) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bw[s], acc, 0, 0, 0);
    }
    for (int e = 0; e < 4; ++e) inpf[(wave * 16 + 4 * hq + e) * MLP_IN_STRIDE + MLP_HEAD_COL + hi] = acc[e];
  }
  __syncthreads();

  // ---- epilogue: one lane per row (x from global: the LDS copy is split)
  if (tid < MLP_M && row0 + tid < N) {
    const int64_t row = row0 + tid;
    const float* src = inpf + tid * MLP_IN_STRIDE;
    float hd[16];
    for (int o = 0; o < 16; ++o) hd[o] = src[MLP_HEAD_COL + o];
    if (TRAIN) {
      for (int o = 0; o < sv.rows_total; ++o) sv.heads[row * sv.rows_total + o] = hd[o];
    } else if (p.mode == FG_MLP_SE3) {
      const float x[3] = {p.x[row * 3], p.x[row * 3 + 1], p.x[row * 3 + 2]};
      mlp_se3_row(hd, x, row, p);
    } else {
      int v = 0;
      for (int h = 0; h < p.n_heads; ++h) {
        const int rows = p.head_rows[h];
        if (float* d = p.out[h])
          for (int j = 0; j < rows; ++j) d[row * rows + j] = hd[v + j];
        v += rows;
      }
    }
  }
}

// mlp_bwd_kernel under FG_MLP_BF16X3: the same chain, arguments and stores; the gradient tile and the head cotangents split
template <bool INPUTS>
__global__ void __launch_bounds__(MLP_BLOCK) __attribute__((amdgpu_waves_per_eu(INPUTS ? 2 : 1)))
mlp_bwd_split_kernel(int64_t N, int tile_begin, int64_t acts_rows, int64_t pre_rows, int rows_total, const float* __restrict__ g_heads,
                     const float* __restrict__ acts, float* __restrict__ g_pre, const float* __restrict__ ws,
                     const float* __restrict__ tin, float* __restrict__ g_enc, int in_ch, int enc_w) {
  __shared__ __attribute__((aligned(16))) __bf16 grad[MLP_M * MLPS_ACT_STRIDE];
  __shared__ __attribute__((aligned(16))) __bf16 gh[MLP_M * MLPS_GH_STRIDE];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int64_t row_begin = (int64_t)tile_begin * MLP_M, row0 = row_begin + (int64_t)blockIdx.x * MLP_M;

  for (int i = tid; i < MLP_M * 16; i += MLP_BLOCK) {
    const int r = i >> 4, o = i & 15;
    __bf16 hi, lo;
    mlp_split((row0 + r < N && o < rows_total) ? g_heads[(row0 + r) * rows_total + o] : 0.f, hi, lo);
    gh[r * MLPS_GH_STRIDE + o] = hi;
    gh[r * MLPS_GH_STRIDE + MLPS_GH_LO + o] = lo;
  }
  __syncthreads();

  const int li = lane & 31, lh = lane >> 5;
  const __bf16* a_grad = grad + li * MLPS_ACT_STRIDE + 8 * lh;
  const __bf16* wsb = reinterpret_cast<const __bf16*>(ws);
  const size_t b_lane = (size_t)(wave * 64 + li) * 16 + 8 * lh;
  f32x16 acc[2][2];
  for (int rb = 0; rb < 2; ++rb)
    for (int cb = 0; cb < 2; ++cb)
      for (int e = 0; e < 16; ++e) acc[rb][cb][e] = 0.f;
  const bool in_block = INPUTS && 32 * wave < enc_w;
  const __bf16* b_in = reinterpret_cast<const __bf16*>(tin) + (size_t)(wave * 32 + li) * 16 + 8 * lh;
  mlp_gemm_split<2>(acc, gh + li * MLPS_GH_STRIDE + 8 * lh, MLPS_GH_STRIDE, MLPS_GH_LO, 1, wsb + 2 * MLP_T_HEAD + b_lane, MLPS_PLANE);  // g(h_7)
  for (int l = MLP_D - 1; l >= 0; --l) {
    const float* h = acts + (int64_t)l * acts_rows * MLP_W;
    float* out = g_pre + ((int64_t)l * pre_rows - row_begin) * MLP_W;
    for (int rb = 0; rb < 2; ++rb)
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = 32 * rb + (e & 3) + 8 * (e >> 2) + 4 * lh, c = wave * 64 + 32 * cb + li;
          const bool live = row0 + r < N;
          const float v = live && h[(row0 + r) * MLP_W + c] > 0.f ? acc[rb][cb][e] : 0.f;
          if (live) out[(row0 + r) * MLP_W + c] = v;
          acc[rb][cb][e] = v;
        }
    if (l == 0 && !INPUTS) break;
    __syncthreads();
    for (int rb = 0; rb < 2; ++rb)
      for (int cb = 0; cb < 2; ++cb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = 32 * rb + (e & 3) + 8 * (e >> 2) + 4 * lh, c = wave * 64 + 32 * cb + li;
          __bf16 hi, lo;
          mlp_split(acc[rb][cb][e], hi, lo);
          grad[r * MLPS_ACT_STRIDE + c] = hi;
          grad[r * MLPS_ACT_STRIDE + MLPS_ACT_LO + c] = lo;
        }
    __syncthreads();
    if (INPUTS && in_block && (l == MLP_SKIP + 1 || l == 0)) {
      const int c = wave * 32 + li;
      f32x16 gin[2][1];
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = 32 * rb + (e & 3) + 8 * (e >> 2) + 4 * lh;
          gin[rb][0][e] = l == 0 && row0 + r < N && c < enc_w ? g_enc[(row0 + r) * enc_w + c] : 0.f;
        }
      mlp_gemm_split<1>(gin, a_grad, MLPS_ACT_STRIDE, MLPS_ACT_LO, MLP_W / 16, b_in + (l == 0 ? 0 : 2 * MLP_TIN_LAYER_FLOATS), MLPS_TIN_PLANE);
      for (int rb = 0; rb < 2; ++rb)
#pragma unroll
        for (int e = 0; e < 16; ++e) {
          const int r = 32 * rb + (e & 3) + 8 * (e >> 2) + 4 * lh;
          if (row0 + r < N && c < enc_w) g_enc[(row0 + r) * enc_w + c] = c < in_ch ? gin[rb][0][e] : 0.f;
        }
    }
    if (INPUTS && l == 0) break;
    // (zeroed here, not where the tile is written: no register holds a zero across the g_enc product)
    for (int rb = 0; rb < 2; ++rb)
      for (int cb = 0; cb < 2; ++cb)
        for (int e = 0; e < 16; ++e) acc[rb][cb][e] = 0.f;
    mlp_gemm_split<2>(acc, a_grad, MLPS_ACT_STRIDE, MLPS_ACT_LO, MLP_W / 16, wsb + 2 * (size_t)(l - 1) * MLP_T_LAYER_FLOATS + b_lane, MLPS_PLANE);  // g(h_{l-1})
  }
}

// the descriptor checks every entry point shares; `inputs`: x and aux are read
int mlp_check_desc(const fg_mlp_desc* d, bool inputs) {
  if (!d || d->size != (int32_t)sizeof(fg_mlp_desc)) return FG_ERR_INVALID_ARG;
  if (d->aux_width < 1 || d->aux_width > 64 || d->aux_stride < 0) return FG_ERR_INVALID_ARG;
  if (d->mode != FG_MLP_SE3 && d->mode != FG_MLP_PLAIN) return FG_ERR_INVALID_ARG;
  if (!fg_mlp_precision_supported(d->precision)) return FG_ERR_INVALID_ARG;
  if (d->n_heads < 1 || d->n_heads > FG_MLP_MAX_HEADS) return FG_ERR_INVALID_ARG;
  int total = 0;
  for (int h = 0; h < d->n_heads; ++h) {
    if (d->head_rows[h] < 1 || d->head_rows[h] > 16) return FG_ERR_INVALID_ARG;
    total += d->head_rows[h];
  }
  if (total > 16) return FG_ERR_INVALID_ARG;
  if (d->mode == FG_MLP_SE3 &&
      (d->n_heads != 4 || d->head_rows[0] != 3 || d->head_rows[1] != 3 || d->head_rows[2] != 4 || d->head_rows[3] != 3))
    return FG_ERR_INVALID_ARG;
  if (d->depth != MLP_D || d->width != MLP_W || d->multires != MLP_FREQS) return FG_ERR_UNSUPPORTED;
  if (inputs && (!d->x || !d->aux)) return FG_ERR_INVALID_ARG;
  for (int l = 0; l < MLP_D; ++l)
    if (!d->weight[l] || !d->bias[l]) return FG_ERR_INVALID_ARG;
  for (int h = 0; h < d->n_heads; ++h)
    if (!d->head_weight[h] || !d->head_bias[h]) return FG_ERR_INVALID_ARG;
  return FG_OK;
}

// (N > 0) the grid's x extent, then the workspace: present, the documented size, 16-byte aligned
int mlp_check_launch(int64_t N, const void* workspace, size_t workspace_bytes, size_t need) {
  if (!workspace) return FG_ERR_INVALID_ARG;
  if (N > ((int64_t)1 << 31) * MLP_M - MLP_M) return FG_ERR_INVALID_ARG;
  if (workspace_bytes < need) return FG_ERR_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(workspace) % 16) return FG_ERR_INVALID_ARG;
  return FG_OK;
}

MlpArgs mlp_args(const fg_mlp_desc* d) {
  MlpArgs p = {};
  p.x = d->x, p.aux = d->aux, p.aux_stride = d->aux_stride;
  for (int l = 0; l < MLP_D; ++l) p.W[l] = d->weight[l], p.b[l] = d->bias[l];
  for (int h = 0; h < d->n_heads; ++h) {
    p.head_W[h] = d->head_weight[h], p.head_b[h] = d->head_bias[h], p.head_rows[h] = d->head_rows[h];
    p.out[h] = d->out[h];
  }
  p.n_heads = d->n_heads, p.A = d->aux_width, p.mode = d->mode;
  return p;
}

// pack, then the network: the two launches of fg_mlp_fwd and fg_mlp_train_fwd
template <bool TRAIN>
int mlp_launch_fwd(int64_t N, const MlpArgs& p, int precision, const MlpSaved& sv, void* workspace, fg_stream_t stream) {
  hipStream_t s = fg_hip_stream(stream);
  float* ws = static_cast<float*>(workspace);
  const dim3 tiles((unsigned)((N + MLP_M - 1) / MLP_M));
  if (precision == FG_MLP_BF16X3) {
    const MlpSplitLayout L = mlp_split_layout(p.A);
    hipLaunchKernelGGL(mlp_pack_split_kernel, dim3((unsigned)((L.total + MLP_BLOCK - 1) / MLP_BLOCK)), dim3(MLP_BLOCK), 0, s, p, L, ws);
    FG_RETURN_IF_LAUNCH_FAILED();
    hipLaunchKernelGGL(mlp_fwd_split_kernel<TRAIN>, tiles, dim3(MLP_BLOCK), 0, s, N, p, L, ws, sv);
    FG_RETURN_IF_LAUNCH_FAILED();
    return FG_OK;
  }
  const MlpLayout L = mlp_layout(p.A);
  hipLaunchKernelGGL(mlp_pack_kernel, dim3((unsigned)((L.total + MLP_BLOCK - 1) / MLP_BLOCK)), dim3(MLP_BLOCK), 0, s, p, L, ws);
  FG_RETURN_IF_LAUNCH_FAILED();
  hipLaunchKernelGGL(mlp_fwd_kernel<TRAIN>, tiles, dim3(MLP_BLOCK), 0, s, N, p, L, ws, sv);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

}  // namespace

extern "C" size_t fg_mlp_workspace_bytes(int64_t N) {
  // (the packed weights alone: the same for every N; sized for the widest input row)
  return N < 0 ? 0 : mlp_layout(64).total * sizeof(float);
}

extern "C" int fg_mlp_fwd(int64_t N, const fg_mlp_desc* d, void* workspace, size_t workspace_bytes, fg_stream_t stream) {
  if (N < 0) return FG_ERR_INVALID_ARG;
  if (N == 0) return FG_OK;
  if (int rc = mlp_check_desc(d, true)) return rc;
  // (the documented size, whatever aux_width)
  if (int rc = mlp_check_launch(N, workspace, workspace_bytes, fg_mlp_workspace_bytes(N))) return rc;
  return mlp_launch_fwd<false>(N, mlp_args(d), d->precision, MlpSaved{}, workspace, stream);
}

extern "C" size_t fg_mlp_train_workspace_bytes(int64_t N) {
  // (one size for both calls: the larger of the forward's and the backward's packed weights; the same for every N)
  const size_t fwd = fg_mlp_workspace_bytes(N), bwd = MLP_T_TOTAL * sizeof(float);
  return N < 0 ? 0 : (fwd > bwd ? fwd : bwd);
}

extern "C" int fg_mlp_train_fwd(int64_t N, const fg_mlp_desc* d, float* heads, float* enc, float* acts, void* workspace,
                                size_t workspace_bytes, fg_stream_t stream) {
  if (N < 0) return FG_ERR_INVALID_ARG;
  if (N == 0) return FG_OK;
  if (int rc = mlp_check_desc(d, true)) return rc;
  if (d->mode != FG_MLP_PLAIN || !heads || !enc || !acts) return FG_ERR_INVALID_ARG;
  if (int rc = mlp_check_launch(N, workspace, workspace_bytes, fg_mlp_train_workspace_bytes(N))) return rc;
  MlpSaved sv = {heads, enc, acts, 0};
  for (int h = 0; h < d->n_heads; ++h) sv.rows_total += d->head_rows[h];
  return mlp_launch_fwd<true>(N, mlp_args(d), d->precision, sv, workspace, stream);
}

// ---- what fg_mlp_train_bwd (mlp_wgrad.hip) shares with the two calls below: mlp_internal.h
int fg_mlp_detail::bwd_check(int64_t N, const fg_mlp_desc* d, const void* workspace, size_t workspace_bytes, size_t need) {
  if (int rc = mlp_check_desc(d, false)) return rc;
  if (d->mode != FG_MLP_PLAIN) return FG_ERR_INVALID_ARG;
  return need ? mlp_check_launch(N, workspace, workspace_bytes, need) : FG_OK;
}

int fg_mlp_detail::bwd_launch_pack(const fg_mlp_desc* d, bool inputs, void* workspace, fg_stream_t stream) {
  const MlpArgs p = mlp_args(d);
  hipStream_t s = fg_hip_stream(stream);
  float* ws = static_cast<float*>(workspace);
  const bool split = d->precision == FG_MLP_BF16X3;
  hipLaunchKernelGGL(split ? mlp_pack_t_split_kernel : mlp_pack_t_kernel, dim3((unsigned)((MLP_T_TOTAL + MLP_BLOCK - 1) / MLP_BLOCK)),
                     dim3(MLP_BLOCK), 0, s, p, ws);
  FG_RETURN_IF_LAUNCH_FAILED();
  if (!inputs) return FG_OK;
  hipLaunchKernelGGL(split ? mlp_pack_tin_split_kernel : mlp_pack_tin_kernel, dim3((unsigned)((MLP_TIN_TOTAL + MLP_BLOCK - 1) / MLP_BLOCK)),
                     dim3(MLP_BLOCK), 0, s, p, ws + MLP_T_TOTAL);
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

int fg_mlp_detail::bwd_launch_rows(int64_t N, const fg_mlp_desc* d, int64_t row_begin, int64_t row_end, const float* g_heads,
                                   const float* acts, float* g_pre, int64_t pre_rows, float* g_enc, const void* workspace,
                                   fg_stream_t stream) {
  int rows_total = 0;
  for (int h = 0; h < d->n_heads; ++h) rows_total += d->head_rows[h];
  hipStream_t s = fg_hip_stream(stream);
  const float* ws = static_cast<const float*>(workspace);
  const dim3 tiles((unsigned)((row_end - row_begin + MLP_M - 1) / MLP_M));
  const bool split = d->precision == FG_MLP_BF16X3;
  if (!g_enc)
    hipLaunchKernelGGL(split ? mlp_bwd_split_kernel<false> : mlp_bwd_kernel<false>, tiles, dim3(MLP_BLOCK), 0, s, row_end, (int)(row_begin / MLP_M), N, pre_rows, rows_total, g_heads, acts,
                       g_pre, ws, nullptr, nullptr, 0, 0);
  else
    hipLaunchKernelGGL(split ? mlp_bwd_split_kernel<true> : mlp_bwd_kernel<true>, tiles, dim3(MLP_BLOCK), 0, s, row_end, (int)(row_begin / MLP_M), N, pre_rows, rows_total, g_heads, acts,
                       g_pre, ws, ws + MLP_T_TOTAL, g_enc, MLP_XCH + d->aux_width, FG_MLP_ENC_WIDTH(d->aux_width));
  FG_RETURN_IF_LAUNCH_FAILED();
  return FG_OK;
}

namespace {

// the launches of fg_mlp_bwd (g_enc null) and fg_mlp_bwd_inputs: the packed weights, then the chain over all the rows
int mlp_launch_bwd(int64_t N, const fg_mlp_desc* d, const float* g_heads, const float* acts, float* g_pre, float* g_enc,
                   void* workspace, fg_stream_t stream) {
  if (int rc = fg_mlp_detail::bwd_launch_pack(d, g_enc != nullptr, workspace, stream)) return rc;
  return fg_mlp_detail::bwd_launch_rows(N, d, 0, N, g_heads, acts, g_pre, N, g_enc, workspace, stream);
}

}  // namespace

extern "C" int fg_mlp_bwd(int64_t N, const fg_mlp_desc* d, const float* g_heads, const float* acts, float* g_pre,
                          void* workspace, size_t workspace_bytes, fg_stream_t stream) {
  if (N < 0) return FG_ERR_INVALID_ARG;
  if (N == 0) return FG_OK;
  if (int rc = mlp_check_desc(d, false)) return rc;
  if (d->mode != FG_MLP_PLAIN || !g_heads || !acts || !g_pre) return FG_ERR_INVALID_ARG;
  if (int rc = mlp_check_launch(N, workspace, workspace_bytes, fg_mlp_train_workspace_bytes(N))) return rc;
  return mlp_launch_bwd(N, d, g_heads, acts, g_pre, nullptr, workspace, stream);
}

extern "C" size_t fg_mlp_bwd_inputs_workspace_bytes(int64_t N) {
  // (the training workspace and, behind it, the input columns of layers 0 and 5; the same for every N)
  return N < 0 ? 0 : fg_mlp_train_workspace_bytes(N) + MLP_TIN_TOTAL * sizeof(float);
}

extern "C" int fg_mlp_bwd_inputs(int64_t N, const fg_mlp_desc* d, const float* g_heads, const float* acts, float* g_pre,
                                 float* g_enc, void* workspace, size_t workspace_bytes, fg_stream_t stream) {
  if (N < 0) return FG_ERR_INVALID_ARG;
  if (N == 0) return FG_OK;
  if (int rc = mlp_check_desc(d, false)) return rc;
  if (d->mode != FG_MLP_PLAIN || !g_heads || !acts || !g_pre || !g_enc) return FG_ERR_INVALID_ARG;
  if (int rc = mlp_check_launch(N, workspace, workspace_bytes, fg_mlp_bwd_inputs_workspace_bytes(N))) return rc;
  return mlp_launch_bwd(N, d, g_heads, acts, g_pre, g_enc, workspace, stream);
}

extern "C" int fg_mlp_precision_supported(int32_t precision) { return precision == FG_MLP_FP32 || precision == FG_MLP_BF16X3; }
