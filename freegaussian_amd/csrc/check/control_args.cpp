// Stand-alone host check of the stage-2 control stage's entry points -- fg_control_supported, fg_control_workspace_bytes,
// fg_control_attr_mean, fg_control_value_rows, fg_control_scatter_fwd, fg_control_scatter_bwd -- for a build of abi.hip and
// control.hip whose HOST code carries AddressSanitizer + UndefinedBehaviorSanitizer (make control-check).  Every call below
// returns before a launch: the program needs no GPU and touches none.
#include <vector>

#include "check_common.h"

// addresses nobody reads, 64 MiB apart from 4 GiB on (the largest span below is under 64 MiB)
template <typename T = float>
static T* at(int i) {
  return reinterpret_cast<T*>(((uintptr_t)1 << 32) + ((uintptr_t)i << 26));
}

static const int64_t n = 1000, N = 5000;
static const int M = 3;
static int32_t counts3[3] = {400, 1000, 1};

static int mean(int64_t n_, int M_, const float* a, int64_t as, const float* b, int64_t bs, const uint32_t* bits, const int32_t* counts,
                void* ws, size_t ws_bytes, float* d_avg) {
  return fg_control_attr_mean(n_, M_, a, as, b, bs, bits, counts, ws, ws_bytes, d_avg, nullptr);
}
static int value(int64_t n_, int M_, const uint32_t* bits, const float* d_avg, float* out) {
  return fg_control_value_rows(n_, M_, bits, d_avg, out, nullptr);
}
static int fwd(int64_t N_, int64_t n_, const int32_t* rank, const float* means, const float* x, int64_t xs, const float* q, int64_t qs,
               const float* s, int64_t ss, float* om, float* orot, float* oscale) {
  return fg_control_scatter_fwd(N_, n_, rank, means, x, xs, q, qs, s, ss, om, orot, oscale, nullptr);
}
static int bwd(int64_t n_, int64_t N_, const int32_t* sel, const float* gm, const float* gr, const float* gs, float* x, int64_t xs, float* q,
               int64_t qs, float* s, int64_t ss) {
  return fg_control_scatter_bwd(n_, N_, sel, gm, gr, gs, x, xs, q, qs, s, ss, nullptr);
}

int main() {
  EXPECT(fg_abi_version(), FG_ABI_VERSION);
  EXPECT(fg_abi_minor(), FG_ABI_MINOR);
  // ---- the two queries
  for (int m : {INT32_MIN, -1, 0, FG_CONTROL_MAX_ATTRS + 1, INT32_MAX}) {
    EXPECT(fg_control_supported(m), 0);
    EXPECT(fg_control_workspace_bytes(n, m), 0);
  }
  for (int m = 1; m <= FG_CONTROL_MAX_ATTRS; ++m) EXPECT(fg_control_supported(m), 1);
  for (int64_t rows : {INT64_MIN, (int64_t)-1, (int64_t)0, (int64_t)FG_CONTROL_MAX_ROWS + 1, INT64_MAX})
    EXPECT(fg_control_workspace_bytes(rows, M), 0);
  EXPECT(fg_control_workspace_bytes(1, 1), 3 * 8);
  EXPECT(fg_control_workspace_bytes(FG_CONTROL_BLOCK_ROWS, 3), 9 * 8);
  EXPECT(fg_control_workspace_bytes(FG_CONTROL_BLOCK_ROWS + 1, 3), 2 * 9 * 8);
  EXPECT(fg_control_workspace_bytes(70001, 32), 69 * 96 * 8);
  EXPECT(fg_control_workspace_bytes(FG_CONTROL_MAX_ROWS, 32), (size_t)(FG_CONTROL_MAX_ROWS / FG_CONTROL_BLOCK_ROWS) * 96 * 8);
  const size_t need = fg_control_workspace_bytes(n, M);
  float *a = at(0), *b = at(1), *d_avg = at(3), *ws = at(4);
  const uint32_t* bits = at<uint32_t>(2);

  // ---- fg_control_attr_mean.  In order but for one argument; the last call of the block has everything in order but an
  // output laid on an input, so that nothing is ever launched
  for (int64_t rows : {INT64_MIN, (int64_t)-1, (int64_t)0}) EXPECT(mean(rows, M, a, 3, b, 3, bits, counts3, ws, BIG, d_avg), FG_ERR_INVALID_ARG);
  for (int64_t rows : {(int64_t)FG_CONTROL_MAX_ROWS + 1, INT64_MAX}) EXPECT(mean(rows, M, a, 3, b, 3, bits, counts3, ws, BIG, d_avg), FG_ERR_UNSUPPORTED);
  for (int m : {INT32_MIN, -1, 0}) EXPECT(mean(n, m, a, 3, b, 3, bits, counts3, ws, BIG, d_avg), FG_ERR_INVALID_ARG);
  for (int m : {FG_CONTROL_MAX_ATTRS + 1, INT32_MAX}) EXPECT(mean(n, m, a, 3, b, 3, bits, counts3, ws, BIG, d_avg), FG_ERR_UNSUPPORTED);
  EXPECT(mean(n, M, nullptr, 3, b, 3, bits, counts3, ws, need, d_avg), FG_ERR_INVALID_ARG);
  EXPECT(mean(n, M, a, 3, nullptr, 3, bits, counts3, ws, need, d_avg), FG_ERR_INVALID_ARG);
  EXPECT(mean(n, M, a, 3, b, 3, nullptr, counts3, ws, need, d_avg), FG_ERR_INVALID_ARG);
  EXPECT(mean(n, M, a, 3, b, 3, bits, nullptr, ws, need, d_avg), FG_ERR_INVALID_ARG);
  EXPECT(mean(n, M, a, 3, b, 3, bits, counts3, nullptr, need, d_avg), FG_ERR_INVALID_ARG);
  EXPECT(mean(n, M, a, 3, b, 3, bits, counts3, ws, need, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(mean(n, M, a, 3, b, 3, bits, counts3, reinterpret_cast<char*>(ws) + 4, BIG, d_avg), FG_ERR_INVALID_ARG);  // misaligned
  for (int64_t s : {INT64_MIN, (int64_t)-3, (int64_t)0, (int64_t)2}) {
    EXPECT(mean(n, M, a, s, b, 3, bits, counts3, ws, need, d_avg), FG_ERR_INVALID_ARG);
    EXPECT(mean(n, M, a, 3, b, s, bits, counts3, ws, need, d_avg), FG_ERR_INVALID_ARG);
  }
  for (int64_t s : {(int64_t)FG_CONTROL_MAX_STRIDE + 1, INT64_MAX}) {
    EXPECT(mean(n, M, a, s, b, 3, bits, counts3, ws, need, d_avg), FG_ERR_UNSUPPORTED);
    EXPECT(mean(n, M, a, 3, b, s, bits, counts3, ws, need, d_avg), FG_ERR_UNSUPPORTED);
  }
  // counts: an attribute without a row, a negative count, more rows than there are; only the first M are read
  for (int32_t bad : {INT32_MIN, -1, 0, (int32_t)n + 1, INT32_MAX})
    for (int m = 0; m < M; ++m) {
      int32_t c[3] = {400, 1000, 1};
      c[m] = bad;
      EXPECT(mean(n, M, a, 3, b, 3, bits, c, ws, need, d_avg), FG_ERR_INVALID_ARG);
    }
  {
    std::vector<int32_t> exact(M, 1);  // (exactly M words: the sanitizer sees a read beyond them)
    EXPECT(mean(n, M, a, 3, b, 3, bits, exact.data(), ws, need, a), FG_ERR_INVALID_ARG);
    std::vector<int32_t> full(FG_CONTROL_MAX_ATTRS, 7);
    EXPECT(mean(n, FG_CONTROL_MAX_ATTRS, a, 3, b, 3, bits, full.data(), ws, BIG, a), FG_ERR_INVALID_ARG);
    full[31] = 0;
    EXPECT(mean(n, FG_CONTROL_MAX_ATTRS, a, 3, b, 3, bits, full.data(), ws, BIG, d_avg), FG_ERR_INVALID_ARG);
    EXPECT(mean(n, FG_CONTROL_MAX_ATTRS - 1, a, 3, b, 3, bits, full.data(), ws, BIG, a), FG_ERR_INVALID_ARG);  // (word 31 not read; d_avg on a)
  }
  // workspace size
  EXPECT(mean(n, M, a, 3, b, 3, bits, counts3, ws, 0, d_avg), FG_ERR_WORKSPACE);
  EXPECT(mean(n, M, a, 3, b, 3, bits, counts3, ws, need - 1, d_avg), FG_ERR_WORKSPACE);
  EXPECT(mean(FG_CONTROL_MAX_ROWS, 32, a, 3, b, 3, bits, std::vector<int32_t>(32, 5).data(), ws, BIG >> 20, d_avg), FG_ERR_WORKSPACE);
  // aliasing: d_avg or the workspace on an input, by the first and by the last float; columns of a [n,10] block as inputs
  const size_t rows3 = (size_t)n * 3, block = (size_t)(n - 1) * 10 + 3;
  for (int64_t s : {(int64_t)3, (int64_t)10}) {
    const size_t in = s == 3 ? rows3 : block;
    EXPECT(mean(n, M, a, s, b, 3, bits, counts3, ws, need, a), FG_ERR_INVALID_ARG);
    EXPECT(mean(n, M, a, s, b, 3, bits, counts3, ws, need, a + (in - 1)), FG_ERR_INVALID_ARG);
    EXPECT(mean(n, M, a, s, b, 3, bits, counts3, ws, need, a - (M * 3 - 1)), FG_ERR_INVALID_ARG);
    EXPECT(mean(n, M, a, 3, b, s, bits, counts3, ws, need, b + (in - 1)), FG_ERR_INVALID_ARG);
    EXPECT(mean(n, M, a, s, b, 3, bits, counts3, a + ((in - 1) & ~(size_t)1), need, d_avg), FG_ERR_INVALID_ARG);  // (8-byte aligned, on a's last floats)
  }
  EXPECT(mean(n, M, a, 3, b, 3, bits, counts3, ws, need, const_cast<float*>(reinterpret_cast<const float*>(bits)) + (n - 1)), FG_ERR_INVALID_ARG);
  EXPECT(mean(n, M, a, 3, b, 3, bits, counts3, ws, need, ws), FG_ERR_INVALID_ARG);
  EXPECT(mean(n, M, a, 3, b, 3, bits, counts3, ws, need, ws + (need / 4 - 1)), FG_ERR_INVALID_ARG);
  EXPECT(mean(n, M, a, 3, a, 3, bits, counts3, ws, need, a), FG_ERR_INVALID_ARG);  // (a == b is in order; d_avg on them is not)

  // ---- fg_control_value_rows
  float* val = at(5);
  for (int64_t rows : {INT64_MIN, (int64_t)-1}) EXPECT(value(rows, M, bits, d_avg, val), FG_ERR_INVALID_ARG);
  EXPECT(value(0, M, bits, d_avg, val), FG_OK);
  EXPECT(value(0, M, bits, d_avg, const_cast<float*>(d_avg)), FG_OK);  // (no row: nothing overlaps)
  EXPECT(value(0, FG_CONTROL_MAX_ATTRS + 1, bits, d_avg, val), FG_ERR_UNSUPPORTED);
  EXPECT(value(0, 0, bits, d_avg, val), FG_ERR_INVALID_ARG);
  for (int64_t rows : {(int64_t)FG_CONTROL_MAX_ROWS + 1, INT64_MAX}) EXPECT(value(rows, M, bits, d_avg, val), FG_ERR_UNSUPPORTED);
  for (int m : {INT32_MIN, -1, 0}) EXPECT(value(n, m, bits, d_avg, val), FG_ERR_INVALID_ARG);
  for (int m : {FG_CONTROL_MAX_ATTRS + 1, INT32_MAX}) EXPECT(value(n, m, bits, d_avg, val), FG_ERR_UNSUPPORTED);
  EXPECT(value(n, M, nullptr, d_avg, val), FG_ERR_INVALID_ARG);
  EXPECT(value(n, M, bits, nullptr, val), FG_ERR_INVALID_ARG);
  EXPECT(value(n, M, bits, d_avg, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(value(n, M, bits, d_avg, d_avg), FG_ERR_INVALID_ARG);
  EXPECT(value(n, M, bits, d_avg, d_avg + (M * 3 - 1)), FG_ERR_INVALID_ARG);
  EXPECT(value(n, M, bits, d_avg, d_avg - (rows3 - 1)), FG_ERR_INVALID_ARG);
  EXPECT(value(n, M, bits, d_avg, const_cast<float*>(reinterpret_cast<const float*>(bits))), FG_ERR_INVALID_ARG);
  EXPECT(value(FG_CONTROL_MAX_ROWS, 32, bits, d_avg, const_cast<float*>(reinterpret_cast<const float*>(bits)) + 100), FG_ERR_INVALID_ARG);

  // ---- fg_control_scatter_fwd
  const int32_t* rank = at<int32_t>(6);
  float *means = at(7), *x = at(8), *q = at(9), *s = at(10), *om = at(11), *orot = at(12), *osc = at(13), *heads = at(14);
  for (int64_t rows : {INT64_MIN, (int64_t)-1}) {
    EXPECT(fwd(rows, 0, rank, means, x, 3, q, 4, s, 3, om, orot, osc), FG_ERR_INVALID_ARG);
    EXPECT(fwd(N, rows, rank, means, x, 3, q, 4, s, 3, om, orot, osc), FG_ERR_INVALID_ARG);
  }
  EXPECT(fwd(N, N + 1, rank, means, x, 3, q, 4, s, 3, om, orot, osc), FG_ERR_INVALID_ARG);  // more selected rows than rows
  EXPECT(fwd(0, 0, rank, means, x, 3, q, 4, s, 3, om, orot, osc), FG_OK);
  EXPECT(fwd(0, 0, rank, means, x, 3, q, 4, s, 3, means, orot, osc), FG_OK);  // (no row: nothing overlaps)
  EXPECT(fwd(0, 0, rank, means, x, 2, q, 4, s, 3, om, orot, osc), FG_ERR_INVALID_ARG);
  for (int64_t rows : {(int64_t)FG_CONTROL_MAX_ROWS + 1, INT64_MAX}) EXPECT(fwd(rows, n, rank, means, x, 3, q, 4, s, 3, om, orot, osc), FG_ERR_UNSUPPORTED);
  EXPECT(fwd(N, n, nullptr, means, x, 3, q, 4, s, 3, om, orot, osc), FG_ERR_INVALID_ARG);
  EXPECT(fwd(N, n, rank, nullptr, x, 3, q, 4, s, 3, om, orot, osc), FG_ERR_INVALID_ARG);
  EXPECT(fwd(N, n, rank, means, nullptr, 3, q, 4, s, 3, om, orot, osc), FG_ERR_INVALID_ARG);
  EXPECT(fwd(N, n, rank, means, x, 3, nullptr, 4, s, 3, om, orot, osc), FG_ERR_INVALID_ARG);
  EXPECT(fwd(N, n, rank, means, x, 3, q, 4, nullptr, 3, om, orot, osc), FG_ERR_INVALID_ARG);
  EXPECT(fwd(N, n, rank, means, x, 3, q, 4, s, 3, nullptr, orot, osc), FG_ERR_INVALID_ARG);
  EXPECT(fwd(N, n, rank, means, x, 3, q, 4, s, 3, om, nullptr, osc), FG_ERR_INVALID_ARG);
  EXPECT(fwd(N, n, rank, means, x, 3, q, 4, s, 3, om, orot, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fwd(N, n, rank, means, x, 3, q, 4, s, 3, om, orot + 1, osc), FG_ERR_INVALID_ARG);  // d_rotation is stored 16 bytes at a time
  for (int64_t st : {INT64_MIN, (int64_t)-3, (int64_t)0, (int64_t)2}) {
    EXPECT(fwd(N, n, rank, means, x, st, q, 4, s, 3, om, orot, osc), FG_ERR_INVALID_ARG);
    EXPECT(fwd(N, n, rank, means, x, 3, q, st, s, 3, om, orot, osc), FG_ERR_INVALID_ARG);
    EXPECT(fwd(N, n, rank, means, x, 3, q, 4, s, st, om, orot, osc), FG_ERR_INVALID_ARG);
  }
  EXPECT(fwd(N, n, rank, means, x, 3, q, 3, s, 3, om, orot, osc), FG_ERR_INVALID_ARG);  // (a rotation row is 4 floats)
  for (int64_t st : {(int64_t)FG_CONTROL_MAX_STRIDE + 1, INT64_MAX}) {
    EXPECT(fwd(N, n, rank, means, x, st, q, 4, s, 3, om, orot, osc), FG_ERR_UNSUPPORTED);
    EXPECT(fwd(N, n, rank, means, x, 3, q, st, s, 3, om, orot, osc), FG_ERR_UNSUPPORTED);
    EXPECT(fwd(N, n, rank, means, x, 3, q, 4, s, st, om, orot, osc), FG_ERR_UNSUPPORTED);
  }
  // aliasing: each output on each input (whole, and by the input's last float), heads contiguous and columns of [n,10]
  const size_t big3 = (size_t)N * 3, big4 = (size_t)N * 4;
  for (int layout = 0; layout < 2; ++layout) {
    const float *hx = layout ? heads : x, *hq = layout ? heads + 3 : q, *hs = layout ? heads + 7 : s;
    const int64_t sx = layout ? 10 : 3, sq = layout ? 10 : 4, ss = layout ? 10 : 3;
    const size_t last_x = (size_t)(n - 1) * sx + 2, last_q = (size_t)(n - 1) * sq + 3, last_s = (size_t)(n - 1) * ss + 2;
    for (int o = 0; o < 3; ++o) {
      const float* victims[5] = {reinterpret_cast<const float*>(rank), means, hx, hq, hs};
      const size_t lasts[5] = {(size_t)N - 1, big3 - 1, last_x, last_q, last_s};
      for (int v = 0; v < 5; ++v)
        for (int how = 0; how < 2; ++how) {
          // (kept 16-byte aligned for d_rotation: the last float rounded down to a multiple of 4 floats still lies inside)
          float* bad = const_cast<float*>(victims[v]) + (how == 0 ? 0 : o == 1 ? (lasts[v] & ~(size_t)3) : lasts[v]);
          if (o == 1 && ((uintptr_t)bad % 16) != 0) bad = reinterpret_cast<float*>((uintptr_t)bad & ~(uintptr_t)15);
          EXPECT(fwd(N, n, rank, means, hx, sx, hq, sq, hs, ss, o == 0 ? bad : om, o == 1 ? bad : orot, o == 2 ? bad : osc), FG_ERR_INVALID_ARG);
        }
    }
    // outputs on each other
    EXPECT(fwd(N, n, rank, means, hx, sx, hq, sq, hs, ss, om, orot, om), FG_ERR_INVALID_ARG);
    EXPECT(fwd(N, n, rank, means, hx, sx, hq, sq, hs, ss, om, orot, om + (big3 - 1)), FG_ERR_INVALID_ARG);
    EXPECT(fwd(N, n, rank, means, hx, sx, hq, sq, hs, ss, orot + (big4 - 1), orot, osc), FG_ERR_INVALID_ARG);
    EXPECT(fwd(N, n, rank, means, hx, sx, hq, sq, hs, ss, om, orot, orot - (big3 - 1)), FG_ERR_INVALID_ARG);
  }

  // ---- fg_control_scatter_bwd
  const int32_t* sel = at<int32_t>(15);
  float *gm = at(16), *gr = at(17), *gs = at(18), *gx = at(19), *gq = at(20), *gsc = at(21), *gheads = at(22);
  for (int64_t rows : {INT64_MIN, (int64_t)-1}) {
    EXPECT(bwd(rows, N, sel, gm, gr, gs, gx, 3, gq, 4, gsc, 3), FG_ERR_INVALID_ARG);
    EXPECT(bwd(0, rows, sel, gm, gr, gs, gx, 3, gq, 4, gsc, 3), FG_ERR_INVALID_ARG);
  }
  EXPECT(bwd(N + 1, N, sel, gm, gr, gs, gx, 3, gq, 4, gsc, 3), FG_ERR_INVALID_ARG);
  EXPECT(bwd(0, N, sel, gm, gr, gs, gx, 3, gq, 4, gsc, 3), FG_OK);
  EXPECT(bwd(0, N, sel, gm, gr, gs, gm, 3, gq, 4, gsc, 3), FG_OK);  // (no row: nothing overlaps)
  EXPECT(bwd(0, N, nullptr, gm, gr, gs, gx, 3, gq, 4, gsc, 3), FG_ERR_INVALID_ARG);
  EXPECT(bwd(n, N, nullptr, gm, gr, gs, gx, 3, gq, 4, gsc, 3), FG_ERR_INVALID_ARG);
  EXPECT(bwd(n, (int64_t)FG_CONTROL_MAX_ROWS + 1, sel, gm, gr, gs, gx, 3, gq, 4, gsc, 3), FG_ERR_UNSUPPORTED);
  // nothing asked for: nothing to do, whatever arrived (the strides of null outputs are not looked at)
  EXPECT(bwd(n, N, sel, gm, gr, gs, nullptr, 0, nullptr, -7, nullptr, INT64_MAX), FG_OK);
  EXPECT(bwd(n, N, sel, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr, 0), FG_OK);
  for (int64_t st : {INT64_MIN, (int64_t)-3, (int64_t)0, (int64_t)2}) {
    EXPECT(bwd(n, N, sel, gm, gr, gs, gx, st, gq, 4, gsc, 3), FG_ERR_INVALID_ARG);
    EXPECT(bwd(n, N, sel, gm, gr, gs, gx, 3, gq, st, gsc, 3), FG_ERR_INVALID_ARG);
    EXPECT(bwd(n, N, sel, gm, gr, gs, gx, 3, gq, 4, gsc, st), FG_ERR_INVALID_ARG);
  }
  EXPECT(bwd(n, N, sel, gm, gr, gs, nullptr, 3, gq, 3, nullptr, 3), FG_ERR_INVALID_ARG);
  for (int64_t st : {(int64_t)FG_CONTROL_MAX_STRIDE + 1, INT64_MAX}) {
    EXPECT(bwd(n, N, sel, gm, gr, gs, gx, st, gq, 4, gsc, 3), FG_ERR_UNSUPPORTED);
    EXPECT(bwd(n, N, sel, gm, gr, gs, gx, 3, gq, st, gsc, 3), FG_ERR_UNSUPPORTED);
    EXPECT(bwd(n, N, sel, gm, gr, gs, gx, 3, gq, 4, gsc, st), FG_ERR_UNSUPPORTED);
  }
  // aliasing: each output on each input, with the other outputs wanted and alone; upstream gradients present or absent
  for (int o = 0; o < 3; ++o) {
    const float* victims[4] = {reinterpret_cast<const float*>(sel), gm, gr, gs};
    const size_t lasts[4] = {(size_t)n - 1, big3 - 1, big4 - 1, big3 - 1};
    for (int v = 0; v < 4; ++v)
      for (int how = 0; how < 2; ++how) {
        float* bad = const_cast<float*>(victims[v]) + (how == 0 ? 0 : lasts[v]);
        EXPECT(bwd(n, N, sel, gm, gr, gs, o == 0 ? bad : gx, 3, o == 1 ? bad : gq, 4, o == 2 ? bad : gsc, 3), FG_ERR_INVALID_ARG);
        EXPECT(bwd(n, N, sel, gm, gr, gs, o == 0 ? bad : nullptr, 3, o == 1 ? bad : nullptr, 4, o == 2 ? bad : nullptr, 3), FG_ERR_INVALID_ARG);
      }
  }
  // outputs on each other: whole, by one float; as columns of one [n,10] block they are in order (and here run into an
  // upstream gradient laid on the block, so that nothing is launched) unless the column ranges meet or the strides differ
  EXPECT(bwd(n, N, sel, gm, gr, gs, gx, 3, gq, 4, gx, 3), FG_ERR_INVALID_ARG);
  EXPECT(bwd(n, N, sel, gm, gr, gs, gx, 3, gx + (rows3 - 1), 4, gsc, 3), FG_ERR_INVALID_ARG);
  EXPECT(bwd(n, N, sel, gheads + 5, gr, gs, gheads, 10, gheads + 3, 10, gheads + 7, 10), FG_ERR_INVALID_ARG);  // (in order but g_means)
  EXPECT(bwd(n, N, sel, gm, gr, gs, gheads, 10, gheads + 2, 10, gheads + 7, 10), FG_ERR_INVALID_ARG);
  EXPECT(bwd(n, N, sel, gm, gr, gs, gheads, 10, gheads + 3, 10, gheads + 6, 10), FG_ERR_INVALID_ARG);
  EXPECT(bwd(n, N, sel, gm, gr, gs, gheads, 10, gheads + 3, 10, gheads + 8, 10), FG_ERR_INVALID_ARG);  // (columns 8..10: into the next row)
  EXPECT(bwd(n, N, sel, gm, gr, gs, gheads, 10, gheads + 3, 11, gheads + 7, 10), FG_ERR_INVALID_ARG);
  EXPECT(bwd(n, N, sel, gm, gr, gs, gheads, 10, reinterpret_cast<float*>(reinterpret_cast<char*>(gheads) + 14), 10, nullptr, 0), FG_ERR_INVALID_ARG);
  return report("control_args");
}
