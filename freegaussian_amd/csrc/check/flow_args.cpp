// Stand-alone host check of the flow supervision's entry points -- fg_flow_disp_fwd, fg_flow_disp_bwd,
// fg_flow_l1_workspace_bytes, fg_flow_l1_fwd, fg_flow_l1_bwd -- for a build of abi.hip, flow_disp.hip and flow_loss.hip whose
// HOST code carries AddressSanitizer + UndefinedBehaviorSanitizer (make flow-check).  Every call below returns before a launch:
// the program needs no GPU and touches none.
#include <cmath>

#include "check_common.h"

// addresses nobody reads, 64 MiB apart from 1 GiB on
static float* at(int i) { return reinterpret_cast<float*>(((uintptr_t)1 << 30) + ((uintptr_t)i << 26)); }
static char* bytes(float* p) { return reinterpret_cast<char*>(p); }

// displacement: means_t 0, means_0 1, viewmat_t 2, viewmat_0 3, K 4, disp / g_disp 5, g_means_t 6, g_means_0 7, a row block 8
static int dfwd(int64_t N, const float* mt, int64_t mts, const float* m0, int64_t m0s, const float* vt, const float* v0, const float* K,
                int w, int h, float near, float margin, float* disp) {
  return fg_flow_disp_fwd(N, mt, mts, m0, m0s, vt, v0, K, w, h, near, margin, disp, nullptr);
}
static int dbwd(int64_t N, const float* mt, int64_t mts, const float* m0, int64_t m0s, const float* vt, const float* v0, const float* K,
                int w, int h, float near, float margin, const float* g, float* gt, float* g0) {
  return fg_flow_disp_bwd(N, mt, mts, m0, m0s, vt, v0, K, w, h, near, margin, g, gt, g0, nullptr);
}

// loss: pred 0, flows 1, mask 2, workspace 3, out / v_out 4, g_pred 5
static int lfwd(int H, int W, const float* pred, int64_t px, int64_t rw, int H0, int W0, int d, const float* flows, const void* mask,
                int mdt, void* ws, size_t nws, float* out) {
  return fg_flow_l1_fwd(H, W, pred, px, rw, H0, W0, d, flows, mask, mdt, ws, nws, out, nullptr);
}
static int lbwd(int H, int W, const float* pred, int64_t px, int64_t rw, int H0, int W0, int d, const float* flows, const void* mask,
                int mdt, const void* ws, const float* v, float* g) {
  return fg_flow_l1_bwd(H, W, pred, px, rw, H0, W0, d, flows, mask, mdt, ws, v, g, nullptr);
}

static void displacement() {
  const int64_t N = 1000;
  const float inf = INFINITY, nan = NAN;
  // ---- row counts
  for (int64_t n : {INT64_MIN, (int64_t)-1}) {
    EXPECT(dfwd(n, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5)), FG_ERR_INVALID_ARG);
    EXPECT(dbwd(n, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5), at(6), at(7)), FG_ERR_INVALID_ARG);
  }
  EXPECT(dfwd(0, at(0), 3, at(1), 3, at(2), nullptr, at(4), 64, 48, 0.01f, inf, at(5)), FG_OK);
  EXPECT(dfwd(0, at(0), 3, at(1), 3, at(2), nullptr, at(4), 64, 48, 0.01f, inf, at(0)), FG_OK);  // (no row: nothing overlaps)
  EXPECT(dbwd(0, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, 64.f, at(5), at(6), at(7)), FG_OK);
  EXPECT(dfwd(0, nullptr, 3, at(1), 3, at(2), nullptr, at(4), 64, 48, 0.01f, inf, at(5)), FG_ERR_INVALID_ARG);
  for (int64_t n : {(int64_t)FG_FLOW_DISP_MAX_ROWS + 1, INT64_MAX}) {
    EXPECT(dfwd(n, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5)), FG_ERR_UNSUPPORTED);
    EXPECT(dbwd(n, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5), at(6), at(7)), FG_ERR_UNSUPPORTED);
  }
  // large and supported: the spans are computed without overflow and, 64 MiB apart, overlap
  EXPECT(dfwd(FG_FLOW_DISP_MAX_ROWS, at(0), 13, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5)), FG_ERR_INVALID_ARG);
  // ---- null and absent pointers: viewmat_0 alone may be absent (one camera); a gradient that is not asked for is absent
  EXPECT(dfwd(N, nullptr, 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5)), FG_ERR_INVALID_ARG);
  EXPECT(dfwd(N, at(0), 3, nullptr, 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5)), FG_ERR_INVALID_ARG);
  EXPECT(dfwd(N, at(0), 3, at(1), 3, nullptr, at(3), at(4), 64, 48, 0.01f, inf, at(5)), FG_ERR_INVALID_ARG);
  EXPECT(dfwd(N, at(0), 3, at(1), 3, at(2), at(3), nullptr, 64, 48, 0.01f, inf, at(5)), FG_ERR_INVALID_ARG);
  EXPECT(dfwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(dbwd(N, nullptr, 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5), at(6), at(7)), FG_ERR_INVALID_ARG);
  EXPECT(dbwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, nullptr, at(6), at(7)), FG_ERR_INVALID_ARG);
  EXPECT(dbwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5), nullptr, nullptr), FG_OK);  // nothing asked for
  EXPECT(dbwd(N, at(0), 3, at(1), 3, at(2), nullptr, at(4), 64, 48, 0.01f, inf, at(5), nullptr, nullptr), FG_OK);
  // ---- scalars
  EXPECT(dfwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 0, 48, 0.01f, inf, at(5)), FG_ERR_INVALID_ARG);
  EXPECT(dfwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, -1, 0.01f, inf, at(5)), FG_ERR_INVALID_ARG);
  for (float near : {-1.f, inf, nan}) EXPECT(dfwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, near, inf, at(5)), FG_ERR_INVALID_ARG);
  for (float margin : {-1.f, nan}) {
    EXPECT(dfwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, margin, at(5)), FG_ERR_INVALID_ARG);
    EXPECT(dbwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, margin, at(5), at(6), at(7)), FG_ERR_INVALID_ARG);
  }
  // ---- strides below the width, and far
  for (int64_t s : {INT64_MIN, (int64_t)-3, (int64_t)0, (int64_t)2}) {
    EXPECT(dfwd(N, at(0), s, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5)), FG_ERR_INVALID_ARG);
    EXPECT(dfwd(N, at(0), 3, at(1), s, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5)), FG_ERR_INVALID_ARG);
    EXPECT(dbwd(N, at(0), 3, at(1), s, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5), at(6), at(7)), FG_ERR_INVALID_ARG);
  }
  for (int64_t s : {(int64_t)FG_FLOW_DISP_MAX_STRIDE + 1, INT64_MAX}) {
    EXPECT(dfwd(N, at(0), s, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5)), FG_ERR_UNSUPPORTED);
    EXPECT(dbwd(N, at(0), 3, at(1), s, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5), at(6), at(7)), FG_ERR_UNSUPPORTED);
  }
  // ---- alignment of the 8-byte displacement words
  EXPECT(dfwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5) + 1), FG_ERR_INVALID_ARG);
  EXPECT(dbwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5) + 1, at(6), at(7)), FG_ERR_INVALID_ARG);
  // ---- overlapping outputs: whole, by the output's last float, by the input's last float; with contiguous means and with
  // columns 0..2 / 3..5 of one [N,13] block
  const size_t r3 = (size_t)N * 3, r2 = (size_t)N * 2;
  for (int64_t s : {(int64_t)3, (int64_t)13}) {
    float* mt = s == 3 ? at(0) : at(8);
    float* m0 = s == 3 ? at(1) : at(8) + 3;
    const size_t in = (size_t)(N - 1) * s + 3;
    float* victims[5] = {mt, m0, at(2), at(3), at(4)};
    const size_t lens[5] = {in, in, 16, 16, 9};
    for (int i = 0; i < 5; ++i) {
      // (steps of two floats keep the displacement words aligned)
      EXPECT(dfwd(N, mt, s, m0, s, at(2), at(3), at(4), 64, 48, 0.01f, inf, victims[i]), FG_ERR_INVALID_ARG);
      EXPECT(dfwd(N, mt, s, m0, s, at(2), at(3), at(4), 64, 48, 0.01f, inf, victims[i] - (r2 - 2)), FG_ERR_INVALID_ARG);
      EXPECT(dfwd(N, mt, s, m0, s, at(2), at(3), at(4), 64, 48, 0.01f, inf, victims[i] + ((lens[i] - 1) & ~(size_t)1)), FG_ERR_INVALID_ARG);
      for (int o = 0; o < 2; ++o)
        for (int how = 0; how < 3; ++how) {
          float* bad = victims[i] + (how == 0 ? 0 : how == 1 ? (ptrdiff_t)(lens[i] - 1) : -(ptrdiff_t)(r3 - 1));
          EXPECT(dbwd(N, mt, s, m0, s, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5), o == 0 ? bad : at(6), o == 1 ? bad : at(7)), FG_ERR_INVALID_ARG);
          EXPECT(dbwd(N, mt, s, m0, s, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5), o == 0 ? bad : nullptr, o == 1 ? bad : nullptr), FG_ERR_INVALID_ARG);
        }
    }
    // an output on g_disp (one camera: the absent viewmat_0 overlaps nothing), and the outputs on each other
    EXPECT(dbwd(N, mt, s, m0, s, at(2), nullptr, at(4), 64, 48, 0.01f, inf, at(5), at(5), nullptr), FG_ERR_INVALID_ARG);  // on g_disp
    EXPECT(dbwd(N, mt, s, m0, s, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5), at(6), at(6)), FG_ERR_INVALID_ARG);        // on each other
    EXPECT(dbwd(N, mt, s, m0, s, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5), at(6), at(6) + (r3 - 1)), FG_ERR_INVALID_ARG);
    EXPECT(dbwd(N, mt, s, m0, s, at(2), at(3), at(4), 64, 48, 0.01f, inf, at(5), at(6), at(6) - (r3 - 1)), FG_ERR_INVALID_ARG);
  }
}

static void loss() {
  // a 33 x 17 render of a (2 * 33 + 1) x (2 * 17 + 1) source at d = 2, pred as channels 4..5 of a 6-channel block
  const int H = 33, W = 17, d = 2, H0 = 67, W0 = 35;
  const int64_t px = 6, rw = 6 * W;
  const size_t need = fg_flow_l1_workspace_bytes(H0, W0, d);
  EXPECT(need, 16 * (1 + (33 * 17 + 255) / 256));
  // ---- the query: 0 for anything unsupported, pure
  for (int bad : {0, 3, 5, 6, 16, -1, -2, INT32_MIN, INT32_MAX}) EXPECT(fg_flow_l1_workspace_bytes(H0, W0, bad), 0);
  EXPECT(fg_flow_l1_workspace_bytes(0, W0, 1), 0);
  EXPECT(fg_flow_l1_workspace_bytes(H0, -5, 1), 0);
  EXPECT(fg_flow_l1_workspace_bytes(32769, W0, 1), 0);
  EXPECT(fg_flow_l1_workspace_bytes(7, 9, 8), 0);  // (no whole block in a 7-row source)
  EXPECT(fg_flow_l1_workspace_bytes(8, 8, 8), 32);
  EXPECT(fg_flow_l1_workspace_bytes(32768, 32768, 1), 16 * (1 + ((size_t)1 << 22)));
  // everything in order but one argument; in order means FG_ERR_WORKSPACE here: a workspace of no bytes keeps the call on the host
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), 0, at(4)), FG_ERR_WORKSPACE);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), FG_TARGET_U8, at(3), need - 1, at(4)), FG_ERR_WORKSPACE);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), FG_TARGET_F32, at(3), 0, at(4)), FG_ERR_WORKSPACE);
  // ---- unsupported d, and H != H0 / d
  for (int bad : {0, 3, 16, -2}) {
    EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, bad, at(1), nullptr, 0, at(3), need, at(4)), FG_ERR_UNSUPPORTED);
    EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, bad, at(1), nullptr, 0, at(3), at(4), at(5)), FG_ERR_UNSUPPORTED);
  }
  for (int h : {H - 1, H + 1, 0, -1, H0}) {
    EXPECT(lfwd(h, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), 0, at(4)), FG_ERR_INVALID_ARG);
    EXPECT(lbwd(h, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), at(4), at(5)), FG_ERR_INVALID_ARG);
  }
  EXPECT(lfwd(H, W + 1, at(0), px, rw + 6, H0, W0, d, at(1), nullptr, 0, at(3), 0, at(4)), FG_ERR_INVALID_ARG);
  EXPECT(lfwd(H, W, at(0), px, rw, 0, W0, d, at(1), nullptr, 0, at(3), 0, at(4)), FG_ERR_INVALID_ARG);
  EXPECT(lfwd(H, W, at(0), px, rw, 40000, W0, d, at(1), nullptr, 0, at(3), 0, at(4)), FG_ERR_UNSUPPORTED);
  // ---- null and absent pointers (the mask alone may be absent; its dtype is then not looked at)
  EXPECT(lfwd(H, W, nullptr, px, rw, H0, W0, d, at(1), nullptr, 0, at(3), 0, at(4)), FG_ERR_INVALID_ARG);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, nullptr, nullptr, 0, at(3), 0, at(4)), FG_ERR_INVALID_ARG);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, nullptr, 0, at(4)), FG_ERR_INVALID_ARG);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), 0, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 77, at(3), 0, at(4)), FG_ERR_WORKSPACE);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), 77, at(3), 0, at(4)), FG_ERR_UNSUPPORTED);
  EXPECT(lbwd(H, W, nullptr, px, rw, H0, W0, d, at(1), nullptr, 0, at(3), at(4), at(5)), FG_ERR_INVALID_ARG);
  EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, d, nullptr, nullptr, 0, at(3), at(4), at(5)), FG_ERR_INVALID_ARG);
  EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, nullptr, at(4), at(5)), FG_ERR_INVALID_ARG);
  EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), nullptr, at(5)), FG_ERR_INVALID_ARG);
  EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), at(4), nullptr), FG_ERR_INVALID_ARG);
  // ---- alignment
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1) + 1, nullptr, 0, at(3), 0, at(4)), FG_ERR_INVALID_ARG);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), bytes(at(2)) + 2, FG_TARGET_F32, at(3), 0, at(4)), FG_ERR_INVALID_ARG);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), bytes(at(2)) + 3, FG_TARGET_U8, at(3), 0, at(4)), FG_ERR_WORKSPACE);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3) + 2, 0, at(4)), FG_ERR_INVALID_ARG);
  EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), at(4), at(5) + 1), FG_ERR_INVALID_ARG);
  // ---- strides below the width
  for (int64_t s : {INT64_MIN, (int64_t)-6, (int64_t)0, (int64_t)1}) {
    EXPECT(lfwd(H, W, at(0), s, rw, H0, W0, d, at(1), nullptr, 0, at(3), 0, at(4)), FG_ERR_INVALID_ARG);
    EXPECT(lbwd(H, W, at(0), s, rw, H0, W0, d, at(1), nullptr, 0, at(3), at(4), at(5)), FG_ERR_INVALID_ARG);
  }
  for (int64_t s : {INT64_MIN, (int64_t)0, (int64_t)(6 * (W - 1) + 1)}) {
    EXPECT(lfwd(H, W, at(0), px, s, H0, W0, d, at(1), nullptr, 0, at(3), 0, at(4)), FG_ERR_INVALID_ARG);
    EXPECT(lbwd(H, W, at(0), px, s, H0, W0, d, at(1), nullptr, 0, at(3), at(4), at(5)), FG_ERR_INVALID_ARG);
  }
  EXPECT(lfwd(H, W, at(0), px, 6 * (W - 1) + 2, H0, W0, d, at(1), nullptr, 0, at(3), 0, at(4)), FG_ERR_WORKSPACE);
  EXPECT(lfwd(H, W, at(0), 2, 2 * W, H0, W0, d, at(1), nullptr, 0, at(3), 0, at(4)), FG_ERR_WORKSPACE);
  EXPECT(lfwd(H, W, at(0), FG_FLOW_L1_MAX_STRIDE + 1, INT64_MAX, H0, W0, d, at(1), nullptr, 0, at(3), 0, at(4)), FG_ERR_UNSUPPORTED);
  // ---- overlapping outputs.  floats of pred's span, of the source, of the float mask
  const size_t n_pred = (size_t)(H - 1) * rw + (size_t)(W - 1) * px + 2, n_flow = (size_t)H0 * W0 * 2, n_mask = (size_t)H0 * W0;
  float* ins[3] = {at(0), at(1), at(2)};
  const size_t lens[3] = {n_pred, n_flow, n_mask};
  for (int i = 0; i < 3; ++i) {
    // the workspace (16-byte steps) and out on each input: at its start and on its last float
    float* last = ins[i] + (lens[i] - 1);
    float* last16 = ins[i] + ((lens[i] - 1) & ~(size_t)3);
    EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), FG_TARGET_F32, ins[i], need, at(4)), FG_ERR_INVALID_ARG);
    EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), FG_TARGET_F32, last16, need, at(4)), FG_ERR_INVALID_ARG);
    EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), FG_TARGET_F32, at(3), need, ins[i]), FG_ERR_INVALID_ARG);
    EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), FG_TARGET_F32, at(3), need, last), FG_ERR_INVALID_ARG);
    // g_pred (8-byte steps) on each input
    EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), FG_TARGET_F32, at(3), at(4), ins[i]), FG_ERR_INVALID_ARG);
    EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), FG_TARGET_F32, at(3), at(4), ins[i] + ((lens[i] - 1) & ~(size_t)1)), FG_ERR_INVALID_ARG);
    EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), FG_TARGET_F32, at(3), at(4), ins[i] - ((size_t)H * W * 2 - 2)), FG_ERR_INVALID_ARG);
  }
  // the byte mask is a quarter as long: an output just behind it is in order (and then short of workspace)
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), FG_TARGET_U8, at(3), 0, at(2) + (n_mask / 4 + 1)), FG_ERR_WORKSPACE);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), at(2), FG_TARGET_U8, at(3), 0, at(2) + (n_mask / 4 - 1)), FG_ERR_INVALID_ARG);
  // out inside the workspace; g_pred on the workspace's totals and on v_out
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), need, at(3) + 4), FG_ERR_INVALID_ARG);
  EXPECT(lfwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), need, at(3) + (need / 4 - 1)), FG_ERR_INVALID_ARG);
  EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), at(4), at(3) + 2), FG_ERR_INVALID_ARG);
  EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), at(4), at(4)), FG_ERR_INVALID_ARG);
  EXPECT(lbwd(H, W, at(0), px, rw, H0, W0, d, at(1), nullptr, 0, at(3), at(4), at(4) - ((size_t)H * W * 2 - 2)), FG_ERR_INVALID_ARG);
}

int main() {
  EXPECT(fg_abi_version(), FG_ABI_VERSION);
  EXPECT(fg_abi_minor(), FG_ABI_MINOR);
  displacement();
  loss();
  return report("flow_args");
}
