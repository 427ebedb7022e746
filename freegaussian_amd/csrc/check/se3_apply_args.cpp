// Stand-alone host check of the SE(3) transform's entry points -- fg_se3_apply_fwd, fg_se3_apply_bwd -- for a build of abi.hip
// and se3_apply.hip whose HOST code carries AddressSanitizer + UndefinedBehaviorSanitizer (make se3-check).  Every call below
// returns before a launch: the program needs no GPU and touches none.
#include "check_common.h"

// addresses nobody reads, 16 MiB apart from 1 GiB on: w, v, pts, out / g_out, g_w, g_v, g_pts, a head block
static float* at(int i) { return reinterpret_cast<float*>(((uintptr_t)1 << 30) + ((uintptr_t)i << 24)); }

// the forward with everything in order but one argument
static int fwd(int64_t N, const float* w, int64_t ws, const float* v, int64_t vs, const float* pts, float* out) {
  return fg_se3_apply_fwd(N, w, ws, v, vs, pts, out, nullptr);
}
static int bwd(int64_t N, const float* w, int64_t ws, const float* v, int64_t vs, const float* pts, const float* g_out, float* g_w,
               int64_t gws, float* g_v, int64_t gvs, float* g_pts) {
  return fg_se3_apply_bwd(N, w, ws, v, vs, pts, g_out, g_w, gws, g_v, gvs, g_pts, nullptr);
}

int main() {
  EXPECT(fg_abi_version(), FG_ABI_VERSION);
  EXPECT(fg_abi_minor(), FG_ABI_MINOR);
  const int64_t N = 1000;  // 12 000 bytes a contiguous array, 52 000 a head block: far inside the 16 MiB between addresses
  // ---- row counts: negative is invalid whatever else holds, zero is nothing to do, beyond the maximum unsupported
  for (int64_t n : {INT64_MIN, (int64_t)INT32_MIN, (int64_t)-1}) {
    EXPECT(fwd(n, at(0), 3, at(1), 3, at(2), at(3)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(n, at(0), 3, at(1), 3, at(2), at(3), at(4), 3, at(5), 3, at(6)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(n, at(0), 3, at(1), 3, at(2), at(3), nullptr, 0, nullptr, 0, nullptr), FG_ERR_INVALID_ARG);
  }
  EXPECT(fwd(0, at(0), 3, at(1), 3, at(2), at(3)), FG_OK);
  EXPECT(fwd(0, at(0), 3, at(1), 3, at(2), at(2)), FG_OK);  // (no row: nothing overlaps)
  EXPECT(bwd(0, at(0), 3, at(1), 3, at(2), at(3), at(4), 3, at(5), 3, at(6)), FG_OK);
  EXPECT(fwd(0, nullptr, 3, at(1), 3, at(2), at(3)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(0, at(0), 2, at(1), 3, at(2), at(3)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(0, at(0), 3, at(1), 3, at(2), nullptr, at(4), 3, at(5), 3, at(6)), FG_ERR_INVALID_ARG);
  for (int64_t n : {(int64_t)FG_SE3_MAX_ROWS + 1, (int64_t)1 << 40, INT64_MAX}) {
    EXPECT(fwd(n, at(0), 3, at(1), 3, at(2), at(3)), FG_ERR_UNSUPPORTED);
    EXPECT(bwd(n, at(0), 3, at(1), 3, at(2), at(3), at(4), 3, at(5), 3, at(6)), FG_ERR_UNSUPPORTED);
  }
  // large and supported: the spans (2^38 rows x 13 floats) are computed without overflow and, 16 MiB apart, overlap
  EXPECT(fwd(FG_SE3_MAX_ROWS, at(7), 13, at(7) + 3, 13, at(2), at(3)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(FG_SE3_MAX_ROWS, at(7), 13, at(7) + 3, 13, at(2), at(3), at(4), 3, at(5), 3, at(6)), FG_ERR_INVALID_ARG);
  EXPECT(fwd((int64_t)1 << 31, at(0), 3, at(1), 3, at(2), at(3)), FG_ERR_INVALID_ARG);
  // one row: the smallest spans
  EXPECT(fwd(1, at(0), 3, at(1), 3, at(2), at(2)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(1, at(0), 3, at(1), 3, at(2), at(2) + 2), FG_ERR_INVALID_ARG);
  EXPECT(bwd(1, at(0), 3, at(1), 3, at(2), at(3), at(0) + 2, 3, nullptr, 0, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(bwd(1, at(0), 3, at(1), 3, at(2), at(3), nullptr, 0, nullptr, 0, nullptr), FG_OK);
  // ---- null pointers
  EXPECT(fwd(N, nullptr, 3, at(1), 3, at(2), at(3)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(N, at(0), 3, nullptr, 3, at(2), at(3)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(N, at(0), 3, at(1), 3, nullptr, at(3)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(N, at(0), 3, at(1), 3, at(2), nullptr), FG_ERR_INVALID_ARG);
  EXPECT(bwd(N, nullptr, 3, at(1), 3, at(2), at(3), at(4), 3, at(5), 3, at(6)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(N, at(0), 3, nullptr, 3, at(2), at(3), at(4), 3, at(5), 3, at(6)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(N, at(0), 3, at(1), 3, nullptr, at(3), at(4), 3, at(5), 3, at(6)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), nullptr, at(4), 3, at(5), 3, at(6)), FG_ERR_INVALID_ARG);
  // no gradient asked for: nothing to do (the strides of null outputs are not looked at)
  EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), nullptr, 0, nullptr, -7, nullptr), FG_OK);
  EXPECT(bwd(N, at(7), 13, at(7) + 3, 13, at(2), at(3), nullptr, 0, nullptr, 0, nullptr), FG_OK);
  // ---- strides: 2 is invalid, 3 and 13 pass (and then meet an overlap further down, so that nothing is launched)
  for (int64_t s : {INT64_MIN, (int64_t)-3, (int64_t)0, (int64_t)1, (int64_t)2}) {
    EXPECT(fwd(N, at(0), s, at(1), 3, at(2), at(3)), FG_ERR_INVALID_ARG);
    EXPECT(fwd(N, at(0), 3, at(1), s, at(2), at(3)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, at(0), s, at(1), 3, at(2), at(3), at(4), 3, at(5), 3, at(6)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, at(0), 3, at(1), s, at(2), at(3), at(4), 3, at(5), 3, at(6)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), s, at(5), 3, at(6)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 3, at(5), s, at(6)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), nullptr, s, nullptr, s, nullptr), FG_OK);
  }
  for (int64_t s : {(int64_t)FG_SE3_MAX_STRIDE + 1, INT64_MAX}) {
    EXPECT(fwd(N, at(0), s, at(1), 3, at(2), at(3)), FG_ERR_UNSUPPORTED);
    EXPECT(fwd(N, at(0), 3, at(1), s, at(2), at(3)), FG_ERR_UNSUPPORTED);
    EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), s, at(5), 3, at(6)), FG_ERR_UNSUPPORTED);
    EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), at(4), 3, at(5), s, at(6)), FG_ERR_UNSUPPORTED);
  }
  // ---- aliasing.  rows = the floats of a contiguous [N,3] array, block = those of w or v inside an [N,13] head block
  const size_t rows = (size_t)N * 3, block = (size_t)(N - 1) * 13 + 3;
  for (int64_t s : {(int64_t)3, (int64_t)13}) {
    const float* w = s == 3 ? at(0) : at(7);
    const float* v = s == 3 ? at(1) : at(7) + 3;
    const size_t in = s == 3 ? rows : block;
    // forward: out on w, v, pts -- whole, by out's last float, by the input's last float
    for (const float* victim : {w, v}) {
      EXPECT(fwd(N, w, s, v, s, at(2), const_cast<float*>(victim)), FG_ERR_INVALID_ARG);
      EXPECT(fwd(N, w, s, v, s, at(2), const_cast<float*>(victim) - (rows - 1)), FG_ERR_INVALID_ARG);
      EXPECT(fwd(N, w, s, v, s, at(2), const_cast<float*>(victim) + (in - 1)), FG_ERR_INVALID_ARG);
    }
    EXPECT(fwd(N, w, s, v, s, at(2), at(2)), FG_ERR_INVALID_ARG);
    EXPECT(fwd(N, w, s, v, s, at(2), at(2) - (rows - 1)), FG_ERR_INVALID_ARG);
    EXPECT(fwd(N, w, s, v, s, at(2), at(2) + (rows - 1)), FG_ERR_INVALID_ARG);
    // backward: each output on each input, whole and by the last float of either
    for (int o = 0; o < 3; ++o)
      for (int i = 0; i < 4; ++i) {
        const float* input = i == 0 ? w : i == 1 ? v : i == 2 ? at(2) : at(3);
        const size_t n_in = i < 2 ? in : rows;
        for (int how = 0; how < 3; ++how) {
          float* bad = const_cast<float*>(input) + (how == 0 ? 0 : how == 1 ? (ptrdiff_t)(n_in - 1) : -(ptrdiff_t)(rows - 1));
          EXPECT(bwd(N, w, s, v, s, at(2), at(3), o == 0 ? bad : at(4), 3, o == 1 ? bad : at(5), 3, o == 2 ? bad : at(6)), FG_ERR_INVALID_ARG);
          // alone as well: the other gradients not asked for
          EXPECT(bwd(N, w, s, v, s, at(2), at(3), o == 0 ? bad : nullptr, 3, o == 1 ? bad : nullptr, 3, o == 2 ? bad : nullptr), FG_ERR_INVALID_ARG);
        }
      }
    // outputs on each other
    EXPECT(bwd(N, w, s, v, s, at(2), at(3), at(4), 3, at(4), 3, at(6)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, w, s, v, s, at(2), at(3), at(4), 3, at(4) + (rows - 1), 3, at(6)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, w, s, v, s, at(2), at(3), at(4), 3, at(5), 3, at(4)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, w, s, v, s, at(2), at(3), at(4), 3, at(5), 3, at(5) + (rows - 1)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, w, s, v, s, at(2), at(3), at(4), 3, at(5), 3, at(4) - (rows - 1)), FG_ERR_INVALID_ARG);
  }
  // g_w and g_v as columns of one block: 3 floats apart at stride 6 and 13 is in order (and here runs into g_pts laid on the
  // block, so that nothing is launched); fewer than 3 apart, more than stride - 3 apart or unequal strides is not
  for (int64_t s : {(int64_t)6, (int64_t)13}) {
    float* blockp = at(4);
    const size_t n_block = (size_t)(N - 1) * s + 6;
    EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), blockp, s, blockp + 3, s, blockp + (n_block - 1)), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), blockp, s, blockp + 2, s, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), blockp, s, blockp + (s - 2), s, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), blockp, s, blockp + 3, s + 1, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), blockp + 3, s, blockp + 1, s, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(bwd(N, at(0), 3, at(1), 3, at(2), at(3), blockp, s, reinterpret_cast<float*>(reinterpret_cast<char*>(blockp) + 14), s, nullptr),
           FG_ERR_INVALID_ARG);
  }
  return report("se3_apply_args");
}
