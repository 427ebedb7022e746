// Stand-alone host check of the bilateral-grid slice's entry points -- fg_bilagrid_supported, fg_bilagrid_bwd_workspace_bytes,
// fg_bilagrid_slice_fwd, fg_bilagrid_slice_bwd -- for a build of abi.hip and bilagrid.hip whose HOST code carries
// AddressSanitizer + UndefinedBehaviorSanitizer (make bilagrid-check).  Every call below returns before a launch: the program
// needs no GPU and touches none.
#include "check_common.h"

// addresses nobody reads, 16 MiB apart: grid, rgb, v_out / out, v_rgb, v_grid, workspace
static float* at(int i) { return reinterpret_cast<float*>((uintptr_t)4096 + ((uintptr_t)i << 24)); }

// the header's rule restated: cell c of an axis with n nodes and S pixels starts at ceil(c (S-1) / (n-1)); the last one ends at S
static long long longest(int S, int n) {
  long long m = 0;
  for (int c = 0; c < n - 1; ++c) {
    const long long a = ((long long)c * (S - 1) + n - 2) / (n - 1);
    const long long b = c == n - 2 ? S : ((long long)(c + 1) * (S - 1) + n - 2) / (n - 1);
    if (b - a > m) m = b - a;
  }
  return m;
}
static long long want_bytes(int H, int W, int GX, int GY, int GL) {
  const long long chunks = (longest(W, GX) * longest(H, GY) + FG_BILAGRID_CHUNK_PIXELS - 1) / FG_BILAGRID_CHUNK_PIXELS;
  return chunks * GL * 48 * (GX - 1) * (GY - 1) * 4;
}

int main() {
  EXPECT(fg_abi_version(), FG_ABI_VERSION);
  EXPECT(fg_abi_minor(), FG_ABI_MINOR);
  // the supported range, and every value around it
  for (int GX : {INT32_MIN, -1, 0, 1, 2, 3, 16, 63, 64, 65, 1 << 20, INT32_MAX})
    for (int GY : {INT32_MIN, 0, 1, 2, 16, 64, 65, INT32_MAX})
      for (int GL : {INT32_MIN, 0, 1, 2, 8, 16, 17, INT32_MAX}) {
        const int ok = GX >= 2 && GX <= 64 && GY >= 2 && GY <= 64 && GL >= 2 && GL <= 16;
        EXPECT(fg_bilagrid_supported(GX, GY, GL), ok);
        EXPECT(fg_bilagrid_bwd_workspace_bytes(270, 480, GX, GY, GL), ok ? want_bytes(270, 480, GX, GY, GL) : 0);
        if (!ok) {
          EXPECT(fg_bilagrid_slice_fwd(270, 480, GX, GY, GL, at(0), at(1), at(2), nullptr), FG_ERR_UNSUPPORTED);
          EXPECT(fg_bilagrid_slice_bwd(270, 480, GX, GY, GL, at(0), at(1), at(2), at(3), at(4), at(5), BIG, nullptr), FG_ERR_UNSUPPORTED);
        }
      }
  // image sizes: below 2 is an invalid argument, beyond 16384 unsupported; the query walks every cell of both axes
  for (int H : {INT32_MIN, -1, 0, 1, 2, 3, 12, 37, 1080, 16384, 16385, INT32_MAX})
    for (int W : {INT32_MIN, 0, 1, 2, 14, 53, 1920, 16384, 16385, INT32_MAX})
      for (int g = 0; g < 3; ++g) {
        const int GX = g == 0 ? 2 : g == 1 ? 16 : 64, GY = g == 0 ? 2 : g == 1 ? 16 : 64, GL = g == 0 ? 2 : g == 1 ? 8 : 16;
        const bool small = H < 2 || W < 2, large = H > 16384 || W > 16384;
        EXPECT(fg_bilagrid_bwd_workspace_bytes(H, W, GX, GY, GL), small || large ? 0 : want_bytes(H, W, GX, GY, GL));
        if (small) {
          EXPECT(fg_bilagrid_slice_fwd(H, W, GX, GY, GL, at(0), at(1), at(2), nullptr), FG_ERR_INVALID_ARG);
          EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), at(3), at(4), at(5), BIG, nullptr), FG_ERR_INVALID_ARG);
        } else if (large) {
          EXPECT(fg_bilagrid_slice_fwd(H, W, GX, GY, GL, at(0), at(1), at(2), nullptr), FG_ERR_UNSUPPORTED);
          EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), at(3), at(4), at(5), BIG, nullptr), FG_ERR_UNSUPPORTED);
        }
      }
  const int H = 37, W = 53, GX = 5, GY = 4, GL = 3;
  const size_t image = (size_t)H * W * 3, need = fg_bilagrid_bwd_workspace_bytes(H, W, GX, GY, GL);
  // forward: null buffers, aliasing (whole and by the last float)
  EXPECT(fg_bilagrid_slice_fwd(H, W, GX, GY, GL, nullptr, at(1), at(2), nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_fwd(H, W, GX, GY, GL, at(0), nullptr, at(2), nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_fwd(H, W, GX, GY, GL, at(0), at(1), nullptr, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_fwd(H, W, GX, GY, GL, at(0), at(1), at(1), nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_fwd(H, W, GX, GY, GL, at(0), at(1), at(1) + image - 1, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_fwd(H, W, GX, GY, GL, at(0), at(1) + image - 1, at(1), nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_fwd(H, W, GX, GY, GL, at(0), at(1), at(0), nullptr), FG_ERR_INVALID_ARG);
  // backward: null inputs, aliasing of either output, the workspace
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, nullptr, at(1), at(2), at(3), at(4), at(5), BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), nullptr, at(2), at(3), at(4), at(5), BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), nullptr, at(3), at(4), at(5), BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), at(1), at(4), at(5), BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), at(2) + image - 1, at(4), at(5), BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), at(3), at(0), at(5), BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), at(3), at(3), at(5), BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), at(3), at(4), nullptr, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), at(3), at(4), at(5) + 1, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), at(3), at(4), at(4), BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), at(3), at(4), at(1), BIG, nullptr), FG_ERR_INVALID_ARG);
  for (size_t bytes : {(size_t)0, (size_t)1, need - 1})
    EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), at(3), at(4), at(5), bytes, nullptr), FG_ERR_WORKSPACE);
  // without v_grid the workspace is not looked at; with neither output there is nothing to do
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), nullptr, at(4), at(5), need - 1, nullptr), FG_ERR_WORKSPACE);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), nullptr, nullptr, nullptr, 0, nullptr), FG_OK);
  EXPECT(fg_bilagrid_slice_bwd(H, W, GX, GY, GL, at(0), at(1), at(2), nullptr, nullptr, at(5) + 1, 0, nullptr), FG_OK);
  return report("bilagrid_args");
}
