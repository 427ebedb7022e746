// Stand-alone host check of the optical flow's entry points -- fg_optflow_supported, fg_optflow_workspace_bytes,
// fg_optflow_pyramid, fg_optflow -- for a build of abi.hip and optflow.hip whose HOST code carries AddressSanitizer +
// UndefinedBehaviorSanitizer (make optflow-check).  Every call below returns before a launch: the program needs no GPU and
// touches none.
#include <cmath>

#include "check_common.h"

// addresses nobody reads, 4 GiB apart from 1 TiB on: a 0, b 1, init 2, flow 3, valid 4, workspace 5
static char* at(int i) { return reinterpret_cast<char*>(((uintptr_t)1 << 40) + ((uintptr_t)i << 32)); }

struct Args {
  int H = 97, W = 131, channels = 3, dtype = FG_TARGET_F32, levels = 4, iters = 4, radius = 3, both = 1;
  float min_eig = 1e-5f, consistency = 1.f;
  size_t bytes = BIG;
  const void* a = at(0);
  const void* b = at(1);
  const float* init = nullptr;
  float* flow = reinterpret_cast<float*>(at(3));
  uint8_t* valid = reinterpret_cast<uint8_t*>(at(4));
  void* ws = at(5);
};

static int run(const Args& g) {
  return fg_optflow(g.H, g.W, g.channels, g.dtype, g.a, g.b, g.levels, g.iters, g.radius, g.min_eig, g.both, g.consistency, g.init, g.flow,
                    g.valid, g.ws, g.bytes, nullptr);
}
static int pyr(const Args& g) { return fg_optflow_pyramid(g.H, g.W, g.channels, g.dtype, g.a, g.levels, g.ws, g.bytes, nullptr); }

static size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// the layout of optflow.hip, restated: two pyramids, the eigenvalue map, u of the levels below 0 (a -> b), u of all levels (b -> a)
static size_t formula(int H, int W, int levels, int both, size_t* pyramid = nullptr) {
  size_t pyr = 0, u = 0;
  int h = H, w = W;
  for (int l = 0; l < levels; ++l) {
    pyr += align256((size_t)h * w * 4);
    const size_t ul = align256((size_t)h * w * 8);
    u += (l ? ul : 0) + (both ? ul : 0);
    h = (h + 1) / 2, w = (w + 1) / 2;
  }
  if (pyramid) *pyramid = pyr;
  return 2 * pyr + align256((size_t)H * W * 4) + u;
}

int main() {
  EXPECT(fg_abi_version(), FG_ABI_VERSION);
  EXPECT(fg_abi_minor(), FG_ABI_MINOR);
  const float inf = INFINITY, nan = NAN;
  // ---- the two queries: the ranges, one step beyond each, and the layout inside
  EXPECT(fg_optflow_supported(16, 16, 1, 1, 1), 1);
  EXPECT(fg_optflow_supported(16, 16, 2, 3, 4), 1);  // an 8-pixel coarsest side
  EXPECT(fg_optflow_supported(16, 16, 3, 3, 4), 0);  // 4
  EXPECT(fg_optflow_supported(15, 16, 1, 3, 4), 0);
  EXPECT(fg_optflow_supported(16, 15, 1, 3, 4), 0);
  EXPECT(fg_optflow_supported(16384, 16384, 8, 7, 16), 1);
  EXPECT(fg_optflow_supported(16385, 16384, 8, 7, 16), 0);
  EXPECT(fg_optflow_supported(16384, 16385, 8, 7, 16), 0);
  EXPECT(fg_optflow_supported(16384, 16384, 9, 7, 16), 0);
  EXPECT(fg_optflow_supported(16384, 16384, 8, 8, 16), 0);
  EXPECT(fg_optflow_supported(16384, 16384, 8, 7, 17), 0);
  EXPECT(fg_optflow_supported(1080, 1920, 0, 3, 4), 0);
  EXPECT(fg_optflow_supported(1080, 1920, 6, 0, 4), 0);
  EXPECT(fg_optflow_supported(1080, 1920, 6, 3, 0), 0);
  EXPECT(fg_optflow_supported(1080, 1920, 8, 3, 4), 1);  // 1080 -> 9 on the shorter side
  EXPECT(fg_optflow_supported(1000, 1920, 8, 3, 4), 1);  // 1000 -> 8
  EXPECT(fg_optflow_supported(896, 1920, 8, 3, 4), 0);   // 896 -> 7
  for (int v : {INT32_MIN, -1, 0, INT32_MAX}) {
    EXPECT(fg_optflow_supported(v, 128, 1, 3, 4), 0);
    EXPECT(fg_optflow_supported(128, v, 1, 3, 4), 0);
    EXPECT(fg_optflow_supported(128, 128, v, 3, 4), 0);
    EXPECT(fg_optflow_supported(128, 128, 1, v, 4), 0);
    EXPECT(fg_optflow_supported(128, 128, 1, 3, v), 0);
    EXPECT(fg_optflow_workspace_bytes(v, 128, 1, 1), 0);
    EXPECT(fg_optflow_workspace_bytes(128, v, 1, 1), 0);
    EXPECT(fg_optflow_workspace_bytes(128, 128, v, 1), 0);
  }
  for (int both : {0, 1}) {
    const int shapes[][3] = {{16, 16, 1}, {16, 16, 2}, {97, 131, 4}, {128, 160, 4}, {270, 480, 5}, {540, 960, 6}, {1080, 1920, 6},
                             {16384, 16384, 8}};
    for (const auto& s : shapes) {
      const size_t need = fg_optflow_workspace_bytes(s[0], s[1], s[2], both);
      EXPECT(need, formula(s[0], s[1], s[2], both));
      EXPECT(need % 256, 0);
    }
    EXPECT(fg_optflow_workspace_bytes(15, 16, 1, both), 0);
    EXPECT(fg_optflow_workspace_bytes(16, 16, 3, both), 0);
    EXPECT(fg_optflow_workspace_bytes(16385, 16, 1, both), 0);
    EXPECT(fg_optflow_workspace_bytes(128, 128, 9, both), 0);
  }
  Args ok;
  size_t pyramid = 0;
  const size_t need = formula(ok.H, ok.W, ok.levels, 1, &pyramid), need_one = formula(ok.H, ok.W, ok.levels, 0);
  // ---- everything in order but the workspace's size keeps the call on the host
  for (size_t bytes : {(size_t)0, need - 1}) {
    Args g;
    g.bytes = bytes;
    EXPECT(run(g), FG_ERR_WORKSPACE);
  }
  {
    Args g;
    g.both = 0, g.bytes = need_one - 1;
    EXPECT(run(g), FG_ERR_WORKSPACE);
    g.both = 1, g.bytes = need_one;  // the one-direction size does not do for both
    EXPECT(run(g), FG_ERR_WORKSPACE);
    g.bytes = pyramid - 1;
    EXPECT(pyr(g), FG_ERR_WORKSPACE);
    g.init = reinterpret_cast<const float*>(at(2)), g.bytes = 0;
    EXPECT(run(g), FG_ERR_WORKSPACE);
    g.dtype = FG_TARGET_U8;
    EXPECT(run(g), FG_ERR_WORKSPACE);
    EXPECT(pyr(g), FG_ERR_WORKSPACE);
    g.dtype = FG_TARGET_F32, g.channels = 1;
    EXPECT(run(g), FG_ERR_WORKSPACE);
    g.H = g.W = 16, g.levels = 2, g.radius = 7, g.iters = 16;
    EXPECT(run(g), FG_ERR_WORKSPACE);
    g.H = g.W = 16384, g.levels = 8;
    EXPECT(run(g), FG_ERR_WORKSPACE);
  }
  // ---- the ranges: one step beyond each is refused, by both calls where both take the argument
#define BOTH_REFUSE(code) \
  do {                    \
    EXPECT(run(g), code); \
    EXPECT(pyr(g), code); \
  } while (0)
  for (int v : {15, 16385, INT32_MAX}) {
    Args g;
    g.H = v;
    BOTH_REFUSE(FG_ERR_UNSUPPORTED);
    g = Args(), g.W = v;
    BOTH_REFUSE(FG_ERR_UNSUPPORTED);
  }
  for (int v : {INT32_MIN, -1, 0}) {
    Args g;
    g.H = v;
    BOTH_REFUSE(FG_ERR_INVALID_ARG);
    g = Args(), g.W = v;
    BOTH_REFUSE(FG_ERR_INVALID_ARG);
    g = Args(), g.levels = v;
    BOTH_REFUSE(FG_ERR_INVALID_ARG);
    g = Args(), g.radius = v;
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.iters = v;
    EXPECT(run(g), FG_ERR_INVALID_ARG);
  }
  {
    Args g;
    g.levels = 9;
    BOTH_REFUSE(FG_ERR_UNSUPPORTED);
    g.levels = 5;  // 97 -> 49 -> 25 -> 13 -> 7
    BOTH_REFUSE(FG_ERR_UNSUPPORTED);
    g = Args(), g.radius = 8;
    EXPECT(run(g), FG_ERR_UNSUPPORTED);
    g = Args(), g.iters = 17;
    EXPECT(run(g), FG_ERR_UNSUPPORTED);
    g = Args(), g.radius = INT32_MAX;
    EXPECT(run(g), FG_ERR_UNSUPPORTED);
    g = Args(), g.iters = INT32_MAX;
    EXPECT(run(g), FG_ERR_UNSUPPORTED);
  }
  // ---- the images: channels, dtype
  for (int c : {INT32_MIN, -1, 0, 2, 4, INT32_MAX}) {
    Args g;
    g.channels = c;
    BOTH_REFUSE(FG_ERR_INVALID_ARG);
  }
  for (int d : {INT32_MIN, -1, 2, INT32_MAX}) {
    Args g;
    g.dtype = d;
    BOTH_REFUSE(FG_ERR_INVALID_ARG);
  }
  {
    Args g;
    g.channels = 1, g.dtype = FG_TARGET_U8;
    BOTH_REFUSE(FG_ERR_UNSUPPORTED);
  }
  // ---- the thresholds and the direction word
  for (float bad : {-1e-30f, -1.f, -inf, inf, nan}) {
    Args g;
    g.min_eig = bad;
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.consistency = bad;
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g.both = 0, g.bytes = 0;  // not looked at without the second direction
    EXPECT(run(g), FG_ERR_WORKSPACE);
  }
  for (int v : {INT32_MIN, -1, 2, INT32_MAX}) {
    Args g;
    g.both = v;
    EXPECT(run(g), FG_ERR_INVALID_ARG);
  }
  // ---- null pointers (init may be null), misaligned ones
  {
    Args g;
    g.a = nullptr;
    BOTH_REFUSE(FG_ERR_INVALID_ARG);
    g = Args(), g.b = nullptr;
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.flow = nullptr;
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.valid = nullptr;
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.ws = nullptr;
    BOTH_REFUSE(FG_ERR_INVALID_ARG);
    g = Args(), g.a = at(0) + 2;
    BOTH_REFUSE(FG_ERR_INVALID_ARG);
    g = Args(), g.b = at(1) + 1;
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.flow = reinterpret_cast<float*>(at(3) + 4);
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.init = reinterpret_cast<const float*>(at(2) + 4);
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.ws = at(5) + 128;
    BOTH_REFUSE(FG_ERR_INVALID_ARG);
    // a uint8 image may lie at any byte
    g = Args(), g.dtype = FG_TARGET_U8, g.a = at(0) + 1, g.b = at(1) + 3, g.bytes = 0;
    EXPECT(run(g), FG_ERR_WORKSPACE);
    EXPECT(pyr(g), FG_ERR_WORKSPACE);
  }
  // ---- the aliasing rule: no output or workspace over an input or another output
  {
    const size_t img = (size_t)97 * 131 * 3 * 4, uv = (size_t)97 * 131 * 8;
    Args g;
    g.flow = reinterpret_cast<float*>(at(0) + img - 4);  // the last float of a (img is 4 short of a multiple of 8)
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g.flow = reinterpret_cast<float*>(at(0) + img + 4);  // the first aligned address behind it
    g.bytes = 0;
    EXPECT(run(g), FG_ERR_WORKSPACE);
    g = Args(), g.valid = reinterpret_cast<uint8_t*>(at(1));
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.valid = reinterpret_cast<uint8_t*>(at(3) + uv - 1);  // over the flow's last byte
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.init = g.flow;  // in place
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.ws = at(1);
    EXPECT(run(g), FG_ERR_INVALID_ARG);
    g = Args(), g.ws = at(0), g.b = at(0);  // a == b is allowed (two inputs), the workspace over them is not
    BOTH_REFUSE(FG_ERR_INVALID_ARG);
    g = Args(), g.b = g.a, g.bytes = 0;
    EXPECT(run(g), FG_ERR_WORKSPACE);
    g = Args(), g.ws = at(3) + 256;  // over the flow
    EXPECT(run(g), FG_ERR_INVALID_ARG);
  }
  return report("optflow_args");
}
