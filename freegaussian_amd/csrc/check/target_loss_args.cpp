// Stand-alone host check of the fused training target's entry points -- fg_target_loss_supported,
// fg_target_loss_workspace_floats, fg_target_loss_fwd, fg_target_loss_bwd -- for a build of abi.hip and target_loss.hip whose
// HOST code carries AddressSanitizer + UndefinedBehaviorSanitizer (make target-loss-check).  Every call below returns before a
// launch: the program needs no GPU and touches none.
#include "check_common.h"

// addresses nobody reads, 16 GiB apart (a 32768 x 32768 image is 12 GiB): src, mask, background, pred, workspace, out, v_out,
// v_pred, and last -- nothing lies beyond them -- the maps (index 4)
static float* at(int i) { return reinterpret_cast<float*>((uintptr_t)4096 + ((uintptr_t)(i == 4 ? 9 : i) << 34)); }
static float* off(float* p, size_t bytes) { return reinterpret_cast<float*>(reinterpret_cast<char*>(p) + bytes); }

static fg_target_desc target(int H0, int W0, int channels, int d, int src_dtype = FG_TARGET_U8, bool mask = false,
                             int mask_dtype = FG_TARGET_U8) {
  fg_target_desc t;
  std::memset(&t, 0, sizeof t);
  t.size = (int32_t)sizeof t, t.src_dtype = src_dtype, t.height = H0, t.width = W0, t.channels = channels, t.downscale = d;
  t.mask_dtype = mask_dtype, t.src = at(0), t.mask = mask ? at(1) : nullptr, t.background = at(2);
  return t;
}

// a call whose buffers are all good but whose workspace is one float short: FG_ERR_WORKSPACE is the last check before the
// launch, so it stands for "everything else passed"
static int fwd_short(const fg_target_desc& t) {
  return fg_target_loss_fwd(&t, at(3), at(4), at(5), fg_target_loss_workspace_floats(&t) - 1, at(6), nullptr);
}
static int fwd(const fg_target_desc& t, float* pred, float* maps, float* ws, float* out) {
  return fg_target_loss_fwd(&t, pred, maps, ws, fg_target_loss_workspace_floats(&t) - 1, out, nullptr);
}
static int bwd(const fg_target_desc& t, float* pred = at(3), float* maps = at(4), float* v_out = at(7), float* v_pred = at(8)) {
  return fg_target_loss_bwd(&t, pred, maps, v_out, v_pred, nullptr);
}

int main() {
  EXPECT(fg_abi_version(), FG_ABI_VERSION);
  EXPECT(fg_abi_minor(), FG_ABI_MINOR);
  // the supported range and every value around it: downscale, channels, the two dtype words
  for (int d : {INT32_MIN, -1, 0, 1, 2, 3, 4, 5, 8, 16, INT32_MAX})
    for (int ch : {INT32_MIN, 0, 1, 2, 3, 4, 5, INT32_MAX})
      for (int dt : {-1, 0, 1, 2})
        for (int mdt : {-1, 0, 1, 2})
          for (int masked = 0; masked < 2; ++masked) {
            const fg_target_desc t = target(1080, 1920, ch, d, dt, masked, mdt);
            const bool ok = (d == 1 || d == 2 || d == 4 || d == 8) && (ch == 3 || ch == 4) && (dt == 0 || dt == 1) &&
                            (!masked || mdt == 0 || mdt == 1);
            EXPECT(fg_target_loss_supported(&t), ok);
            const long long H = ok ? 1080 / d : 0, W = ok ? 1920 / d : 0;
            EXPECT(fg_target_loss_workspace_floats(&t), 4 * ((W + 31) / 32) * ((H + 15) / 16) * 3);
            EXPECT(fwd_short(t), ok ? FG_ERR_WORKSPACE : FG_ERR_UNSUPPORTED);
            if (!ok) EXPECT(bwd(t), FG_ERR_UNSUPPORTED);
          }
  // source sizes: not positive is an invalid argument; beyond 32768, or an output below 11 x 11, unsupported
  for (int H0 : {INT32_MIN, -1, 0, 1, 10, 11, 21, 22, 43, 44, 87, 88, 1080, 32768, 32769, INT32_MAX})
    for (int W0 : {INT32_MIN, 0, 1, 10, 11, 22, 45, 88, 1920, 32768, 32769, INT32_MAX})
      for (int d : {1, 2, 4, 8}) {
        const fg_target_desc t = target(H0, W0, 4, d);
        const bool bad = H0 <= 0 || W0 <= 0, out = !bad && (H0 > 32768 || W0 > 32768 || H0 / d < 11 || W0 / d < 11);
        EXPECT(fg_target_loss_supported(&t), !bad && !out);
        const long long H = H0 / d, W = W0 / d;
        EXPECT(fg_target_loss_workspace_floats(&t), bad || out ? 0 : 4 * ((W + 31) / 32) * ((H + 15) / 16) * 3);
        EXPECT(fwd_short(t), bad ? FG_ERR_INVALID_ARG : out ? FG_ERR_UNSUPPORTED : FG_ERR_WORKSPACE);
        if (bad || out) EXPECT(bwd(t), bad ? FG_ERR_INVALID_ARG : FG_ERR_UNSUPPORTED);
      }
  // the descriptor itself
  EXPECT(fg_target_loss_supported(nullptr), 0);
  EXPECT(fg_target_loss_workspace_floats(nullptr), 0);
  EXPECT(fg_target_loss_fwd(nullptr, at(3), at(4), at(5), BIG, at(6), nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_target_loss_bwd(nullptr, at(3), at(4), at(7), at(8), nullptr), FG_ERR_INVALID_ARG);
  for (int size : {0, (int)sizeof(fg_target_desc) - 8, (int)sizeof(fg_target_desc) + 8}) {
    fg_target_desc t = target(107, 213, 4, 2);
    t.size = size;
    EXPECT(fg_target_loss_supported(&t), 0);
    EXPECT(fwd_short(t), FG_ERR_INVALID_ARG);
    EXPECT(bwd(t), FG_ERR_INVALID_ARG);
  }
  // one good shape: 107 x 213 RGBA uint8 with a float mask at d = 2 -> 53 x 106
  const int H0 = 107, W0 = 213, H = 53, W = 106;
  const size_t image = (size_t)H * W * 3 * 4, maps = (size_t)9 * (H - 10) * (W - 10) * 4, src = (size_t)H0 * W0 * 4, mask = (size_t)H0 * W0 * 4;
  const fg_target_desc good = target(H0, W0, 4, 2, FG_TARGET_U8, true, FG_TARGET_F32);
  const size_t need = fg_target_loss_workspace_floats(&good);
  EXPECT(need, 4 * 4 * 4 * 3);
  EXPECT(fwd_short(good), FG_ERR_WORKSPACE);
  for (size_t floats : {(size_t)0, (size_t)1, need - 1})
    EXPECT(fg_target_loss_fwd(&good, at(3), at(4), at(5), floats, at(6), nullptr), FG_ERR_WORKSPACE);
  // (a null maps is legal: the forward alone)
  EXPECT(fwd(good, at(3), nullptr, at(5), at(6)), FG_ERR_WORKSPACE);
  // null pointers
  {
    fg_target_desc t = good;
    t.src = nullptr;
    EXPECT(fwd_short(t), FG_ERR_INVALID_ARG);
    EXPECT(bwd(t), FG_ERR_INVALID_ARG);
    t = good, t.background = nullptr;  // four channels want a background
    EXPECT(fwd_short(t), FG_ERR_INVALID_ARG);
    EXPECT(bwd(t), FG_ERR_INVALID_ARG);
    t = target(H0, W0, 3, 2), t.background = nullptr;  // three do not
    EXPECT(fwd_short(t), FG_ERR_WORKSPACE);
  }
  EXPECT(fwd(good, nullptr, at(4), at(5), at(6)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), at(4), nullptr, at(6)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), at(4), at(5), nullptr), FG_ERR_INVALID_ARG);
  EXPECT(bwd(good, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(bwd(good, at(3), nullptr), FG_ERR_INVALID_ARG);
  EXPECT(bwd(good, at(3), at(4), nullptr), FG_ERR_INVALID_ARG);
  EXPECT(bwd(good, at(3), at(4), at(7), nullptr), FG_ERR_INVALID_ARG);
  // alignment: the source to its pixel, a float mask, the background, the workspace
  {
    fg_target_desc t = good;
    t.src = off(at(0), 1);
    EXPECT(fwd_short(t), FG_ERR_INVALID_ARG);
    t = target(H0, W0, 3, 2), t.src = off(at(0), 1);  // (3-channel uint8: any byte)
    EXPECT(fwd_short(t), FG_ERR_WORKSPACE);
    t = target(H0, W0, 4, 2, FG_TARGET_F32), t.src = off(at(0), 4);
    EXPECT(fwd_short(t), FG_ERR_INVALID_ARG);
    t = target(H0, W0, 3, 2, FG_TARGET_F32), t.src = off(at(0), 4);
    EXPECT(fwd_short(t), FG_ERR_WORKSPACE);
    t.src = off(at(0), 2);
    EXPECT(fwd_short(t), FG_ERR_INVALID_ARG);
    t = good, t.mask = off(at(1), 2);
    EXPECT(fwd_short(t), FG_ERR_INVALID_ARG);
    EXPECT(bwd(t), FG_ERR_INVALID_ARG);
    t = good, t.background = off(at(2), 1);
    EXPECT(fwd_short(t), FG_ERR_INVALID_ARG);
  }
  EXPECT(fwd(good, at(3), at(4), off(at(5), 4), at(6)), FG_ERR_INVALID_ARG);
  // aliasing, forward: each output against each input (whole and by the last byte), and against the other outputs
  EXPECT(fwd(good, at(3), at(3), at(5), at(6)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), off(at(3), image - 4), at(5), at(6)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, off(at(4), maps - 4), at(4), at(5), at(6)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), at(0), at(5), at(6)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), off(at(0), src - 4), at(5), at(6)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), off(at(0), src), at(5), at(6)), FG_ERR_WORKSPACE);  // (just past the source: apart)
  EXPECT(fwd(good, at(3), at(4), at(1), at(6)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), at(4), off(at(1), mask - 12), at(6)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), at(4), at(5), at(2)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), at(4), at(5), off(at(2), 8)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), at(4), at(4), at(6)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), at(4), at(5), at(5)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), at(4), at(5), off(at(5), need * 4 - 4)), FG_ERR_INVALID_ARG);
  EXPECT(fwd(good, at(3), at(4), at(5), off(at(4), maps - 4)), FG_ERR_INVALID_ARG);
  // aliasing, backward: v_pred against every input
  EXPECT(bwd(good, at(3), at(4), at(7), at(3)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(good, at(3), at(4), at(7), off(at(3), image - 4)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(good, at(3), at(4), at(7), at(4)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(good, at(3), at(4), at(7), at(7)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(good, at(3), at(4), off(at(8), image - 4), at(8)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(good, at(3), at(4), at(7), at(0)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(good, at(3), at(4), at(7), at(1)), FG_ERR_INVALID_ARG);
  EXPECT(bwd(good, at(3), at(4), at(7), at(2)), FG_ERR_INVALID_ARG);
  return report("target_loss_args");
}
