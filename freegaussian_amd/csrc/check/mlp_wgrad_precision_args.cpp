// Stand-alone host check of the three entry points of the weight-gradient precision word -- fg_mlp_wgrad_precision_supported,
// fg_mlp_param_grads_p, fg_mlp_train_bwd_p -- for a build of abi.hip, mlp.hip and mlp_wgrad.hip whose HOST code carries
// AddressSanitizer + UndefinedBehaviorSanitizer (make wgrad-precision-check).  Every call below returns before a launch: the
// program needs no GPU and touches none.
#include "check_common.h"

int main() {
  EXPECT(fg_abi_version(), FG_ABI_VERSION);
  EXPECT(fg_abi_minor(), FG_ABI_MINOR);
  const int32_t values[] = {0, 1, 7, -1, 2, INT32_MAX, INT32_MIN};
  const int supported[] = {1, 1, 0, 0, 0, 0, 0};
  for (int i = 0; i < 7; ++i) EXPECT(fg_mlp_wgrad_precision_supported(values[i]), supported[i]);

  fg_mlp_desc d = desc();
  fg_mlp_grads all = grads(true), none = grads(false);
  // an unknown value is refused before anything else about the call is looked at
  for (int32_t bad : {7, 2, -1, INT32_MAX, INT32_MIN}) {
    EXPECT(fg_mlp_param_grads_p(100, &d, PTR, PTR, PTR, PTR, &all, bad, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_param_grads_p(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, bad, nullptr, 0, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_train_bwd_p(100, &d, PTR, PTR, PTR, PTR, &all, 0, bad, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_train_bwd_p(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, bad, nullptr, 0, nullptr), FG_ERR_INVALID_ARG);
  }
  for (int32_t good : {FG_MLP_FP32, FG_MLP_BF16X3}) {
    // nothing to do: no rows, nothing asked for
    EXPECT(fg_mlp_param_grads_p(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, good, nullptr, 0, nullptr), FG_OK);
    EXPECT(fg_mlp_train_bwd_p(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, good, nullptr, 0, nullptr), FG_OK);
    EXPECT(fg_mlp_param_grads_p(100, &d, nullptr, nullptr, nullptr, nullptr, &none, good, nullptr, 0, nullptr), FG_OK);
    EXPECT(fg_mlp_train_bwd_p(100, &d, nullptr, nullptr, nullptr, nullptr, &none, 0, good, nullptr, 0, nullptr), FG_OK);
    // the old calls' refusals
    EXPECT(fg_mlp_param_grads_p(-1, &d, PTR, PTR, PTR, PTR, &all, good, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_param_grads_p(100, nullptr, PTR, PTR, PTR, PTR, &all, good, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_param_grads_p(100, &d, PTR, PTR, PTR, PTR, nullptr, good, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_param_grads_p(100, &d, nullptr, PTR, PTR, PTR, &all, good, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_param_grads_p(100, &d, PTR, PTR, PTR, PTR, &all, good, nullptr, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_param_grads_p(100, &d, PTR, PTR, PTR, PTR, &all, good, PTR + 1, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_train_bwd_p(-1, &d, PTR, PTR, PTR, PTR, &all, 0, good, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_train_bwd_p(100, nullptr, PTR, PTR, PTR, PTR, &all, 0, good, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_train_bwd_p(100, &d, PTR, PTR, PTR, PTR, &all, -1, good, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_train_bwd_p(100, &d, PTR, PTR, PTR, PTR, nullptr, 0, good, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_train_bwd_p(100, &d, nullptr, PTR, PTR, PTR, &all, 0, good, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_train_bwd_p(100, &d, PTR, PTR, PTR, PTR, &all, 0, good, nullptr, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_train_bwd_p(100, &d, PTR, PTR, PTR, PTR, &all, 0, good, PTR + 1, BIG, nullptr), FG_ERR_INVALID_ARG);
    // a workspace one byte short, at sizes around every change of the cut: the queries are the old calls'
    for (int64_t n : {(int64_t)1, (int64_t)100, (int64_t)513, (int64_t)5000, (int64_t)240000, (int64_t)1000000}) {
      EXPECT(fg_mlp_param_grads_p(n, &d, PTR, PTR, PTR, PTR, &all, good, PTR, fg_mlp_param_grads_workspace_bytes(n) - 1, nullptr), FG_ERR_WORKSPACE);
      for (int32_t c : {0, 1, 3, 1 << 30})
        for (int g_enc = 0; g_enc < 2; ++g_enc)
          EXPECT(fg_mlp_train_bwd_p(n, &d, PTR, PTR, PTR, g_enc ? PTR : nullptr, &all, c, good, PTR,
                                    fg_mlp_train_bwd_workspace_bytes(n, c, g_enc) - 1, nullptr),
                 FG_ERR_WORKSPACE);
    }
    // the two words are independent: the descriptor's governs the chain alone
    fg_mlp_desc s = desc(21, FG_MLP_BF16X3), b = desc(21, 7);
    EXPECT(fg_mlp_train_bwd_p(100, &s, PTR, PTR, PTR, PTR, &all, 0, good, PTR, 0, nullptr), FG_ERR_WORKSPACE);
    EXPECT(fg_mlp_train_bwd_p(100, &b, PTR, PTR, PTR, PTR, &all, 0, good, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    EXPECT(fg_mlp_param_grads_p(100, &b, PTR, PTR, PTR, PTR, &all, good, PTR, 0, nullptr), FG_ERR_WORKSPACE);
    b = desc();
    b.depth = 6;
    EXPECT(fg_mlp_param_grads_p(100, &b, PTR, PTR, PTR, PTR, &all, good, PTR, BIG, nullptr), FG_ERR_UNSUPPORTED);
    EXPECT(fg_mlp_train_bwd_p(100, &b, PTR, PTR, PTR, PTR, &all, 0, good, PTR, BIG, nullptr), FG_ERR_UNSUPPORTED);
  }
  return report("mlp_wgrad_precision_args");
}
