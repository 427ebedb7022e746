// Stand-alone host check of fg_mlp_train_bwd's argument validation and of its two queries, for a build of abi.hip, mlp.hip
// and mlp_wgrad.hip whose HOST code carries AddressSanitizer + UndefinedBehaviorSanitizer (make train-bwd-check).  Every
// call below returns before a launch: the program needs no GPU and touches none.
#include "check_common.h"

int main() {
  EXPECT(fg_abi_version(), FG_ABI_VERSION);
  EXPECT(fg_abi_minor(), FG_ABI_MINOR);
  // the queries: sizes around every change of the cut, every kind of chunk_slabs, sizes beyond 2^31 rows
  const int64_t sizes[] = {-5, 0, 1, 63, 64, 65, 511, 512, 513, 5000, 33000, 131072, 131073, 240000, 1000000, (int64_t)1 << 33};
  const int32_t chunks[] = {-1, 0, 1, 3, 16, 1 << 30, INT32_MAX};
  for (int64_t n : sizes)
    for (int32_t c : chunks) {
      const int64_t rows = fg_mlp_train_bwd_chunk_rows(n, c);
      const int slab = fg_mlp_param_grads_slab_rows(n);
      if (n <= 0 || c < 0) {
        EXPECT(rows, 0);
        EXPECT(fg_mlp_train_bwd_workspace_bytes(n, c, 1), 0);
        continue;
      }
      const int64_t slabs = (n + slab - 1) / slab, want = (c == 0 ? FG_MLP_TRAIN_BWD_CHUNK_SLABS : c);
      EXPECT(rows, (want < slabs ? want : slabs) * slab);
      EXPECT(rows % FG_MLP_ROW_TILE, 0);
      for (int32_t g_enc = 0; g_enc < 2; ++g_enc)
        EXPECT(fg_mlp_train_bwd_workspace_bytes(n, c, g_enc),
               ((g_enc ? fg_mlp_bwd_inputs_workspace_bytes(n) : fg_mlp_train_workspace_bytes(n)) + FG_MLP_TRAIN_BWD_ALIGN - 1) /
                       FG_MLP_TRAIN_BWD_ALIGN * FG_MLP_TRAIN_BWD_ALIGN +
                   (size_t)8 * rows * 256 * 4 +
                   fg_mlp_param_grads_workspace_bytes(n));
    }

  // the call: every refusal, and the two ways of having nothing to do
  fg_mlp_desc d = desc();
  fg_mlp_grads all = grads(true), none = grads(false);
  EXPECT(fg_mlp_train_bwd(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 0, nullptr), FG_OK);
  EXPECT(fg_mlp_train_bwd(-1, &d, PTR, PTR, PTR, PTR, &all, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_mlp_train_bwd(100, nullptr, PTR, PTR, PTR, PTR, &all, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_mlp_train_bwd(100, &d, PTR, PTR, PTR, PTR, &all, -1, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_mlp_train_bwd(100, &d, PTR, PTR, PTR, PTR, nullptr, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_mlp_train_bwd(100, &d, nullptr, nullptr, nullptr, nullptr, &none, 0, nullptr, 0, nullptr), FG_OK);
  EXPECT(fg_mlp_train_bwd(100, &d, nullptr, PTR, PTR, PTR, &none, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_mlp_train_bwd(100, &d, PTR, PTR, nullptr, nullptr, &all, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_mlp_train_bwd(100, &d, PTR, nullptr, PTR, nullptr, &all, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_mlp_train_bwd(100, &d, PTR, PTR, PTR, PTR, &all, 0, nullptr, BIG, nullptr), FG_ERR_INVALID_ARG);
  EXPECT(fg_mlp_train_bwd(100, &d, PTR, PTR, PTR, PTR, &all, 0, PTR + 1, BIG, nullptr), FG_ERR_INVALID_ARG);
  for (int64_t n : {(int64_t)100, (int64_t)5000, (int64_t)240000})
    for (int32_t c : {0, 1, 3, 1 << 30})
      for (int g_enc = 0; g_enc < 2; ++g_enc)
        EXPECT(fg_mlp_train_bwd(n, &d, PTR, PTR, PTR, g_enc ? PTR : nullptr, &all, c, PTR, fg_mlp_train_bwd_workspace_bytes(n, c, g_enc) - 1,
                                nullptr),
               FG_ERR_WORKSPACE);
  {
    fg_mlp_desc b = desc();
    b.size -= 8;
    EXPECT(fg_mlp_train_bwd(100, &b, PTR, PTR, PTR, PTR, &all, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    b = desc();
    b.mode = FG_MLP_SE3;
    EXPECT(fg_mlp_train_bwd(100, &b, PTR, PTR, PTR, PTR, &all, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    for (int aux : {0, 65}) {
      b = desc(aux);
      EXPECT(fg_mlp_train_bwd(100, &b, PTR, PTR, PTR, PTR, &all, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    }
    b = desc();
    b.head_rows[1] = 17;
    EXPECT(fg_mlp_train_bwd(100, &b, PTR, PTR, PTR, PTR, &all, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    b = desc();
    b.n_heads = FG_MLP_MAX_HEADS + 1;
    EXPECT(fg_mlp_train_bwd(100, &b, PTR, PTR, PTR, PTR, &all, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    b = desc();
    b.weight[6] = nullptr;
    EXPECT(fg_mlp_train_bwd(100, &b, PTR, PTR, PTR, PTR, &all, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
    b = desc();
    b.depth = 6;
    EXPECT(fg_mlp_train_bwd(100, &b, PTR, PTR, PTR, PTR, &all, 0, PTR, BIG, nullptr), FG_ERR_UNSUPPORTED);
    fg_mlp_grads g = grads(true);
    g.size -= 8;
    EXPECT(fg_mlp_train_bwd(100, &d, PTR, PTR, PTR, PTR, &g, 0, PTR, BIG, nullptr), FG_ERR_INVALID_ARG);
  }
  return report("mlp_train_bwd_args");
}
