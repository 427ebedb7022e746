// What the MLP translation units share (not part of the C ABI, not exported): fg_mlp_train_bwd (mlp_wgrad.hip) runs the
// backward data chain of mlp.hip over one chunk of rows at a time, between the launches of fg_mlp_param_grads.
#pragma once
#include "fg_common.h"

namespace fg_mlp_detail {
#pragma GCC visibility push(hidden)

// The checks of fg_mlp_bwd / fg_mlp_bwd_inputs on the descriptor (its weight pointers included; x / aux / out are not
// looked at, the mode must be FG_MLP_PLAIN) and, where need > 0, on the workspace (present, need bytes, 16-byte aligned).
int bwd_check(int64_t N, const fg_mlp_desc* d, const void* workspace, size_t workspace_bytes, size_t need);

// The weight re-ordering launches of the chain into the front of the workspace: Tp, and behind it Tin where `inputs`
// (fg_mlp_train_workspace_bytes / fg_mlp_bwd_inputs_workspace_bytes bytes).
int bwd_launch_pack(const fg_mlp_desc* d, bool inputs, void* workspace, fg_stream_t stream);

// The chain over the rows [row_begin, row_end) of arrays of N rows (row_begin a multiple of FG_MLP_ROW_TILE, row_end <= N):
// g_heads, acts (N rows to a layer) and g_enc (null: not formed) at the rows themselves, g_pre at the row less row_begin,
// pre_rows rows to a layer.  `workspace` as bwd_launch_pack left it.
int bwd_launch_rows(int64_t N, const fg_mlp_desc* d, int64_t row_begin, int64_t row_end, const float* g_heads, const float* acts,
                    float* g_pre, int64_t pre_rows, float* g_enc, const void* workspace, fg_stream_t stream);

#pragma GCC visibility pop
}  // namespace fg_mlp_detail
