"""ctypes binding of ``libfgraster.so`` (the C ABI declared in ``include/fgraster.h``).

There is NO fallback: if the HIP library is missing or a symbol is absent, importing the ops
raises.  PyTorch is only used by callers for device memory and streams; nothing here takes a
torch type -- pointers are plain integers."""
from __future__ import annotations

import ctypes
import os
from ctypes import c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_size_t, c_void_p

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libfgraster.so")

P = c_void_p

# name -> (restype, argtypes); must list every symbol of include/fgraster.h
SIGNATURES = {
    "fg_abi_version": (c_int, []),
    "fg_abi_minor": (c_int, []),
    "fg_error_string": (c_char_p, [c_int]),
    "fg_project_fwd": (c_int, [c_int, P, P, P, P, P, c_int, c_int, c_float, c_float, c_float, c_float, c_int,
                               P, P, P, P, P, P, P]),
    "fg_project_bwd": (c_int, [c_int, P, P, P, P, P, c_int, c_int, c_float, P, P, P, P, P, P, P, P, P, P, P]),
    "fg_sh_fwd": (c_int, [c_int, c_int, c_int, P, P, P, P, P, P]),
    "fg_sh_bwd": (c_int, [c_int, c_int, c_int, P, P, P, P, P, P, P, P, P]),
    "fg_scan_workspace_bytes": (c_size_t, [c_int]),
    "fg_scan_tiles": (c_int, [c_int, P, P, P, c_size_t, P]),
    "fg_tile_bin": (c_int, [c_int, P, P, P, P, c_int, c_int, c_int, P, P, P]),
    "fg_sort_workspace_bytes": (c_size_t, [c_int64]),
    "fg_sort_pairs": (c_int, [c_int64, P, P, c_int, P, c_size_t, P]),
    "fg_tile_ranges": (c_int, [c_int64, P, c_int, P, P]),
    "fg_sort32_workspace_bytes": (c_size_t, [c_int64]),
    "fg_sort_pairs32": (c_int, [c_int64, P, P, c_int, P, c_size_t, P]),
    "fg_bin_prepare_workspace_bytes": (c_size_t, [c_int]),
    "fg_bin_prepare": (c_int, [c_int, P, P, P, P, P, P, c_size_t, P]),
    "fg_bin_prepare_rects": (c_int, [c_int, P, P, P, c_int, c_int, c_int, P, P, P, P, c_size_t, P]),
    "fg_bin_prepare_keys": (c_int, [c_int, P, P, P, P, P, P, P, c_size_t, P]),
    "fg_bin_emit_workspace_bytes": (c_size_t, [c_int64]),
    "fg_bin_emit_sort": (c_int, [c_int, c_int64, P, P, P, P, P, c_int, c_int, c_int, P, P, P, P, c_size_t, P]),
    "fg_bin_emit_sort_capacity": (c_int, [c_int, c_int64, P, P, P, P, P, c_int, c_int, c_int, P, P, P, P, c_size_t,
                                          P]),
    "fg_stbin_supported": (c_int, [c_int, c_int, c_int]),
    "fg_stbin_count_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "fg_stbin_count": (c_int, [c_int, P, P, c_int, c_int, P, P, P, c_size_t, P]),
    "fg_stbin_fill_workspace_bytes": (c_size_t, [c_int64]),
    "fg_stbin_fill": (c_int, [c_int, P, P, P, c_int, c_int, c_int64, P, P, P, P, P, c_size_t, c_int, P]),
    "fg_stbin_fill_jobs": (c_int, [c_int, P, P, P, c_int, c_int, c_int64, P, P, P, P, P, c_size_t, c_int, c_int, c_int, P, P,
                                   c_int, P, c_int, P, P]),
    "fg_isect_keys": (c_int, [c_int64, P, P, P, P, P]),
    "fg_densify_stats": (c_int, [c_int, P, P, c_float, P, P, P, P]),
    "fg_adam_step_multi": (c_int, [c_int, P, P]),  # (count, fg_adam_tensor[count], stream)
    "fg_adam_step": (c_int, [c_int64, P, P, P, P, c_double, c_double, c_double, c_double, c_int64, P]),
    "fg_l1_ssim_workspace_floats": (c_size_t, [c_int, c_int, c_int]),
    "fg_l1_ssim_fwd": (c_int, [c_int, c_int, c_int, P, P, P, P, c_size_t, P, P]),
    "fg_l1_ssim_bwd": (c_int, [c_int, c_int, c_int, P, P, P, P, P, P]),
    "fg_pack_splats": (c_int, [c_int, c_int, P, P, P, P, P, P]),
    # (the pointer before the stream of every raster entry point is the `const fg_raster_config*`)
    "fg_raster_config_init": (None, [P]),
    "fg_raster_fwd": (c_int, [c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, P]),
    "fg_raster_bwd": (c_int, [c_int, c_int, c_int, c_int, P, P, P, P, P, P, P, P, P, P]),
    "fg_raster_composite_fwd": (c_int, [c_int, c_int, c_int, c_int, P, P, P, P, c_int, P, P, P, P, P, P]),
    "fg_raster_composite_bwd": (c_int, [c_int, c_int, c_int, c_int, P, P, P, P, c_int, P, P, P, P, P, P, P, P]),
    "fg_raster_jobs_words": (c_int64, [c_int, c_int, c_int, P]),
    "fg_raster_build_jobs": (c_int, [c_int, c_int, c_int, P, P, P, c_int, P, P]),
    "fg_raster_jobs_fwd": (c_int, [c_int, c_int, c_int, c_int, P, P, P, P, P, c_int, P, P, P, P, P, P, P, c_int64, P, P, P]),
    "fg_raster_seg_ckpt_floats": (c_int64, [c_int, c_int, c_int, c_int, c_int64, P]),
    "fg_raster_jobs_bwd": (c_int, [c_int, c_int, c_int, c_int, P, P, P, P, P, c_int, P, P, P, P, P, P, P, P, P, P, P]),
    "fg_unpack_grads": (c_int, [c_int, c_int, P, P, P, P, P, P, P]),
    "fg_preprocess_fwd": (c_int, [c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, P, c_int, P, P, c_int, c_int,
                                  c_float, c_float, c_float, c_float, c_int, c_int, P, P, P, P, P, P, P, P, P, P, P, P]),
    "fg_viewmat_bwd_workspace_bytes": (c_size_t, [c_int]),
    "fg_viewmat_bwd": (c_int, [c_int, c_int, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, c_int,
                               c_float, c_int, P, P, P, c_int, P, P, P, P, P, c_size_t, P]),
    "fg_sh_pack_fwd": (c_int, [c_int, P, P, P, c_int, c_int, c_int, c_int, P, c_int, P, c_int, P, P, P, P, P, P, P]),
    "fg_preprocess_bwd": (c_int, [c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, c_int, P, P, c_int, c_int,
                                  c_float, c_int, P, P, P, c_int, P, P, P, P, P, P, P, P, P, P]),
    "fg_preprocess_raw_fwd": (c_int, [c_int, P, P, P, P, P, P, P, P, c_int, c_int, c_int, P, c_int, P, P, c_int,
                                      c_int, c_float, c_float, c_float, c_float, c_int, c_int, P, P, P, P, P, P, P,
                                      P, P, P, P, P]),
    "fg_preprocess_raw_bwd": (c_int, [c_int, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, c_int, c_int,
                                      c_float, c_int, P, P, P, c_int, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "fg_preprocess_bwd_factored": (c_int, [c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, c_int, c_int,
                                           c_float, c_int, P, P, P, c_int, P, P, P, P, P, P, P, c_int, P, P, P]),
    "fg_sh_grad_accumulate": (c_int, [c_int, c_int, c_int, c_int, P, P, c_int64, c_int, c_float, P, P]),
    "fg_payload_compact": (c_int, [c_int, c_int, P, P, c_int64, P, P]),
    "fg_payload_expand": (c_int, [c_int, c_int, c_int, P, c_int64, c_int64, P, c_int64, P]),
    "fg_step_layout_query": (c_int, [P, P, P]),
    "fg_step_fwd": (c_int, [P, P, P, P, P, P, P]),
    "fg_step_bwd": (c_int, [P, P, P, P, P, P]),
    "fg_sh_grad_accumulate_split": (c_int, [c_int, c_int, c_int, c_int, P, P, c_int64, c_int, c_float, P, P, P]),
    "fg_preprocess_raw_bwd_factored": (c_int, [c_int, P, P, P, P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, c_int, c_int,
                                               c_float, c_int, P, P, P, c_int, P, P, P, P, P, P, P, P, P, c_int, P, P, P]),
    "fg_densify_flags": (c_int, [c_int, c_int, c_float, c_float, c_float, c_float, c_float, c_float, c_float, P, P, P,
                                 P, P, P, P]),
    "fg_densify_map": (c_int, [c_int, P, P, P, P, P, c_int, c_int, c_int, c_int, P, P, P]),
    "fg_gather_rows": (c_int, [c_int64, c_int, P, P, c_int64, P, P]),
    "fg_split_children": (c_int, [c_int, c_int, P, P, P, P, P, P]),
    "fg_mask_backproject": (c_int, [c_int, P, P, P, P, c_int, c_int, P, P, c_int, c_int, P, P]),
    "fg_camera_flow": (c_int, [c_int, c_int, P, P, P, P, P, P]),
    "fg_reprojection_flow": (c_int, [c_int, c_int, P, P, P, P, c_float, P, P]),
    "fg_flow_fwd": (c_int, [c_int, P, P, P, P, P, P, P, P, P, P]),
    "fg_flow_bwd": (c_int, [c_int, P, P, P, P, P, P, P, P, P, P, P, P, P]),
    "fg_knn_workspace_bytes": (c_size_t, [c_int64]),
    "fg_knn": (c_int, [c_int64, P, c_int, P, P, P, c_size_t, P]),
    "fg_mlp_precision_supported": (c_int, [c_int32]),  # (FG_MLP_FP32 / FG_MLP_BF16X3 / ...) -> 1 or 0
    "fg_mlp_workspace_bytes": (c_size_t, [c_int64]),
    "fg_mlp_fwd": (c_int, [c_int64, P, P, c_size_t, P]),  # (N, const fg_mlp_desc*, workspace, bytes, stream)
    "fg_mlp_train_workspace_bytes": (c_size_t, [c_int64]),
    "fg_mlp_train_fwd": (c_int, [c_int64, P, P, P, P, P, c_size_t, P]),  # (N, desc, heads, enc, acts, workspace, bytes, stream)
    "fg_mlp_bwd": (c_int, [c_int64, P, P, P, P, P, c_size_t, P]),  # (N, desc, g_heads, acts, g_pre, workspace, bytes, stream)
    "fg_mlp_bwd_inputs_workspace_bytes": (c_size_t, [c_int64]),
    # (N, desc, g_heads, acts, g_pre, g_enc, workspace, bytes, stream)
    "fg_mlp_bwd_inputs": (c_int, [c_int64, P, P, P, P, P, P, c_size_t, P]),
    "fg_mlp_param_grads_workspace_bytes": (c_size_t, [c_int64]),
    "fg_mlp_param_grads_slab_rows": (c_int, [c_int64]),
    # (N, desc, enc, acts, g_pre, g_heads, const fg_mlp_grads*, workspace, bytes, stream)
    "fg_mlp_param_grads": (c_int, [c_int64, P, P, P, P, P, P, P, c_size_t, P]),
    "fg_mlp_train_bwd_chunk_rows": (c_int64, [c_int64, c_int32]),  # (N, chunk_slabs)
    "fg_mlp_train_bwd_workspace_bytes": (c_size_t, [c_int64, c_int32, c_int32]),  # (N, chunk_slabs, want_g_enc)
    # (N, desc, g_heads, enc, acts, g_enc, const fg_mlp_grads*, chunk_slabs, workspace, bytes, stream)
    "fg_mlp_train_bwd": (c_int, [c_int64, P, P, P, P, P, P, c_int32, P, c_size_t, P]),
    # the two calls above with a precision word for the weight-gradient products (FG_MLP_FP32 / FG_MLP_BF16X3)
    "fg_mlp_wgrad_precision_supported": (c_int, [c_int32]),
    # (N, desc, enc, acts, g_pre, g_heads, const fg_mlp_grads*, wgrad_precision, workspace, bytes, stream)
    "fg_mlp_param_grads_p": (c_int, [c_int64, P, P, P, P, P, P, c_int32, P, c_size_t, P]),
    # (N, desc, g_heads, enc, acts, g_enc, const fg_mlp_grads*, chunk_slabs, wgrad_precision, workspace, bytes, stream)
    "fg_mlp_train_bwd_p": (c_int, [c_int64, P, P, P, P, P, P, c_int32, c_int32, P, c_size_t, P]),
    # bilateral-grid slice of one camera's grid [12,GL,GY,GX] over an [H,W,3] image (csrc/bilagrid.hip)
    "fg_bilagrid_supported": (c_int, [c_int, c_int, c_int]),  # (GX, GY, GL) -> 1 or 0
    "fg_bilagrid_bwd_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int]),  # (H, W, GX, GY, GL)
    "fg_bilagrid_slice_fwd": (c_int, [c_int, c_int, c_int, c_int, c_int, P, P, P, P]),  # (H, W, GX, GY, GL, grid, rgb, out, stream)
    # (H, W, GX, GY, GL, grid, rgb, v_out, v_rgb, v_grid, workspace, bytes, stream)
    "fg_bilagrid_slice_bwd": (c_int, [c_int, c_int, c_int, c_int, c_int, P, P, P, P, P, P, c_size_t, P]),
    # the iterated colour-correction fit of the metrics, on the device (csrc/color_correct.hip)
    "fg_color_correct_workspace_bytes": (c_size_t, [c_int64, c_int]),  # (P, num_iters)
    # (P, img, ref, num_iters, eps, out, warps, rank, workspace, bytes, stream)
    "fg_color_correct": (c_int, [c_int64, P, P, c_int, c_double, P, P, P, P, c_size_t, P]),
    # the SE(3) exponential of the (w, v) heads applied to points (csrc/se3_apply.hip); strides in floats
    "fg_se3_apply_fwd": (c_int, [c_int64, P, c_int64, P, c_int64, P, P, P]),  # (N, w, w_stride, v, v_stride, pts, out, stream)
    # (N, w, w_stride, v, v_stride, pts, g_out, g_w, gw_stride, g_v, gv_stride, g_pts, stream)
    "fg_se3_apply_bwd": (c_int, [c_int64, P, c_int64, P, c_int64, P, P, P, c_int64, P, c_int64, P, P]),
    # the stage-2 control stage on a plan of the mask (csrc/control.hip); strides in floats
    "fg_control_supported": (c_int, [c_int]),  # (M) -> 1 or 0
    "fg_control_workspace_bytes": (c_size_t, [c_int64, c_int]),  # (n, M)
    # (n, M, a, a_stride, b, b_stride, bits, counts (HOST int32[M]), workspace, bytes, d_avg, stream)
    "fg_control_attr_mean": (c_int, [c_int64, c_int, P, c_int64, P, c_int64, P, P, P, c_size_t, P, P]),
    "fg_control_value_rows": (c_int, [c_int64, c_int, P, P, P, P]),  # (n, M, bits, d_avg, value, stream)
    # (N, n, rank, means, d_xyz, xyz_stride, d_rot, rot_stride, d_scale, scale_stride, out_means, d_rotation, d_scaling, stream)
    "fg_control_scatter_fwd": (c_int, [c_int64, c_int64, P, P, P, c_int64, P, c_int64, P, c_int64, P, P, P, P]),
    # (n, N, sel_index, g_means, g_rotation, g_scaling, g_d_xyz, xyz_stride, g_d_rot, rot_stride, g_d_scale, scale_stride, stream)
    "fg_control_scatter_bwd": (c_int, [c_int64, c_int64, P, P, P, P, P, c_int64, P, c_int64, P, c_int64, P]),
    # loss and squared error straight from the raw batch image (csrc/target_loss.hip); the first pointer is a `const fg_target_desc*`
    "fg_target_loss_supported": (c_int, [P]),
    "fg_target_loss_workspace_floats": (c_size_t, [P]),
    "fg_target_loss_fwd": (c_int, [P, P, P, P, c_size_t, P, P]),  # (target, pred, maps or null, workspace, floats, out[3], stream)
    "fg_target_loss_bwd": (c_int, [P, P, P, P, P, P]),  # (target, pred, maps, v_out[2], v_pred, stream)
    # the displacement of the projected centres between two frames (csrc/flow_disp.hip); strides in floats
    # (N, means_t, mt_stride, means_0, m0_stride, viewmat_t, viewmat_0 or null, K, width, height, near, margin, disp, stream)
    "fg_flow_disp_fwd": (c_int, [c_int64, P, c_int64, P, c_int64, P, P, P, c_int, c_int, c_float, c_float, P, P]),
    # (..., margin, g_disp, g_means_t or null, g_means_0 or null, stream)
    "fg_flow_disp_bwd": (c_int, [c_int64, P, c_int64, P, c_int64, P, P, P, c_int, c_int, c_float, c_float, P, P, P, P]),
    # the masked flow L1 against the full-resolution batch array (csrc/flow_loss.hip)
    "fg_flow_l1_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),  # (H0, W0, downscale)
    # (H, W, pred, pixel_stride, row_stride, H0, W0, downscale, flows, mask or null, mask_dtype, workspace, bytes, out[1], stream)
    "fg_flow_l1_fwd": (c_int, [c_int, c_int, P, c_int64, c_int64, c_int, c_int, c_int, P, P, c_int, P, c_size_t, P, P]),
    # (..., mask_dtype, workspace, v_out[1], g_pred, stream)
    "fg_flow_l1_bwd": (c_int, [c_int, c_int, P, c_int64, c_int64, c_int, c_int, c_int, P, P, c_int, P, P, P, P]),
    # exact DBSCAN over [n,3] points (csrc/dbscan.hip)
    "fg_dbscan_workspace_bytes": (c_size_t, [c_int64]),
    # (n, xyz, eps, min_samples, labels_out int32[n], core_out uint8[n], counts_out int32[2] = {K, status}, workspace, bytes, stream)
    "fg_dbscan": (c_int, [c_int64, P, c_float, c_int, P, P, P, P, c_size_t, P]),
    # dense optical flow from two frames (csrc/optflow.hip)
    "fg_optflow_supported": (c_int, [c_int, c_int, c_int, c_int, c_int]),  # (H, W, levels, radius, iters) -> 1 or 0
    "fg_optflow_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int]),  # (H, W, levels, both_directions)
    # (H, W, channels, dtype, img, levels, workspace, bytes, stream)
    "fg_optflow_pyramid": (c_int, [c_int, c_int, c_int, c_int, P, c_int, P, c_size_t, P]),
    # (H, W, channels, dtype, a, b, levels, iters, radius, min_eig, both_directions, consistency, init or null, flow [H,W,2],
    #  valid uint8 [H,W], workspace, bytes, stream)
    "fg_optflow": (c_int, [c_int, c_int, c_int, c_int, P, P, c_int, c_int, c_int, c_float, c_int, c_float, P, P, P, P, c_size_t, P]),
}  # fmt: skip

# test hooks, not declared in the public header
_EXTRA = {"fg_debug_wave_reduce16": (c_int, [P, P, P]), "fg_debug_knn_grid": (c_int, [c_int64, P, c_int, P, P]),
          "fg_debug_color_correct_solve": (c_int, [P, P, P, P]),  # (G[10,10], r[10], w[10], rank[1]): host float64
          # fg_dbscan's arguments, then ms_host float[6] (per stage, between device events) and staged_out int32[1]
          "fg_debug_dbscan_stages": (c_int, [c_int64, P, c_float, c_int, P, P, P, P, c_size_t, P, P, P])}

ABI_VERSION = 14
ABI_MINOR = 1  # FG_ABI_MINOR: the least the binding needs (symbols added without raising FG_ABI_VERSION)
KNN_MAX_K = 8  # FG_KNN_MAX_K
DBSCAN_MAX_ROWS, DBSCAN_MAX_MIN_SAMPLES = 1 << 24, 65535  # FG_DBSCAN_MAX_ROWS, FG_DBSCAN_MAX_MIN_SAMPLES
DBSCAN_MIN_EPS, DBSCAN_MAX_EPS = 1e-18, 1e18  # FG_DBSCAN_MIN_EPS, FG_DBSCAN_MAX_EPS
OPTFLOW_MIN_SIDE, OPTFLOW_MAX_SIDE = 16, 16384  # FG_OPTFLOW_MIN_SIDE, FG_OPTFLOW_MAX_SIDE
OPTFLOW_MAX_LEVELS, OPTFLOW_MIN_COARSEST = 8, 8  # FG_OPTFLOW_MAX_LEVELS, FG_OPTFLOW_MIN_COARSEST
OPTFLOW_MAX_RADIUS, OPTFLOW_MAX_ITERS = 7, 16  # FG_OPTFLOW_MAX_RADIUS, FG_OPTFLOW_MAX_ITERS
MLP_ROW_TILE = 64  # FG_MLP_ROW_TILE
MLP_MAX_HEADS = 4  # FG_MLP_MAX_HEADS
MLP_SE3, MLP_PLAIN = 0, 1  # FG_MLP_SE3, FG_MLP_PLAIN
MLP_FP32, MLP_BF16X3 = 0, 1  # FG_MLP_FP32, FG_MLP_BF16X3: fg_mlp_desc::precision
MLP_WGRAD_MAX_SLAB, MLP_WGRAD_MIN_SPLIT = 4096, 512  # FG_MLP_WGRAD_MAX_SLAB, FG_MLP_WGRAD_MIN_SPLIT
MLP_TRAIN_BWD_CHUNK_SLABS = 16  # FG_MLP_TRAIN_BWD_CHUNK_SLABS
COLOR_CORRECT_MAX_ITERS = 8  # FG_COLOR_CORRECT_MAX_ITERS
CONTROL_MAX_ATTRS = 32  # FG_CONTROL_MAX_ATTRS
TARGET_U8, TARGET_F32 = 0, 1  # FG_TARGET_U8, FG_TARGET_F32: fg_target_desc::src_dtype / mask_dtype


def mlp_enc_width(aux_width: int) -> int:
    """FG_MLP_ENC_WIDTH: floats of one encoded input row as fg_mlp_train_fwd stores it (padded to a multiple of 8)."""
    return (63 + aux_width + 7) // 8 * 8


STBIN_LONG_SEGMENTS = 1  # FG_STBIN_LONG_SEGMENTS
STBIN_TEST_SMALL_SLABS = 4  # FG_STBIN_TEST_SMALL_SLABS (tests: the sample sort's overflow path)
STEP_NO_FOOTPRINT_MASKS = 2  # FG_STEP_NO_FOOTPRINT_MASKS
SH_JAC_FLOATS = 10  # FG_SH_JAC_FLOATS
_lib = None


class FgRasterError(RuntimeError):
    pass


class RasterConfig(ctypes.Structure):
    """``fg_raster_config`` of include/fgraster.h: the launch policy of the raster kernels, handed to every
    raster entry point (the library itself reads no environment variable).  Field order = the header's."""

    _fields_ = [(n, ctypes.c_int32) for n in (
        "size", "ppt_fwd", "ppt_bwd", "tile_order", "bands_nx", "tail4_fwd", "tail2_fwd", "tail4_bwd", "tail2_bwd",
        "split4_fwd", "split2_fwd", "split4_bwd", "split2_bwd", "use_liveness", "seg_parts", "seg_tail", "seg_parts2",
        "seg_tail2", "debug_only_xcd", "debug_k_mod", "balance_bands", "heavy_tiles", "seg_slots", "prio_fwd", "prio_bwd",
        "heavy_wide", "seg_fine")]  # fmt: skip

    FIELDS = tuple(n for n, _ in _fields_)[1:]

    @classmethod
    def defaults(cls) -> "RasterConfig":
        cfg = cls()
        load().fg_raster_config_init(ctypes.byref(cfg))
        return cfg

    def ptr(self) -> int:
        return ctypes.addressof(self)


STEP_BUFFERS = ("radii", "means2d", "depths", "conics", "comp", "tiles", "splats", "depth_keys", "tile_rects", "tile_masks", "sh_jac",
                "tile_offsets", "list_offsets", "flatten_ids", "jobs", "live", "seg_ckpt", "v_splats", "render", "alphas",
                "last_ids", "clamp_mask", "count_ws", "fill_ws")  # the FG_STEP_* enum of include/fgraster.h, in order
STEP_BUFFER = {n: i for i, n in enumerate(STEP_BUFFERS)}


class StepDesc(ctypes.Structure):
    """``fg_step_desc``: field order = the header's."""

    _fields_ = [(n, ctypes.c_int32) for n in (
        "size", "N", "width", "height", "tile_size", "raw", "sh_degree", "k_stored", "n_color", "with_depth", "n_extra",
        "antialiased", "n_clamp", "want_backward", "list_shares", "flags")] + [
        (n, ctypes.c_float) for n in ("eps2d", "near_plane", "far_plane", "radius_clip")] + [("capacity", ctypes.c_int64)]  # fmt: skip


class StepIO(ctypes.Structure):
    """``fg_step_io``: device pointers as integers."""

    _fields_ = [(n, ctypes.c_void_p) for n in (
        "means", "quats", "d_quats", "scales", "d_scales", "opacities", "colors", "features_rest", "extra", "viewmat", "K",
        "background", "count_out", "v_render", "v_alphas", "v_depths", "v_conics", "v_means", "v_quats", "v_d_quats",
        "v_scales", "v_d_scales", "v_opacities", "v_colors", "v_features_rest", "v_extra", "v_rgb")] + [
        ("v_rgb_floats", ctypes.c_int32), ("ev_raster_begin", ctypes.c_void_p), ("ev_raster_end", ctypes.c_void_p),
        ("ckpt_need_out", ctypes.c_void_p)]  # fmt: skip


class StepLayout(ctypes.Structure):
    """``fg_step_layout``."""

    _fields_ = [("keep_bytes", ctypes.c_int64), ("tmp_bytes", ctypes.c_int64),
                ("offset", ctypes.c_int64 * len(STEP_BUFFERS)), ("nbytes", ctypes.c_int64 * len(STEP_BUFFERS)),
                ("jobs_words", ctypes.c_int64), ("seg_ckpt_floats", ctypes.c_int64), ("channels", ctypes.c_int32)]  # fmt: skip


class MlpDesc(ctypes.Structure):
    """``fg_mlp_desc``: field order = the header's; device pointers as integers."""

    _fields_ = [(n, ctypes.c_int32) for n in ("size", "mode", "depth", "width", "multires", "aux_width", "n_heads")] + [
        ("head_rows", ctypes.c_int32 * MLP_MAX_HEADS), ("precision", ctypes.c_int32), ("aux_stride", ctypes.c_int64),
        ("x", ctypes.c_void_p), ("aux", ctypes.c_void_p), ("weight", ctypes.c_void_p * 8), ("bias", ctypes.c_void_p * 8),
        ("head_weight", ctypes.c_void_p * MLP_MAX_HEADS), ("head_bias", ctypes.c_void_p * MLP_MAX_HEADS),
        ("out", ctypes.c_void_p * MLP_MAX_HEADS)]  # fmt: skip


class MlpGrads(ctypes.Structure):
    """``fg_mlp_grads``: where ``fg_mlp_param_grads`` writes; a null pointer = that gradient is not formed."""

    _fields_ = [("size", ctypes.c_int32), ("reserved", ctypes.c_int32), ("weight", ctypes.c_void_p * 8),
                ("bias", ctypes.c_void_p * 8), ("head_weight", ctypes.c_void_p * MLP_MAX_HEADS),
                ("head_bias", ctypes.c_void_p * MLP_MAX_HEADS)]  # fmt: skip


class TargetDesc(ctypes.Structure):
    """``fg_target_desc``: field order = the header's; device pointers as integers."""

    _fields_ = [(n, ctypes.c_int32) for n in ("size", "src_dtype", "height", "width", "channels", "downscale", "mask_dtype",
                                              "reserved")] + [
        ("src", ctypes.c_void_p), ("mask", ctypes.c_void_p), ("background", ctypes.c_void_p)]  # fmt: skip


def load() -> ctypes.CDLL:
    """Load the library once; raise loudly when it is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise FgRasterError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C freegaussian_amd/csrc`.  There is no CPU fallback."
        )
    # FG_RASTER_LIB: load another build of the same library (the instrumented `make stats` one)
    lib = ctypes.CDLL(os.environ.get("FG_RASTER_LIB", LIB_PATH))
    for name, (res, args) in {**SIGNATURES, **_EXTRA}.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is absent
        fn.restype = res
        fn.argtypes = args
    if lib.fg_abi_version() != ABI_VERSION:
        raise FgRasterError(f"ABI mismatch: library {lib.fg_abi_version()} vs binding {ABI_VERSION}")
    if ABI_MINOR and lib.fg_abi_minor() < ABI_MINOR:
        raise FgRasterError(f"ABI mismatch: library minor {lib.fg_abi_minor()} below the binding's {ABI_MINOR}")
    _lib = lib
    return lib


def check(code: int, what: str) -> None:
    if code != 0:
        msg = load().fg_error_string(code).decode()
        raise FgRasterError(f"{what} failed: {msg} ({code})")
