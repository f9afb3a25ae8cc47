"""ctypes binding of ``libgdrnpp_hip.so`` (the C ABI declared in ``include/gdrnpp_hip.h``).

PyTorch is used here only as the owner of device memory and streams: every wrapper checks
device / dtype / contiguity, then hands raw ``data_ptr()``s and the current HIP stream to the
C entry point.  There is NO CPU fallback: if the shared library is missing or a call returns a
non-zero status, a ``RuntimeError`` is raised (reference behaviour for misuse is
``TORCH_CHECK`` -> ``RuntimeError``, ransac_voting.cpp:7-19).

This file is the namespace and nothing else.  The modules, in dependency order (a module imports only from those in front of it):
``abi`` (signature table, structs and constants read from the header, loader, pointer checks, the one launch path), ``dispatch`` (kernel-choice thresholds), ``range_words``
(three-product range words and launch count), ``cv_resize`` (the request of an 8-bit cv2.resize, which the tables of ``roi`` and ``yolox`` carry), then one module per
kernel family: ``gemm``, ``net``, ``pose``, ``roi``, ``yolox``.
State that somebody assigns lives in its owner and is assigned there (``hip_lib.dispatch.SPLIT2_MIN_TILES = 1``); the three
``SPLIT2_*`` thresholds can be READ here, always as the owner's current value.
"""
from . import abi, cv_resize, dispatch, gemm, net, pose, range_words, roi, yolox  # noqa: F401
from .abi import (LIB_PATH, SIGNATURES, LaunchTimer, check, copy_d2d, current_stream, dev_ptr, gdrnpp_meshes,  # noqa: F401
                  gdrnpp_roi_table, get_option, load, set_launch_timer, set_option, spin)
from .cv_resize import RESIZE_MODES, cv_round, resize_request  # noqa: F401
from .dispatch import (set_conv_splitk, shared_min_rows, shared_min_tiles, shared_min_tiles_scope, split2_tiles_ok,  # noqa: F401
                       split_gemm_tiles)
from .gemm import (A_F16X2_ROWS, C_F16X2_ROWS, X3, conv2d_f32_split, conv3x3_f32_split, conv3x3_groupnorm_act,  # noqa: F401
                   conv_transpose2d_f32_split, conv_transpose2d_groupnorm_act, convnext_mlp_f32_fused, f16x2_rows_decode,
                   linear_f32_split, linear_f32_split_grouped, linear_f32_splitk, mlp_fused_rows_in_range, mlp_fused_supported,
                   pack_conv3x3_weight_bf16x3, pack_conv_weight_bf16x3, pack_conv_weight_f16x2, pack_deconv_weight_bf16x3, pack_deconv_weight_f16x2,
                   pack_mlp_fused_f16x2, pack_upconv_weight_bf16x3, pack_upconv_weight_f16x2, pack_weight_bf16x3, pack_weight_f16x2,
                   packed_rows_in_range, unpack_weight_bf16x3, unpack_weight_f16x2, upsample2x_conv3x3_groupnorm_act, upsample2x_conv3x3_raw)
from .gemm import (colsum_f32, convnext_mlp_backward, convnext_mlp_forward_train, gelu_f32, gemm_tn_f32, linear_f32_exact, mlp_bwd_act_,  # noqa: F401
                   pack_weight_bf16x3_t)
from .gemm import (conv3x3_backward, conv3x3_f32_mfma, conv3x3_weight_kn, conv3x3_weight_kn_flipped, conv3x3_wgrad_f32,  # noqa: F401
                   conv_transpose2d_backward, conv_transpose2d_train, deconv_im2col, deconv_weight_kn, groupnorm_apply)
from .gemm import grouped_linear_dinput, grouped_linear_wgrad  # noqa: F401
from .gemm import (conv3x3s2_backward, conv3x3s2_dinput_f32, conv3x3s2_dinput_weight, conv3x3s2_f32_mfma, conv3x3s2_weight_kn,  # noqa: F401
                   conv3x3s2_wgrad_f32, nhwc_flatten_nchw, nhwc_unflatten_nchw, pnp_fc_heads_backward, workspace)
from .net import (DENSE_MASK_TYPES, DENSE_SUMS, DENSE_XYZ_TYPES, LOSS_MASKS, PM_TYPES, POINT_PNP_TILE, ROT_DIMS, ROT_MODES, T_MODES,  # noqa: F401
                  bias_act_nhwc_, dwconv7x7_ln, dwconv7x7_ln_backward, gdrn_dense_losses, gdrn_dense_losses_backward, gdrn_pose_losses, groupnorm_act,
                  groupnorm_act_backward, groupnorm_act_train, head_tail_backward, head_tail_nhwc,
                  layernorm_nhwc, pnp_fc_heads, pnp_fc_heads_pose, point_pnp_fc, point_pnp_pool, stem_conv4x4_ln, upsample_bilinear2x, upsample_bilinear2x_backward)
from .net import (downsample_backward, downsample_weight_nk, layernorm_patch2x2, layernorm_patch2x2_backward,  # noqa: F401
                  stem_conv4x4_ln_backward)
from .net import (RANGER_COEFS, RANGER_LONG_ROW, RANGER_LOOKAHEAD, RANGER_NAN_TO_NUM, RANGER_RECTIFIED, RANGER_TENSOR, RANGER_TILE,  # noqa: F401
                  RANGER_WORK, RangerTables, ranger_plan, ranger_same_layout, ranger_step, ranger_tensor_ok)
from .net import EMA_TENSOR, EMA_TILE, EMA_WORK, EmaTables, ema_plan, ema_tensor_ok, ema_update  # noqa: F401
from .pose import (GT_INFO_COLUMNS, XYZ_CROP_COLUMNS, MeshSet, bop_errors, decode_correspondences, depth_refine, epnp_batched, epnp_ransac,  # noqa: F401
                   flow_forward, fps, gt_visibility, gt_xyz_crops, nnd_backward, nnd_forward, pack_pose_records, paste_masks_rle, pnp_iter_from_correspondences, pose_from_pred,
                   pose_errors, pose_from_pred_centroid_z, refine_kernel_name, refine_to_records, render_depth, set_refine_event_sink,
                   sym_errors, uncertainty_pnp_batched, vsd_counts, vsd_errors, zoom_K)
from .range_words import (X3_NONFINITE, X3_SLOTS, X3_SMALL_ROWS, range_words_of, split2_nonfinite, split2_range_words,  # noqa: F401
                          x3_flag_ptr, x3_flag_scope, x3_flags, x3_launch_count)
from .roi import (REPLACE_BG_COLUMNS, REPLACE_BG_CUTS, REPLACE_BG_MODES, ROI_BIN_MASKS, ROI_TABLE_COLUMNS, ROI_TARGET_KEYS, crop_resize_roi,  # noqa: F401
                  replace_bg, replace_bg_table, roi_align, roi_pool, roi_table, roi_train_targets, rois_from_dets)
from .yolox import (CONV_ACTS, conv_bias_act_f32, letterbox_sizes, pack_conv_weight_kmajor, spp_maxpool_5_9_13,  # noqa: F401
                    upsample_nearest2x_slice, yolox_focus, yolox_letterbox, yolox_postprocess)
from .yolox import (bn_silu_apply, bn_silu_backward, bn_train_stats, conv3x3s2_dinput_any_f32, conv_backward, conv_train_f32,  # noqa: F401
                    conv_wgrad_f32)
from .yolox import YOLOX_CLS_LOSSES, YOLOX_IOU_LOSSES, YOLOX_LOSS_KEYS, yolox_assign, yolox_losses, yolox_losses_backward  # noqa: F401
from .yolox import (YOLOX_AUG_BRANCHES, YOLOX_AUG_COLUMNS, YOLOX_AUG_FLAGS, YOLOX_AUG_MODES, YOLOX_AUG_SOURCE_COLUMNS, yolox_aug_table,  # noqa: F401
                    yolox_train_inputs)


def __getattr__(name):
    if name in ("SPLIT2_MIN_TILES", "SPLIT2_SHARED_MIN_TILES", "SPLIT2_SHARED_MIN_ROWS"):
        return getattr(dispatch, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
