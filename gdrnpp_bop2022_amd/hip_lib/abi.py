"""The C ABI of ``libgdrnpp_hip.so`` (``include/gdrnpp_hip.h``): signature table, loader, pointer checks, and the one path every
status-returning entry point is launched through (``launch``).  The only module that touches ctypes function objects."""
from __future__ import annotations

import ctypes
import os
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_long, c_longlong, c_size_t, c_void_p

import torch

_PKG_DIR = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # the library sits beside the package, where csrc/Makefile puts it
LIB_PATH = os.environ.get("GDRNPP_HIP_LIB", os.path.join(_PKG_DIR, "libgdrnpp_hip.so"))

_lib = None


class gdrnpp_meshes(ctypes.Structure):
    _fields_ = [
        ("verts", c_void_p),
        ("faces", c_void_p),
        ("vert_off", c_void_p),
        ("face_off", c_void_p),
        ("n_obj", c_int),
        ("max_verts", c_int),
        ("max_faces", c_int),
    ]


class gdrnpp_roi_table(ctypes.Structure):
    _fields_ = [(k, c_void_p) for k in ("center64", "scale64", "im_idx", "roi_cls", "roi_cam", "roi_center", "roi_wh", "scale",
                                        "resize_ratio", "roi_extent", "score", "roi_id")]


# name -> (restype, argtypes); must list every symbol of include/gdrnpp_hip.h
_P = c_void_p
SIGNATURES = {
    "gdrnpp_version": (c_int, []),
    "gdrnpp_set_option": (c_int, [c_char_p, c_int]),
    "gdrnpp_get_option": (c_int, [c_char_p, POINTER(c_int)]),
    "gdrnpp_copy_d2d": (c_int, [_P, _P, c_size_t, _P]),
    "gdrnpp_epnp_ransac_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gdrnpp_epnp_ransac": (c_int, [_P, _P, _P, c_int, _P, _P, c_int, c_int, c_float, c_double, _P, _P, _P, _P, _P,
                                   c_int, _P, c_size_t, _P]),
    "gdrnpp_epnp_batched": (c_int, [_P, _P, c_int, _P, _P, _P, _P, c_int, _P]),
    "gdrnpp_last_error": (c_char_p, []),
    "farthest_point_sampling": (None, [_P, _P, c_int, c_int]),
    "farthest_point_sampling_init_center": (None, [_P, _P, c_int, c_int]),
    "uncertainty_pnp": (None, [_P, _P, _P, _P, _P, _P, c_int]),
    "gdrnpp_fps_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gdrnpp_fps": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "gdrnpp_nnd_forward": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "gdrnpp_nnd_backward": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "gdrnpp_generate_hypothesis": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "gdrnpp_voting_for_hypothesis": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_float, _P]),
    "gdrnpp_generate_hypothesis_vanishing_point": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "gdrnpp_voting_for_hypothesis_vanishing_point": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_float, _P]),
    "gdrnpp_vote_count": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_float, c_int, _P]),
    "gdrnpp_uncertainty_pnp_batched": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    "gdrnpp_pnp_iter_from_correspondences": (c_int, [_P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, c_int, _P]),
    "gdrnpp_decode_correspondences": (
        c_int, [_P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_float, _P]),
    "gdrnpp_pose_from_pred_centroid_z": (c_int, [_P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "gdrnpp_zoom_K": (c_int, [_P, _P, _P, _P, c_int, c_float, _P]),
    "gdrnpp_render_depth": (
        c_int, [POINTER(gdrnpp_meshes), _P, _P, _P, _P, _P, _P, c_int, c_int, c_float, c_float, _P]),
    "gdrnpp_depth_refine_workspace_bytes": (c_size_t, [POINTER(gdrnpp_meshes), c_int]),
    "gdrnpp_depth_refine": (
        c_int, [POINTER(gdrnpp_meshes), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float,
                c_int, c_int, c_float, c_float, _P, c_size_t, _P]),
    "gdrnpp_refine_to_records": (
        c_int, [POINTER(gdrnpp_meshes), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int,
                c_float, c_int, c_int, c_float, c_float, _P, c_size_t, _P]),
    "gdrnpp_pose_errors_workspace_bytes": (c_size_t, [POINTER(gdrnpp_meshes), c_int]),
    "gdrnpp_pose_errors": (c_int, [POINTER(gdrnpp_meshes), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "gdrnpp_bop_errors_workspace_bytes": (c_size_t, [POINTER(gdrnpp_meshes), _P, c_int]),
    "gdrnpp_bop_errors": (c_int, [POINTER(gdrnpp_meshes), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "gdrnpp_sym_errors_workspace_bytes": (c_size_t, [POINTER(gdrnpp_meshes), _P, c_int]),
    "gdrnpp_sym_errors": (c_int, [POINTER(gdrnpp_meshes), _P, _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "gdrnpp_vsd_counts_workspace_bytes": (c_size_t, [POINTER(gdrnpp_meshes), c_int]),
    "gdrnpp_vsd_counts": (c_int, [POINTER(gdrnpp_meshes), _P, _P, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P, c_int, c_float,
                                  c_double, c_double, _P, c_int, _P, c_size_t, _P]),
    "gdrnpp_gt_visibility_workspace_bytes": (c_size_t, [POINTER(gdrnpp_meshes), c_int]),
    "gdrnpp_gt_visibility": (c_int, [POINTER(gdrnpp_meshes), _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_float, c_double,
                                     c_double, _P, _P, _P, c_int, _P, c_size_t, _P]),
    "gdrnpp_gt_xyz_crop_workspace_bytes": (c_size_t, [POINTER(gdrnpp_meshes), c_int]),
    "gdrnpp_gt_xyz_crop": (c_int, [POINTER(gdrnpp_meshes), _P, _P, _P, _P, c_int, c_int, c_double, c_double, _P, c_longlong, _P, _P, c_int,
                                   _P, c_size_t, _P]),
    "gdrnpp_roi_train_targets": (c_int, [_P, c_longlong, _P, _P, _P, c_int, _P, _P, _P, c_int, c_int, _P, _P, _P, _P, c_int, _P, c_int, c_int,
                                         c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_int, _P]),
    "gdrnpp_pose_from_pred": (c_int, [_P, c_int, _P, c_int, _P, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    "gdrnpp_debug_refine_profile": (c_int, [_P]),
    "gdrnpp_pack_weight_bf16x3": (c_int, [_P, _P, c_int, c_int, _P]),
    "gdrnpp_linear_f32_split": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_linear_f32_split_grouped": (c_int, [_P, _P, _P, _P, c_int, c_int, _P, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_stem_conv4x4_ln": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P]),
    "gdrnpp_head_tail_nhwc": (c_int, [_P, c_int, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "gdrnpp_linear_f32_splitk_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gdrnpp_linear_f32_splitk": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, c_size_t, _P]),
    "gdrnpp_conv2d_f32_split": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_conv3x3_f32_split": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_roi_align": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, c_int, c_int, _P]),
    "gdrnpp_conv2d_f32_splitk_workspace_bytes": (c_size_t, [c_int, c_int, c_int, c_int, c_int, c_int, c_int]),
    "gdrnpp_conv2d_f32_splitk": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P,
                                         c_size_t, _P]),
    "gdrnpp_roi_pool": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_float, _P]),
    "gdrnpp_debug_stream_read": (c_int, [_P, c_size_t, c_int, _P, c_int, _P]),
    "gdrnpp_debug_spin": (c_int, [c_int, _P]),
    "gdrnpp_crop_resize_roi": (
        c_int, [_P, _P, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P]),
    "gdrnpp_yolox_postprocess_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gdrnpp_yolox_postprocess": (c_int, [_P, c_int, c_int, c_int, c_float, c_float, c_int, _P, _P, c_int, _P, c_size_t, _P]),
    "gdrnpp_conv_bias_act_f32": (c_int, [_P, c_int, c_int, _P, c_int, _P, _P, c_int, c_int, _P, c_int, c_int, c_long, c_long, c_int, c_int,
                                         c_int, c_int, c_int, c_int, c_int, c_int, c_float, _P]),
    "gdrnpp_yolox_focus": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_spp_maxpool_5_9_13": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_yolox_letterbox": (c_int, [_P, c_int, c_int, c_int, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_rois_from_dets_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gdrnpp_rois_from_dets": (c_int, [_P, _P, c_int, c_int, c_int, c_float, c_int, c_int, c_double, c_int, _P, c_int, _P, c_double, c_int,
                                      c_int, _P, _P, _P, _P, c_size_t, _P]),
    "gdrnpp_upsample_nearest2x_slice": (c_int, [_P, c_int, c_int, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_paste_masks_rle": (c_int, [_P, _P, c_int, c_int, c_int, c_int, c_int, c_float, _P, _P, c_int, _P]),
    "gdrnpp_flow_forward": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "gdrnpp_pack_pose_records": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, _P]),
    "gdrnpp_dwconv7x7_ln_nhwc": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, _P]),
    "gdrnpp_dwconv7x7_ln_nhwc_rows": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, c_int, _P]),
    "gdrnpp_layernorm_nhwc": (c_int, [_P, _P, _P, _P, c_long, c_int, c_float, _P]),
    "gdrnpp_upsample_bilinear2x_nhwc": (c_int, [_P, _P, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_groupnorm_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gdrnpp_groupnorm_act_nhwc": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, c_int, _P]),
    "gdrnpp_bias_act_nhwc": (c_int, [_P, _P, _P, _P, c_long, c_int, c_int, _P]),
    "gdrnpp_deconv_col2im_nhwc": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_deconv_col2im_gn_nhwc": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_pnp_fc_heads": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "gdrnpp_pnp_fc_heads_pose": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, c_int, _P]),
    "gdrnpp_point_pnp_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gdrnpp_point_pnp_pool": (c_int, [_P, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _P, c_size_t, _P]),
    "gdrnpp_point_pnp_fc": (c_int, [_P, c_size_t, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    "gdrnpp_upconv_gather_partials": (c_int, [c_int, c_int, c_int]),
    "gdrnpp_upconv_gather_gn_nhwc": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_conv3x3_gnstats_partials": (c_int, [c_int, c_int]),
    "gdrnpp_conv3x3_f32_split_gnstats": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_groupnorm_apply_nhwc": (c_int, [_P, _P, c_int, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, c_int, _P]),
    "gdrnpp_pack_weight_f16x2_bytes": (c_size_t, [c_int, c_int]),
    "gdrnpp_pack_weight_f16x2": (c_int, [_P, _P, c_int, c_int, _P]),
    "gdrnpp_linear_f32_split2": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "gdrnpp_linear_f32_split2_rows": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "gdrnpp_conv3x3_f32_split2": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "gdrnpp_conv2d_f32_split2": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "gdrnpp_split2_range_word": (c_int, [_P, c_int, _P]),
    "gdrnpp_pack_mlp_fused_f16x2_bytes": (c_size_t, [c_int, c_int]),
    "gdrnpp_pack_mlp_fused_f16x2": (c_int, [_P, _P, _P, c_int, c_int, _P]),
    "gdrnpp_convnext_mlp_f32_fused": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P]),
    "gdrnpp_gdrn_dense_losses_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gdrnpp_gdrn_dense_losses": (c_int, [_P, _P, _P, c_int, _P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int,
                                         c_int, c_int, c_int, _P, _P, _P, c_size_t, _P]),
    "gdrnpp_gdrn_dense_losses_backward": (c_int, [_P, _P, _P, c_int, _P, _P, _P, c_int, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int,
                                                  c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    "gdrnpp_gdrn_pose_losses_workspace_bytes": (c_size_t, [c_int]),
    "gdrnpp_gdrn_pose_losses": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, _P, _P, c_int, _P, _P, _P, _P, c_int, c_int, c_int, c_int,
                                        c_double, c_int, _P, _P, _P, _P, _P, _P, c_size_t, _P]),
    "gdrnpp_ranger_step": (c_int, [_P, c_int, _P, c_int, _P, c_int, _P, _P]),
}


def load(path: str | None = None) -> ctypes.CDLL:
    """Load the shared library and bind every declared symbol (no compute, no GPU needed)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise RuntimeError(
            f"gdrnpp_bop2022_amd: HIP extension {p} is missing — run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` (or `make -C gdrnpp_bop2022_amd/csrc`).  There is no CPU fallback."
        )
    lib = ctypes.CDLL(p)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the .so does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().gdrnpp_last_error()
        raise RuntimeError(f"{what} failed with status {rc}: {msg.decode() if msg else ''}")


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)     # the handle without building a torch.cuda.Stream object


def current_stream() -> int:
    """hipStream_t of the current device's current stream.  Called once per launch (~150 per step): the raw accessor takes
    ~0.3 us against ~8 us for torch.cuda.current_stream().cuda_stream — 1-2 ms per step of host time, which is what bounds the
    small batches once two steps are in flight."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


class LaunchTimer:
    """Optional per-launch timing of the split-GEMM entry points (kinds "linear", "conv3x3", ...) and of the memory-bound
    network kernels (kinds "hbm:<kernel>", flops 0) with HIP events recorded on the stream the kernel is launched on
    (bench.py's roofline leg).  records: (kind, fp32-equivalent flops, start event, end event, algorithmic bytes =
    operands read once + result written once)."""

    def __init__(self):
        self.records = []

    def launch(self, kind, flops, fn, nbytes=0.0):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        rc = fn()
        e1.record()
        self.records.append((kind, flops, e0, e1, nbytes))
        return rc


_LAUNCH_TIMER = None


def set_launch_timer(timer):
    global _LAUNCH_TIMER
    _LAUNCH_TIMER = timer


def launch(name: str, *args, timed=None) -> None:
    """Call the status-returning entry point ``name`` with ``args`` + the current stream; a non-zero status raises RuntimeError
    with the library's last error, named after ``name``.  ``timed`` = (kind, flops, nbytes): what an installed LaunchTimer records
    for this launch (without a timer the call is direct, no closure is built)."""
    fn = getattr(_lib if _lib is not None else load(), name)
    stream = current_stream()
    if timed is None or _LAUNCH_TIMER is None:
        rc = fn(*args, stream)
    else:
        rc = _LAUNCH_TIMER.launch(timed[0], timed[1], lambda: fn(*args, stream), timed[2])
    if rc != 0:
        check(rc, name)


def copy_d2d(dst_ptr: int, src: torch.Tensor) -> None:
    """Copy a contiguous device tensor into a raw device pointer on the current stream (``gdrnpp_copy_d2d``)."""
    if not src.is_cuda or not src.is_contiguous():
        raise RuntimeError("copy_d2d: src must be a contiguous CUDA(HIP) tensor")
    launch("gdrnpp_copy_d2d", c_void_p(int(dst_ptr)), src.data_ptr(), src.numel() * src.element_size())


def spin(micros: int) -> None:
    """One wave busy-waiting ``micros`` microseconds of the device's wall clock on the current stream (``gdrnpp_debug_spin``): the
    probe kernel of engine.streams_overlap_ratio — occupies a hardware queue, computes nothing."""
    launch("gdrnpp_debug_spin", int(micros))


def set_option(name: str, value: int) -> None:
    """Process-wide tuning switch of the library (``gdrnpp_set_option``; the one entry point without a stream)."""
    check(load().gdrnpp_set_option(name.encode(), int(value)), "gdrnpp_set_option")


def get_option(name: str) -> int:
    """Current value of a process-wide tuning switch (``gdrnpp_get_option``)."""
    value = c_int(0)
    check(load().gdrnpp_get_option(name.encode(), ctypes.byref(value)), "gdrnpp_get_option")
    return value.value


def dev_ptr(t: torch.Tensor, dtype: torch.dtype, name: str) -> int:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA(HIP) tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t.data_ptr()


def f32_ptr(t: torch.Tensor, name: str) -> int:
    """``dev_ptr(t, torch.float32, name)`` with the checks in one test: one Python call per argument, as ``dev_ptr`` itself."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        dev_ptr(t, torch.float32, name)    # raises, saying which
    return t.data_ptr()


def opt_f32_ptr(t: torch.Tensor | None, name: str):
    """``f32_ptr`` of an optional argument: None = NULL."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        dev_ptr(t, torch.float32, name)
    return t.data_ptr()


def nhwc_ptr(t: torch.Tensor, name: str) -> int:
    """A network-side NHWC layer's tensor: logically NCHW with channels_last strides."""
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError(f"{name} must be a 4-D float32 CUDA(HIP) tensor")
    if not t.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError(f"{name} must be channels_last contiguous")
    return t.data_ptr()


def channels_last_f32(x_cl, what: str):
    if not x_cl.is_contiguous(memory_format=torch.channels_last) or x_cl.dtype != torch.float32 or not x_cl.is_cuda:
        raise ValueError("%s expects a float32 channels_last device tensor" % what)
    return x_cl.shape
