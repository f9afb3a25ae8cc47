"""ctypes binding of ``libgdrnpp_hip.so`` (the C ABI declared in ``include/gdrnpp_hip.h``).

PyTorch is used here only as the owner of device memory and streams: every wrapper checks
device / dtype / contiguity, then hands raw ``data_ptr()``s and the current HIP stream to the
C entry point.  There is NO CPU fallback: if the shared library is missing or a call returns a
non-zero status, a ``RuntimeError`` is raised (reference behaviour for misuse is
``TORCH_CHECK`` -> ``RuntimeError``, ransac_voting.cpp:7-19).
"""
from __future__ import annotations

import ctypes
import os
import threading
from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_long, c_size_t, c_void_p

import torch

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
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


# name -> (restype, argtypes); must list every symbol of include/gdrnpp_hip.h
_P = c_void_p
SIGNATURES = {
    "gdrnpp_version": (c_int, []),
    "gdrnpp_set_option": (c_int, [ctypes.c_char_p, c_int]),
    "gdrnpp_copy_d2d": (c_int, [_P, _P, c_size_t, _P]),
    "gdrnpp_epnp_ransac_workspace_bytes": (c_size_t, [c_int, c_int, c_int]),
    "gdrnpp_epnp_ransac": (c_int, [_P, _P, _P, c_int, _P, _P, c_int, c_int, ctypes.c_float, ctypes.c_double, _P, _P, _P, _P, _P,
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
    "gdrnpp_bias_act_nhwc": (c_int, [_P, _P, _P, _P, ctypes.c_long, c_int, c_int, _P]),
    "gdrnpp_deconv_col2im_nhwc": (c_int, [_P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_deconv_col2im_gn_nhwc": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_pnp_fc_heads": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P]),
    "gdrnpp_pnp_fc_heads_pose": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P, _P, _P, _P, _P, c_int, _P]),
    "gdrnpp_point_pnp_workspace_bytes": (c_size_t, [c_int, c_int]),
    "gdrnpp_point_pnp_pool": (c_int, [_P, c_int, c_int, _P, _P, _P, _P, _P, _P, _P, c_int, c_int, _P, c_size_t, _P]),
    "gdrnpp_point_pnp_fc": (c_int, [_P, c_size_t, _P, _P, _P, _P, _P, c_int, c_int, _P]),
    "gdrnpp_conv3x3_gnstats_partials": (c_int, [c_int, c_int]),
    "gdrnpp_conv3x3_f32_split_gnstats": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, _P]),
    "gdrnpp_groupnorm_apply_nhwc": (c_int, [_P, _P, c_int, _P, _P, _P, c_int, c_int, c_int, c_int, c_float, c_int, _P]),
    "gdrnpp_pack_weight_f16x2_bytes": (ctypes.c_size_t, [c_int, c_int]),
    "gdrnpp_pack_weight_f16x2": (c_int, [_P, _P, c_int, c_int, _P]),
    "gdrnpp_linear_f32_split2": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, _P, _P]),
    "gdrnpp_linear_f32_split2_rows": (c_int, [_P, _P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "gdrnpp_conv3x3_f32_split2": (c_int, [_P, _P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "gdrnpp_conv2d_f32_split2": (c_int, [_P, _P, _P, _P, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, c_int, _P, _P]),
    "gdrnpp_split2_range_word": (c_int, [_P, c_int, _P]),
    "gdrnpp_pack_mlp_fused_f16x2_bytes": (ctypes.c_size_t, [c_int, c_int]),
    "gdrnpp_pack_mlp_fused_f16x2": (c_int, [_P, _P, _P, c_int, c_int, _P]),
    "gdrnpp_convnext_mlp_f32_fused": (c_int, [_P, _P, _P, _P, _P, _P, _P, c_int, c_int, c_int, _P, _P, _P]),
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


def copy_d2d(dst_ptr: int, src: torch.Tensor) -> None:
    """Copy a contiguous device tensor into a raw device pointer on the current stream (``gdrnpp_copy_d2d``)."""
    if not src.is_cuda or not src.is_contiguous():
        raise RuntimeError("copy_d2d: src must be a contiguous CUDA(HIP) tensor")
    _check(load().gdrnpp_copy_d2d(c_void_p(int(dst_ptr)), src.data_ptr(), src.numel() * src.element_size(), _stream()),
           "gdrnpp_copy_d2d")


def spin(micros: int) -> None:
    """One wave busy-waiting ``micros`` microseconds of the device's wall clock on the current stream (``gdrnpp_debug_spin``): the
    probe kernel of engine.streams_overlap_ratio — occupies a hardware queue, computes nothing."""
    _check(load().gdrnpp_debug_spin(int(micros), _stream()), "gdrnpp_debug_spin")


def set_option(name: str, value: int) -> None:
    """Process-wide tuning switch of the library (``gdrnpp_set_option``)."""
    _check(load().gdrnpp_set_option(name.encode(), int(value)), "gdrnpp_set_option")


def _check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().gdrnpp_last_error()
        raise RuntimeError(f"{what} failed with status {rc}: {msg.decode() if msg else ''}")


_RAW_STREAM = getattr(torch._C, "_cuda_getCurrentRawStream", None)     # the handle without building a torch.cuda.Stream object


def _stream() -> int:
    """hipStream_t of the current device's current stream.  Called once per launch (~150 per step): the raw accessor takes
    ~0.3 us against ~8 us for torch.cuda.current_stream().cuda_stream — 1-2 ms per step of host time, which is what bounds the
    small batches once two steps are in flight."""
    if _RAW_STREAM is not None:
        return _RAW_STREAM(torch.cuda.current_device())
    return torch.cuda.current_stream().cuda_stream


def _dev(t: torch.Tensor, dtype: torch.dtype, name: str) -> int:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA(HIP) tensor")
    if t.dtype != dtype:
        raise RuntimeError(f"{name} must have dtype {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t.data_ptr()


def _f32(t: torch.Tensor, name: str) -> int:
    """``_dev(t, torch.float32, name)`` with the checks in one test: one Python call per argument, as ``_dev`` itself."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        _dev(t, torch.float32, name)    # raises, saying which
    return t.data_ptr()


def _opt_f32(t: torch.Tensor | None, name: str):
    """``_f32`` of an optional argument: None = NULL."""
    if t is None:
        return None
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        _dev(t, torch.float32, name)
    return t.data_ptr()


# ------------------------------------------------------------------------------------------
class MeshSet:
    """All object models of a dataset, flat and resident in HBM (``gdrnpp_meshes``)."""

    def __init__(self, vertices: list, faces: list, device="cuda"):
        import numpy as np

        assert len(vertices) == len(faces) and len(vertices) > 0
        v_off, f_off = [0], [0]
        for v, f in zip(vertices, faces):
            v_off.append(v_off[-1] + int(len(v)))
            f_off.append(f_off[-1] + int(len(f)))
        self.n_obj = len(vertices)
        self.verts = torch.from_numpy(np.ascontiguousarray(np.concatenate(vertices, 0), np.float32)).to(device)
        self.faces = torch.from_numpy(np.ascontiguousarray(np.concatenate(faces, 0), np.int32)).to(device)
        self.vert_off = torch.tensor(v_off, dtype=torch.int32, device=device)
        self.face_off = torch.tensor(f_off, dtype=torch.int32, device=device)
        self.n_verts = v_off[1:]
        self.n_faces = f_off[1:]
        self._c = gdrnpp_meshes(self.verts.data_ptr(), self.faces.data_ptr(), self.vert_off.data_ptr(),
                                self.face_off.data_ptr(), self.n_obj, max(len(v) for v in vertices),
                                max(len(f) for f in faces))

    @property
    def c(self):
        return ctypes.byref(self._c)

    def bytes_per_render(self, obj: int) -> int:
        return 12 * (self.n_verts[obj] - (self.n_verts[obj - 1] if obj else 0)) + 12 * (
            self.n_faces[obj] - (self.n_faces[obj - 1] if obj else 0))


# ------------------------------------------------------------------------------------------
def fps(pts: torch.Tensor, sn: int, init_center: bool = True, start_idx: torch.Tensor | None = None) -> torch.Tensor:
    """pts f32[b,pn,3] -> idxs i32[b,sn]."""
    lib = load()
    assert pts.dim() == 3 and pts.shape[2] == 3
    b, pn, _ = pts.shape
    idxs = torch.empty((b, sn), dtype=torch.int32, device=pts.device)
    ws_bytes = lib.gdrnpp_fps_workspace_bytes(b, pn)
    ws = torch.empty((max(ws_bytes, 4),), dtype=torch.uint8, device=pts.device)
    sp = _dev(start_idx, torch.int32, "start_idx") if start_idx is not None else None
    _check(lib.gdrnpp_fps(_f32(pts, "pts"), idxs.data_ptr(), sp, b, pn, sn, 1 if init_center else 0, ws.data_ptr(), _stream()), "gdrnpp_fps")
    return idxs


def nnd_forward(xyz1, xyz2, dist1, dist2, idx1, idx2) -> int:
    lib = load()
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    _check(lib.gdrnpp_nnd_forward(_f32(xyz1, "xyz1"), _f32(xyz2, "xyz2"), _f32(dist1, "dist1"), _f32(dist2, "dist2"),
                                  _dev(idx1, torch.int32, "idx1"), _dev(idx2, torch.int32, "idx2"), b, n, m,
                                  _stream()), "gdrnpp_nnd_forward")
    return 1


def nnd_backward(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2) -> int:
    lib = load()
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    _check(lib.gdrnpp_nnd_backward(_f32(xyz1, "xyz1"), _f32(xyz2, "xyz2"), _f32(gradxyz1, "gradxyz1"), _f32(gradxyz2, "gradxyz2"),
                                   _f32(graddist1, "graddist1"), _f32(graddist2, "graddist2"), _dev(idx1, torch.int32, "idx1"),
                                   _dev(idx2, torch.int32, "idx2"), b, n, m, _stream()), "gdrnpp_nnd_backward")
    return 1


def uncertainty_pnp_batched(pts2d, pts3d, wgt2d, K, init_rt, return_info: bool = False):
    lib = load()
    b, pn, _ = pts2d.shape
    out = torch.empty((b, 6), dtype=torch.float64, device=pts2d.device)
    info = torch.zeros((b, 2), dtype=torch.int32, device=pts2d.device)
    _check(lib.gdrnpp_uncertainty_pnp_batched(_dev(pts2d, torch.float64, "pts2d"), _dev(pts3d, torch.float64, "pts3d"),
                                              _dev(wgt2d, torch.float64, "wgt2d"), _dev(K, torch.float64, "K"),
                                              _dev(init_rt, torch.float64, "init_rt"), out.data_ptr(),
                                              info.data_ptr(), b, pn, _stream()), "gdrnpp_uncertainty_pnp_batched")
    return (out, info) if return_info else out


def decode_correspondences(coor_x, coor_y, coor_z, mask_raw, coord2d, extent, im_wh, mask_type: int = 0,
                           mask_thr: float = 0.5, want_mask: bool = True):
    """Maps [b,1,h,w] (or [b,h,w]) -> (count i32[b], sel_idx i32[b,hw], img_pts f32[b,hw,2], mdl_pts f32[b,hw,3],
    out_mask f32[b,1,h,w] | None).  Rows >= count[b] are undefined."""
    lib = load()
    b = coor_x.shape[0]
    hw = coor_x[0].numel()
    dev = coor_x.device
    count = torch.empty((b,), dtype=torch.int32, device=dev)
    sel_idx = torch.empty((b, hw), dtype=torch.int32, device=dev)
    img_pts = torch.empty((b, hw, 2), dtype=torch.float32, device=dev)
    mdl_pts = torch.empty((b, hw, 3), dtype=torch.float32, device=dev)
    out_mask = torch.empty_like(mask_raw) if want_mask else None
    _check(lib.gdrnpp_decode_correspondences(
        _f32(coor_x, "coor_x"), _f32(coor_y, "coor_y"), _f32(coor_z, "coor_z"), _f32(mask_raw, "mask"),
        _f32(coord2d, "coord2d"), _f32(extent, "extent"), _f32(im_wh, "im_wh"), out_mask.data_ptr() if want_mask else None, count.data_ptr(),
        sel_idx.data_ptr(), img_pts.data_ptr(), mdl_pts.data_ptr(), b, hw, mask_type, float(mask_thr), _stream()),
        "gdrnpp_decode_correspondences")
    return count, sel_idx, img_pts, mdl_pts, out_mask


def pose_from_pred_centroid_z(rot6d, t_, cams, centers, whs, resize_ratios, z_type: str = "REL", is_allo: bool = True):
    lib = load()
    b = rot6d.shape[0]
    rot = torch.empty((b, 3, 3), dtype=torch.float32, device=rot6d.device)
    trans = torch.empty((b, 3), dtype=torch.float32, device=rot6d.device)
    _check(lib.gdrnpp_pose_from_pred_centroid_z(
        _f32(rot6d, "rot6d"), _f32(t_, "t_"), _f32(cams, "cams"), _f32(centers, "centers"), _f32(whs, "whs"),
        _f32(resize_ratios, "resize_ratios"), rot.data_ptr(), trans.data_ptr(), b,
        {"REL": 0, "ABS": 1}[z_type], 1 if is_allo else 0, _stream()), "gdrnpp_pose_from_pred_centroid_z")
    return rot, trans


def pose_from_pred(rot_in, t_, cams, centers=None, whs=None, resize_ratios=None, rot_mode: str = "rot6d",
                   t_mode: str = "centroid_z_rel", is_allo: bool = True):
    """``gdrnpp_pose_from_pred``: every ROT_TYPE (rot6d / quat / log_quat / lie_vec / matrix) x TRANS_TYPE (centroid_z REL or
    ABS, centroid_z_abs, trans) combination of GDRN_double_mask.py:162-200 -> (R_ego f32[b,3,3], t f32[b,3])."""
    b = rot_in.shape[0]
    rot = torch.empty((b, 3, 3), dtype=torch.float32, device=rot_in.device)
    trans = torch.empty((b, 3), dtype=torch.float32, device=rot_in.device)
    rm, tm = ROT_MODES[rot_mode], T_MODES[t_mode]
    _check(load().gdrnpp_pose_from_pred(_f32(rot_in, "rot_in"), rm, _f32(t_, "t_"), tm,
                                        _f32(cams, "cams"), _opt_f32(centers, "centers"), _opt_f32(whs, "whs"),
                                        _opt_f32(resize_ratios, "resize_ratios"), rot.data_ptr(), trans.data_ptr(), b,
                                        1 if is_allo else 0, _stream()), "gdrnpp_pose_from_pred")
    return rot, trans


def zoom_K(K, centers, scales, out_res: float):
    lib = load()
    b = K.shape[0]
    out = torch.empty_like(K)
    _check(lib.gdrnpp_zoom_K(_f32(K, "K"), _f32(centers, "centers"), _f32(scales, "scales"), out.data_ptr(), b, float(out_res), _stream()),
           "gdrnpp_zoom_K")
    return out


def render_depth(meshes: MeshSet, obj, K, R, t, res: int, z_near: float = 0.1, z_far: float = 100.0,
                 want_xyz: bool = False):
    lib = load()
    b = obj.shape[0]
    depth = torch.empty((b, res, res), dtype=torch.float32, device=obj.device)
    xyz = torch.empty((b, res, res, 3), dtype=torch.float32, device=obj.device) if want_xyz else None
    _check(lib.gdrnpp_render_depth(meshes.c, _dev(obj, torch.int32, "obj"), _f32(K, "K"), _f32(R, "R"), _f32(t, "t"), depth.data_ptr(),
                                   xyz.data_ptr() if want_xyz else None, b, res, z_near, z_far, _stream()),
           "gdrnpp_render_depth")
    return (depth, xyz) if want_xyz else depth


def _refine_workspace(meshes: MeshSet, b: int, device):
    nbytes = load().gdrnpp_depth_refine_workspace_bytes(meshes.c, b)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=device) if nbytes else None
    return ws, nbytes


def depth_refine(meshes: MeshSet, obj, coor_x, coor_y, coor_z, mask_raw, roi_depth, K_crop, R, t, res: int = 64,
                 iters: int = 2, threshold: float = 0.8, mask_type: int = 0, use_coor_z: bool = False,
                 z_near: float = 0.1, z_far: float = 100.0, debug: bool = False, out: torch.Tensor | None = None):
    """-> t_refined f64[b,3] (and the per-iteration renders f32[b,iters,res,res] when debug)."""
    lib = load()
    b = obj.shape[0]
    t_out = out if out is not None else torch.empty((b, 3), dtype=torch.float64, device=obj.device)
    dbg = torch.zeros((b, iters, res, res), dtype=torch.float32, device=obj.device) if debug else None
    if roi_depth.shape[-1] != roi_depth.shape[-2]:
        raise RuntimeError(f"depth_refine: roi_depth must be square, got {tuple(roi_depth.shape[-2:])}")
    ws, nbytes = _refine_workspace(meshes, b, obj.device)
    ev = None
    if _REFINE_EVENT_SINK is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _check(lib.gdrnpp_depth_refine(
        meshes.c, _dev(obj, torch.int32, "obj"), _f32(coor_x, "coor_x"), _f32(coor_y, "coor_y"), _f32(coor_z, "coor_z"),
        _f32(mask_raw, "mask"), _f32(roi_depth, "roi_depth"), _f32(K_crop, "K_crop"), _f32(R, "R"), _f32(t, "t"),
        _dev(t_out, torch.float64, "t_out"), dbg.data_ptr() if debug else None, b, res, int(roi_depth.shape[-1]), iters,
        float(threshold), mask_type, 1 if use_coor_z else 0, z_near, z_far, ws.data_ptr() if ws is not None else None, nbytes,
        _stream()), "gdrnpp_depth_refine")
    if ev is not None:
        ev[1].record()
        _REFINE_EVENT_SINK.append(ev)
    return (t_out, dbg) if debug else t_out


def refine_to_records(meshes: MeshSet, obj, coor_x, coor_y, coor_z, mask_raw, roi_depth, cam, center, scale, R, t, score=None,
                      roi_id=None, res: int = 64, iters: int = 2, threshold: float = 0.8, mask_type: int = 0,
                      use_coor_z: bool = False, z_near: float = 0.1, z_far: float = 100.0):
    """The refine configuration's post-processing tail in ONE launch (``gdrnpp_refine_to_records``): K_crop from cam /
    center / scale, the depth refinement, and the f32[b,16] pose records."""
    lib = load()
    b = obj.shape[0]
    rec = torch.empty((b, 16), dtype=torch.float32, device=obj.device)
    if b == 0:
        return rec
    ws, nbytes = _refine_workspace(meshes, b, obj.device)
    ev = None
    if _REFINE_EVENT_SINK is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    _check(lib.gdrnpp_refine_to_records(
        meshes.c, _dev(obj, torch.int32, "obj"), _f32(coor_x, "coor_x"), _f32(coor_y, "coor_y"),
        _f32(coor_z, "coor_z"), _f32(mask_raw, "mask"), _f32(roi_depth, "roi_depth"), _f32(cam, "cam"), _f32(center, "center"), _f32(scale, "scale"),
        _f32(R, "R"), _f32(t, "t"), _opt_f32(score, "score"),
        _dev(roi_id, torch.int32, "roi_id") if roi_id is not None else None, rec.data_ptr(), b, res, int(roi_depth.shape[-1]),
        iters, float(threshold), mask_type, 1 if use_coor_z else 0, z_near, z_far, ws.data_ptr() if ws is not None else None,
        nbytes, _stream()), "gdrnpp_refine_to_records")
    if ev is not None:
        ev[1].record()
        _REFINE_EVENT_SINK.append(ev)
    return rec


_REFINE_EVENT_SINK = None


def set_refine_event_sink(sink):
    """bench.py's roofline pass: a list that receives one (start, stop) HIP event pair per depth-refine launch, recorded
    on the launch stream (torch's current stream); None switches it off."""
    global _REFINE_EVENT_SINK
    _REFINE_EVENT_SINK = sink


def refine_kernel_name() -> str:
    return "depth_refine_kernel"


def pack_pose_records(R, t_refined, t_net, score, obj_id, roi_id):
    lib = load()
    b = R.shape[0]
    rec = torch.empty((b, 16), dtype=torch.float32, device=R.device)
    _check(lib.gdrnpp_pack_pose_records(
        _f32(R, "R"), _dev(t_refined, torch.float64, "t_refined") if t_refined is not None else None,
        _opt_f32(t_net, "t_net"), _opt_f32(score, "score"), _dev(obj_id, torch.int32, "obj_id") if obj_id is not None else None,
        _dev(roi_id, torch.int32, "roi_id") if roi_id is not None else None, rec.data_ptr(), b, _stream()),
        "gdrnpp_pack_pose_records")
    return rec


# ------------------------------------------------------------------------------------------
# network-side NHWC layers (tensors are logically NCHW with channels_last strides)
# ------------------------------------------------------------------------------------------
def _nhwc(t: torch.Tensor, name: str) -> int:
    if not t.is_cuda or t.dtype != torch.float32 or t.dim() != 4:
        raise RuntimeError(f"{name} must be a 4-D float32 CUDA(HIP) tensor")
    if not t.is_contiguous(memory_format=torch.channels_last):
        raise RuntimeError(f"{name} must be channels_last contiguous")
    return t.data_ptr()


def dwconv7x7_ln(x, w49c, bias, ln_w=None, ln_b=None, eps: float = 1e-6, y_rows: bool = False):
    """x (N,C,H,W) channels_last -> depthwise 7x7 (+ LayerNorm over C), same shape/format.  ``y_rows``: the result is written as an
    "f16x2 rows" tensor (include/gdrnpp_hip.h: every 8 consecutive channels of a pixel replaced by their fp16 h and l halves) for
    ``linear_f32_split(..., a_rows=True)`` — same shape and dtype, NOT readable as floats."""
    n, c, h, w = x.shape
    y = torch.empty_like(x, memory_format=torch.channels_last)
    args = (_nhwc(x, "x"), _f32(w49c, "w49c"), _f32(bias, "bias"),
            _opt_f32(ln_w, "ln_w"), _opt_f32(ln_b, "ln_b"), y.data_ptr(), n, h, w, c, float(eps), int(bool(y_rows)), _stream())
    _check(_timed("hbm:dwconv7_ln", 0.0, lambda: load().gdrnpp_dwconv7x7_ln_nhwc_rows(*args), 8.0 * x.numel()),
           "gdrnpp_dwconv7x7_ln_nhwc")
    return y


A_F16X2_ROWS, C_F16X2_ROWS = 1, 2      # include/gdrnpp_hip.h


def f16x2_rows_decode(t: torch.Tensor) -> tuple[torch.Tensor, torch.Tensor]:
    """(h, l) as float16 tensors of ``t``'s shape from an "f16x2 rows" tensor (tests / debugging): x ~ h + l."""
    k = t.shape[-1]
    v = t.contiguous().view(torch.float16).view(*t.shape[:-1], k // 8, 2, 8)
    return v[..., 0, :].reshape(t.shape), v[..., 1, :].reshape(t.shape)


def layernorm_nhwc(x, weight, bias, eps: float = 1e-6):
    """x (N,C,H,W) channels_last -> LayerNorm over C per pixel, same shape/format."""
    n, c, h, w = x.shape
    y = torch.empty_like(x, memory_format=torch.channels_last)
    args = (_nhwc(x, "x"), _f32(weight, "weight"), _f32(bias, "bias"), y.data_ptr(), n * h * w, c, float(eps), _stream())
    _check(_timed("hbm:layernorm", 0.0, lambda: load().gdrnpp_layernorm_nhwc(*args), 8.0 * x.numel()), "gdrnpp_layernorm_nhwc")
    return y


def upsample_bilinear2x(x):
    n, c, h, w = x.shape
    y = torch.empty((n, c, 2 * h, 2 * w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    args = (_nhwc(x, "x"), y.data_ptr(), n, h, w, c, _stream())
    _check(_timed("hbm:upsample2x", 0.0, lambda: load().gdrnpp_upsample_bilinear2x_nhwc(*args), 20.0 * x.numel()),
           "gdrnpp_upsample_bilinear2x_nhwc")
    return y


def groupnorm_act(x, gamma, beta, groups: int, eps: float = 1e-5, gelu: bool = False):
    n, c, h, w = x.shape
    y = torch.empty_like(x, memory_format=torch.channels_last)
    ws = torch.empty((load().gdrnpp_groupnorm_workspace_bytes(n, h * w, groups),), dtype=torch.uint8, device=x.device)
    args = (_nhwc(x, "x"), _f32(gamma, "gamma"), _f32(beta, "beta"), y.data_ptr(),
            ws.data_ptr(), n, h * w, c, groups, float(eps), 1 if gelu else 0, _stream())
    _check(_timed("hbm:groupnorm", 0.0, lambda: load().gdrnpp_groupnorm_act_nhwc(*args), 12.0 * x.numel()),   # read twice, write once
           "gdrnpp_groupnorm_act_nhwc")
    return y


def crop_resize_roi(images, depths, im_idx, centers, scales, out_res: int = 256, out_res_small: int = 64,
                    pixel_mean=(0.0, 0.0, 0.0), pixel_std=(255.0, 255.0, 255.0), want_img=True, want_coord2d=True):
    """GPU ROI preparation (read_data_test, data_loader.py:754-797).  images u8[n_im,H,W,3] BGR, depths f32[n_im,H,W]
    or None, im_idx i32[b] or None, centers f64[b,2], scales f64[b] ->
    (roi_img f32[b,3,out,out] | None, roi_depth f32[b,1,out,out] | None, roi_coord_2d f32[b,2,os,os] | None)."""
    lib = load()
    n_im, H, W, _ = images.shape
    b = centers.shape[0]
    dev = images.device
    roi_img = torch.empty((b, 3, out_res, out_res), dtype=torch.float32, device=dev) if want_img else None
    roi_depth = torch.empty((b, 1, out_res, out_res), dtype=torch.float32, device=dev) if depths is not None else None
    roi_c2d = (torch.empty((b, 2, out_res_small, out_res_small), dtype=torch.float32, device=dev)
               if want_coord2d else None)
    mean = (ctypes.c_double * 3)(*[float(v) for v in pixel_mean])
    std = (ctypes.c_double * 3)(*[float(v) for v in pixel_std])
    _check(lib.gdrnpp_crop_resize_roi(
        _dev(images, torch.uint8, "images"), _opt_f32(depths, "depths"),
        n_im, H, W, _dev(im_idx, torch.int32, "im_idx") if im_idx is not None else None,
        _dev(centers, torch.float64, "centers"), _dev(scales, torch.float64, "scales"),
        roi_img.data_ptr() if want_img else None, roi_depth.data_ptr() if roi_depth is not None else None,
        roi_c2d.data_ptr() if want_coord2d else None, b, out_res, out_res_small,
        ctypes.cast(mean, c_void_p), ctypes.cast(std, c_void_p), _stream()), "gdrnpp_crop_resize_roi")
    return roi_img, roi_depth, roi_c2d


def roi_align(x, rois, output_size, spatial_scale: float = 1.0, sampling_ratio: int = 0, aligned: bool = True):
    """detectron2.layers.ROIAlign(output_size, spatial_scale, sampling_ratio, aligned)(x, rois): x f32[B,C,H,W] (NCHW
    contiguous), rois f32[N,5] -> f32[N,C,oh,ow]."""
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else output_size
    bsz, c, h, w = x.shape
    n = rois.shape[0]
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    _check(load().gdrnpp_roi_align(_f32(x, "x"), _f32(rois, "rois"), out.data_ptr(), n, c,
                                   h, w, oh, ow, float(spatial_scale), int(sampling_ratio), 1 if aligned else 0,
                                   _stream()), "gdrnpp_roi_align")
    return out


def roi_pool(x, rois, output_size, spatial_scale: float = 1.0):
    """torchvision.ops.RoIPool(output_size, spatial_scale)(x, rois): x f32[B,C,H,W] (NCHW contiguous), rois f32[N,5] ->
    f32[N,C,oh,ow] (max over integer pixel bins)."""
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else output_size
    bsz, c, h, w = x.shape
    n = rois.shape[0]
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    _check(load().gdrnpp_roi_pool(_f32(x, "x"), _f32(rois, "rois"), out.data_ptr(), n, c, h, w,
                                  oh, ow, float(spatial_scale), _stream()), "gdrnpp_roi_pool")
    return out


def pnp_iter_from_correspondences(img_pts, mdl_pts, count, K, R_net, t_net, return_info: bool = False):
    """Net-initialised iterative PnP (gdrn_evaluator.py:241-371, pnp_type="iter") for all ROIs at once."""
    b, stride, _ = img_pts.shape
    R_out = torch.empty((b, 3, 3), dtype=torch.float32, device=img_pts.device)
    t_out = torch.empty((b, 3), dtype=torch.float32, device=img_pts.device)
    info = torch.zeros((b, 2), dtype=torch.int32, device=img_pts.device)
    _check(load().gdrnpp_pnp_iter_from_correspondences(
        _f32(img_pts, "img_pts"), _f32(mdl_pts, "mdl_pts"), _dev(count, torch.int32, "count"),
        stride, _f32(K, "K"), _f32(R_net, "R_net"), _f32(t_net, "t_net"),
        R_out.data_ptr(), t_out.data_ptr(), info.data_ptr(), b, _stream()), "gdrnpp_pnp_iter_from_correspondences")
    return (R_out, t_out, info) if return_info else (R_out, t_out)


def epnp_ransac(img_pts, mdl_pts, count, K, iters: int = 100, reproj_err: float = 3.0, confidence: float = 0.99,
                draws: "torch.Tensor | None" = None):
    """cv2.solvePnPRansac(flags=SOLVEPNP_EPNP) for every ROI (``gdrnpp_epnp_ransac``): img_pts f32[b,stride,2], mdl_pts
    f32[b,stride,3], count i32[b] (``decode_correspondences`` outputs), K f32[b,9|3,3]; ``draws`` i32/u32[b,n] injects the
    random words of the minimal sets (default: OpenCV's fixed-seed cv::RNG).  -> (R f32[b,3,3], t f32[b,3], n_inliers
    i32[b], status i32[b], inlier_mask u8[b,stride])."""
    lib = load()
    b, stride, _ = img_pts.shape
    dev = img_pts.device
    Rm = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((b, 3), dtype=torch.float32, device=dev)
    n_inl = torch.empty((b,), dtype=torch.int32, device=dev)
    status = torch.empty((b,), dtype=torch.int32, device=dev)
    mask = torch.empty((b, stride), dtype=torch.uint8, device=dev)
    if b == 0:
        return Rm, t, n_inl, status, mask
    nbytes = lib.gdrnpp_epnp_ransac_workspace_bytes(b, stride, iters)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    n_draws = 0
    if draws is not None:
        if draws.dtype not in (torch.int32, torch.uint32) or not draws.is_cuda or not draws.is_contiguous() or draws.shape[0] != b:
            raise RuntimeError("draws must be a contiguous 32-bit integer CUDA(HIP) tensor [b, n_words]")
        n_draws = int(draws.shape[1])
    _check(lib.gdrnpp_epnp_ransac(
        _f32(img_pts, "img_pts"), _f32(mdl_pts, "mdl_pts"), _dev(count, torch.int32, "count"),
        stride, _f32(K.reshape(b, 9), "K"), draws.data_ptr() if draws is not None else None, n_draws, int(iters),
        float(reproj_err), float(confidence), Rm.data_ptr(), t.data_ptr(), n_inl.data_ptr(), status.data_ptr(), mask.data_ptr(),
        b, ws.data_ptr(), nbytes, _stream()), "gdrnpp_epnp_ransac")
    return Rm, t, n_inl, status, mask


def epnp_batched(img_pts, mdl_pts, K):
    """Plain EPnP on all n >= 4 points of each problem: img_pts f32[b,n,2], mdl_pts f32[b,n,3], K f32[b,9|3,3]
    -> (R f32[b,3,3], t f32[b,3], status i32[b])."""
    b, n, _ = img_pts.shape
    dev = img_pts.device
    Rm = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((b, 3), dtype=torch.float32, device=dev)
    status = torch.empty((b,), dtype=torch.int32, device=dev)
    _check(load().gdrnpp_epnp_batched(_f32(img_pts, "img_pts"), _f32(mdl_pts, "mdl_pts"), n,
                                      _f32(K.reshape(b, 9), "K"), Rm.data_ptr(), t.data_ptr(), status.data_ptr(),
                                      b, _stream()), "gdrnpp_epnp_batched")
    return Rm, t, status


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


def _timed(kind, flops, fn, nbytes=0.0):
    return _LAUNCH_TIMER.launch(kind, flops, fn, nbytes) if _LAUNCH_TIMER is not None else fn()


def pack_weight_bf16x3(weight):
    """nn.Linear weight f32[N,K] -> bf16[N/128, K/16, 3, 2, 128, 8]: exact 3-way bf16 split (w == h + m + l) of every
    128x16 tile, laid out as gdrnpp_linear_f32_split stages it (split, k-block, row, 8 k)."""
    n, k = weight.shape
    packed = torch.empty((n // 128, k // 16, 3, 2, 128, 8), dtype=torch.bfloat16, device=weight.device)
    _check(load().gdrnpp_pack_weight_bf16x3(_f32(weight, "weight"), packed.data_ptr(), n, k, _stream()),
           "gdrnpp_pack_weight_bf16x3")
    return packed


def pack_weight_f16x2(weight):
    """nn.Linear weight f32[N,K] -> fp16[N/128, K/16, 2, 2, 128, 8]: two-way fp16 split (w * 2^e ~ h + l, 22 significant bits) of
    every 128x16 tile for the three-product kernels (csrc/gemm_split2_pipe.hip).  The returned tensor is a VIEW of a buffer that
    also carries the 16-byte trailer with the power-of-two scale behind the tiles: pass it on as it is (a copy loses the trailer)."""
    n, k = weight.shape
    nbytes = load().gdrnpp_pack_weight_f16x2_bytes(n, k)
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=weight.device)
    _check(load().gdrnpp_pack_weight_f16x2(_f32(weight, "weight"), buf.data_ptr(), n, k, _stream()),
           "gdrnpp_pack_weight_f16x2")
    packed = buf[:n * k * 4].view(torch.float16).view(n // 128, k // 16, 2, 2, 128, 8)
    packed._gdrnpp_base = buf
    return packed


def mlp_fused_supported(c: int, hidden: int) -> bool:
    return load().gdrnpp_pack_mlp_fused_f16x2_bytes(int(c), int(hidden)) > 0


def pack_mlp_fused_f16x2(w1, w2):
    """fc1.weight f32[hidden,C], fc2.weight f32[C,hidden] -> the packed image of ``convnext_mlp_f32_fused`` (u8 buffer: per hidden
    tile of 32 the fp16 h / l fragments of both layers in LDS order + a 32-byte trailer with the two power-of-two scales)."""
    hidden, c = w1.shape
    if tuple(w2.shape) != (c, hidden):
        raise ValueError("pack_mlp_fused_f16x2: fc2.weight must be [C, hidden] for fc1.weight [hidden, C]")
    nbytes = load().gdrnpp_pack_mlp_fused_f16x2_bytes(c, hidden)
    if nbytes == 0:
        raise ValueError(f"the fused MLP exists for C = 128, hidden = 512, not {c} / {hidden}")
    buf = torch.empty((nbytes,), dtype=torch.uint8, device=w1.device)
    _check(load().gdrnpp_pack_mlp_fused_f16x2(_f32(w1, "w1"), _f32(w2, "w2"), buf.data_ptr(), c, hidden, _stream()), "gdrnpp_pack_mlp_fused_f16x2")
    return buf


def mlp_fused_rows_in_range(packed_buf) -> tuple:
    """(fc1 ok, fc2 ok): False when the pack kernel found a non-zero weight row of that layer below the three-product range."""
    tr = packed_buf[-32:].view(torch.int32).cpu()
    return int(tr[3]) == 0, int(tr[7]) == 0


def convnext_mlp_f32_fused(x2d, packed_buf, b1, b2, gamma, resid, slot_fc1: int = 0, slot_fc2: int = 0):
    """y = resid + gamma * fc2(gelu(fc1(x))) in one launch (``gdrnpp_convnext_mlp_f32_fused``, three-product form, C = 128)."""
    m, c = x2d.shape
    hidden = b1.shape[0]
    y = torch.empty((m, c), dtype=torch.float32, device=x2d.device)
    _count_x3()
    args = (_f32(x2d, "x"), packed_buf.data_ptr(), _f32(b1, "b1"), _f32(b2, "b2"),
            _f32(gamma, "gamma"), _f32(resid, "resid"), y.data_ptr(), m, c, hidden, _x3_flag_ptr(slot_fc1), _x3_flag_ptr(slot_fc2), _stream())
    nbytes = 4.0 * m * c * 3 + 8.0 * c * hidden       # x + residual + y, both weights once
    _check(_timed("mlp_fused" + X3, 4.0 * m * c * hidden, lambda: load().gdrnpp_convnext_mlp_f32_fused(*args), nbytes),
           "gdrnpp_convnext_mlp_f32_fused")
    return y


def packed_rows_in_range(packed) -> bool:
    """False when gdrnpp_pack_weight_f16x2 found a non-zero weight row whose scaled rms is below 2^-4 (trailer word 3): the layer
    belongs on the six-product kernels.  One 16-byte read-back, done once per packed weight (x3_policy caches it)."""
    trailer = packed._gdrnpp_base[packed.numel() * 2:].view(torch.int32)
    return int(trailer[3].item()) == 0


def unpack_weight_f16x2(packed):
    """For tests: (fp16[2, N, K] planes h / l of the SCALED weight, 2^-e) of a pack_weight_f16x2 result."""
    tn, tk = packed.shape[:2]
    planes = packed.permute(2, 0, 4, 1, 3, 5).reshape(2, tn * 128, tk * 16)
    trailer = packed._gdrnpp_base[packed.numel() * 2:].view(torch.float32)
    return planes, float(trailer[1])


def pack_conv_weight_f16x2(weight):
    """nn.Conv2d weight [Cout, Cin, KH, KW] -> pack_weight_f16x2 of the (tap, channel)-ordered [Cout, KH*KW*Cin] matrix."""
    cout, cin, kh, kw = weight.shape
    return pack_weight_f16x2(weight.detach().permute(0, 2, 3, 1).reshape(cout, kh * kw * cin).contiguous())


SPLIT2_MIN_TILES = int(os.environ.get("GDRNPP_SPLIT2_MIN_TILES", "256"))   # tests lower it to run the three-product kernels on the 4-ROI reference fixtures; the env var is for A/B runs


# With a second step in flight on another stream (engine.StepStreams) a launch need not fill the chip by itself: from
# SPLIT2_SHARED_MIN_TILES tiles on, if it has at least SPLIT2_SHARED_MIN_ROWS rows (fewer: the 128 x 128-tile six-product kernels stay ahead).
SPLIT2_SHARED_MIN_TILES = int(os.environ.get("GDRNPP_SPLIT2_SHARED_MIN_TILES", "0"))      # 0 = off
SPLIT2_SHARED_MIN_ROWS = int(os.environ.get("GDRNPP_SPLIT2_SHARED_MIN_ROWS", "4096"))


_SHARED_TLS = threading.local()     # .min_tiles: the shared-chip rule of the calling HOST THREAD (engine.StepStreams.next sets it for
                                    # the launches of one step); unset = the process default above.  Two host threads driving
                                    # their own dealers never see each other's setting.


def shared_min_tiles() -> int:
    """The shared-chip tile rule in force for the calling host thread (0 = off)."""
    v = getattr(_SHARED_TLS, "min_tiles", None)
    return SPLIT2_SHARED_MIN_TILES if v is None else v


def shared_min_rows() -> int:
    """Fewest rows of a launch that takes the three-product form under the shared-chip rule, for the calling host thread."""
    v = getattr(_SHARED_TLS, "min_rows", None)
    return SPLIT2_SHARED_MIN_ROWS if v is None else v


class shared_min_tiles_scope:
    """``with shared_min_tiles_scope(n, rows):`` — launches of the calling host thread inside choose their GEMM kernels for a chip
    shared with other steps (three-product 256-row form from ``n`` tiles on, for launches of at least ``rows`` rows); ``None`` =
    leave whatever is in force."""

    def __init__(self, n, rows=None):
        self.n = None if n is None else int(n)
        self.rows = None if rows is None else int(rows)

    def __enter__(self):
        self.prev = getattr(_SHARED_TLS, "min_tiles", None), getattr(_SHARED_TLS, "min_rows", None)
        if self.n is not None:
            _SHARED_TLS.min_tiles = self.n
        if self.rows is not None:
            _SHARED_TLS.min_rows = self.rows
        return self

    def __exit__(self, *exc):
        _SHARED_TLS.min_tiles, _SHARED_TLS.min_rows = self.prev
        return False


def split2_tiles_ok(m: int, n: int) -> bool:
    """The three-product kernels exist as 256-row tiles only: used from 256 tiles of 256 x 128 on (every CU gets a workgroup)."""
    if n % 128:
        return False
    tiles = ((m + 255) // 256) * (n // 128)
    return tiles >= SPLIT2_MIN_TILES or (0 < shared_min_tiles() <= tiles and m >= shared_min_rows())


# Range words of the three-product launches (include/gdrnpp_hip.h: GDRNPP_SPLIT2_NONFINITE | GDRNPP_SPLIT2_SMALL_ROWS).  Every
# (device, stream) owns one i32[X3_SLOTS] device buffer; a launch ORs its word into the entry of its LAYER (slot numbers are
# handed out by x3_policy.slot, slot 0 = launches that name no layer), so that the reader knows which layer left the range.
X3_SLOTS = 1024
X3_NONFINITE, X3_SMALL_ROWS = 1, 2
_X3_FLAGS = {}   # (device index, stream handle) -> i32[X3_SLOTS]


def x3_flags():
    """The range words of the current device + stream (or of the enclosing x3_flag_scope)."""
    if _X3_FLAG_OVERRIDE is not None:
        return _X3_FLAG_OVERRIDE
    key = (torch.cuda.current_device(), _stream())
    f = _X3_FLAGS.get(key)
    if f is None:
        f = _X3_FLAGS[key] = torch.zeros((X3_SLOTS,), dtype=torch.int32, device=f"cuda:{key[0]}")
    return f


def _x3_flag_ptr(slot: int) -> int:
    f = x3_flags()
    return f.data_ptr() + 4 * (slot if 0 <= slot < f.numel() else 0)


_X3_FLAG_OVERRIDE = None


class x3_flag_scope:
    """``with x3_flag_scope(words):`` — three-product launches inside record into ``words`` (i32[X3_SLOTS] device tensor) instead of
    the current stream's: a captured hipGraph must write to words its owner can read after every replay (engine.GraphedInference)."""

    def __init__(self, flag):
        if flag.dtype != torch.int32 or not flag.is_cuda or flag.numel() < 1:
            raise ValueError("x3_flag_scope needs an int32 device tensor")
        self.flag = flag

    def __enter__(self):
        global _X3_FLAG_OVERRIDE
        self.prev, _X3_FLAG_OVERRIDE = _X3_FLAG_OVERRIDE, self.flag
        return self.flag

    def __exit__(self, *exc):
        global _X3_FLAG_OVERRIDE
        _X3_FLAG_OVERRIDE = self.prev
        return False


def range_words_of(host_words) -> dict:
    """{slot: word} of the non-zero entries of a host copy of a range-word buffer."""
    nz = torch.nonzero(host_words).reshape(-1).tolist()
    return {int(i): int(host_words[i]) for i in nz}


def split2_range_words(reset: bool = True) -> dict:
    """{slot: word} of the layers whose three-product launches on the current stream left the fp16x2 range since the last reset
    (empty dict: all inside).  Synchronises the current stream (one X3_SLOTS * 4 byte read-back)."""
    f = x3_flags()
    words = range_words_of(f.cpu())
    if words and reset:
        f.zero_()
    return words


def split2_nonfinite(reset: bool = True) -> bool:
    """True when a three-product kernel launched on the current stream raised ANY bit of its range word since the last reset:
    a stored value / an A element was inf or NaN (activation beyond the fp16 range), or an A row sat below the range (rms < 2^-4).
    The caller repeats the work with the six-product kernels.  Synchronises the current stream."""
    return bool(split2_range_words(reset))


def unpack_weight_bf16x3(packed):
    """Inverse view of pack_weight_bf16x3 for tests: bf16[3, N, K] planes."""
    tn, tk = packed.shape[:2]
    return packed.permute(2, 0, 4, 1, 3, 5).reshape(3, tn * 128, tk * 16)


_X3_LAUNCHES = 0   # launches of the three-product kernels by this process (engine.inference_step: is there a flag to check?)


def x3_launch_count() -> int:
    return _X3_LAUNCHES


def _count_x3():
    global _X3_LAUNCHES
    _X3_LAUNCHES += 1


X3 = "_x3"   # LaunchTimer kind suffix of the three-product (fp16x2) kernels: 3 instead of 6 MFMA flops per fp32-equivalent flop


_EPILOGUES = {"none": 0, "gelu": 1, "scale_res": 2}


def _packed_weight(weight_packed, k: int, what: str, contiguous: bool = False):
    """Validate a packed split-GEMM weight with GEMM depth ``k`` (``contiguous``: and that it is contiguous); returns
    (N, True for the three-product fp16x2 format).  ``what`` is the caller's message."""
    fp16x2 = weight_packed.dtype == torch.float16     # pack_weight_f16x2: the three-product kernel
    if weight_packed.dtype not in (torch.bfloat16, torch.float16) or weight_packed.dim() != 6 \
            or (contiguous and not weight_packed.is_contiguous()) \
            or weight_packed.shape[1] * 16 != k or weight_packed.shape[2] != (2 if fp16x2 else 3):
        raise ValueError(what)
    return weight_packed.shape[0] * 128, fp16x2


def _channels_last_f32(x_cl, what: str):
    if not x_cl.is_contiguous(memory_format=torch.channels_last) or x_cl.dtype != torch.float32 or not x_cl.is_cuda:
        raise ValueError("%s expects a float32 channels_last device tensor" % what)
    return x_cl.shape


def linear_f32_split(x2d, weight_packed, bias, epilogue: str = "none", gamma=None, resid=None, _kind: str = "linear", x3_slot: int = 0,
                     a_rows: bool = False, c_rows: bool = False):
    """out = epilogue(x2d @ W^T + bias) with the weight given as pack_weight_bf16x3(weight); runs on the bf16 matrix cores
    with six partial products per fp32 product (fp32-accurate, see csrc/gemm_split.hip).  With a pack_weight_f16x2 weight: the
    three-product kernel; there ``a_rows`` = x2d is an "f16x2 rows" tensor (epilogues gelu / scale_res), ``c_rows`` = write the
    result as one (epilogues none / gelu) — gdrnpp_linear_f32_split2_rows, bit-identical to the fp32 hand-over."""
    m, k = x2d.shape
    n, fp16x2 = _packed_weight(weight_packed, k, "weight_packed must be the contiguous tensor from pack_weight_bf16x3 / pack_weight_f16x2 with matching K",
                               contiguous=True)
    out = torch.empty((m, n), dtype=torch.float32, device=x2d.device)
    args = (_f32(x2d, "x"), weight_packed.data_ptr(),
            _opt_f32(bias, "bias"), _opt_f32(gamma, "gamma"), _opt_f32(resid, "resid"), out.data_ptr(), m, n, k,
            _EPILOGUES[epilogue]) + \
        (((A_F16X2_ROWS if a_rows else 0) | (C_F16X2_ROWS if c_rows else 0), _x3_flag_ptr(x3_slot)) if fp16x2 else ()) + (_stream(),)
    if (a_rows or c_rows) and not fp16x2:
        raise ValueError("f16x2-rows tensors exist for the three-product kernel (pack_weight_f16x2) only")
    nbytes = 4.0 * m * k + (4.0 if fp16x2 else 6.0) * n * k + 4.0 * m * n * (2 if epilogue == "scale_res" else 1)
    if fp16x2:
        _count_x3()
        _check(_timed(_kind + X3, 2.0 * m * n * k, lambda: load().gdrnpp_linear_f32_split2_rows(*args), nbytes), "gdrnpp_linear_f32_split2")
    else:
        _check(_timed(_kind, 2.0 * m * n * k, lambda: load().gdrnpp_linear_f32_split(*args), nbytes), "gdrnpp_linear_f32_split")
    return out


def linear_f32_split_grouped(x2d, weight_packed_stack, bias_stack, group_sel, rows_per_group: int, n_store: int | None = None):
    """out[m] = x2d[m] @ W[sel[m // rows_per_group]]^T + bias[sel[...]]: the class-sliced output layer of the geometry head.
    ``weight_packed_stack`` = pack_weight_bf16x3 of the slices stacked along N ([groups * N, K]), ``bias_stack`` f32[groups, N],
    ``group_sel`` i32[M / rows_per_group].  Returns f32[M, N]; columns >= n_store are left unwritten.  Rows whose selector is
    outside [0, groups) come back as NaN (nothing is read out of bounds)."""
    m, k = x2d.shape
    n = bias_stack.shape[1]
    if weight_packed_stack.dtype != torch.bfloat16 or weight_packed_stack.dim() != 6 or weight_packed_stack.shape[1] * 16 != k \
            or (weight_packed_stack.shape[0] * 128) % n:
        raise ValueError("weight_packed_stack must come from pack_weight_bf16x3 of the stacked [groups*N, K] weight")
    out = torch.empty((m, n), dtype=torch.float32, device=x2d.device)
    args = (_f32(x2d, "x"), weight_packed_stack.data_ptr(), _f32(bias_stack, "bias_stack"),
            _dev(group_sel, torch.int32, "group_sel"), int(bias_stack.shape[0]), int(rows_per_group), out.data_ptr(), m, n, k,
            int(n_store if n_store is not None else n), _stream())
    nbytes = 4.0 * m * k + 6.0 * n * k * group_sel.numel() + 4.0 * m * (n_store or n)
    _check(_timed("linear_grouped", 2.0 * m * n * k, lambda: load().gdrnpp_linear_f32_split_grouped(*args), nbytes),
           "gdrnpp_linear_f32_split_grouped")
    return out


def stem_conv4x4_ln(x_nchw, weight, bias, ln_weight, ln_bias, eps: float):
    """ConvNeXt stem in one kernel: Conv2d(3 -> 128, 4x4/4) + bias + LayerNorm2d; NCHW image in, channels_last [N,128,H/4,W/4] out."""
    n, cin, h, w = x_nchw.shape
    cout = weight.shape[0]
    out = torch.empty((n, cout, h // 4, w // 4), dtype=torch.float32, device=x_nchw.device, memory_format=torch.channels_last)
    _check(load().gdrnpp_stem_conv4x4_ln(_f32(x_nchw, "x"), _f32(weight, "weight"),
                                         _opt_f32(bias, "bias"), _f32(ln_weight, "ln_weight"), _f32(ln_bias, "ln_bias"),
                                         out.data_ptr(), n, h, w, cout, float(eps), _stream()), "gdrnpp_stem_conv4x4_ln")
    return out


def head_tail_nhwc(out_nhwc, coord2d, extents, double_mask: bool):
    """Tail of the geometry head on the NHWC result [B*HW, pitch] of the class-sliced output layer: returns
    (pnp_in f32[B, HW, 96] — Patch-PnP's input, NHWC with Cin padded to 96 — and planes f32[P, B, HW]: vis, (full,) x, y, z)."""
    b = coord2d.shape[0]
    hw = coord2d.shape[2] * coord2d.shape[3]
    pitch = out_nhwc.shape[1]
    n_planes = 5 if double_mask else 4
    pnp_in = torch.empty((b, hw, 96), dtype=torch.float32, device=out_nhwc.device)
    planes = torch.empty((n_planes, b, hw), dtype=torch.float32, device=out_nhwc.device)
    _check(load().gdrnpp_head_tail_nhwc(_f32(out_nhwc, "out_nhwc"), pitch, _f32(coord2d, "coord2d"),
                                        _f32(extents, "extents"), pnp_in.data_ptr(), planes.data_ptr(), b, hw,
                                        1 if double_mask else 0, _stream()), "gdrnpp_head_tail_nhwc")
    return pnp_in, planes


def linear_f32_splitk(x2d, weight_packed, bias, epilogue: str = "none", gamma=None, resid=None):
    """Same contract as linear_f32_split for problems with few output tiles: split-K with a deterministic reduction that
    also applies bias and epilogue."""
    m, k = x2d.shape
    if weight_packed.dtype != torch.bfloat16 or weight_packed.dim() != 6 or weight_packed.shape[1] * 16 != k:   # six-product only
        raise ValueError("weight_packed must be the contiguous bf16 tensor from pack_weight_bf16x3 with matching K")
    n = weight_packed.shape[0] * 128
    out = torch.empty((m, n), dtype=torch.float32, device=x2d.device)
    nbytes = load().gdrnpp_linear_f32_splitk_workspace_bytes(m, n, k)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=x2d.device)
    args = (_f32(x2d, "x"), weight_packed.data_ptr(), _opt_f32(bias, "bias"), _opt_f32(gamma, "gamma"),
            _opt_f32(resid, "resid"), out.data_ptr(), m, n, k,
            _EPILOGUES[epilogue], ws.data_ptr(), nbytes, _stream())
    nb = 4.0 * m * k + 6.0 * n * k + 4.0 * m * n * (2 if epilogue == "scale_res" else 1)
    _check(_timed("linear_splitk", 2.0 * m * n * k, lambda: load().gdrnpp_linear_f32_splitk(*args), nb), "gdrnpp_linear_f32_splitk")
    return out


def split_gemm_tiles(m: int, n: int) -> int:
    """Output tiles (128x128) of an [m, n] result — the dispatch quantity between the plain and the split-K launch."""
    return ((m + 127) // 128) * (n // 128)


def pack_conv_weight_bf16x3(weight):
    """nn.Conv2d weight f32[Cout,Cin,KH,KW] -> packed split image of the [Cout, (ky,kx,Cin)] GEMM weight."""
    cout, cin, kh, kw = weight.shape
    return pack_weight_bf16x3(weight.permute(0, 2, 3, 1).reshape(cout, kh * kw * cin).contiguous())


pack_conv3x3_weight_bf16x3 = pack_conv_weight_bf16x3


_CONV_SPLITK = True


def set_conv_splitk(flag: bool) -> None:
    """A/B switch: convolutions with too few output tiles for the chip run split-K (default) or as one launch."""
    global _CONV_SPLITK
    _CONV_SPLITK = bool(flag)


def conv2d_f32_split(x_cl, weight_packed, bias, kh: int, kw: int, stride: int, pad: int, gelu: bool = False, _kind: str = "conv",
                     x3_slot: int = 0):
    """KHxKW / stride / zero-pad convolution of a channels_last tensor [N,Cin,H,W] on the bf16 matrix cores (fp32-accurate
    split GEMM, implicit im2col) -> channels_last [N,Cout,OH,OW]."""
    n, cin, h, w = _channels_last_f32(x_cl, "conv2d_f32_split")
    cout, fp16x2 = _packed_weight(weight_packed, kh * kw * cin, "weight_packed must come from pack_conv_weight_bf16x3 / pack_conv_weight_f16x2 with matching Cin and kernel size")
    oh, ow = (h + 2 * pad - kh) // stride + 1, (w + 2 * pad - kw) // stride + 1
    out = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x_cl.device, memory_format=torch.channels_last)
    if fp16x2:
        if kh * kw > 32:
            raise ValueError("the three-product convolution takes at most 32 taps")
        _count_x3()
        a2 = (x_cl.data_ptr(), weight_packed.data_ptr(), _opt_f32(bias, "bias"),
              out.data_ptr(), n, h, w, cin, cout, kh, kw, stride, pad, 1 if gelu else 0, _x3_flag_ptr(x3_slot), _stream())
        _check(_timed(_kind + X3, 2.0 * n * oh * ow * cout * kh * kw * cin, lambda: load().gdrnpp_conv2d_f32_split2(*a2),
                      4.0 * n * (h * w * cin + oh * ow * cout) + 4.0 * cout * kh * kw * cin), "gdrnpp_conv2d_f32_split2")
        return out
    args = (x_cl.data_ptr(), weight_packed.data_ptr(), _opt_f32(bias, "bias"),
            out.data_ptr(), n, h, w, cin, cout, kh, kw, stride, pad, 1 if gelu else 0)
    nbytes = 4.0 * n * (h * w * cin + oh * ow * cout) + 6.0 * cout * kh * kw * cin
    flops = 2.0 * n * oh * ow * cout * kh * kw * cin
    ws_bytes = load().gdrnpp_conv2d_f32_splitk_workspace_bytes(n, oh, ow, cin, cout, kh, kw) if _CONV_SPLITK else 0
    if ws_bytes:    # few output tiles (small ROI batches): K in chunks, partial sums through a workspace
        ws = torch.empty((ws_bytes,), dtype=torch.uint8, device=x_cl.device)
        _check(_timed("conv_splitk", flops, lambda: load().gdrnpp_conv2d_f32_splitk(*args, ws.data_ptr(), ws_bytes, _stream()), nbytes),
               "gdrnpp_conv2d_f32_splitk")
    else:
        _check(_timed(_kind, flops, lambda: load().gdrnpp_conv2d_f32_split(*args, _stream()), nbytes), "gdrnpp_conv2d_f32_split")
    return out


def conv3x3_f32_split(x_cl, weight_packed, bias, gelu: bool = False, x3_slot: int = 0):
    """3x3 / stride 1 / pad 1 convolution of a channels_last tensor [N,Cin,H,W] on the bf16 matrix cores (fp32-accurate
    split GEMM, implicit im2col) -> channels_last [N,Cout,H,W] (gdrnpp_conv3x3_f32_split = the general entry with 3, 3, 1, 1)."""
    return conv2d_f32_split(x_cl, weight_packed, bias, 3, 3, 1, 1, gelu, _kind="conv3x3", x3_slot=x3_slot)


def bias_act_nhwc_(x_cl, bias, resid=None, relu: bool = True):
    """In place: x = act(x + bias[c] (+ resid)) on a channels_last float32 tensor [N,C,H,W] (C % 4 == 0)."""
    n, c, h, w = _channels_last_f32(x_cl, "bias_act_nhwc_")
    if resid is not None and (resid.shape != x_cl.shape or not resid.is_contiguous(memory_format=torch.channels_last)
                              or resid.dtype != torch.float32 or resid.device != x_cl.device):
        raise ValueError("resid must match x (float32, channels_last, same device)")
    _check(load().gdrnpp_bias_act_nhwc(x_cl.data_ptr(), _f32(bias, "bias"),
                                       resid.data_ptr() if resid is not None else None, x_cl.data_ptr(), n * h * w, c,
                                       1 if relu else 0, _stream()), "gdrnpp_bias_act_nhwc")
    return x_cl


def pack_deconv_weight_bf16x3(weight):
    """nn.ConvTranspose2d weight [Cin, Cout, KS, KS] -> packed GEMM weight with rows (ky, kx, co), K = Cin."""
    cin, cout, kh, kw = weight.shape
    return pack_weight_bf16x3(weight.detach().permute(2, 3, 1, 0).reshape(kh * kw * cout, cin).contiguous())


def pack_deconv_weight_f16x2(weight):
    """pack_deconv_weight_bf16x3 in the three-product format."""
    cin, cout, kh, kw = weight.shape
    return pack_weight_f16x2(weight.detach().permute(2, 3, 1, 0).reshape(kh * kw * cout, cin).contiguous())


def _deconv_cols(x_cl, weight_packed, ks: int, stride: int, pad: int, out_pad: int, x3_slot: int, what: str):
    """First half of a transposed convolution: the GEMM into ``cols`` [N*H*W, KS*KS*Cout] and the empty channels_last result
    the col2im gather fills; returns (cols, y, cout, oh, ow)."""
    n, cin, h, w = _channels_last_f32(x_cl, what)
    cout = weight_packed.shape[0] * 128 // (ks * ks)
    cols = linear_f32_split(x_cl.permute(0, 2, 3, 1).reshape(n * h * w, cin), weight_packed, None, _kind="deconv", x3_slot=x3_slot)
    oh, ow = (h - 1) * stride - 2 * pad + ks + out_pad, (w - 1) * stride - 2 * pad + ks + out_pad
    y = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x_cl.device, memory_format=torch.channels_last)
    return cols, y, cout, oh, ow


def conv_transpose2d_f32_split(x_cl, weight_packed, bias, ks: int, stride: int, pad: int, out_pad: int, x3_slot: int = 0):
    """nn.ConvTranspose2d of a channels_last tensor [N,Cin,H,W] as split GEMM + col2im gather -> channels_last
    [N,Cout,OH,OW] (``weight_packed`` from pack_deconv_weight_bf16x3)."""
    n, _, h, w = x_cl.shape
    cols, y, cout, _, _ = _deconv_cols(x_cl, weight_packed, ks, stride, pad, out_pad, x3_slot, "conv_transpose2d_f32_split")
    _check(load().gdrnpp_deconv_col2im_nhwc(cols.data_ptr(), _opt_f32(bias, "bias"),
                                            y.data_ptr(), n, h, w, cout, ks, stride, pad, out_pad, _stream()),
           "gdrnpp_deconv_col2im_nhwc")
    return y


def conv_transpose2d_groupnorm_act(x_cl, weight_packed, bias, ks: int, stride: int, pad: int, out_pad: int, gamma, beta, groups: int,
                                   eps: float = 1e-5, gelu: bool = False, x3_slot: int = 0):
    """nn.ConvTranspose2d -> GroupNorm(groups) [-> GELU] of a channels_last tensor: split GEMM, then the col2im gather leaves the
    GroupNorm partial sums (``gdrnpp_deconv_col2im_gn_nhwc``) and the norm is one more pass (``gdrnpp_groupnorm_apply_nhwc``) —
    bitwise the result of conv_transpose2d_f32_split + groupnorm_act, one launch fewer."""
    n, _, h, w = x_cl.shape
    cols, y, cout, oh, ow = _deconv_cols(x_cl, weight_packed, ks, stride, pad, out_pad, x3_slot, "conv_transpose2d_groupnorm_act")
    nbytes = load().gdrnpp_groupnorm_workspace_bytes(n, oh * ow, groups)
    P = nbytes // (16 * n * groups)
    part = torch.empty((n, P, groups, 2), dtype=torch.float64, device=x_cl.device)
    _check(load().gdrnpp_deconv_col2im_gn_nhwc(cols.data_ptr(), _opt_f32(bias, "bias"),
                                               y.data_ptr(), part.data_ptr(), n, h, w, cout, ks, stride, pad, out_pad, groups, _stream()),
           "gdrnpp_deconv_col2im_gn_nhwc")
    out = torch.empty_like(y)
    a2 = (y.data_ptr(), part.data_ptr(), P, _f32(gamma, "gamma"), _f32(beta, "beta"),
          out.data_ptr(), n, oh * ow, cout, groups, float(eps), 1 if gelu else 0, _stream())
    _check(_timed("hbm:groupnorm_apply", 0.0, lambda: load().gdrnpp_groupnorm_apply_nhwc(*a2), 8.0 * y.numel()),
           "gdrnpp_groupnorm_apply_nhwc")
    return out


def pnp_fc_heads(x, w_r, b_r, w_t, b_t):
    """Patch-PnP's output layers in one launch (``gdrnpp_pnp_fc_heads``): x f32[b,K] -> (fc_r(x) f32[b,rot_dim], fc_t(x) f32[b,3])."""
    b, k = x.shape
    rot_dim = w_r.shape[0]
    rot_ = torch.empty((b, rot_dim), dtype=torch.float32, device=x.device)
    t_ = torch.empty((b, 3), dtype=torch.float32, device=x.device)
    _check(load().gdrnpp_pnp_fc_heads(_f32(x, "x"), _f32(w_r, "w_r"), _opt_f32(b_r, "b_r"), _f32(w_t, "w_t"),
                                      _opt_f32(b_t, "b_t"), rot_.data_ptr(), t_.data_ptr(),
                                      b, k, rot_dim, _stream()), "gdrnpp_pnp_fc_heads")
    return rot_, t_


POINT_PNP_TILE = 128     # points per workgroup of gdrnpp_point_pnp_pool: hw must be a multiple


def point_pnp_pool(x2d, cin: int, w1, b1, w2, b2, w3, b3, b: int, hw: int, want_pooled: bool = True):
    """SimplePointPnPNet's point-wise MLP + max over the points (``gdrnpp_point_pnp_pool``): x2d f32[b*hw, pitch] (NHWC rows, the
    first ``cin`` channels used), Conv1d weights w1 [128,cin(,1)], w2 [128,128(,1)], w3 [1024,128(,1)] with their biases
    -> (pooled f32[b,1024] or None, workspace holding the per-tile maxima for ``point_pnp_fc``)."""
    if x2d.dim() != 2 or x2d.shape[0] != b * hw:
        raise RuntimeError(f"point_pnp_pool: x2d must be [b*hw, pitch] = [{b * hw}, pitch], got {tuple(x2d.shape)}")
    if tuple(w1.shape[:2]) != (128, cin) or tuple(w2.shape[:2]) != (128, 128) or tuple(w3.shape[:2]) != (1024, 128) \
            or w1.numel() != 128 * cin or w2.numel() != 128 * 128 or w3.numel() != 1024 * 128 \
            or b1.numel() != 128 or b2.numel() != 128 or b3.numel() != 1024:
        raise RuntimeError("point_pnp_pool: weights must be Conv1d(cin,128,1), Conv1d(128,128,1), Conv1d(128,1024,1) with biases")
    lib = load()
    nbytes = lib.gdrnpp_point_pnp_workspace_bytes(b, hw)
    if nbytes == 0:
        raise RuntimeError(f"point_pnp_pool: b={b} hw={hw}: hw must be a positive multiple of {POINT_PNP_TILE}")
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x2d.device)
    pooled = torch.empty((b, 1024), dtype=torch.float32, device=x2d.device) if want_pooled else None
    a = (_f32(x2d, "x"), x2d.shape[1], cin, _f32(w1, "w1"), _f32(b1, "b1"), _f32(w2, "w2"), _f32(b2, "b2"), _f32(w3, "w3"), _f32(b3, "b3"),
         pooled.data_ptr() if want_pooled else None, b, hw, ws.data_ptr(), nbytes, _stream())
    _check(_timed("mfma_f32:point_pnp_pool", 2.0 * b * hw * (128 * cin + 128 * 128 + 1024 * 128), lambda: lib.gdrnpp_point_pnp_pool(*a)),
           "gdrnpp_point_pnp_pool")
    return pooled, ws


def point_pnp_fc(ws, w_fc1, b_fc1, w_fc2, b_fc2, b: int, hw: int):
    """fc1 -> LeakyReLU(0.1) -> fc2 -> LeakyReLU(0.1) on the max over the tiles of ``ws`` (``gdrnpp_point_pnp_fc``) -> f32[b,256]."""
    if tuple(w_fc1.shape) != (512, 1024) or tuple(w_fc2.shape) != (256, 512) or b_fc1.numel() != 512 or b_fc2.numel() != 256:
        raise RuntimeError("point_pnp_fc: weights must be Linear(1024,512) and Linear(512,256) with biases")
    feat = torch.empty((b, 256), dtype=torch.float32, device=ws.device)
    _check(load().gdrnpp_point_pnp_fc(_f32(ws, "workspace"), ws.numel() * 4, _f32(w_fc1, "w_fc1"), _f32(b_fc1, "b_fc1"), _f32(w_fc2, "w_fc2"),
                                      _f32(b_fc2, "b_fc2"), feat.data_ptr(), b, hw, _stream()), "gdrnpp_point_pnp_fc")
    return feat


ROT_MODES = {"rot6d": 0, "quat": 1, "mat": 2, "log_quat": 3, "lie_vec": 4}
T_MODES = {"centroid_z_rel": 0, "centroid_z_abs_z": 1, "centroid_z_abs": 2, "trans": 3}
ROT_DIMS = {"rot6d": 6, "quat": 4, "mat": 9, "log_quat": 3, "lie_vec": 3}     # outputs of the rotation head per mode


def pnp_fc_heads_pose(x, w_r, b_r, w_t, b_t, cams, centers=None, whs=None, resize_ratios=None, rot_mode: str = "rot6d",
                      t_mode: str = "centroid_z_rel", is_allo: bool = True):
    """``pnp_fc_heads`` + ``pose_from_pred`` in one launch (``gdrnpp_pnp_fc_heads_pose``) -> (rot_ f32[b,rot_dim], t_ f32[b,3],
    R_ego f32[b,3,3], trans f32[b,3])."""
    b, k = x.shape
    rot_dim = w_r.shape[0]
    if rot_dim != ROT_DIMS[rot_mode]:
        raise ValueError(f"fc_r has {rot_dim} outputs, rot_mode {rot_mode!r} needs another count")
    dev = x.device
    rot_ = torch.empty((b, rot_dim), dtype=torch.float32, device=dev)
    t_ = torch.empty((b, 3), dtype=torch.float32, device=dev)
    rot = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    trans = torch.empty((b, 3), dtype=torch.float32, device=dev)
    _check(load().gdrnpp_pnp_fc_heads_pose(
        _f32(x, "x"), _f32(w_r, "w_r"), _opt_f32(b_r, "b_r"), _f32(w_t, "w_t"), _opt_f32(b_t, "b_t"),
        rot_.data_ptr(), t_.data_ptr(), b, k, ROT_MODES[rot_mode], T_MODES[t_mode], _f32(cams, "cams"), _opt_f32(centers, "centers"),
        _opt_f32(whs, "whs"), _opt_f32(resize_ratios, "resize_ratios"), rot.data_ptr(), trans.data_ptr(), 1 if is_allo else 0, _stream()),
        "gdrnpp_pnp_fc_heads_pose")
    return rot_, t_, rot, trans


def conv3x3_groupnorm_act(x_cl, weight_packed, bias, gamma, beta, groups: int, eps: float = 1e-5, gelu: bool = False, x3_slot: int = 0,
                          _min_tiles: int = 256):
    """conv3x3 (stride 1, pad 1) -> GroupNorm(groups) [-> GELU] of a channels_last tensor: the convolution's epilogue
    leaves the GroupNorm partial sums, the norm is one more pass (``gdrnpp_conv3x3_f32_split_gnstats`` +
    ``gdrnpp_groupnorm_apply_nhwc``).  Returns None when the shape is outside the fused form (H*W % 256, 8 channels
    per group) or the launch has fewer than 256 tiles of 256 x 128 (a dispatch rule, not a limit of the kernels; ``_min_tiles`` is a
    test / A-B knob like ``_kind``, not a tuning parameter: tests lower it to reach the kernels' smallest shape): the caller then runs the two layers separately."""
    n, cin, h, w = _channels_last_f32(x_cl, "conv3x3_groupnorm_act")
    cout, fp16x2 = _packed_weight(weight_packed, 9 * cin, "weight_packed must come from pack_conv_weight_bf16x3 / pack_conv_weight_f16x2 with matching Cin")
    P = load().gdrnpp_conv3x3_gnstats_partials(h, w)
    if P <= 0 or cout != 8 * groups or (n * h * w // 256) * (cout // 128) < _min_tiles:   # below: the 128x128-tile kernels are faster
        return None
    y = torch.empty((n, cout, h, w), dtype=torch.float32, device=x_cl.device, memory_format=torch.channels_last)
    part = torch.empty((n, P, groups, 2), dtype=torch.float64, device=x_cl.device)
    args = (x_cl.data_ptr(), weight_packed.data_ptr(), _opt_f32(bias, "bias"), y.data_ptr(), part.data_ptr(), n, h, w, cin, cout, groups, _stream())
    nbytes = 4.0 * n * h * w * (cin + cout) + (4.0 if fp16x2 else 6.0) * cout * 9 * cin
    if fp16x2:
        _count_x3()
        a3 = args[:4] + (part.data_ptr(), n, h, w, cin, cout, groups, 0, _x3_flag_ptr(x3_slot), _stream())
        _check(_timed("conv3x3" + X3, 2.0 * n * h * w * cout * 9 * cin, lambda: load().gdrnpp_conv3x3_f32_split2(*a3), nbytes),
               "gdrnpp_conv3x3_f32_split2")
    else:
        _check(_timed("conv3x3", 2.0 * n * h * w * cout * 9 * cin, lambda: load().gdrnpp_conv3x3_f32_split_gnstats(*args), nbytes),
               "gdrnpp_conv3x3_f32_split_gnstats")
    out = torch.empty_like(y)
    a2 = (y.data_ptr(), part.data_ptr(), P, _f32(gamma, "gamma"), _f32(beta, "beta"),
          out.data_ptr(), n, h * w, cout, groups, float(eps), 1 if gelu else 0, _stream())
    _check(_timed("hbm:groupnorm_apply", 0.0, lambda: load().gdrnpp_groupnorm_apply_nhwc(*a2), 8.0 * y.numel()),
           "gdrnpp_groupnorm_apply_nhwc")
    return out


def yolox_postprocess(det_preds, num_classes: int, conf_thre: float = 0.7, nms_thre: float = 0.45, class_agnostic: bool = False,
                      max_det: int = 0):
    """det_preds f32[B,A,5+C] (device) -> (dets f32[B,max_det,7], count i32[B]); rows = (x1,y1,x2,y2,obj,class_conf,class)
    in NMS keep order.  max_det = 0 sizes the output for every anchor."""
    b, a, s = det_preds.shape
    if s != 5 + num_classes:
        raise ValueError(f"det_preds last dim {s} != 5 + num_classes {num_classes}")
    max_det = max_det or a
    dets = torch.zeros((b, max_det, 7), dtype=torch.float32, device=det_preds.device)
    count = torch.zeros((b,), dtype=torch.int32, device=det_preds.device)
    nbytes = load().gdrnpp_yolox_postprocess_workspace_bytes(b, a)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=det_preds.device)
    _check(load().gdrnpp_yolox_postprocess(_f32(det_preds, "det_preds"), b, a, num_classes, float(conf_thre),
                                           float(nms_thre), 1 if class_agnostic else 0, dets.data_ptr(), count.data_ptr(), max_det,
                                           ws.data_ptr(), nbytes, _stream()), "gdrnpp_yolox_postprocess")
    return dets, count


# ---- YOLOX detector forward (csrc/yolox_net.hip) ------------------------------------------------------------------------------
CONV_ACTS = {"none": 0, "silu": 1, "sigmoid": 2, "yolox_box": 3}


def pack_conv_weight_kmajor(weight: torch.Tensor) -> torch.Tensor:
    """Conv2d weight f32[Cout,Cin,k,k] -> the B operand of ``gdrnpp_conv_bias_act_f32``: f32[k*k*Cin, ldw], row
    (ky * k + kx) * Cin + ci, column = output channel, ldw = Cout rounded up to 4 (zero columns)."""
    cout, cin, kh, kw = weight.shape
    ldw = (cout + 3) // 4 * 4
    out = torch.zeros((kh * kw * cin, ldw), dtype=torch.float32, device=weight.device)
    out[:, :cout] = weight.detach().float().permute(2, 3, 1, 0).reshape(kh * kw * cin, cout)
    return out


def _nhwc_buf(t: torch.Tensor, name: str) -> int:
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous float32 CUDA(HIP) tensor")
    return t.data_ptr()


def conv_bias_act_f32(a, a_off: int, cin: int, w_kmajor, bias, c, c_off: int, cout: int, ks: int, stride: int, act: str = "none",
                      res=None, r_off: int = 0, c_img_rows: int = 0, c_row0: int = 0, dec_stride: float = 0.0):
    """``gdrnpp_conv_bias_act_f32``: channels [a_off, a_off + cin) of a f32[B,H,W,lda] -> channels [c_off, c_off + cout) of c
    (f32[B,OH,OW,ldc], or f32[B,c_img_rows,ldc] written from row c_row0 of every image); res (same pixels as c) is added after
    the activation.  w_kmajor from ``pack_conv_weight_kmajor``.  Returns c."""
    if a.dim() != 4:
        raise RuntimeError(f"conv_bias_act_f32: a must be [B,H,W,lda], got {tuple(a.shape)}")
    b, h, w, lda = a.shape
    pad = (ks - 1) // 2
    oh, ow = (h + 2 * pad - ks) // max(stride, 1) + 1, (w + 2 * pad - ks) // max(stride, 1) + 1
    ldc = c.shape[-1]
    want = (b, c_img_rows, ldc) if c_img_rows else (b, oh, ow, ldc)
    if tuple(c.shape) != want:
        raise RuntimeError(f"conv_bias_act_f32: c must be {want}, got {tuple(c.shape)}")
    if res is not None and tuple(res.shape[:3]) != (b, oh, ow):
        raise RuntimeError(f"conv_bias_act_f32: res must be [{b},{oh},{ow},ldr], got {tuple(res.shape)}")
    if w_kmajor.dim() != 2 or w_kmajor.shape[0] != ks * ks * cin:
        raise RuntimeError(f"conv_bias_act_f32: weight must be [{ks * ks * cin}, ldw], got {tuple(w_kmajor.shape)}")
    if bias is not None and bias.numel() != cout:
        raise RuntimeError(f"conv_bias_act_f32: bias must hold {cout} values")
    args = (_nhwc_buf(a, "a"), lda, a_off, _nhwc_buf(w_kmajor, "weight"), w_kmajor.shape[1],
            _opt_f32(bias, "bias"), None if res is None else _nhwc_buf(res, "res"),
            0 if res is None else res.shape[-1], r_off, _nhwc_buf(c, "c"), ldc, c_off, c_img_rows, c_row0, b, h, w, cin, cout, ks, stride,
            CONV_ACTS[act], float(dec_stride), _stream())
    _check(_timed("mfma_f32:conv_bias_act", 2.0 * b * oh * ow * cout * ks * ks * cin, lambda: load().gdrnpp_conv_bias_act_f32(*args),
                  4.0 * b * (h * w * cin + oh * ow * cout) + 4.0 * cout * ks * ks * cin), "gdrnpp_conv_bias_act_f32")
    return c


def yolox_focus(x_nchw, y, y_off: int = 0):
    """``gdrnpp_yolox_focus``: x f32[B,3,H,W] -> 12 channels at y_off of y f32[B,H/2,W/2,ldy]."""
    b, ch, h, w = x_nchw.shape
    if ch != 3 or tuple(y.shape[:3]) != (b, h // 2, w // 2):
        raise RuntimeError(f"yolox_focus: x [B,3,H,W] -> y [B,H/2,W/2,ldy], got {tuple(x_nchw.shape)} -> {tuple(y.shape)}")
    _check(load().gdrnpp_yolox_focus(_f32(x_nchw, "x"), _nhwc_buf(y, "y"), y.shape[-1], y_off, b, h, w, _stream()),
           "gdrnpp_yolox_focus")
    return y


def spp_maxpool_5_9_13(buf, off: int, c: int):
    """``gdrnpp_spp_maxpool_5_9_13`` on buf f32[B,H,W,ld]: channels [off, off + c) -> their 5 / 9 / 13 max pools in the next three
    slices of c channels."""
    b, h, w, ld = buf.shape
    _check(load().gdrnpp_spp_maxpool_5_9_13(_nhwc_buf(buf, "buf"), ld, off, c, b, h, w, _stream()), "gdrnpp_spp_maxpool_5_9_13")
    return buf


def upsample_nearest2x_slice(x, x_off: int, y, y_off: int, c: int):
    """``gdrnpp_upsample_nearest2x_slice``: channels [x_off, x_off + c) of x f32[B,h,w,ldx] -> [y_off, y_off + c) of y f32[B,2h,2w,ldy]."""
    b, h, w, ldx = x.shape
    if tuple(y.shape[:3]) != (b, 2 * h, 2 * w):
        raise RuntimeError(f"upsample_nearest2x_slice: y must be [{b},{2 * h},{2 * w},ldy], got {tuple(y.shape)}")
    _check(load().gdrnpp_upsample_nearest2x_slice(_nhwc_buf(x, "x"), ldx, x_off, _nhwc_buf(y, "y"), y.shape[-1], y_off, b, h, w, c,
                                                  _stream()), "gdrnpp_upsample_nearest2x_slice")
    return y


# ---- the detector's two ends (csrc/yolox_pre.hip) -----------------------------------------------------------------------------
def letterbox_sizes(H: int, W: int, test_size) -> tuple:
    """``preproc``'s size arithmetic (det/yolox/data/data_augment.py:167-173) with Python floats, as the reference does it:
    -> (r, rh, rw) = (min(Ht / H, Wt / W), int(H * r), int(W * r))."""
    r = min(test_size[0] / H, test_size[1] / W)
    return r, int(H * r), int(W * r)


def yolox_letterbox(images_u8, test_size=(640, 640), out=None, y_off: int = 0, focus: bool = False, legacy: bool = False):
    """``gdrnpp_yolox_letterbox``: images u8[B,H,W,3] (BGR, device) -> (the letterboxed float image, r).  ``focus=False``:
    f32[B,3,Ht,Wt], what ``YOLOX.forward`` takes.  ``focus=True``: the Focus stem's 12 channels at ``y_off`` of
    f32[B,Ht/2,Wt/2,ld] (``out``, or a fresh 12-channel buffer).  ``ValTransform(legacy=True)`` is not implemented."""
    if legacy:
        raise NotImplementedError("yolox_letterbox: legacy=True (RGB flip and ImageNet normalisation) is not implemented")
    if images_u8.dim() != 4 or images_u8.shape[-1] != 3:
        raise RuntimeError(f"yolox_letterbox: images must be u8[B,H,W,3], got {tuple(images_u8.shape)}")
    b, H, W, _ = images_u8.shape
    ht, wt = int(test_size[0]), int(test_size[1])
    r, rh, rw = letterbox_sizes(H, W, (ht, wt))
    if out is None:
        shape = (b, ht // 2, wt // 2, 12) if focus else (b, 3, ht, wt)
        out = torch.empty(shape, dtype=torch.float32, device=images_u8.device)
    want = (b, ht // 2, wt // 2) if focus else (b, 3, ht, wt)
    if tuple(out.shape[:3] if focus else out.shape) != want:
        raise RuntimeError(f"yolox_letterbox: out must be {want + (('ld',) if focus else ())}, got {tuple(out.shape)}")
    _check(load().gdrnpp_yolox_letterbox(_dev(images_u8, torch.uint8, "images"), b, H, W, rh, rw, _nhwc_buf(out, "out"), ht, wt,
                                         1 if focus else 0, out.shape[-1] if focus else 0, int(y_off) if focus else 0, _stream()),
           "gdrnpp_yolox_letterbox")
    return out, r


class gdrnpp_roi_table(ctypes.Structure):
    _fields_ = [(k, c_void_p) for k in ("center64", "scale64", "im_idx", "roi_cls", "roi_cam", "roi_center", "roi_wh", "scale",
                                        "resize_ratio", "roi_extent", "score", "roi_id")]


# column -> (torch dtype, trailing shape): the keys and dtypes of roi_stream.roi_host_arrays, in its order
ROI_TABLE_COLUMNS = {
    "center64": (torch.float64, (2,)), "scale64": (torch.float64, ()), "im_idx": (torch.int32, ()), "roi_cls": (torch.int64, ()),
    "roi_cam": (torch.float32, (3, 3)), "roi_center": (torch.float32, (2,)), "roi_wh": (torch.float32, (2,)),
    "scale": (torch.float32, ()), "resize_ratio": (torch.float32, ()), "roi_extent": (torch.float32, (3,)),
    "score": (torch.float32, ()), "roi_id": (torch.int32, ()),
}


def roi_table(cap: int, device) -> dict:
    """An empty ROI table of ``cap`` rows: one device allocation, every column a 16-byte aligned typed view of it."""
    sizes, total = {}, 0
    for k, (dt, tail) in ROI_TABLE_COLUMNS.items():
        n = cap * torch.empty((), dtype=dt).element_size()
        for t in tail:
            n *= t
        total = (total + 15) & ~15
        sizes[k] = (total, n)
        total += n
    raw = torch.zeros((total,), dtype=torch.uint8, device=device)
    return {k: raw[off:off + n].view(ROI_TABLE_COLUMNS[k][0]).reshape((cap,) + ROI_TABLE_COLUMNS[k][1]) for k, (off, n) in sizes.items()}


def rois_from_dets(dets, count, ratio: float, H: int, W: int, cam, extents, dzi_pad_scale: float = 1.5, out_res: int = 64,
                   score_thr: float = 0.0, top_k_per_obj: int = 0, cap: int = 256, table: dict | None = None, counts=None):
    """``gdrnpp_rois_from_dets``: ``yolox_postprocess`` output -> (table, counts).  ``table`` = {column: tensor of ``cap`` rows}
    (``roi_table``; the keys and dtypes of ``roi_stream.roi_host_arrays``), ``counts`` i32[1 + B] = (n_rois, per-image counts);
    rows from n_rois on are not written.  cam f32[3,3] or f32[B,3,3], extents f32[C,3], all on the device."""
    b, max_det, seven = dets.shape
    if seven != 7 or count.numel() != b:
        raise RuntimeError(f"rois_from_dets: dets f32[B,max_det,7] and count i32[B], got {tuple(dets.shape)} and {tuple(count.shape)}")
    if cam.numel() not in (9, 9 * b) or extents.dim() != 2 or extents.shape[1] != 3:
        raise RuntimeError(f"rois_from_dets: cam f32[3,3] or f32[B,3,3], extents f32[C,3], got {tuple(cam.shape)} and {tuple(extents.shape)}")
    table = table if table is not None else roi_table(cap, dets.device)
    if any(table[k].shape[0] != cap for k in ROI_TABLE_COLUMNS):
        raise RuntimeError(f"rois_from_dets: every table column must hold cap = {cap} rows")
    counts = counts if counts is not None else torch.zeros((1 + b,), dtype=torch.int32, device=dets.device)
    lib = load()
    nbytes = lib.gdrnpp_rois_from_dets_workspace_bytes(b, max_det)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dets.device)
    ctab = gdrnpp_roi_table(**{k: _dev(table[k], ROI_TABLE_COLUMNS[k][0], k) for k in ROI_TABLE_COLUMNS})
    cnt = _dev(counts, torch.int32, "counts")
    _check(lib.gdrnpp_rois_from_dets(
        _f32(dets, "dets"), _dev(count, torch.int32, "count"), b, max_det, extents.shape[0], float(ratio), int(H), int(W),
        float(dzi_pad_scale), int(out_res), _f32(cam, "cam"), 1 if cam.dim() == 3 else 0,
        _f32(extents, "extents"), float(score_thr), int(top_k_per_obj), int(cap), ctypes.byref(ctab), cnt, cnt + 4,
        ws.data_ptr(), nbytes, _stream()), "gdrnpp_rois_from_dets")
    return table, counts


def paste_masks_rle(mask_probs, boxes_xyxy, im_h: int, im_w: int, threshold: float = 0.5, max_runs: int = 4096):
    """mask_probs f32[B,hm,wm], boxes f32[B,4] (device) -> list of B uncompressed COCO count lists (column-major, first
    run = zeros).  The launch is repeated with a larger buffer if an instance needs more than ``max_runs`` runs."""
    b, hm, wm = mask_probs.shape
    while True:
        counts = torch.empty((b, max_runs), dtype=torch.int32, device=mask_probs.device)
        n_runs = torch.empty((b,), dtype=torch.int32, device=mask_probs.device)
        _check(load().gdrnpp_paste_masks_rle(_f32(mask_probs, "mask_probs"), _f32(boxes_xyxy, "boxes"),
                                             b, hm, wm, im_h, im_w, float(threshold), counts.data_ptr(), n_runs.data_ptr(), max_runs,
                                             _stream()), "gdrnpp_paste_masks_rle")
        n = n_runs.tolist()
        if max(n) <= max_runs:
            c = counts.cpu().numpy().view("uint32")
            return [c[i, :n[i]].astype("int64").tolist() for i in range(b)]
        max_runs = max(n)


def flow_forward(depth_src, depth_tgt, KT, Kinv):
    """depth f32[B,1,H,W] x2, KT f32[B,3,4], Kinv f32[B,3,3] (device) -> flow f32[B,2,H,W], valid f32[B,1,H,W]."""
    b, _, h, w = depth_src.shape
    flow = torch.empty((b, 2, h, w), dtype=torch.float32, device=depth_src.device)
    valid = torch.empty((b, 1, h, w), dtype=torch.float32, device=depth_src.device)
    _check(load().gdrnpp_flow_forward(_f32(depth_src, "depth_src"), _f32(depth_tgt, "depth_tgt"), _f32(KT, "KT"), _f32(Kinv, "Kinv"), flow.data_ptr(),
                                      valid.data_ptr(), b, h, w, _stream()), "gdrnpp_flow_forward")
    return flow, valid
