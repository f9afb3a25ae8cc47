"""Network-side layers outside the split GEMMs: the ConvNeXt NHWC kernels (tensors are logically NCHW with channels_last strides),
the geometry head's tail and the Patch-PnP / point-PnP heads."""
from __future__ import annotations

import torch

from .abi import channels_last_f32, f32_ptr, launch, load, nhwc_ptr, opt_f32_ptr


def dwconv7x7_ln(x, w49c, bias, ln_w=None, ln_b=None, eps: float = 1e-6, y_rows: bool = False):
    """x (N,C,H,W) channels_last -> depthwise 7x7 (+ LayerNorm over C), same shape/format.  ``y_rows``: the result is written as an
    "f16x2 rows" tensor (include/gdrnpp_hip.h: every 8 consecutive channels of a pixel replaced by their fp16 h and l halves) for
    ``linear_f32_split(..., a_rows=True)`` — same shape and dtype, NOT readable as floats."""
    n, c, h, w = x.shape
    y = torch.empty_like(x, memory_format=torch.channels_last)
    launch("gdrnpp_dwconv7x7_ln_nhwc_rows", nhwc_ptr(x, "x"), f32_ptr(w49c, "w49c"), f32_ptr(bias, "bias"), opt_f32_ptr(ln_w, "ln_w"),
           opt_f32_ptr(ln_b, "ln_b"), y.data_ptr(), n, h, w, c, float(eps), int(bool(y_rows)), timed=("hbm:dwconv7_ln", 0.0, 8.0 * x.numel()))
    return y


def layernorm_nhwc(x, weight, bias, eps: float = 1e-6):
    """x (N,C,H,W) channels_last -> LayerNorm over C per pixel, same shape/format."""
    n, c, h, w = x.shape
    y = torch.empty_like(x, memory_format=torch.channels_last)
    launch("gdrnpp_layernorm_nhwc", nhwc_ptr(x, "x"), f32_ptr(weight, "weight"), f32_ptr(bias, "bias"), y.data_ptr(), n * h * w, c, float(eps),
           timed=("hbm:layernorm", 0.0, 8.0 * x.numel()))
    return y


def upsample_bilinear2x(x):
    n, c, h, w = x.shape
    y = torch.empty((n, c, 2 * h, 2 * w), dtype=x.dtype, device=x.device, memory_format=torch.channels_last)
    launch("gdrnpp_upsample_bilinear2x_nhwc", nhwc_ptr(x, "x"), y.data_ptr(), n, h, w, c, timed=("hbm:upsample2x", 0.0, 20.0 * x.numel()))
    return y


def groupnorm_act(x, gamma, beta, groups: int, eps: float = 1e-5, gelu: bool = False):
    n, c, h, w = x.shape
    y = torch.empty_like(x, memory_format=torch.channels_last)
    ws = torch.empty((load().gdrnpp_groupnorm_workspace_bytes(n, h * w, groups),), dtype=torch.uint8, device=x.device)
    launch("gdrnpp_groupnorm_act_nhwc", nhwc_ptr(x, "x"), f32_ptr(gamma, "gamma"), f32_ptr(beta, "beta"), y.data_ptr(), ws.data_ptr(),
           n, h * w, c, groups, float(eps), 1 if gelu else 0, timed=("hbm:groupnorm", 0.0, 12.0 * x.numel()))   # read twice, write once
    return y


def bias_act_nhwc_(x_cl, bias, resid=None, relu: bool = True):
    """In place: x = act(x + bias[c] (+ resid)) on a channels_last float32 tensor [N,C,H,W] (C % 4 == 0)."""
    n, c, h, w = channels_last_f32(x_cl, "bias_act_nhwc_")
    if resid is not None and (resid.shape != x_cl.shape or not resid.is_contiguous(memory_format=torch.channels_last)
                              or resid.dtype != torch.float32 or resid.device != x_cl.device):
        raise ValueError("resid must match x (float32, channels_last, same device)")
    launch("gdrnpp_bias_act_nhwc", x_cl.data_ptr(), f32_ptr(bias, "bias"), resid.data_ptr() if resid is not None else None, x_cl.data_ptr(),
           n * h * w, c, 1 if relu else 0)
    return x_cl


def stem_conv4x4_ln(x_nchw, weight, bias, ln_weight, ln_bias, eps: float):
    """ConvNeXt stem in one kernel: Conv2d(3 -> 128, 4x4/4) + bias + LayerNorm2d; NCHW image in, channels_last [N,128,H/4,W/4] out."""
    n, cin, h, w = x_nchw.shape
    cout = weight.shape[0]
    out = torch.empty((n, cout, h // 4, w // 4), dtype=torch.float32, device=x_nchw.device, memory_format=torch.channels_last)
    launch("gdrnpp_stem_conv4x4_ln", f32_ptr(x_nchw, "x"), f32_ptr(weight, "weight"), opt_f32_ptr(bias, "bias"), f32_ptr(ln_weight, "ln_weight"),
           f32_ptr(ln_bias, "ln_bias"), out.data_ptr(), n, h, w, cout, float(eps))
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
    launch("gdrnpp_head_tail_nhwc", f32_ptr(out_nhwc, "out_nhwc"), pitch, f32_ptr(coord2d, "coord2d"), f32_ptr(extents, "extents"),
           pnp_in.data_ptr(), planes.data_ptr(), b, hw, 1 if double_mask else 0)
    return pnp_in, planes


def pnp_fc_heads(x, w_r, b_r, w_t, b_t):
    """Patch-PnP's output layers in one launch (``gdrnpp_pnp_fc_heads``): x f32[b,K] -> (fc_r(x) f32[b,rot_dim], fc_t(x) f32[b,3])."""
    b, k = x.shape
    rot_dim = w_r.shape[0]
    rot_ = torch.empty((b, rot_dim), dtype=torch.float32, device=x.device)
    t_ = torch.empty((b, 3), dtype=torch.float32, device=x.device)
    launch("gdrnpp_pnp_fc_heads", f32_ptr(x, "x"), f32_ptr(w_r, "w_r"), opt_f32_ptr(b_r, "b_r"), f32_ptr(w_t, "w_t"), opt_f32_ptr(b_t, "b_t"),
           rot_.data_ptr(), t_.data_ptr(), b, k, rot_dim)
    return rot_, t_


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
    launch("gdrnpp_pnp_fc_heads_pose", f32_ptr(x, "x"), f32_ptr(w_r, "w_r"), opt_f32_ptr(b_r, "b_r"), f32_ptr(w_t, "w_t"), opt_f32_ptr(b_t, "b_t"),
           rot_.data_ptr(), t_.data_ptr(), b, k, ROT_MODES[rot_mode], T_MODES[t_mode], f32_ptr(cams, "cams"), opt_f32_ptr(centers, "centers"),
           opt_f32_ptr(whs, "whs"), opt_f32_ptr(resize_ratios, "resize_ratios"), rot.data_ptr(), trans.data_ptr(), 1 if is_allo else 0)
    return rot_, t_, rot, trans


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
    nbytes = load().gdrnpp_point_pnp_workspace_bytes(b, hw)
    if nbytes == 0:
        raise RuntimeError(f"point_pnp_pool: b={b} hw={hw}: hw must be a positive multiple of {POINT_PNP_TILE}")
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x2d.device)
    pooled = torch.empty((b, 1024), dtype=torch.float32, device=x2d.device) if want_pooled else None
    launch("gdrnpp_point_pnp_pool", f32_ptr(x2d, "x"), x2d.shape[1], cin, f32_ptr(w1, "w1"), f32_ptr(b1, "b1"), f32_ptr(w2, "w2"), f32_ptr(b2, "b2"),
           f32_ptr(w3, "w3"), f32_ptr(b3, "b3"), pooled.data_ptr() if want_pooled else None, b, hw, ws.data_ptr(), nbytes,
           timed=("mfma_f32:point_pnp_pool", 2.0 * b * hw * (128 * cin + 128 * 128 + 1024 * 128), 0.0))
    return pooled, ws


def point_pnp_fc(ws, w_fc1, b_fc1, w_fc2, b_fc2, b: int, hw: int):
    """fc1 -> LeakyReLU(0.1) -> fc2 -> LeakyReLU(0.1) on the max over the tiles of ``ws`` (``gdrnpp_point_pnp_fc``) -> f32[b,256]."""
    if tuple(w_fc1.shape) != (512, 1024) or tuple(w_fc2.shape) != (256, 512) or b_fc1.numel() != 512 or b_fc2.numel() != 256:
        raise RuntimeError("point_pnp_fc: weights must be Linear(1024,512) and Linear(512,256) with biases")
    feat = torch.empty((b, 256), dtype=torch.float32, device=ws.device)
    launch("gdrnpp_point_pnp_fc", f32_ptr(ws, "workspace"), ws.numel() * 4, f32_ptr(w_fc1, "w_fc1"), f32_ptr(b_fc1, "b_fc1"), f32_ptr(w_fc2, "w_fc2"),
           f32_ptr(b_fc2, "b_fc2"), feat.data_ptr(), b, hw)
    return feat
