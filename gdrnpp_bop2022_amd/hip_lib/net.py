"""Network-side layers outside the split GEMMs: the ConvNeXt NHWC kernels (tensors are logically NCHW with channels_last strides),
the geometry head's tail, the Patch-PnP / point-PnP heads, the training losses over the network's outputs and the optimiser step."""
from __future__ import annotations

import numpy as np
import torch

from .abi import DEFINES, STRUCTS, channels_last_f32, dev_ptr, f32_ptr, launch, load, nhwc_ptr, opt_f32_ptr
from .gemm import colsum_f32, gemm_tn_f32, linear_f32_exact


def dwconv7x7_ln(x, w49c, bias, ln_w=None, ln_b=None, eps: float = 1e-6, y_rows: bool = False):
    """x (N,C,H,W) channels_last -> depthwise 7x7 (+ LayerNorm over C), same shape/format.  ``y_rows``: the result is written as an
    "f16x2 rows" tensor (include/gdrnpp_hip.h: every 8 consecutive channels of a pixel replaced by their fp16 h and l halves) for
    ``linear_f32_split(..., a_rows=True)`` — same shape and dtype, NOT readable as floats."""
    n, c, h, w = x.shape
    y = torch.empty_like(x, memory_format=torch.channels_last)
    launch("gdrnpp_dwconv7x7_ln_nhwc_rows", nhwc_ptr(x, "x"), f32_ptr(w49c, "w49c"), f32_ptr(bias, "bias"), opt_f32_ptr(ln_w, "ln_w"),
           opt_f32_ptr(ln_b, "ln_b"), y.data_ptr(), n, h, w, c, float(eps), int(bool(y_rows)), timed=("hbm:dwconv7_ln", 0.0, 8.0 * x.numel()))
    return y


def dwconv7x7_ln_backward(x, weight, bias, ln_weight, ln_bias, eps: float, grad_y, want=(True,) * 5, w49c=None):
    """``gdrnpp_dwconv7x7_ln_backward``: the gradients of ``dwconv7x7_ln(x, ...)`` (with its LayerNorm) for grad_y = dL/dy
    -> (dx, dweight, dbias, dln_weight, dln_bias).  x, grad_y (N,C,H,W) channels_last; weight [C,1,7,7] (conv.weight) and dweight in the
    same layout; the others f32[C].  ``want``: five flags in the order of the result — an entry is None where its flag is false, and
    the pass only it needs is not launched.  ``w49c``: the tap-major copy [49,C] of ``weight`` when the caller has one (the forward's),
    else it is made here.  u and the statistics are recomputed from x: nothing of the forward is needed.  Fixed summation order: two
    calls give the same bits."""
    what = "dwconv7x7_ln_backward"
    want = tuple(bool(w) for w in want)
    if len(want) != 5 or not any(want):
        raise RuntimeError(f"{what}: want must hold five flags, at least one of them set")
    px = nhwc_ptr(x, "x")
    n, c, h, w = x.shape
    if not isinstance(grad_y, torch.Tensor) or tuple(grad_y.shape) != (n, c, h, w):
        raise RuntimeError(f"{what}: grad_y must be f32[{n},{c},{h},{w}] as x is, got {tuple(getattr(grad_y, 'shape', ()))}")
    pg = nhwc_ptr(grad_y, "grad_y")
    if tuple(weight.shape) != (c, 1, 7, 7):
        raise RuntimeError(f"{what}: weight must be f32[{c},1,7,7], got {tuple(weight.shape)}")
    for name, t in (("bias", bias), ("ln_weight", ln_weight), ("ln_bias", ln_bias)):
        if t is None or t.numel() != c:
            raise RuntimeError(f"{what}: {name} must be f32[{c}]")
    if w49c is None:
        w49c = weight.detach().reshape(c, 49).t().contiguous()
    elif tuple(w49c.shape) != (49, c):
        raise RuntimeError(f"{what}: w49c must be f32[49,{c}], got {tuple(w49c.shape)}")
    pw, pb, pl = f32_ptr(w49c, "w49c"), f32_ptr(bias, "bias"), f32_ptr(ln_weight, "ln_weight")
    f32_ptr(ln_bias, "ln_bias")
    nbytes = load().gdrnpp_dwconv7x7_ln_backward_workspace_bytes(n, h, w, c)
    ws = torch.empty((max(nbytes, 16) // 8,), dtype=torch.float64, device=x.device)
    dx = torch.empty_like(x, memory_format=torch.channels_last) if want[0] else None
    dweight = torch.empty((c, 1, 7, 7), dtype=torch.float32, device=x.device) if want[1] else None
    dbias, dln_w, dln_b = (torch.empty((c,), dtype=torch.float32, device=x.device) if f else None for f in want[2:])
    # pass A reads x and g and writes du; dx reads du and writes dx; dw reads du and x (7 kernel rows, from L2)
    launch("gdrnpp_dwconv7x7_ln_backward", px, pw, pb, pl, pg, *(t.data_ptr() if t is not None else None for t in (dx, dweight, dbias, dln_w, dln_b)),
           n, h, w, c, float(eps), ws.data_ptr(), nbytes, timed=("hbm:dwconv7_ln_bwd", 0.0, 4.0 * x.numel() * (3 + 2 * want[0] + 2 * want[1])))
    return dx, dweight, dbias, dln_w, dln_b


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


def upsample_bilinear2x_backward(grad_y):
    """``gdrnpp_upsample_bilinear2x_backward_nhwc``: dx (N,C,H,W) channels_last of ``upsample_bilinear2x`` for grad_y (N,C,2H,2W)."""
    n, c, oh, ow = grad_y.shape
    if oh % 2 or ow % 2:
        raise RuntimeError(f"upsample_bilinear2x_backward: grad_y must be (N,C,2H,2W), got {tuple(grad_y.shape)}")
    dx = torch.empty((n, c, oh // 2, ow // 2), dtype=torch.float32, device=grad_y.device, memory_format=torch.channels_last)
    launch("gdrnpp_upsample_bilinear2x_backward_nhwc", nhwc_ptr(grad_y, "grad_y"), dx.data_ptr(), n, oh // 2, ow // 2, c,
           timed=("hbm:upsample2x_bwd", 0.0, 5.0 * grad_y.numel()))
    return dx


def groupnorm_act_train(z, gamma, beta, groups: int, eps: float = 1e-5, gelu: bool = False):
    """GroupNorm(groups) [+ exact GELU] of z (N,C,H,W) channels_last for training -> (y, partials f64[N,P,groups,2]): the statistics
    pass alone (``gdrnpp_groupnorm_stats_nhwc``), then ``gdrnpp_groupnorm_apply_nhwc``.  z and the partials are what
    ``groupnorm_act_backward`` takes."""
    n, c, h, w = z.shape
    P = load().gdrnpp_groupnorm_workspace_bytes(n, h * w, groups) // (16 * n * groups)
    part = torch.empty((n, P, groups, 2), dtype=torch.float64, device=z.device)
    y = torch.empty_like(z, memory_format=torch.channels_last)
    launch("gdrnpp_groupnorm_stats_nhwc", nhwc_ptr(z, "z"), part.data_ptr(), n, h * w, c, groups, timed=("hbm:groupnorm_stats", 0.0, 4.0 * z.numel()))
    launch("gdrnpp_groupnorm_apply_nhwc", z.data_ptr(), part.data_ptr(), P, f32_ptr(gamma, "gamma"), f32_ptr(beta, "beta"), y.data_ptr(), n, h * w, c,
           groups, float(eps), 1 if gelu else 0, timed=("hbm:groupnorm_apply", 0.0, 8.0 * z.numel()))
    return y, part


def groupnorm_act_backward(z, partials, gamma, beta, groups: int, eps: float, gelu: bool, grad_y, want=(True,) * 3):
    """``gdrnpp_groupnorm_act_backward``: gradients of y = act(GroupNorm(z)) for grad_y = dL/dy -> (dz, dgamma, dbeta).  z, grad_y
    (N,C,H,W) channels_last; ``partials`` f64[N,P,groups,2] from the forward.  ``want``: three flags in the order of the result — an
    entry is None where its flag is false and the launches only it needs are left out.  Fixed summation order: two calls give the
    same bits."""
    what = "groupnorm_act_backward"
    want = tuple(bool(f) for f in want)
    if len(want) != 3 or not any(want):
        raise RuntimeError(f"{what}: want must hold three flags, at least one of them set")
    pz = nhwc_ptr(z, "z")
    n, c, h, w = z.shape
    if not isinstance(grad_y, torch.Tensor) or tuple(grad_y.shape) != (n, c, h, w):
        raise RuntimeError(f"{what}: grad_y must be f32[{n},{c},{h},{w}] as z is, got {tuple(getattr(grad_y, 'shape', ()))}")
    if partials.dim() != 4 or partials.shape[0] != n or tuple(partials.shape[2:]) != (groups, 2) or gamma.numel() != c or beta.numel() != c:
        raise RuntimeError(f"{what}: partials must be f64[{n},P,{groups},2], gamma and beta f32[{c}]")
    nbytes = load().gdrnpp_groupnorm_act_backward_workspace_bytes(n, h * w, c, groups)
    if nbytes == 0:
        raise RuntimeError(f"{what}: shape C={c} G={groups} N={n} is outside the kernel")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=z.device)
    dz = torch.empty_like(z, memory_format=torch.channels_last) if want[0] else None
    dgamma, dbeta = (torch.empty((c,), dtype=torch.float32, device=z.device) if f else None for f in want[1:])
    launch("gdrnpp_groupnorm_act_backward", pz, dev_ptr(partials, torch.float64, "partials"), int(partials.shape[1]), f32_ptr(gamma, "gamma"),
           f32_ptr(beta, "beta"), nhwc_ptr(grad_y, "grad_y"), dz.data_ptr() if want[0] else None, dgamma.data_ptr() if want[1] else None,
           dbeta.data_ptr() if want[2] else None, n, h * w, c, groups, float(eps), 1 if gelu else 0, ws.data_ptr(), nbytes,
           timed=("hbm:groupnorm_bwd", 0.0, 4.0 * z.numel() * (2 + 3 * want[0])))
    return dz, dgamma, dbeta


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


def _want(what: str, want, n: int):
    want = tuple(bool(f) for f in want)
    if len(want) != n or not any(want):
        raise RuntimeError(f"{what}: want must hold {n} flags, at least one of them set")
    return want


def stem_conv4x4_ln_backward(x_nchw, weight, bias, ln_weight, eps: float, grad_y, want=(True,) * 4):
    """``gdrnpp_stem_conv4x4_ln_backward``: the parameter gradients of ``stem_conv4x4_ln(x, ...)`` for grad_y = dL/dy (N,128,H/4,W/4)
    channels_last -> (dweight [128,3,4,4], dbias, dln_weight, dln_bias).  ``want``: four flags in the order of the result — an entry is
    None where its flag is false; without dweight the kernel runs without its matrix instructions.  ``ln_weight`` None: no LayerNorm
    (du = grad_y; the last two flags must be false).  The pre-norm activation and the statistics are recomputed from x; the gradient with
    respect to x is not formed.  Fixed summation order: two calls give the same bits."""
    what = "stem_conv4x4_ln_backward"
    want = _want(what, want, 4)
    if ln_weight is None and (want[2] or want[3]):
        raise RuntimeError(f"{what}: dln_weight / dln_bias asked for without a LayerNorm")
    px = f32_ptr(x_nchw, "x")
    if x_nchw.dim() != 4 or x_nchw.shape[1] != 3:
        raise RuntimeError(f"{what}: x must be f32[N,3,H,W] (NCHW), got {tuple(x_nchw.shape)}")
    n, _, h, w = x_nchw.shape
    cout = weight.shape[0]
    if tuple(weight.shape) != (cout, 3, 4, 4):
        raise RuntimeError(f"{what}: weight must be f32[Cout,3,4,4], got {tuple(weight.shape)}")
    nbytes = load().gdrnpp_stem_conv4x4_ln_backward_workspace_bytes(n, h, w, cout)
    if nbytes == 0:
        raise RuntimeError(f"{what}: N={n} H={h} W={w} Cout={cout} is outside the kernel (H % 4 == 0, W % 16 == 0, W <= 1024, Cout = 128)")
    if not isinstance(grad_y, torch.Tensor) or tuple(grad_y.shape) != (n, cout, h // 4, w // 4):
        raise RuntimeError(f"{what}: grad_y must be f32[{n},{cout},{h // 4},{w // 4}] channels_last, got {tuple(getattr(grad_y, 'shape', ()))}")
    pg = nhwc_ptr(grad_y, "grad_y")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x_nchw.device)
    dweight = torch.empty((cout, 3, 4, 4), dtype=torch.float32, device=x_nchw.device) if want[0] else None
    dbias, dln_w, dln_b = (torch.empty((cout,), dtype=torch.float32, device=x_nchw.device) if f else None for f in want[1:])
    m = n * (h // 4) * (w // 4)
    launch("gdrnpp_stem_conv4x4_ln_backward", px, f32_ptr(weight, "weight"), opt_f32_ptr(bias, "bias"), opt_f32_ptr(ln_weight, "ln_weight"), pg,
           *(t.data_ptr() if t is not None else None for t in (dweight, dbias, dln_w, dln_b)), n, h, w, cout, float(eps), ws.data_ptr(), nbytes,
           timed=("mfma_f32:stem_bwd" if want[0] else "hbm:stem_bwd", 2.0 * m * cout * 48 * (want[0] + (ln_weight is not None)),
                  4.0 * (x_nchw.numel() + grad_y.numel())))
    return dweight, dbias, dln_w, dln_b


def _patch_shape(what: str, x):
    px = nhwc_ptr(x, "x")
    n, c, h, w = x.shape
    if load().gdrnpp_layernorm_patch2x2_backward_workspace_bytes(n, h, w, c) == 0:
        raise RuntimeError(f"{what}: x {tuple(x.shape)} is outside the kernel (H, W even; C = 128, 256, 512 or 1024)")
    return px, n, c, h, w


def layernorm_patch2x2(x, ln_weight=None, ln_bias=None, eps: float = 1e-6):
    """x (N,C,H,W) channels_last -> A f32[N H/2 W/2, 4 C]: LayerNorm over C per pixel — the bits of ``layernorm_nhwc`` — stored as the
    operand of a 2x2 / stride 2 convolution run as a product: row = output pixel, column = (ky, kx, ci)
    (``gdrnpp_layernorm_patch2x2_nhwc``).  ``ln_weight`` and ``ln_bias`` None: the space-to-depth copy alone."""
    what = "layernorm_patch2x2"
    px, n, c, h, w = _patch_shape(what, x)
    if (ln_weight is None) != (ln_bias is None) or (ln_weight is not None and (ln_weight.numel() != c or ln_bias.numel() != c)):
        raise RuntimeError(f"{what}: ln_weight and ln_bias must be f32[{c}], or both None")
    a = torch.empty((n * (h // 2) * (w // 2), 4 * c), dtype=torch.float32, device=x.device)
    launch("gdrnpp_layernorm_patch2x2_nhwc", px, opt_f32_ptr(ln_weight, "ln_weight"), opt_f32_ptr(ln_bias, "ln_bias"), a.data_ptr(), n, h, w, c,
           float(eps), timed=("hbm:ln_patch2x2", 0.0, 8.0 * x.numel()))
    return a


def layernorm_patch2x2_backward(x, ln_weight, eps: float, d_a, want=(True,) * 3):
    """``gdrnpp_layernorm_patch2x2_backward``: the adjoint of ``layernorm_patch2x2`` for d_a = dL/dA f32[N H/2 W/2, 4 C] -> (dx (N,C,H,W)
    channels_last, dln_weight, dln_bias).  ``want``: three flags in that order, an entry is None where its flag is false.  The statistics
    are recomputed from x.  ``ln_weight`` None: the inverse copy (dx alone; x gives the shape)."""
    what = "layernorm_patch2x2_backward"
    want = _want(what, want, 3)
    px, n, c, h, w = _patch_shape(what, x)
    if ln_weight is None and want != (True, False, False):
        raise RuntimeError(f"{what}: without a LayerNorm dx alone is formed")
    if not isinstance(d_a, torch.Tensor) or tuple(d_a.shape) != (n * (h // 2) * (w // 2), 4 * c):
        raise RuntimeError(f"{what}: d_a must be f32[{n * (h // 2) * (w // 2)},{4 * c}], got {tuple(getattr(d_a, 'shape', ()))}")
    nbytes = load().gdrnpp_layernorm_patch2x2_backward_workspace_bytes(n, h, w, c)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
    dx = torch.empty_like(x, memory_format=torch.channels_last) if want[0] else None
    dln_w, dln_b = (torch.empty((c,), dtype=torch.float32, device=x.device) if f else None for f in want[1:])
    launch("gdrnpp_layernorm_patch2x2_backward", px, opt_f32_ptr(ln_weight, "ln_weight"), f32_ptr(d_a, "d_a"),
           *(t.data_ptr() if t is not None else None for t in (dx, dln_w, dln_b)), n, h, w, c, float(eps), ws.data_ptr(), nbytes,
           timed=("hbm:ln_patch2x2_bwd", 0.0, 4.0 * x.numel() * (2 + want[0])))
    return dx, dln_w, dln_b


def downsample_weight_nk(weight):
    """nn.Conv2d weight [Cout,C,2,2] -> Wp f32[Cout, 4 C], column (ky, kx, ci): the nn.Linear form of the convolution over
    ``layernorm_patch2x2``'s rows.  A view when the weight is held channels_last."""
    cout, c = weight.shape[:2]
    return weight.detach().permute(0, 2, 3, 1).reshape(cout, 4 * c).contiguous()


def downsample_backward(x, a, ln_weight, eps: float, weight, dz, want=(True,) * 5):
    """Gradients of z = conv2x2/2(LayerNorm2d(x)) run as z2d = A Wp^T + b with A = ``layernorm_patch2x2(x, ...)`` and Wp =
    ``downsample_weight_nk(weight)``, for dz = dL/dz (N,Cout,H/2,W/2) channels_last -> (dx, dln_weight, dln_bias, dweight [Cout,C,2,2],
    dbias).  ``want``: five flags in that order — an entry is None where its flag is false and the launches only it needs are left out;
    the others keep their bits.  dA = dz Wp on ``linear_f32_exact``, then ``layernorm_patch2x2_backward``; dWp = dz^T A on
    ``gemm_tn_f32`` (its slot tiles in the persistent workspace), returned as the [Cout,C,2,2] view of [Cout,2,2,C]; dbias =
    ``colsum_f32``.  ``a`` is needed for dweight alone (None otherwise)."""
    what = "downsample_backward"
    want = _want(what, want, 5)
    n, c, h, w = x.shape
    cout = weight.shape[0]
    if tuple(weight.shape) != (cout, c, 2, 2) or tuple(dz.shape) != (n, cout, h // 2, w // 2):
        raise RuntimeError(f"{what}: weight {tuple(weight.shape)} / dz {tuple(dz.shape)} do not fit x {tuple(x.shape)}")
    nhwc_ptr(dz, "dz")
    dz2d = dz.permute(0, 2, 3, 1).reshape(n * (h // 2) * (w // 2), cout)      # a view of the NHWC memory
    dx = dln_w = dln_b = dweight = dbias = None
    if any(want[:3]):
        d_a = linear_f32_exact(dz2d, downsample_weight_nk(weight), weight_kn=True)
        dx, dln_w, dln_b = layernorm_patch2x2_backward(x, ln_weight, eps, d_a, want=want[:3])
    if want[3]:
        if a is None or tuple(a.shape) != (dz2d.shape[0], 4 * c):
            raise RuntimeError(f"{what}: dweight needs a f32[{dz2d.shape[0]},{4 * c}]")
        dweight = gemm_tn_f32(dz2d, a, persistent_ws=True).view(cout, 2, 2, c).permute(0, 3, 1, 2)
    if want[4]:
        dbias = colsum_f32(dz2d)[1]
    return dx, dln_w, dln_b, dweight, dbias


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


def head_tail_backward(out_nhwc, extents, double_mask: bool, g_pnp_in=None, g_planes=None, g_out=None):
    """Adjoint of ``head_tail_nhwc`` (``gdrnpp_head_tail_backward_nhwc``) -> d_out f32[B*HW, pitch]: the gradient of the class-sliced
    output layer's result from the gradients of pnp_in f32[B, HW, 96], of planes f32[P, B, HW] and the one that reached ``out_nhwc``
    directly (the region map is a view of it).  Each may be None: it contributes nothing and is not read.  The columns from the
    layer's width on are 0."""
    bhw, pitch = out_nhwc.shape
    b = extents.shape[0]
    hw = bhw // b
    n_planes = 5 if double_mask else 4
    if b * hw != bhw or tuple(extents.shape) != (b, 3):
        raise RuntimeError(f"head_tail_backward: out {tuple(out_nhwc.shape)} does not fit extents {tuple(extents.shape)}")
    for name, g, shape in (("g_pnp_in", g_pnp_in, (b * hw * 96,)), ("g_planes", g_planes, (n_planes * b * hw,)), ("g_out", g_out, (bhw * pitch,))):
        if g is not None and g.numel() != shape[0]:
            raise RuntimeError(f"head_tail_backward: {name} has {g.numel()} elements, {shape[0]} expected")
    d_out = torch.empty((bhw, pitch), dtype=torch.float32, device=out_nhwc.device)
    n_in = sum(g is not None for g in (g_pnp_in, g_planes, g_out))
    launch("gdrnpp_head_tail_backward_nhwc", f32_ptr(out_nhwc, "out_nhwc"), pitch, f32_ptr(extents, "extents"), opt_f32_ptr(g_pnp_in, "g_pnp_in"),
           opt_f32_ptr(g_planes, "g_planes"), opt_f32_ptr(g_out, "g_out"), d_out.data_ptr(), b, hw, 1 if double_mask else 0,
           timed=("hbm:head_tail_bwd", 0.0, 4.0 * bhw * (pitch + (72 + 96 if g_pnp_in is not None else 0) + (n_planes if g_planes is not None else 0)
                                                        + (72 if g_out is not None else 0)) if n_in else 4.0 * bhw * pitch))
    return d_out


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


# ---- GDRN's training losses (csrc/gdrn_loss.hip) ----------------------------------------------------------------------------------------
LOSS_MASKS = ("trunc", "visib", "obj", "full")     # LOSS_CFG.*_MASK_GT / MASK_LOSS_GT -> the kernels' mask selector (roi.ROI_BIN_MASKS's order)
DENSE_XYZ_TYPES = {"L1": 0, "CE_coor": 1}
DENSE_MASK_TYPES = {"L1": 0, "BCE": 1}
PM_TYPES = {"L1": 0, "Smooth_L1": 1, "MSE": 2}
DENSE_SUMS = ("x", "y", "z", "mask", "mask_full", "region", "n_xyz", "n_region")      # the f64[8] of gdrn_dense_losses


def _dense_args(what, out_x, out_y, out_z, out_mask, out_mask_full, out_region, gt_xyz, gt_xyz_bin, gt_region, masks, xyz_type, xyz_mask,
                mask_type, mask_gt, full_type, region_mask):
    """The checks and the argument tuple that ``gdrn_dense_losses`` and its backward share -> (args, B, o, Cx, Cr)."""
    for name, table, v in (("xyz_type", DENSE_XYZ_TYPES, xyz_type), ("mask_type", DENSE_MASK_TYPES, mask_type), ("full_type", DENSE_MASK_TYPES, full_type)):
        if v not in table:
            raise RuntimeError(f"{what}: {name} must be one of {tuple(table)}, got {v!r}")
    for name, v in (("xyz_mask", xyz_mask), ("mask_gt", mask_gt), ("region_mask", region_mask)):
        if v not in LOSS_MASKS:
            raise RuntimeError(f"{what}: {name} must be one of {LOSS_MASKS}, got {v!r}")
    maps = [("out_x", out_x), ("out_y", out_y), ("out_z", out_z), ("out_mask", out_mask), ("out_mask_full", out_mask_full), ("out_region", out_region)]
    first = next((t for _, t in maps if t is not None), None)
    if first is None or first.dim() != 4 or first.shape[2] != first.shape[3]:
        raise RuntimeError(f"{what}: needs at least one map, f32[B,C,o,o]")
    B, o = int(first.shape[0]), int(first.shape[2])
    masks = dict(masks)
    unknown = set(masks) - set(LOSS_MASKS)
    if unknown:
        raise RuntimeError(f"{what}: unknown masks {sorted(unknown)}; the names are {LOSS_MASKS}")
    mp = []
    for k in LOSS_MASKS:
        m = masks.get(k)
        if m is not None and tuple(m.shape) != (B, o, o):
            raise RuntimeError(f"{what}: mask {k!r} must be f32[{B},{o},{o}], got {tuple(m.shape)}")
        mp.append(opt_f32_ptr(m, f"masks[{k!r}]"))

    def need_mask(term, k):
        if masks.get(k) is None:
            raise RuntimeError(f"{what}: the {term} term selects mask {k!r}, which is missing")

    Cx = Cr = 0
    if (out_x is None) != (out_y is None) or (out_x is None) != (out_z is None):
        raise RuntimeError(f"{what}: out_x, out_y and out_z come together")
    p_gt_xyz = p_gt_bin = p_gt_region = None
    if out_x is not None:
        Cx = int(out_x.shape[1])
        for name, t in maps[:3]:
            if tuple(t.shape) != (B, Cx, o, o):
                raise RuntimeError(f"{what}: {name} must be f32[{B},{Cx},{o},{o}], got {tuple(t.shape)}")
        need_mask("xyz", xyz_mask)
        if xyz_type == "L1":
            if Cx != 1:
                raise RuntimeError(f"{what}: the L1 xyz term takes one channel per axis, got C = {Cx}")
            if gt_xyz is None or tuple(gt_xyz.shape) != (B, 3, o, o):
                raise RuntimeError(f"{what}: gt_xyz must be f32[{B},3,{o},{o}]")
            p_gt_xyz = f32_ptr(gt_xyz, "gt_xyz")
        else:
            if not 2 <= Cx <= 256:
                raise RuntimeError(f"{what}: the CE_coor xyz term takes 2 <= C <= 256 channels, got C = {Cx}")
            if gt_xyz_bin is None or tuple(gt_xyz_bin.shape) != (B, 3, o, o):
                raise RuntimeError(f"{what}: gt_xyz_bin must be u8[{B},3,{o},{o}]")
            p_gt_bin = dev_ptr(gt_xyz_bin, torch.uint8, "gt_xyz_bin")
    for name, t, k in (("out_mask", out_mask, mask_gt), ("out_mask_full", out_mask_full, "full")):
        if t is not None:
            if tuple(t.shape) != (B, 1, o, o):
                raise RuntimeError(f"{what}: {name} must be f32[{B},1,{o},{o}], got {tuple(t.shape)}")
            need_mask(name[4:], k)
    if out_region is not None:
        Cr = int(out_region.shape[1])
        if Cr < 2 or tuple(out_region.shape) != (B, Cr, o, o):
            raise RuntimeError(f"{what}: out_region must be f32[{B},C,{o},{o}] with C >= 2, got {tuple(out_region.shape)}")
        if gt_region is None or tuple(gt_region.shape) != (B, o, o):
            raise RuntimeError(f"{what}: gt_region must be i32[{B},{o},{o}]")
        p_gt_region = dev_ptr(gt_region, torch.int32, "gt_region")
        need_mask("region", region_mask)
    args = (opt_f32_ptr(out_x, "out_x"), opt_f32_ptr(out_y, "out_y"), opt_f32_ptr(out_z, "out_z"), Cx, opt_f32_ptr(out_mask, "out_mask"),
            opt_f32_ptr(out_mask_full, "out_mask_full"), opt_f32_ptr(out_region, "out_region"), Cr, p_gt_xyz, p_gt_bin, p_gt_region, *mp,
            DENSE_XYZ_TYPES[xyz_type], LOSS_MASKS.index(xyz_mask), DENSE_MASK_TYPES[mask_type], LOSS_MASKS.index(mask_gt),
            DENSE_MASK_TYPES[full_type], LOSS_MASKS.index(region_mask), B, o)
    return args, B, o, Cx, Cr


def gdrn_dense_losses(out_x, out_y, out_z, out_mask, out_mask_full, out_region, *, gt_xyz=None, gt_xyz_bin=None, gt_region=None, masks,
                      xyz_type: str = "L1", xyz_mask: str = "visib", mask_type: str = "L1", mask_gt: str = "trunc", full_type: str = "BCE",
                      region_mask: str = "visib"):
    """``gdrnpp_gdrn_dense_losses``: gdrn_loss's terms over the head's maps in one pass -> (sums f64[8] in the order of ``DENSE_SUMS``,
    bad i32[1] = targets outside [0, C), which are left out).  out_x / out_y / out_z f32[B,C,o,o] (C = 1 for "L1", n_bin + 1 for "CE_coor"),
    out_mask / out_mask_full f32[B,1,o,o], out_region f32[B,C,o,o]; a map given as None has no term.  gt_xyz f32[B,3,o,o] or gt_xyz_bin
    u8[B,3,o,o], gt_region i32[B,o,o], masks {name of ``LOSS_MASKS``: f32[B,o,o]}: the dtypes of ``roi_train_targets``."""
    what = "gdrn_dense_losses"
    args, B, o, _, _ = _dense_args(what, out_x, out_y, out_z, out_mask, out_mask_full, out_region, gt_xyz, gt_xyz_bin, gt_region, masks, xyz_type,
                                   xyz_mask, mask_type, mask_gt, full_type, region_mask)
    dev = next(t for t in (out_x, out_mask, out_mask_full, out_region) if t is not None).device
    nbytes = load().gdrnpp_gdrn_dense_losses_workspace_bytes(B, o)
    if nbytes == 0:
        raise RuntimeError(f"{what}: B = {B}, o = {o}: too many pixels for one launch")
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    sums = torch.empty((8,), dtype=torch.float64, device=dev)
    bad = torch.empty((1,), dtype=torch.int32, device=dev)
    launch("gdrnpp_gdrn_dense_losses", *args, sums.data_ptr(), bad.data_ptr(), ws.data_ptr(), nbytes)
    return sums, bad


def gdrn_dense_losses_backward(out_x, out_y, out_z, out_mask, out_mask_full, out_region, sums, scale, *, want, gt_xyz=None, gt_xyz_bin=None,
                               gt_region=None, masks, xyz_type: str = "L1", xyz_mask: str = "visib", mask_type: str = "L1",
                               mask_gt: str = "trunc", full_type: str = "BCE", region_mask: str = "visib"):
    """``gdrnpp_gdrn_dense_losses_backward``: the gradients of sum_k scale[k] * term_k with respect to the maps, recomputed from the forward's
    inputs -> (g_x, g_y, g_z, g_mask, g_mask_full, g_region), None where ``want`` (six flags in that order) is false: no tensor is
    allocated or written for it.  sums f64[8]: ``gdrn_dense_losses``'s result; scale f32[6] = grad_output * weight per term (x, y, z, mask,
    full mask, region).  Both stay on the device."""
    what = "gdrn_dense_losses_backward"
    maps = (out_x, out_y, out_z, out_mask, out_mask_full, out_region)
    want = tuple(bool(w) for w in want)
    if len(want) != 6 or any(w and t is None for w, t in zip(want, maps)):
        raise RuntimeError(f"{what}: want must hold six flags and name only maps that are given")
    args, B, o, _, _ = _dense_args(what, out_x, out_y, out_z, out_mask, out_mask_full, out_region, gt_xyz, gt_xyz_bin, gt_region, masks, xyz_type,
                                   xyz_mask, mask_type, mask_gt, full_type, region_mask)
    if sums.numel() != 8 or scale.numel() != 6:
        raise RuntimeError(f"{what}: sums f64[8] and scale f32[6], got {tuple(sums.shape)} and {tuple(scale.shape)}")
    grads = tuple(torch.empty_like(t) if w else None for w, t in zip(want, maps))
    launch("gdrnpp_gdrn_dense_losses_backward", *args, dev_ptr(sums, torch.float64, "sums"), f32_ptr(scale, "scale"),
           *(g.data_ptr() if g is not None else None for g in grads))
    return grads


def gdrn_pose_losses(R_pred, R_gt, obj, points, *, t_pred=None, t_gt=None, sym_rots=None, sym_off=None, extents=None, pred_t_=None,
                     gt_trans_ratio=None, gt_trans=None, symmetric: bool = False, r_only: bool = True, z_type: str = "REL",
                     pm_type: str = "L1", beta: float = 1.0):
    """``gdrnpp_gdrn_pose_losses``: the per-ROI terms in fp64 -> (sums f64[3] = the PM, centroid and z sums, R_gt' f32[B,3,3] = the closest
    symmetric ground truth, dR f32[B,3,3] and dt f32[B,3] = d sums[0] / d R_pred, t_pred, dpt f32[B,3] = d sums[1] / d pred_t_[:, :2] and
    d sums[2] / d pred_t_[:, 2]; dpt is None without pred_t_).  R_pred, R_gt f32[B,3,3|9]; obj i32[B] into points f32[n_obj,P,3], extents
    f32[n_obj,3] (given = PM_NORM_BY_EXTENT) and sym_off i32[n_obj+1] into sym_rots f64[n_sym,3,3|9] (``pose_errors``'s layout; an empty
    range is an asymmetric object).  t_pred / t_gt f32[B,3] are needed unless r_only; pred_t_, gt_trans_ratio, gt_trans f32[B,3]."""
    what = "gdrn_pose_losses"
    B = int(R_pred.shape[0])
    if R_pred.numel() != 9 * B or R_gt.numel() != 9 * B or obj.numel() != B or B == 0:
        raise RuntimeError(f"{what}: R_pred, R_gt f32[B,3,3] and obj i32[B] with B > 0, got {tuple(R_pred.shape)}, {tuple(R_gt.shape)}, {tuple(obj.shape)}")
    if points.dim() != 3 or points.shape[2] != 3 or points.shape[0] == 0 or points.shape[1] == 0:
        raise RuntimeError(f"{what}: points must be f32[n_obj,P,3], got {tuple(points.shape)}")
    n_obj, P = int(points.shape[0]), int(points.shape[1])
    if pm_type not in PM_TYPES or z_type not in ("REL", "ABS"):
        raise RuntimeError(f"{what}: pm_type one of {tuple(PM_TYPES)}, z_type REL or ABS; got {pm_type!r}, {z_type!r}")
    for name, t in (("t_pred", t_pred), ("t_gt", t_gt), ("pred_t_", pred_t_), ("gt_trans_ratio", gt_trans_ratio), ("gt_trans", gt_trans)):
        if t is not None and tuple(t.shape) != (B, 3):
            raise RuntimeError(f"{what}: {name} must be f32[{B},3], got {tuple(t.shape)}")
    if not r_only and (t_pred is None or t_gt is None):
        raise RuntimeError(f"{what}: r_only=False needs t_pred and t_gt")
    if pred_t_ is not None and (gt_trans_ratio is None or (z_type == "ABS" and gt_trans is None)):
        raise RuntimeError(f"{what}: pred_t_ needs gt_trans_ratio, and gt_trans with z_type ABS")
    if extents is not None and tuple(extents.shape) != (n_obj, 3):
        raise RuntimeError(f"{what}: extents must be f32[{n_obj},3], got {tuple(extents.shape)}")
    sp = so = None
    n_sym = 0
    if symmetric:
        if sym_rots is None or sym_off is None:
            raise RuntimeError(f"{what}: symmetric needs sym_rots and sym_off")
        if sym_off.numel() != n_obj + 1 or sym_rots.numel() % 9:
            raise RuntimeError(f"{what}: sym_off must hold n_obj + 1 = {n_obj + 1} offsets into sym_rots f64[n_sym,9]")
        n_sym = sym_rots.numel() // 9
        sp, so = dev_ptr(sym_rots, torch.float64, "sym_rots") if n_sym else None, dev_ptr(sym_off, torch.int32, "sym_off")
    dev = R_pred.device
    sums = torch.empty((3,), dtype=torch.float64, device=dev)
    R_sel = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    dR = torch.empty((B, 3, 3), dtype=torch.float32, device=dev)
    dt = torch.empty((B, 3), dtype=torch.float32, device=dev)
    dpt = torch.empty((B, 3), dtype=torch.float32, device=dev) if pred_t_ is not None else None
    nbytes = load().gdrnpp_gdrn_pose_losses_workspace_bytes(B)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=dev)
    launch("gdrnpp_gdrn_pose_losses", f32_ptr(R_pred, "R_pred"), f32_ptr(R_gt, "R_gt"), opt_f32_ptr(t_pred, "t_pred"), opt_f32_ptr(t_gt, "t_gt"),
           dev_ptr(obj, torch.int32, "obj"), f32_ptr(points, "points"), n_obj, P, sp, so, n_sym, opt_f32_ptr(extents, "extents"),
           opt_f32_ptr(pred_t_, "pred_t_"), opt_f32_ptr(gt_trans_ratio, "gt_trans_ratio"), opt_f32_ptr(gt_trans, "gt_trans"),
           1 if symmetric else 0, 1 if r_only else 0, 0 if z_type == "REL" else 1, PM_TYPES[pm_type], float(beta), B, sums.data_ptr(),
           R_sel.data_ptr(), dR.data_ptr(), dt.data_ptr(), dpt.data_ptr() if dpt is not None else None, ws.data_ptr(), nbytes)
    return sums, R_sel, dR, dt, dpt


# ---- Ranger optimiser step over all tensors of an optimiser (csrc/ranger.hip) ------------------------------------------------------------
RANGER_TILE = DEFINES["GDRNPP_RANGER_TILE"]          # elements per work item (one workgroup, the piece of the gradient it holds in LDS)
RANGER_RECTIFIED, RANGER_LOOKAHEAD, RANGER_NAN_TO_NUM = (DEFINES["GDRNPP_RANGER_" + k] for k in ("RECTIFIED", "LOOKAHEAD", "NAN_TO_NUM"))
RANGER_TENSOR, RANGER_WORK, RANGER_LONG_ROW = (np.dtype(STRUCTS["gdrnpp_ranger_" + k]) for k in ("tensor", "work", "long_row"))
RANGER_COEFS = tuple(k for k in RANGER_TENSOR.names if RANGER_TENSOR[k] == np.float32)      # beta1 .. step_lr, the struct's float members


def ranger_plan(numels, row_lens, tile: int = RANGER_TILE):
    """The work items of ``gdrnpp_ranger_step`` for tensors of ``numels`` elements -> (work ``RANGER_WORK``[n_work], long_rows
    ``RANGER_LONG_ROW``[n_long]).  row_len 0: pieces of ``tile`` elements.  0 < row_len <= tile: runs of whole rows, as many as fit a tile —
    a multiple of 4 rows where 4 fit, so that every item starts on a 16-byte boundary of the tensor whatever the row length.  row_len >
    tile: every row is a long row with a slot for its mean and is cut into pieces inside it.  Host code, no device needed."""
    work, long_rows = [], []
    n_long = 0
    for t, (n, L) in enumerate(zip(numels, row_lens)):
        n, L = int(n), int(L)
        if n == 0:
            continue
        if L < 0 or (L and n % L):
            raise RuntimeError(f"ranger_plan: tensor {t}: row_len {L} does not divide numel {n}")
        slot = None
        if L == 0:
            start = np.arange(0, n, tile, dtype=np.int64)
            count = np.minimum(tile, n - start)
        elif L <= tile:
            per = tile // L
            per -= per % 4 if per >= 4 else 0
            start = np.arange(0, n, per * L, dtype=np.int64)
            count = np.minimum(per * L, n - start)
        else:
            rows = n // L
            inner = np.arange(0, L, tile, dtype=np.int64)
            start = (np.arange(rows, dtype=np.int64)[:, None] * L + inner[None, :]).reshape(-1)
            count = np.tile(np.minimum(tile, L - inner), rows)
            slot = np.repeat(np.arange(n_long, n_long + rows, dtype=np.int64), len(inner))
            lr = np.zeros(rows, RANGER_LONG_ROW)
            lr["row"], lr["tensor"] = np.arange(rows), t
            long_rows.append(lr)
            n_long += rows
        w = np.zeros(len(start), RANGER_WORK)
        w["start"], w["tensor"], w["count"], w["mean_slot"] = start, t, count, -1 if slot is None else slot
        work.append(w)
    return (np.concatenate(work) if work else np.zeros(0, RANGER_WORK),
            np.concatenate(long_rows) if long_rows else np.zeros(0, RANGER_LONG_ROW))


class RangerTables:
    """What one optimiser keeps between steps for ``ranger_step``: per layout (the numels and row lengths of the tensors that have a
    gradient) the work items on the device, the device copy of the per-tensor table, and pinned staging buffers for its upload.  A staging
    buffer is written again only after the event recorded behind its copy has completed (``query``, never a wait: if none is free, another
    one is allocated), so a step neither waits for the device nor disturbs a copy that is still in flight."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.plans = {}          # (numels, row_lens) -> (n_work, work on the device, n_long, long rows on the device, means f32[n_long], pinned sources)
        self.staging = []        # [pinned uint8 buffer, event recorded after its last copy]
        self.table = None        # uint8 device buffer of the per-tensor table
        self.uploads = 0         # asynchronous table copies issued (one per step)

    def close(self):
        """Wait for the device and drop the tables and the staging buffers (their memory goes back to torch's allocators here and now)."""
        torch.cuda.synchronize(self.device)
        self.plans, self.staging, self.table = {}, [], None

    def _pinned(self, nbytes):
        for slot in self.staging:
            if slot[0].numel() >= nbytes and slot[1].query():
                return slot
        slot = [torch.empty((max(nbytes, 4096),), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        self.staging.append(slot)
        return slot

    def _upload(self, host_bytes, dst):
        """One asynchronous host-to-device copy of ``host_bytes`` (uint8 ndarray) through a free pinned buffer."""
        slot = self._pinned(host_bytes.size)
        slot[0].numpy()[:host_bytes.size] = host_bytes
        dst[:host_bytes.size].copy_(slot[0][:host_bytes.size], non_blocking=True)
        slot[1].record()

    def plan(self, numels, row_lens):
        key = (tuple(numels), tuple(row_lens))
        hit = self.plans.get(key)
        if hit is None:
            work, long_rows = ranger_plan(numels, row_lens)
            dev = []
            for a in (work, long_rows):
                d = torch.empty((max(a.nbytes, 16),), dtype=torch.uint8, device=self.device)
                if a.nbytes:
                    self._upload(a.view(np.uint8).reshape(-1), d)
                dev.append(d)
            means = torch.empty((max(len(long_rows), 1),), dtype=torch.float32, device=self.device)
            hit = self.plans[key] = (len(work), dev[0], len(long_rows), dev[1], means)
        return hit


def ranger_tensor_ok(t, like=None) -> bool:
    """Whether ``ranger_step`` takes ``t``: an fp32 device tensor that is dense with dimension 0 outermost (contiguous, or 4-D
    channels_last: a row of numel / shape[0] elements is one run of memory either way) and, given ``like``, laid out as ``like`` is."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float32 or t.is_sparse:
        return False
    if not (t.is_contiguous() or (t.dim() == 4 and t.is_contiguous(memory_format=torch.channels_last))):
        return False
    return like is None or (t.shape == like.shape and t.device == like.device and ranger_same_layout(t, like))


def ranger_same_layout(t, like) -> bool:
    """Equal strides wherever a dimension has more than one element (the stride of a dimension of one element places nothing: a [C,1,7,7]
    weight is contiguous and channels_last at once, and torch reports either set of strides for it)."""
    a, b = t.stride(), like.stride()
    return a == b or all(x == y for x, y, n in zip(a, b, like.shape) if n > 1)


def ranger_step(tables: RangerTables, params, grads, exp_avgs, exp_avg_sqs, slows, row_lens, flags, coefs, validate: bool = True):
    """``gdrnpp_ranger_step``: one Ranger step of every listed tensor, in place, in one launch (two with centralised rows longer than
    ``RANGER_TILE``).  Five lists of f32 device tensors, tensor i of every list laid out alike (``ranger_tensor_ok``); row_lens[i] = numel / shape[0] where the gradient is
    centralised, else 0; flags[i] = RANGER_RECTIFIED | RANGER_LOOKAHEAD | RANGER_NAN_TO_NUM; coefs[i] = the eight numbers of
    ``RANGER_COEFS``, rounded to fp32 here.  The per-tensor table is rebuilt on the host and uploaded with one asynchronous copy on the
    current stream; nothing is read back and nothing waits.  ``validate=False`` is for a caller that has just held every tensor to
    ``ranger_tensor_ok`` itself (``solver.Ranger``): the per-tensor checks are the larger part of this function's host time."""
    n = len(params)
    if not (len(grads) == len(exp_avgs) == len(exp_avg_sqs) == len(slows) == len(row_lens) == len(flags) == len(coefs) == n):
        raise RuntimeError("ranger_step: the per-tensor lists differ in length")
    if n == 0:
        return
    host = np.zeros(n, RANGER_TENSOR)
    numels = [int(p.numel()) for p in params]
    for field, ts in (("p", params), ("g", grads), ("m", exp_avgs), ("v", exp_avg_sqs), ("slow", slows)):
        if validate:
            for i, t in enumerate(ts):
                if not ranger_tensor_ok(t, params[i]) or t.device != tables.device:
                    raise RuntimeError(f"ranger_step: {field}[{i}] must be a dense float32 tensor on {tables.device}, shaped and laid out as p[{i}] "
                                       f"{tuple(params[i].shape)} is")
        host[field] = [t.data_ptr() for t in ts]
    host["numel"], host["row_len"], host["flags"] = numels, row_lens, flags
    c = np.asarray(coefs, dtype=np.float64).reshape(n, len(RANGER_COEFS)).astype(np.float32)
    for j, k in enumerate(RANGER_COEFS):
        host[k] = c[:, j]
    n_work, work, n_long, long_rows, means = tables.plan(numels, [int(L) for L in row_lens])
    if n_work == 0:
        return
    nbytes = host.nbytes
    if tables.table is None or tables.table.numel() < nbytes:
        tables.table = torch.empty((2 * nbytes,), dtype=torch.uint8, device=tables.device)
    tables._upload(host.view(np.uint8).reshape(-1), tables.table)
    tables.uploads += 1
    launch("gdrnpp_ranger_step", tables.table.data_ptr(), n, work.data_ptr(), n_work, long_rows.data_ptr() if n_long else None, n_long,
           means.data_ptr() if n_long else None)


# ---- ModelEMA update over all floating-point tensors of a model (csrc/model_ema.hip) ------------------------------------------------------
# The header declares the two tables as bytes and describes their records in its comment; csrc/model_ema.hip asserts the same offsets.
EMA_TILE = 8192                                      # elements per work item (one workgroup): the kernel's GDRNPP_EMA_TILE, its straight-line path
EMA_TENSOR = np.dtype({"names": ["ema", "model", "numel"], "formats": ["<u8", "<u8", "<i8"], "offsets": [0, 8, 16], "itemsize": 24})
EMA_WORK = np.dtype({"names": ["start", "tensor", "count"], "formats": ["<i8", "<i4", "<i4"], "offsets": [0, 8, 12], "itemsize": 16})


def ema_plan(numels, tile: int = EMA_TILE):
    """The work items of ``gdrnpp_model_ema_update`` for tensors of ``numels`` elements -> ``EMA_WORK``[n_work]: every tensor cut into
    pieces of ``tile`` elements and a shorter last one; an empty tensor gets none.  Host code, no device needed."""
    work = []
    for t, n in enumerate(numels):
        start = np.arange(0, int(n), tile, dtype=np.int64)
        w = np.zeros(len(start), EMA_WORK)
        w["start"], w["tensor"], w["count"] = start, t, np.minimum(tile, int(n) - start)
        work.append(w)
    return np.concatenate(work) if work else np.zeros(0, EMA_WORK)


class EmaTables:
    """What one ``ModelEMA`` keeps between updates for ``ema_update``: the per-tensor table and the work items on the device, under the
    key they were built from (the ``(data_ptr, numel)`` of every EMA and model tensor), and the pinned staging buffers of their upload.
    Unlike the Ranger step's table nothing here changes from one update to the next (the coefficients are arguments of the launch), so
    a steady-state update uploads nothing; the tables are built again when the key changes (a parameter's ``.data`` replaced, a model
    moved)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.key = None
        self.n_tensors = self.n_work = self.numel = 0
        self.table = self.work = None        # uint8 device buffers
        self.staging = []                    # pinned uint8 buffers of the last build, kept until the next one (their copies are asynchronous)
        self.uploads = 0                     # asynchronous table copies issued so far (two per build)
        self.builds = 0

    def close(self):
        """Wait for the device and drop the tables and the staging buffers (their memory goes back to torch's allocators here and now)."""
        torch.cuda.synchronize(self.device)
        self.key, self.table, self.work, self.staging = None, None, None, []
        self.n_tensors = self.n_work = self.numel = 0

    def _upload(self, host):
        src = torch.empty((max(host.nbytes, 16),), dtype=torch.uint8, pin_memory=True)
        src.numpy()[:host.nbytes] = host.view(np.uint8).reshape(-1)
        dst = torch.empty((src.numel(),), dtype=torch.uint8, device=self.device)
        dst.copy_(src, non_blocking=True)
        self.staging.append(src)
        self.uploads += 1
        return dst

    def build(self, key, ema_tensors, model_tensors):
        if self.staging:         # a rebuild: the copies of the last build may still read the buffers about to be dropped
            torch.cuda.synchronize(self.device)
        self.staging = []
        host = np.zeros(len(ema_tensors), EMA_TENSOR)
        host["ema"] = [t.data_ptr() for t in ema_tensors]
        host["model"] = [t.data_ptr() for t in model_tensors]
        host["numel"] = [t.numel() for t in ema_tensors]
        work = ema_plan(host["numel"])
        self.n_tensors, self.n_work, self.numel = len(host), len(work), int(host["numel"].sum())
        self.table, self.work = (self._upload(host), self._upload(work)) if len(work) else (None, None)
        self.key = key
        self.builds += 1


def ema_tensor_ok(e, m) -> bool:
    """Whether ``ema_update`` takes the pair: both dense fp32 tensors on one GPU (contiguous, or 4-D channels_last), of one shape and
    one layout (``ranger_same_layout``: element i of one is element i of the other in memory order)."""
    return ranger_tensor_ok(e) and ranger_tensor_ok(m, e)


def ema_update(tables: EmaTables, ema_tensors, model_tensors, decay: float, one_minus_decay: float, validate: bool = True):
    """``gdrnpp_model_ema_update``: ``e = fadd(fmul(e, decay), fmul(one_minus_decay, m))`` over every listed pair, in place, in one launch.
    Two lists of f32 device tensors, pair i laid out alike (``ema_tensor_ok``).  The coefficients are rounded to fp32 here and passed by
    value.  The device tables are those of ``tables`` while the ``(data_ptr, numel)`` of both lists are the ones they were built from,
    else they are built and uploaded now (two asynchronous copies); nothing is read back and nothing waits.  ``validate=False`` is for a
    caller that has just held every pair to ``ema_tensor_ok`` itself (``ModelEMA``).  The caller advances the EMA tensors' version counters."""
    n = len(ema_tensors)
    if len(model_tensors) != n:
        raise RuntimeError("ema_update: the two lists differ in length")
    if n == 0:
        return
    if validate:
        for i, (e, m) in enumerate(zip(ema_tensors, model_tensors)):
            if not ema_tensor_ok(e, m) or e.device != tables.device:
                raise RuntimeError(f"ema_update: pair {i} must be two dense float32 tensors on {tables.device} of one shape and layout, got "
                                   f"{tuple(e.shape)} {e.dtype} {e.device} and {tuple(m.shape)} {m.dtype} {m.device}")
    key = tuple((e.data_ptr(), m.data_ptr(), e.numel()) for e, m in zip(ema_tensors, model_tensors))
    if key != tables.key:
        tables.build(key, ema_tensors, model_tensors)
    if tables.n_work == 0:
        return
    launch("gdrnpp_model_ema_update", tables.table.data_ptr(), tables.n_tensors, tables.work.data_ptr(), tables.n_work,
           float(np.float32(decay)), float(np.float32(one_minus_decay)), timed=("hbm:model_ema", 0.0, 12.0 * tables.numel))
