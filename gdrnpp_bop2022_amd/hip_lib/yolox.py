"""The YOLOX detector: its forward on NHWC slice buffers (csrc/yolox_net.hip), its two ends, letterbox and
post-processing (csrc/yolox_pre.hip), and its training: SimOTA assignment and losses (csrc/yolox_loss.hip) and the forward and backward
of a [convolution, BatchNorm with batch statistics, SiLU] layer (csrc/conv_bn_bwd.hip), and its training batches: mosaic, affine, mixup,
HSV, mirror and preproc for a batch in one call (csrc/yolox_aug.hip)."""
from __future__ import annotations

import torch

from .abi import DEFINES, channels_last_f32, dev_ptr, f32_ptr, launch, load, opt_f32_ptr
from .cv_resize import RESIZE_MODES


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
    launch("gdrnpp_yolox_postprocess", f32_ptr(det_preds, "det_preds"), b, a, num_classes, float(conf_thre), float(nms_thre),
           1 if class_agnostic else 0, dets.data_ptr(), count.data_ptr(), max_det, ws.data_ptr(), nbytes)
    return dets, count


CONV_ACTS = {k: DEFINES["GDRNPP_ACT_" + k.upper()] for k in ("none", "silu", "sigmoid", "yolox_box")}


def pack_conv_weight_kmajor(weight: torch.Tensor) -> torch.Tensor:
    """Conv2d weight f32[Cout,Cin,k,k] -> the B operand of ``gdrnpp_conv_bias_act_f32``: f32[k*k*Cin, ldw], row
    (ky * k + kx) * Cin + ci, column = output channel, ldw = Cout rounded up to 4 (zero columns)."""
    cout, cin, kh, kw = weight.shape
    ldw = (cout + 3) // 4 * 4
    out = torch.zeros((kh * kw * cin, ldw), dtype=torch.float32, device=weight.device)
    out[:, :cout] = weight.detach().float().permute(2, 3, 1, 0).reshape(kh * kw * cin, cout)
    return out


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
    launch("gdrnpp_conv_bias_act_f32", f32_ptr(a, "a"), lda, a_off, f32_ptr(w_kmajor, "weight"), w_kmajor.shape[1], opt_f32_ptr(bias, "bias"),
           opt_f32_ptr(res, "res"), 0 if res is None else res.shape[-1], r_off, f32_ptr(c, "c"), ldc, c_off, c_img_rows, c_row0,
           b, h, w, cin, cout, ks, stride, CONV_ACTS[act], float(dec_stride),
           timed=("mfma_f32:conv_bias_act", 2.0 * b * oh * ow * cout * ks * ks * cin,
                  4.0 * b * (h * w * cin + oh * ow * cout) + 4.0 * cout * ks * ks * cin))
    return c


def yolox_focus(x_nchw, y, y_off: int = 0):
    """``gdrnpp_yolox_focus``: x f32[B,3,H,W] -> 12 channels at y_off of y f32[B,H/2,W/2,ldy]."""
    b, ch, h, w = x_nchw.shape
    if ch != 3 or tuple(y.shape[:3]) != (b, h // 2, w // 2):
        raise RuntimeError(f"yolox_focus: x [B,3,H,W] -> y [B,H/2,W/2,ldy], got {tuple(x_nchw.shape)} -> {tuple(y.shape)}")
    launch("gdrnpp_yolox_focus", f32_ptr(x_nchw, "x"), f32_ptr(y, "y"), y.shape[-1], y_off, b, h, w)
    return y


def spp_maxpool_5_9_13(buf, off: int, c: int):
    """``gdrnpp_spp_maxpool_5_9_13`` on buf f32[B,H,W,ld]: channels [off, off + c) -> their 5 / 9 / 13 max pools in the next three
    slices of c channels."""
    b, h, w, ld = buf.shape
    launch("gdrnpp_spp_maxpool_5_9_13", f32_ptr(buf, "buf"), ld, off, c, b, h, w)
    return buf


def upsample_nearest2x_slice(x, x_off: int, y, y_off: int, c: int):
    """``gdrnpp_upsample_nearest2x_slice``: channels [x_off, x_off + c) of x f32[B,h,w,ldx] -> [y_off, y_off + c) of y f32[B,2h,2w,ldy]."""
    b, h, w, ldx = x.shape
    if tuple(y.shape[:3]) != (b, 2 * h, 2 * w):
        raise RuntimeError(f"upsample_nearest2x_slice: y must be [{b},{2 * h},{2 * w},ldy], got {tuple(y.shape)}")
    launch("gdrnpp_upsample_nearest2x_slice", f32_ptr(x, "x"), ldx, x_off, f32_ptr(y, "y"), y.shape[-1], y_off, b, h, w, c)
    return y


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
    launch("gdrnpp_yolox_letterbox", dev_ptr(images_u8, torch.uint8, "images"), b, H, W, rh, rw, f32_ptr(out, "out"), ht, wt,
           1 if focus else 0, out.shape[-1] if focus else 0, int(y_off) if focus else 0)
    return out, r


YOLOX_IOU_LOSSES = {"iou": 0, "giou": 1}
YOLOX_CLS_LOSSES = {"bce": 0, "focal": 1}
YOLOX_LOSS_KEYS = ("loss_iou", "loss_conf", "loss_l1", "loss_cls")      # the order of ``yolox_losses``'s result and of ``scale``


def _yolox_train_args(what: str, raw, anchors, labels):
    if raw.dim() != 3 or raw.shape[-1] < 6:
        raise RuntimeError(f"{what}: raw must be f32[B,A,5+C], got {tuple(raw.shape)}")
    b, a, s = raw.shape
    if tuple(anchors.shape) != (a, 3):
        raise RuntimeError(f"{what}: anchors must be f32[{a},3] (x_shift, y_shift, stride), got {tuple(anchors.shape)}")
    if labels.dim() != 3 or labels.shape[0] != b or labels.shape[2] != 5:
        raise RuntimeError(f"{what}: labels must be f32[{b},G,5] (class, cx, cy, w, h), got {tuple(labels.shape)}")
    return (f32_ptr(raw, "raw"), f32_ptr(anchors, "anchors"), f32_ptr(labels, "labels")), b, a, s - 5, labels.shape[1]


def yolox_assign(raw, anchors, labels):
    """``gdrnpp_yolox_assign``: SimOTA for the whole batch, nothing read back.  raw f32[B,A,5+C] (the head's undecoded rows), anchors
    f32[A,3], labels f32[B,G,5] -> (matched_gt i32[B,A] with -1 = background, matched_iou f32[B,A], num_fg i32[B], num_gt i32[B])."""
    what = "yolox_assign"
    ptrs, b, a, c, g = _yolox_train_args(what, raw, anchors, labels)
    dev = raw.device
    nbytes = load().gdrnpp_yolox_assign_workspace_bytes(b, a)
    if nbytes == 0:
        raise RuntimeError(f"{what}: B = {b}, A = {a}: too many anchors for one launch")
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=dev)
    matched_gt = torch.empty((b, a), dtype=torch.int32, device=dev)
    matched_iou = torch.empty((b, a), dtype=torch.float32, device=dev)
    num_fg = torch.empty((b,), dtype=torch.int32, device=dev)
    num_gt = torch.empty((b,), dtype=torch.int32, device=dev)
    launch("gdrnpp_yolox_assign", *ptrs, b, a, c, g, matched_gt.data_ptr(), matched_iou.data_ptr(), num_fg.data_ptr(), num_gt.data_ptr(),
           ws.data_ptr(), nbytes)
    return matched_gt, matched_iou, num_fg, num_gt


def _yolox_loss_opts(what: str, iou_loss_type: str, cls_loss_type: str, fl_alpha: float, fl_gamma: float, use_l1: bool):
    if iou_loss_type not in YOLOX_IOU_LOSSES or cls_loss_type not in YOLOX_CLS_LOSSES:
        raise NotImplementedError(f"{what}: iou_loss_type {iou_loss_type!r} / cls_loss_type {cls_loss_type!r}: the kernel has "
                                  f"{tuple(YOLOX_IOU_LOSSES)} and {tuple(YOLOX_CLS_LOSSES)}")
    return YOLOX_IOU_LOSSES[iou_loss_type], YOLOX_CLS_LOSSES[cls_loss_type], float(fl_alpha), float(fl_gamma), 1 if use_l1 else 0


def yolox_losses(raw, anchors, labels, matched_gt, num_fg, num_gt, *, iou_loss_type: str = "iou", cls_loss_type: str = "bce",
                 fl_alpha: float = 0.25, fl_gamma: float = 2.0, use_l1: bool = False):
    """``gdrnpp_yolox_losses`` on ``yolox_assign``'s result -> out f64[6]: the four losses in the order of ``YOLOX_LOSS_KEYS`` (already
    divided by num_fg, loss_iou already times 5), max(sum num_fg, 1), sum num_gt."""
    what = "yolox_losses"
    ptrs, b, a, c, g = _yolox_train_args(what, raw, anchors, labels)
    opts = _yolox_loss_opts(what, iou_loss_type, cls_loss_type, fl_alpha, fl_gamma, use_l1)
    if tuple(matched_gt.shape) != (b, a) or num_fg.numel() != b or num_gt.numel() != b:
        raise RuntimeError(f"{what}: matched_gt i32[{b},{a}], num_fg / num_gt i32[{b}], got {tuple(matched_gt.shape)}, {tuple(num_fg.shape)}, "
                           f"{tuple(num_gt.shape)}")
    nbytes = load().gdrnpp_yolox_losses_workspace_bytes(b, a)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=raw.device)
    out = torch.empty((6,), dtype=torch.float64, device=raw.device)
    launch("gdrnpp_yolox_losses", *ptrs, dev_ptr(matched_gt, torch.int32, "matched_gt"), dev_ptr(num_fg, torch.int32, "num_fg"),
           dev_ptr(num_gt, torch.int32, "num_gt"), b, a, c, g, *opts, out.data_ptr(), ws.data_ptr(), nbytes)
    return out


def yolox_losses_backward(raw, anchors, labels, matched_gt, out, scale, *, iou_loss_type: str = "iou", cls_loss_type: str = "bce",
                          fl_alpha: float = 0.25, fl_gamma: float = 2.0, use_l1: bool = False):
    """``gdrnpp_yolox_losses_backward``: grad_raw f32[B,A,5+C] = the gradient of sum_k scale[k] * loss_k by raw, recomputed from the
    forward's inputs.  out f64[6]: ``yolox_losses``'s result; scale f32[4] in the order of ``YOLOX_LOSS_KEYS``.  Both stay on the device."""
    what = "yolox_losses_backward"
    ptrs, b, a, c, g = _yolox_train_args(what, raw, anchors, labels)
    opts = _yolox_loss_opts(what, iou_loss_type, cls_loss_type, fl_alpha, fl_gamma, use_l1)
    if tuple(matched_gt.shape) != (b, a) or out.numel() != 6 or scale.numel() != 4:
        raise RuntimeError(f"{what}: matched_gt i32[{b},{a}], out f64[6], scale f32[4], got {tuple(matched_gt.shape)}, {tuple(out.shape)}, "
                           f"{tuple(scale.shape)}")
    grad = torch.empty_like(raw)
    launch("gdrnpp_yolox_losses_backward", *ptrs, dev_ptr(matched_gt, torch.int32, "matched_gt"), dev_ptr(out, torch.float64, "out"),
           f32_ptr(scale, "scale"), b, a, c, g, *opts, grad.data_ptr())
    return grad


# ---- training a BaseConv: convolution, BatchNorm2d with batch statistics, SiLU (csrc/conv_bn_bwd.hip) --------------------------------
# All tensors channels_last [N,C,H,W], the NHWC rows the kernels read; the per-channel vectors are f32[C].

def _rows(t_cl, what: str):
    n, c, h, w = channels_last_f32(t_cl, what)
    if t_cl.dim() != 4 or c % 4:
        raise RuntimeError(f"{what}: a 4-D tensor with C % 4 == 0, got {tuple(t_cl.shape)}")
    return n * h * w, c


def _channel_ptrs(what: str, c: int, **vectors):
    for name, v in vectors.items():
        if v.numel() != c:
            raise RuntimeError(f"{what}: {name} must hold {c} values, got {tuple(v.shape)}")
    return [f32_ptr(v, name) for name, v in vectors.items()]


def bn_train_stats(z_cl, eps: float, running_mean=None, running_var=None, momentum: float = 0.1):
    """``gdrnpp_bn_train_stats_nhwc``: the batch statistics of z [N,C,H,W] -> (mean f32[C], invstd f32[C] = 1 / sqrt(biased var + eps)),
    what PyTorch's batch_norm saves.  ``running_mean`` / ``running_var``, where given, are updated IN PLACE with ``momentum`` and the
    unbiased variance.  N H W >= 2."""
    what = "bn_train_stats"
    m, c = _rows(z_cl, what)
    nbytes = load().gdrnpp_bn_train_stats_workspace_bytes(m, c)      # 0: the entry point refuses the shape, in its words
    ws = torch.empty((max(nbytes, 16) // 8,), dtype=torch.float64, device=z_cl.device)
    mean = torch.empty((c,), dtype=torch.float32, device=z_cl.device)
    invstd = torch.empty_like(mean)
    launch("gdrnpp_bn_train_stats_nhwc", z_cl.data_ptr(), mean.data_ptr(), invstd.data_ptr(), opt_f32_ptr(running_mean, "running_mean"),
           opt_f32_ptr(running_var, "running_var"), m, c, float(eps), float(momentum), ws.data_ptr(), nbytes,
           timed=("hbm:bn_train_stats", 0.0, 4.0 * z_cl.numel()))
    return mean, invstd


def bn_silu_apply(z_cl, mean, invstd, gamma, beta):
    """``gdrnpp_bn_silu_apply_nhwc``: y = silu(gamma (z - mean) invstd + beta), channels_last as z."""
    what = "bn_silu_apply"
    m, c = _rows(z_cl, what)
    y = torch.empty_like(z_cl)      # preserves channels_last
    launch("gdrnpp_bn_silu_apply_nhwc", z_cl.data_ptr(), *_channel_ptrs(what, c, mean=mean, invstd=invstd, gamma=gamma, beta=beta), y.data_ptr(),
           m, c, timed=("hbm:bn_silu_apply", 0.0, 8.0 * z_cl.numel()))
    return y


def bn_silu_backward(grad_y_cl, z_cl, mean, invstd, gamma, beta, want=(True, True, True)):
    """``gdrnpp_bn_silu_backward``: the gradients of y = silu(BatchNorm(z)) under batch statistics -> (dz, dgamma, dbeta).  ``want``:
    three flags in that order — an entry is None where its flag is false and its launches are left out; the others keep their bits."""
    what = "bn_silu_backward"
    want = tuple(bool(f) for f in want)
    if len(want) != 3 or not any(want):
        raise RuntimeError(f"{what}: want must hold three flags, at least one of them set")
    m, c = _rows(z_cl, what)
    if tuple(grad_y_cl.shape) != tuple(z_cl.shape):
        raise RuntimeError(f"{what}: grad_y {tuple(grad_y_cl.shape)} does not fit z {tuple(z_cl.shape)}")
    channels_last_f32(grad_y_cl, what)
    nbytes = load().gdrnpp_bn_silu_backward_workspace_bytes(m, c)
    ws = torch.empty((max(nbytes, 16) // 8,), dtype=torch.float64, device=z_cl.device)
    dz = torch.empty_like(z_cl) if want[0] else None
    dgamma = torch.empty((c,), dtype=torch.float32, device=z_cl.device) if want[1] else None
    dbeta = torch.empty((c,), dtype=torch.float32, device=z_cl.device) if want[2] else None
    launch("gdrnpp_bn_silu_backward", grad_y_cl.data_ptr(), z_cl.data_ptr(), *_channel_ptrs(what, c, mean=mean, invstd=invstd, gamma=gamma, beta=beta),
           *(None if t is None else t.data_ptr() for t in (dz, dgamma, dbeta)), m, c, ws.data_ptr(), nbytes,
           timed=("hbm:bn_silu_backward", 0.0, 4.0 * z_cl.numel() * (2 + 3 * want[0])))
    return dz, dgamma, dbeta


def _conv_out(h: int, w: int, ks: int, stride: int):
    pad = (ks - 1) // 2
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


def conv_train_f32(x_cl, weight, bias=None, stride: int = 1):
    """The training forward's convolution: z = conv(x, weight) (+ bias), ks x ks / ``stride`` / pad (ks - 1) // 2, on
    ``gdrnpp_conv_bias_act_f32`` -> channels_last [N,Cout,OH,OW].  The operand is made per call: the weight changes every step."""
    n, cin, h, w = channels_last_f32(x_cl, "conv_train_f32")
    cout, ks = weight.shape[0], weight.shape[2]
    oh, ow = _conv_out(h, w, ks, stride)
    z = torch.empty((n, cout, oh, ow), dtype=torch.float32, device=x_cl.device, memory_format=torch.channels_last)
    conv_bias_act_f32(x_cl.permute(0, 2, 3, 1), 0, cin, pack_conv_weight_kmajor(weight), bias, z.permute(0, 2, 3, 1), 0, cout, ks, stride)
    return z


def conv_wgrad_f32(dz_cl, x_cl, ks: int, stride: int):
    """dW f32[Cout,Cin,ks,ks] of a ks x ks / ``stride`` / pad (ks - 1) // 2 convolution for dz [N,Cout,OH,OW] and its input x
    [N,Cin,H,W], both channels_last (``gdrnpp_conv_wgrad_f32``: implicit TN GEMM on the exact-f32 matrix instruction, fixed slots, fp64
    finalize, one rounding).  ks in {1, 3}, stride in {1, 2}, any Cin % 4 == 0 and Cout % 4 == 0."""
    what = "conv_wgrad_f32"
    n, cout, oh, ow = channels_last_f32(dz_cl, what)
    xn, cin, h, w = channels_last_f32(x_cl, what)
    if ks not in (1, 3) or stride not in (1, 2) or (xn, *_conv_out(h, w, ks, stride)) != (n, oh, ow):
        raise RuntimeError(f"{what}: dz {tuple(dz_cl.shape)} does not fit x {tuple(x_cl.shape)} at ks={ks}, stride={stride}")
    nbytes = load().gdrnpp_conv_wgrad_f32_workspace_bytes(n, h, w, cin, cout, ks, stride)      # 0: the entry point refuses the shape, in its words
    ws = torch.empty((max(nbytes, 16) // 8,), dtype=torch.float64, device=x_cl.device)
    dw = torch.empty((cout, cin, ks, ks), dtype=torch.float32, device=x_cl.device)
    launch("gdrnpp_conv_wgrad_f32", dz_cl.data_ptr(), x_cl.data_ptr(), dw.data_ptr(), n, h, w, cin, cout, ks, stride, ws.data_ptr(), nbytes,
           timed=("mfma_f32:conv_wgrad", 2.0 * n * oh * ow * cout * ks * ks * cin, 4.0 * n * (h * w * cin + oh * ow * cout) + 4.0 * ks * ks * cin * cout))
    return dw


def conv3x3s2_dinput_any_f32(dz_cl, w_op, cin: int):
    """dx [N,cin,2 OH,2 OW] channels_last of a 3x3 / stride 2 / pad 1 convolution for dz [N,Cout,OH,OW] channels_last and ``w_op``
    f32[9 Cout, cin], row (ky 3 + kx) Cout + co (``gdrnpp_conv3x3s2_dinput_any_f32``, by parity class; any cin % 4 == 0, Cout % 4 == 0)."""
    what = "conv3x3s2_dinput_any_f32"
    n, cout, oh, ow = channels_last_f32(dz_cl, what)
    if tuple(w_op.shape) != (9 * cout, cin):
        raise RuntimeError(f"{what}: w_op must be f32[{9 * cout}, {cin}], got {tuple(w_op.shape)}")
    dx = torch.empty((n, cin, 2 * oh, 2 * ow), dtype=torch.float32, device=dz_cl.device, memory_format=torch.channels_last)
    launch("gdrnpp_conv3x3s2_dinput_any_f32", dz_cl.data_ptr(), f32_ptr(w_op, "w_op"), dx.data_ptr(), n, 2 * oh, 2 * ow, cin, cout,
           timed=("mfma_f32:conv3x3s2_dinput_any", 2.0 * n * oh * ow * cout * 9 * cin, 4.0 * n * oh * ow * (4 * cin + cout) + 36.0 * cin * cout))
    return dx


def _dinput_weight(weight, stride: int):
    """nn.Conv2d weight [Cout,Cin,ks,ks] -> the data gradient's operand, rows (ky, kx, co), columns ci.  Stride 1: flipped, for the
    forward-shaped convolution of dz.  Stride 2: as it lies, for the parity kernel — a 1x1 weight as the centre tap of a 3x3 one,
    whose other eight taps multiply zeros and whose three other parity classes so come out zero, as they are."""
    cout, cin, ks, _ = weight.shape
    w = weight.detach()
    if stride == 1:
        return w.flip(2, 3).permute(2, 3, 0, 1).reshape(ks * ks * cout, cin).contiguous()
    if ks == 1:
        out = torch.zeros((3, 3, cout, cin), dtype=torch.float32, device=weight.device)
        out[1, 1] = w[:, :, 0, 0]
        return out.view(9 * cout, cin)
    return w.permute(2, 3, 0, 1).reshape(9 * cout, cin).contiguous()


def conv_backward(x_cl, weight, stride: int, dz_cl, want=(True, True)):
    """Gradients of z = conv(x, weight), ks x ks / ``stride`` / pad (ks - 1) // 2, for dz = dL/dz -> (dx, dweight).  ``want``: two flags
    in that order — an entry is None where its flag is false and its launches are left out; the other keeps its bits.  dx at stride 1
    is the forward-shaped convolution of dz with the flipped, transposed weight (``gdrnpp_conv_bias_act_f32``), at stride 2
    ``conv3x3s2_dinput_any_f32``; dweight is ``conv_wgrad_f32``.  The operands are formed here, per call."""
    want = tuple(bool(f) for f in want)
    if len(want) != 2 or not any(want):
        raise RuntimeError("conv_backward: want must hold two flags, at least one of them set")
    cout, cin, ks, _ = weight.shape
    dx = None
    if want[0]:
        w_op = _dinput_weight(weight, stride)
        if stride == 1:
            n, _, h, w = channels_last_f32(dz_cl, "conv_backward")
            dx = torch.empty((n, cin, h, w), dtype=torch.float32, device=dz_cl.device, memory_format=torch.channels_last)
            conv_bias_act_f32(dz_cl.permute(0, 2, 3, 1), 0, cout, w_op, None, dx.permute(0, 2, 3, 1), 0, cin, ks, 1)
        else:
            dx = conv3x3s2_dinput_any_f32(dz_cl, w_op, cin)
    dw = conv_wgrad_f32(dz_cl, x_cl, ks, stride) if want[1] else None
    return dx, dw


# ---- training batches: mosaic, affine, mixup, HSV, mirror, preproc for a batch in one call (csrc/yolox_aug.hip) ------------------------
# the columns of yolox_train_inputs' host table (include/gdrnpp_hip.h); the matrix and the scales hold the bits of an fp64
YOLOX_AUG_SOURCE_COLUMNS = ("off", "w", "h", "dw", "dh", "mode", "scale_x", "scale_y", "l_x", "l_y", "s_x", "s_y", "pw", "ph")
YOLOX_AUG_SOURCES = 5                                                         # four mosaic tiles (plain: the first), then the mixup image
YOLOX_AUG_COLUMNS = (("branch", "flags", "m00", "m01", "m02", "m10", "m11", "m12", "mix_w", "mix_h", "mix_mode", "mix_scale_x", "mix_scale_y",
                      "mix_x_off", "mix_y_off") + tuple(f"s{k}_{c}" for k in range(YOLOX_AUG_SOURCES) for c in YOLOX_AUG_SOURCE_COLUMNS))
YOLOX_AUG_F64 = frozenset(("m00", "m01", "m02", "m10", "m11", "m12", "mix_scale_x", "mix_scale_y")
                          + tuple(f"s{k}_scale_{a}" for k in range(YOLOX_AUG_SOURCES) for a in "xy"))
YOLOX_AUG_BRANCHES = ("plain", "mosaic", "mixup")                             # branch = index
YOLOX_AUG_MODES = RESIZE_MODES                                                # cv2.resize's forms: mode = index
YOLOX_AUG_FLAGS = {"hsv1": 1, "hsv1_rgb": 2, "mirror": 4, "fallback": 8, "hsv2": 16, "hsv2_rgb": 32, "mix_flip": 64}
assert len(YOLOX_AUG_COLUMNS) == 85      # i64[B,85] in include/gdrnpp_hip.h


def yolox_aug_table(rows):
    """[{column: value}] -> the i64[B,85] host table of ``yolox_train_inputs``; a column left out is 0, the fp64 columns are stored as their
    bits."""
    import numpy as np

    table = np.zeros((len(rows), len(YOLOX_AUG_COLUMNS)), np.int64)
    index = {name: k for k, name in enumerate(YOLOX_AUG_COLUMNS)}
    for b, row in enumerate(rows):
        unknown = set(row) - set(index)
        if unknown:
            raise RuntimeError(f"yolox_aug_table: unknown columns {sorted(unknown)}; the columns are {YOLOX_AUG_COLUMNS}")
        for name, value in row.items():
            table[b, index[name]] = np.float64(value).view(np.int64) if name in YOLOX_AUG_F64 else int(value)
    return table


def yolox_train_inputs(src, table, lut, H: int, W: int, *, out=None):
    """``gdrnpp_yolox_train_inputs``: the pixel work of ``MosaicDetection.__getitem__`` over ``TrainTransform`` for B items in one call.

    src: a flat u8 device tensor of decoded source images, HWC, rows dense.  table: host i64[B,85] with the columns ``YOLOX_AUG_COLUMNS``
    (``yolox_aug_table``): per item the branch (``YOLOX_AUG_BRANCHES``), the flags (``YOLOX_AUG_FLAGS``), the affine matrix, the mixup's
    second resize and crop, and per source where it lies in ``src``, the size, form and scales of its cv2.resize and its paste.  lut:
    u8[B,2,3,256] on the device, the hue / saturation / value LUTs of the two HSV passes.  The library checks every value the kernels
    index with before it uploads the table in one copy; a bad row raises RuntimeError.
    -> (out f32[B,3,H,W] holding integers 0..255, flags i32[B]: 1 where the affine matrix was singular).  Nothing is read back."""
    import numpy as np

    what = "yolox_train_inputs"
    dev_ptr(src, torch.uint8, "src")
    table = np.ascontiguousarray(table.cpu().numpy() if isinstance(table, torch.Tensor) else table)
    if table.ndim != 2 or table.shape[1] != len(YOLOX_AUG_COLUMNS) or table.dtype != np.int64:
        raise RuntimeError(f"{what}: table must be a host i64[B,{len(YOLOX_AUG_COLUMNS)}], got {table.shape} of {table.dtype}")
    B, H, W = table.shape[0], int(H), int(W)
    dev_ptr(lut, torch.uint8, "lut")
    if tuple(lut.shape) != (B, 2, 3, 256):
        raise RuntimeError(f"{what}: lut must be u8[{B},2,3,256], got {tuple(lut.shape)}")
    dev = src.device
    if out is None:
        out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    f32_ptr(out, "out")
    if tuple(out.shape) != (B, 3, H, W):
        raise RuntimeError(f"{what}: out must be f32[{B},3,{H},{W}], got {tuple(out.shape)}")
    flags = torch.zeros((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return out, flags
    nbytes = load().gdrnpp_yolox_train_inputs_workspace_bytes(B, H, W)      # 0: the entry point refuses the shape, in its words
    ws = torch.empty((max(nbytes, 16) // 4,), dtype=torch.int32, device=dev)
    launch("gdrnpp_yolox_train_inputs", src.data_ptr(), src.numel(), table.ctypes.data, lut.data_ptr(), B, H, W, out.data_ptr(), flags.data_ptr(),
           ws.data_ptr(), nbytes, timed=("hbm:yolox_train_inputs", 0.0, 32.0 * B * H * W))
    return out, flags
