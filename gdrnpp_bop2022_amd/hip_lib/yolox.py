"""The YOLOX detector: its forward on NHWC slice buffers (csrc/yolox_net.hip) and its two ends, letterbox and
post-processing (csrc/yolox_pre.hip)."""
from __future__ import annotations

import torch

from .abi import DEFINES, dev_ptr, f32_ptr, launch, load, opt_f32_ptr


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
