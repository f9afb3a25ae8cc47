"""The YOLOX forward on csrc/yolox_net.hip: every BaseConv is one launch of ``gdrnpp_conv_bias_act_f32`` (BatchNorm folded,
SiLU and the Bottleneck's residual in the epilogue) that reads and writes channel slices, so no concatenation, permute or
decode kernel runs: CSPLayer / SPP / PAFPN concatenations are buffers filled side by side, the prediction layers write their
columns of ``det_preds`` at the level's anchor offset with the sigmoid / box decode applied.

Activation buffers are allocated once per (input shape, device, stream) and reused; ``det_preds`` is fresh on every call."""
import torch

from .... import hip_lib
from ....gdrn_modeling import slice_layers as L
from .network_blocks import BaseConv

S = L.NhwcSlice
_MAX_PLANS = 4


def supported_size(model, H: int, W: int) -> bool:
    """H, W multiples of the coarsest stride (what the module path's concatenations need as well), three levels."""
    head = model.head
    return (H % 32 == 0 and W % 32 == 0 and H > 0 and W > 0
            and list(head.strides) == [8, 16, 32] and len(head.stems) == 3 and hasattr(model.backbone, "C3_n4"))


def supported(model, x) -> bool:
    """[B,3,H,W] of a ``supported_size``."""
    return x.dim() == 4 and x.shape[1] == 3 and supported_size(model, x.shape[2], x.shape[3])


class _Buffers:
    def __init__(self, b, device):
        self.b, self.device, self.t = b, device, {}

    def __call__(self, name, h, w, c):
        t = self.t.get(name)
        if t is None:
            t = self.t[name] = torch.empty((self.b, h, w, c), dtype=torch.float32, device=self.device)
        return t


def _conv(m: BaseConv, src, dst, resid=None):
    return L.conv_bn_act_slice(m.conv, m.bn, "silu", src, dst, resid)


def _csp(layer, src, dst, buf, name, h, w):
    hid = layer.conv1.conv.out_channels
    cat = buf(name + ".cat", h, w, 2 * hid)
    tmp = buf(name + ".tmp", h, w, hid)
    x1 = S(cat, 0, hid)
    _conv(layer.conv1, src, x1)
    _conv(layer.conv2, src, S(cat, hid, hid))
    for blk in layer.m:          # in place on the first half: the 3x3 reads tmp, adds the half it then overwrites
        _conv(blk.conv1, x1, S(tmp))
        _conv(blk.conv2, S(tmp), x1, x1 if blk.use_add else None)
    return _conv(layer.conv3, S(cat), dst)


def _plan(model, b, H, W, device) -> _Buffers:
    plans = model.__dict__.setdefault("_gdrnpp_yolox_buffers", {})
    key = (b, H, W, device, hip_lib.current_stream())
    buf = plans.get(key)
    if buf is None:
        if len(plans) >= _MAX_PLANS:
            plans.clear()
        buf = plans[key] = _Buffers(b, device)
    return buf


def focus_buffer(model, b: int, H: int, W: int, device) -> torch.Tensor:
    """The Focus stem's input f32[b,H/2,W/2,12] of the plan for a [b,3,H,W] image on the current stream: a producer that writes
    the Focus layout itself (``hip_lib.yolox_letterbox(..., focus=True)``) fills it and calls ``forward(model, None, focus=...)``."""
    return _plan(model, b, H, W, device)("focus", H // 2, W // 2, 12)


def forward(model, x, focus=None):
    """``x`` f32[B,3,H,W] — or ``x=None`` and ``focus`` = the filled ``focus_buffer``: the space-to-depth launch is skipped (one
    write and one read of the image less)."""
    if focus is not None:
        b, h2, w2, _ = focus.shape
        H, W, device = 2 * h2, 2 * w2, focus.device
        buf = _plan(model, b, H, W, device)
        if x is not None or focus is not buf("focus", h2, w2, 12):
            raise RuntimeError("hip_forward.forward: focus must be the plan's own focus_buffer (same stream), with x=None")
    else:
        b, _, H, W = x.shape
        device = x.device
        buf = _plan(model, b, H, W, device)
    fpn, head = model.backbone, model.head
    bb = fpn.backbone
    h2, w2, h4, w4, h8, w8, h16, w16, h32, w32 = H // 2, W // 2, H // 4, W // 4, H // 8, W // 8, H // 16, W // 16, H // 32, W // 32
    c3, c4, c5 = (m.conv.in_channels for m in head.stems)

    # CSPDarknet; dark3 / dark4 land in the second halves of the top-down concatenations
    foc = S(focus) if focus is not None else L.focus_slice(x, S(buf("focus", h2, w2, 12)))
    stem = _conv(bb.stem.conv, foc, S(buf("stem", h2, w2, bb.stem.conv.conv.out_channels)))
    d2a = _conv(bb.dark2[0], stem, S(buf("d2a", h4, w4, bb.dark2[0].conv.out_channels)))
    d2 = _csp(bb.dark2[1], d2a, S(buf("d2", h4, w4, d2a.c)), buf, "d2", h4, w4)
    d3a = _conv(bb.dark3[0], d2, S(buf("d3a", h8, w8, c3)))
    cat_p3 = buf("cat_p3", h8, w8, 2 * c3)
    x2 = _csp(bb.dark3[1], d3a, S(cat_p3, c3, c3), buf, "d3", h8, w8)
    d4a = _conv(bb.dark4[0], x2, S(buf("d4a", h16, w16, c4)))
    cat_p4 = buf("cat_p4", h16, w16, 2 * c4)
    x1 = _csp(bb.dark4[1], d4a, S(cat_p4, c4, c4), buf, "d4", h16, w16)
    d5a = _conv(bb.dark5[0], x1, S(buf("d5a", h32, w32, c5)))
    spp = bb.dark5[1]
    if tuple(spp.kernel_sizes) != (5, 9, 13):
        raise NotImplementedError(f"SPPBottleneck kernel_sizes={spp.kernel_sizes}: the HIP forward has the (5, 9, 13) pools")
    hid = spp.conv1.conv.out_channels
    spp_cat = buf("spp.cat", h32, w32, 4 * hid)
    _conv(spp.conv1, d5a, S(spp_cat, 0, hid))
    L.spp_slice(S(spp_cat), hid)
    d5b = _conv(spp.conv2, S(spp_cat), S(buf("d5b", h32, w32, c5)))
    x0 = _csp(bb.dark5[2], d5b, S(buf("x0", h32, w32, c5)), buf, "d5", h32, w32)

    # PAFPN; the two reduced maps land in the second halves of the bottom-up concatenations
    cat_n4 = buf("cat_n4", h32, w32, 2 * c4)
    cat_n3 = buf("cat_n3", h16, w16, 2 * c3)
    fpn_out0 = _conv(fpn.lateral_conv0, x0, S(cat_n4, c4, c4))
    L.upsample2x_slice(fpn_out0, S(cat_p4, 0, c4))
    f_out0 = _csp(fpn.C3_p4, S(cat_p4), S(buf("f_out0", h16, w16, c4)), buf, "p4", h16, w16)
    fpn_out1 = _conv(fpn.reduce_conv1, f_out0, S(cat_n3, c3, c3))
    L.upsample2x_slice(fpn_out1, S(cat_p3, 0, c3))
    pan_out2 = _csp(fpn.C3_p3, S(cat_p3), S(buf("pan_out2", h8, w8, c3)), buf, "p3", h8, w8)
    _conv(fpn.bu_conv2, pan_out2, S(cat_n3, 0, c3))
    pan_out1 = _csp(fpn.C3_n3, S(cat_n3), S(buf("pan_out1", h16, w16, c4)), buf, "n3", h16, w16)
    _conv(fpn.bu_conv1, pan_out1, S(cat_n4, 0, c4))
    pan_out0 = _csp(fpn.C3_n4, S(cat_n4), S(buf("pan_out0", h32, w32, c5)), buf, "n4", h32, w32)

    # head: the prediction layers write det_preds[B, A, 5 + C] in place
    levels = [(pan_out2, h8, w8), (pan_out1, h16, w16), (pan_out0, h32, w32)]
    head.hw = [(h, w) for _, h, w in levels]
    A = sum(h * w for _, h, w in levels)
    nc = head.num_classes
    det = torch.empty((b, A, 5 + nc), dtype=torch.float32, device=device)
    row0 = 0
    for k, (feat, h, w) in enumerate(levels):
        ch = head.stems[k].conv.out_channels
        s = _conv(head.stems[k], feat, S(buf(f"head{k}.stem", h, w, ch)))
        ta, tb = S(buf(f"head{k}.a", h, w, ch)), S(buf(f"head{k}.b", h, w, ch))
        _conv(head.cls_convs[k][0], s, ta)
        cls_feat = _conv(head.cls_convs[k][1], ta, tb)
        L.conv_bn_act_slice(head.cls_preds[k], None, "sigmoid", cls_feat, S(det, 5, nc), None, A, row0)
        tc = S(buf(f"head{k}.c", h, w, ch))
        _conv(head.reg_convs[k][0], s, ta)
        reg_feat = _conv(head.reg_convs[k][1], ta, tc)
        L.conv_bn_act_slice(head.reg_preds[k], None, "yolox_box" if head.decode_in_inference else "none", reg_feat, S(det, 0, 4), None, A, row0,
                            float(head.strides[k]))
        L.conv_bn_act_slice(head.obj_preds[k], None, "sigmoid", reg_feat, S(det, 4, 1), None, A, row0)
        row0 += h * w
    return {"det_preds": det} if head.decode_in_inference else det
