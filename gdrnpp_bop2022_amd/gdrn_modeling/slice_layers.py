"""Layers of the YOLOX detector on channel slices of NHWC buffers (csrc/yolox_net.hip): a layer reads its input from a slice and
writes its result into one, so a concatenation is a buffer its producers fill side by side."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import hip_lib
from .hip_layers import _fallback, enabled_for, folded_conv_bn
from .weight_cache import cached, module_cache, weight_tag


class NhwcSlice:
    """Channels [off, off + c) of a contiguous NHWC buffer f32[B,H,W,ld]: where a layer reads its input and writes its result,
    so a concatenation is a buffer its producers fill side by side."""
    __slots__ = ("buf", "off", "c")

    def __init__(self, buf: torch.Tensor, off: int = 0, c: int | None = None):
        self.buf, self.off, self.c = buf, off, buf.shape[-1] - off if c is None else c

    def view(self) -> torch.Tensor:
        return self.buf[..., self.off:self.off + self.c]

    def nchw(self) -> torch.Tensor:
        return self.view().permute(0, 3, 1, 2)


def _conv_slice_ok(conv: nn.Conv2d, src: NhwcSlice) -> bool:
    """Shapes ``gdrnpp_conv_bias_act_f32`` takes: dense 1x1 / 3x3, stride 1 / 2, padding (k - 1) / 2, Cin and the slice's
    placement multiples of 4."""
    k, s = conv.kernel_size, conv.stride
    return (k[0] == k[1] and k[0] in (1, 3) and s[0] == s[1] and s[0] in (1, 2) and conv.padding == ((k[0] - 1) // 2,) * 2
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros" and conv.in_channels % 4 == 0
            and src.off % 4 == 0 and src.buf.shape[-1] % 4 == 0 and src.c == conv.in_channels)


def conv_bn_act_slice(conv: nn.Conv2d, bn: nn.BatchNorm2d | None, act: str, src: NhwcSlice, dst: NhwcSlice, resid: NhwcSlice | None = None,
                      img_rows: int = 0, row0: int = 0, dec_stride: float = 0.0) -> NhwcSlice:
    """dst = act(bn(conv(src))) + resid in ONE launch of ``gdrnpp_conv_bias_act_f32``: BatchNorm (inference) folded into weight
    and bias in float64 (``folded_conv_bn``), the k-major weight cached on the conv module until a parameter or statistic
    changes.  ``act`` in none / silu / sigmoid / yolox_box; ``img_rows`` / ``row0``: dst.buf is f32[B,img_rows,ld] and the layer
    writes from row ``row0`` of every image (the head's prediction layers).  Shapes outside the kernel run as PyTorch operators
    into the same slice, counted as a fallback."""
    x = src.buf
    if not enabled_for(x):
        raise RuntimeError("conv_bn_act_slice: the slice layers exist on the GPU with the HIP layers enabled only")
    if bn is not None and (bn.training or not bn.affine or not bn.track_running_stats):
        raise RuntimeError("conv_bn_act_slice: BatchNorm must be in inference mode with affine parameters and running statistics")
    w, b = folded_conv_bn(conv, bn) if bn is not None else (conv.weight.detach(), None if conv.bias is None else conv.bias.detach())
    if _conv_slice_ok(conv, src):
        cache = module_cache(conv)
        hit = cached(cache, "w_kmajor", weight_tag(w), lambda: (hip_lib.pack_conv_weight_kmajor(w),), w)
        hip_lib.conv_bias_act_f32(x, src.off, src.c, hit[1], b, dst.buf, dst.off, dst.c, conv.kernel_size[0], conv.stride[0], act,
                                  None if resid is None else resid.buf, 0 if resid is None else resid.off, img_rows, row0, dec_stride)
        return dst
    _fallback("conv_bn_act_slice: convolution outside gdrnpp_conv_bias_act_f32 (PyTorch operators)", x)
    y = F.conv2d(src.nchw(), w, b, conv.stride, conv.padding, conv.dilation, conv.groups).permute(0, 2, 3, 1)
    if act == "silu":
        y = F.silu(y)
    elif act == "sigmoid":
        y = torch.sigmoid(y)
    elif act == "yolox_box":
        oh, ow = y.shape[1:3]
        g = torch.stack(torch.meshgrid(torch.arange(ow, device=y.device), torch.arange(oh, device=y.device), indexing="xy"), -1).to(y.dtype)
        y = torch.cat([(y[..., :2] + g) * dec_stride, torch.exp(y[..., 2:4]) * dec_stride], -1)
    if resid is not None:
        y = y + resid.view()
    if img_rows:
        dst.buf[:, row0:row0 + y.shape[1] * y.shape[2], dst.off:dst.off + dst.c] = y.reshape(y.shape[0], -1, y.shape[3])
    else:
        dst.view().copy_(y)
    return dst


def focus_slice(x_nchw: torch.Tensor, dst: NhwcSlice) -> NhwcSlice:
    """The Focus stem's 2x2 space-to-depth from the NCHW image into a 12-channel NHWC slice (``gdrnpp_yolox_focus``)."""
    hip_lib.yolox_focus(x_nchw.contiguous(), dst.buf, dst.off)
    return dst


def spp_slice(cat: NhwcSlice, c: int) -> NhwcSlice:
    """The 5 / 9 / 13 max pools of the first ``c`` channels of ``cat`` into its next three groups of ``c`` channels, one launch."""
    hip_lib.spp_maxpool_5_9_13(cat.buf, cat.off, c)
    return cat


def upsample2x_slice(src: NhwcSlice, dst: NhwcSlice) -> NhwcSlice:
    """Nearest x2 of a slice into a slice (``gdrnpp_upsample_nearest2x_slice``)."""
    hip_lib.upsample_nearest2x_slice(src.buf, src.off, dst.buf, dst.off, src.c)
    return dst
