"""Building blocks of the YOLOX detector (Ge et al., "YOLOX: Exceeding YOLO Series in 2021").

Sub-module names follow the published implementation so its checkpoints load with ``strict=True``:
``BaseConv.{conv,bn,act}``, ``Bottleneck.{conv1,conv2}``, ``CSPLayer.{conv1,conv2,conv3,m}``, ``SPPBottleneck.{conv1,m,conv2}``,
``Focus.conv``.  The forwards below are the plain-PyTorch module path (CPU, fixtures, A/B baseline); the GPU forward of a
whole ``YOLOX`` walks the same modules through ``hip_forward``.  In training mode a ``BaseConv`` asks ``train_layers.conv_bn_silu``
first: with ``hip_layers.set_train_kernels(True)`` its three layers run, forward and backward, on csrc/conv_bn_bwd.hip."""
import torch
import torch.nn as nn

from .train_layers import conv_bn_silu


def _no_depthwise(depthwise: bool) -> None:
    if depthwise:
        raise NotImplementedError("depthwise=True (the DWConv blocks of YOLOX-nano) is not implemented")


def _activation(act: str) -> nn.Module:
    if act != "silu":
        raise NotImplementedError(f"act={act!r}: only act='silu' is implemented")
    return nn.SiLU(inplace=True)


class BaseConv(nn.Module):
    """Conv2d (no bias unless asked) -> BatchNorm2d -> SiLU, padding (ksize - 1) // 2."""

    def __init__(self, in_channels, out_channels, ksize, stride, groups=1, bias=False, act="silu"):
        super().__init__()
        self.conv = nn.Conv2d(in_channels, out_channels, ksize, stride, (ksize - 1) // 2, groups=groups, bias=bias)
        self.bn = nn.BatchNorm2d(out_channels)
        self.act = _activation(act)

    def forward(self, x):
        if self.training:      # the three layers as one autograd node on this library's kernels, where train_layers takes them
            y = conv_bn_silu(self.conv, self.bn, x)
            if y is not None:
                return y
        return self.act(self.bn(self.conv(x)))


class Bottleneck(nn.Module):
    """1x1 -> 3x3, plus the input when ``shortcut`` and the widths agree."""

    def __init__(self, in_channels, out_channels, shortcut=True, expansion=0.5, depthwise=False, act="silu"):
        super().__init__()
        _no_depthwise(depthwise)
        hidden = int(out_channels * expansion)
        self.conv1 = BaseConv(in_channels, hidden, 1, 1, act=act)
        self.conv2 = BaseConv(hidden, out_channels, 3, 1, act=act)
        self.use_add = bool(shortcut) and in_channels == out_channels

    def forward(self, x):
        y = self.conv2(self.conv1(x))
        return y + x if self.use_add else y


class SPPBottleneck(nn.Module):
    """1x1 to half the width, stride-1 max pools (5, 9, 13) beside the identity, 1x1 over the concatenation."""

    def __init__(self, in_channels, out_channels, kernel_sizes=(5, 9, 13), activation="silu"):
        super().__init__()
        hidden = in_channels // 2
        self.conv1 = BaseConv(in_channels, hidden, 1, 1, act=activation)
        self.m = nn.ModuleList([nn.MaxPool2d(k, 1, k // 2) for k in kernel_sizes])
        self.conv2 = BaseConv(hidden * (len(kernel_sizes) + 1), out_channels, 1, 1, act=activation)
        self.kernel_sizes = tuple(kernel_sizes)

    def forward(self, x):
        x = self.conv1(x)
        return self.conv2(torch.cat([x] + [m(x) for m in self.m], 1))


class CSPLayer(nn.Module):
    """Cross-stage-partial block: two 1x1 branches, ``n`` bottlenecks on the first, 1x1 over both."""

    def __init__(self, in_channels, out_channels, n=1, shortcut=True, expansion=0.5, depthwise=False, act="silu"):
        super().__init__()
        _no_depthwise(depthwise)
        hidden = int(out_channels * expansion)
        self.conv1 = BaseConv(in_channels, hidden, 1, 1, act=act)
        self.conv2 = BaseConv(in_channels, hidden, 1, 1, act=act)
        self.conv3 = BaseConv(2 * hidden, out_channels, 1, 1, act=act)
        self.m = nn.Sequential(*[Bottleneck(hidden, hidden, shortcut, 1.0, depthwise, act=act) for _ in range(n)])

    def forward(self, x):
        return self.conv3(torch.cat((self.m(self.conv1(x)), self.conv2(x)), 1))


def space_to_depth(x):
    """[B,C,H,W] -> [B,4C,H/2,W/2]: the 2x2 cell's top-left, bottom-left, top-right, bottom-right pixels, in this order."""
    return torch.cat((x[..., ::2, ::2], x[..., 1::2, ::2], x[..., ::2, 1::2], x[..., 1::2, 1::2]), 1)


class Focus(nn.Module):
    """2x2 space-to-depth, then a BaseConv."""

    def __init__(self, in_channels, out_channels, ksize=1, stride=1, act="silu"):
        super().__init__()
        self.conv = BaseConv(in_channels * 4, out_channels, ksize, stride, act=act)

    def forward(self, x):
        return self.conv(space_to_depth(x))
