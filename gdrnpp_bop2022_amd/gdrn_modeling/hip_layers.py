"""Dispatch of the memory-bound network layers to the hand-written NHWC HIP kernels
(csrc/net_kernels.hip) when the tensors live on the GPU; plain PyTorch otherwise (CPU unit tests,
or ``set_enabled(False)`` for A/B measurements).  Same math as the PyTorch operators, different summation order."""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import hip_lib
# the names below are the owners' own objects: this module stays the namespace the package, the tests and the tools import.
# Functions and classes only — an int or a dict re-exported here would be a stale copy the moment somebody assigns it.
from .weight_cache import cache_fills, cached, module_cache, weight_tag  # noqa: F401
from .x3_policy import (forced_gemm_products, gemm_products, is_demoted, note_launch, set_gemm_products, six_product_weight,  # noqa: F401
                        split_weight)
from .x3_policy import (demote as demote_x3, demoted as x3_demoted, launch_order as x3_launch_order,  # noqa: F401
                        reset as reset_x3_demotions, slot as x3_slot, weight_for as x3_for)

_ENABLED = True


def set_enabled(flag: bool) -> None:
    global _ENABLED
    _ENABLED = bool(flag)


def is_enabled() -> bool:
    return _ENABLED


def enabled_for(x: torch.Tensor) -> bool:
    return _ENABLED and x.is_cuda and x.dtype == torch.float32 and not torch.is_grad_enabled()


# ---- launches that are NOT this library's ------------------------------------------------------------------------------------
# Every layer below falls back to PyTorch's operator (ATen / MIOpen / hipBLASLt kernels) when its shape is outside the HIP kernel.
# One stream does not care.  Two steps in flight do: MI355X returns wrong values from packed-fp32 instructions with op_sel swizzles
# while another wave of the SIMD issues double-rate 16-bit MFMAs (profiles/r05p_two_stream_hazard.md) — this library is built
# and link-checked without that instruction form, foreign kernels are not.  So every fallback taken WHILE THE HIP PATH IS ON is
# counted, and engine.inference_step_async refuses to leave such a step beside another one (it drops the dealer to one stream
# and repeats the step alone).
_FOREIGN = {"n": 0, "last": None}


def note_foreign_launch(what: str) -> None:
    _FOREIGN["n"] += 1
    _FOREIGN["last"] = what


def fallback_launches() -> int:
    """Module-path (PyTorch operator) launches taken so far while the HIP layers were enabled and the tensor was theirs to take."""
    return _FOREIGN["n"]


def last_fallback():
    return _FOREIGN["last"]


def _fallback(what: str, x: torch.Tensor) -> None:
    if enabled_for(x):
        note_foreign_launch(what)


foreign = _fallback      # for the modules: "a PyTorch operator is about to run on ``x`` although the HIP path is on"


def _cl(x):
    return x if x.is_contiguous(memory_format=torch.channels_last) else x.contiguous(memory_format=torch.channels_last)


def upsample2x(layer: nn.Module, x: torch.Tensor) -> torch.Tensor:
    if _train_ok(x) and x.shape[1] % 4 == 0:
        return Upsample2x.apply(_cl(x))
    if enabled_for(x) and x.shape[1] % 4 == 0:
        return hip_lib.upsample_bilinear2x(_cl(x))
    _fallback("upsample2x: C % 4 != 0", x)
    return layer(x)


def _gn_ok(gn: nn.GroupNorm, x) -> bool:
    c, g = gn.num_channels, gn.num_groups
    q = c // 4
    return (enabled_for(x) and c % 4 == 0 and (c // g) % 4 == 0 and q <= 256 and 256 % q == 0 and g <= 64
            and x.shape[0] <= 65535 and gn.affine)


def _exact_gelu_or_none(act: nn.Module | None) -> bool:
    return act is None or (isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "none")


def groupnorm_act(gn: nn.GroupNorm, act: nn.Module | None, x: torch.Tensor) -> torch.Tensor:
    """GroupNorm followed by ``act`` (fused when act is the exact GELU or None).  With gradients enabled and
    ``set_train_kernels(True)`` the pair is ``GroupNormAct``."""
    if isinstance(gn, nn.GroupNorm) and _gn_train_ok(gn, x) and _exact_gelu_or_none(act):
        return GroupNormAct.apply(_cl(x), gn.weight, gn.bias, gn.num_groups, gn.eps, act is not None)
    if isinstance(gn, nn.GroupNorm) and _gn_ok(gn, x) and _exact_gelu_or_none(act):
        return hip_lib.groupnorm_act(_cl(x), gn.weight, gn.bias, gn.num_groups, gn.eps, gelu=act is not None)
    _fallback("groupnorm_act: " + type(gn).__name__ + " / activation outside the HIP kernel", x)
    x = gn(x)
    return act(x) if act is not None else x


def layernorm2d(ln: nn.LayerNorm, x: torch.Tensor) -> torch.Tensor:
    """timm LayerNorm2d (LayerNorm over the channel dim of an NCHW tensor)."""
    c = x.shape[1]
    q = c // 4
    if (enabled_for(x) and c % 4 == 0 and q <= 256 and 256 % q == 0 and ln.elementwise_affine
            and tuple(ln.normalized_shape) == (c,)):
        return hip_lib.layernorm_nhwc(_cl(x), ln.weight, ln.bias, ln.eps)
    _fallback("layernorm2d: channel count outside the HIP kernel", x)
    y = F.layer_norm(x.permute(0, 2, 3, 1), ln.normalized_shape, ln.weight, ln.bias, ln.eps)
    return y.permute(0, 3, 1, 2)


def _stem_shape_ok(conv: nn.Conv2d, ln: nn.LayerNorm, x: torch.Tensor) -> bool:
    """Shapes the fused 4x4 stem kernel takes, forward and backward."""
    return (_MLP_GEMM == "split" and x.dim() == 4 and x.is_contiguous() and x.dtype == torch.float32
            and conv.in_channels == 3 and conv.out_channels == 128 and conv.kernel_size == (4, 4) and conv.stride == (4, 4)
            and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1 and ln.elementwise_affine
            and x.shape[2] % 4 == 0 and x.shape[3] % 16 == 0 and x.shape[3] <= 1024)


def stem(conv: nn.Conv2d, ln: nn.LayerNorm, x: torch.Tensor) -> torch.Tensor:
    """ConvNeXt stem: 4x4 / stride 4 convolution from 3 channels + LayerNorm2d.  One fused HIP kernel for the ConvNeXt-B shape
    (NCHW-contiguous fp32 image, 128 output channels), else the module path.  With gradients enabled and ``set_train_kernels(True)``
    the layer is ``StemConvLN`` when the image itself needs no gradient."""
    if _train_ok(x):
        if (_stem_shape_ok(conv, ln, x) and not x.requires_grad and not torch.is_autocast_enabled() and conv.padding_mode == "zeros"
                and tuple(ln.normalized_shape) == (128,) and conv.weight.is_cuda and conv.weight.dtype == torch.float32
                and (conv.bias is None or _param_ok(conv.bias)) and _param_ok(ln.weight, ln.bias)):
            return StemConvLN.apply(x, conv.weight, conv.bias, ln.weight, ln.bias, ln.eps)
        note_foreign_launch("stem: under autograd outside StemConvLN (image with a gradient, AMP, shape or layout outside the fused 4x4 stem kernel)")
    if enabled_for(x) and _stem_shape_ok(conv, ln, x):
        cache = module_cache(conv)
        # the kernel reads [co][ci][ky][kx]; the module may hold the weight channels_last
        hit = cached(cache, "w_oihw", weight_tag(conv.weight),
                     lambda: (conv.weight.detach().contiguous(memory_format=torch.contiguous_format).clone(),), conv.weight)
        return hip_lib.stem_conv4x4_ln(x, hit[1], conv.bias, ln.weight, ln.bias, ln.eps)
    _fallback("stem: input shape / layout outside the fused 4x4 stem kernel (needs NCHW fp32, H % 4 == 0, W % 16 == 0)", x)
    return ln(conv(x.contiguous(memory_format=torch.channels_last)))


def _dwconv_hip_ok(conv: nn.Conv2d, x: torch.Tensor) -> bool:
    c = conv.in_channels
    q = c // 4
    return enabled_for(x) and conv.kernel_size == (7, 7) and conv.groups == c and c % 4 == 0 and q <= 256 and 256 % q == 0


# Training: layers that have a backward on this library's kernels take it under autograd when this switch is on (off by default:
# with it off a forward under enable_grad runs PyTorch's operators, as it always has).  So far: dwconv_ln (DwConvLN) and convnext_mlp
# (ConvNeXtMlp) — with both, a ConvNeXt block trains without a kernel that is not this library's — the stem (StemConvLN, for an image
# that needs no gradient) and the stage entries (downsample: DownsampleLNConv), which close the ConvNeXt backbone, and the geometry head's layers:
# conv3x3_groupnorm_act (Conv3x3GnAct), conv_transpose2d_groupnorm_act (ConvTranspose2dGn), groupnorm_act (GroupNormAct) and
# upsample2x (Upsample2x), and the head's tail — the class-sliced 1x1 output layer, the class gather, the region softmax, the xyz
# de-normalisation and the concatenation into Patch-PnP's input (HeadTail) — and Patch-PnP in its shipped ConvNeXt configuration on
# the prepared input: the three [conv3x3 / stride 2, GroupNorm, GELU] layers (Conv3x3S2GnAct), the NCHW flatten (FlattenNCHW), fc1 and
# fc2 with their GELU (LinearGelu) and the two pose heads (PnPHeads).  The detector's BaseConv layers take the same switch in
# det/yolox/models/train_layers.py (ConvBnSilu), which imports this module.  The ResNet path, AMP and
# Patch-PnP outside that configuration (act "relu", another norm, mask attention, odd sizes, the module path ``forward``) keep
# PyTorch's graph.
_TRAIN_KERNELS = False


def set_train_kernels(flag: bool) -> None:
    global _TRAIN_KERNELS
    _TRAIN_KERNELS = bool(flag)


def train_kernels() -> bool:
    return _TRAIN_KERNELS


class DwConvLN(torch.autograd.Function):
    """Depthwise 7x7 + LayerNorm over C with its backward on HIP kernels (csrc/dwconv_ln_bwd.hip).  x (N,C,H,W) channels_last,
    weight = conv.weight [C,1,7,7], w49c = its tap-major copy (a constant of the graph: the gradient goes to ``weight``) -> y
    (N,C,H,W) channels_last, the bits of the inference forward.  The backward recomputes the convolution from x, which the block
    keeps as its shortcut anyway; nothing else is saved but the parameters."""

    @staticmethod
    def forward(ctx, x, weight, w49c, bias, ln_weight, ln_bias, eps):
        ctx.save_for_backward(x, weight, w49c, bias, ln_weight, ln_bias)
        ctx.eps = eps
        return hip_lib.dwconv7x7_ln(x, w49c, bias, ln_weight, ln_bias, eps, y_rows=False)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, weight, w49c, bias, ln_weight, ln_bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = (need[0], need[1], need[3], need[4], need[5])
        if not any(want):
            return (None,) * 7
        dx, dw, db, dg, dbeta = hip_lib.dwconv7x7_ln_backward(x, weight, bias, ln_weight, ln_bias, ctx.eps, _cl(grad_y), want=want, w49c=w49c)
        return dx, dw, None, db, dg, dbeta, None


def _train_ok(x: torch.Tensor) -> bool:
    """The part of every training guard that does not depend on the layer: switch on, gradients enabled, a 4-D fp32 device tensor."""
    return _TRAIN_KERNELS and _ENABLED and torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4


def _gn_train_shape_ok(gn: nn.GroupNorm, n: int) -> bool:
    """Shapes ``gdrnpp_groupnorm_act_backward`` takes (those of ``_gn_ok``) for ``n`` images."""
    c, g = gn.num_channels, gn.num_groups
    q = c // 4
    return (gn.affine and c % 4 == 0 and (c // g) % 4 == 0 and q <= 256 and 256 % q == 0 and g <= 64 and 0 < n <= 65535
            and gn.weight.is_cuda and gn.weight.dtype == torch.float32)


def _gn_train_ok(gn: nn.GroupNorm, x: torch.Tensor) -> bool:
    return _train_ok(x) and x.shape[1] == gn.num_channels and _gn_train_shape_ok(gn, x.shape[0])


def _conv_gn_train_ok(conv: nn.Conv2d, gn: nn.GroupNorm, act, x: torch.Tensor) -> bool:
    return (_train_ok(x) and isinstance(conv, nn.Conv2d) and isinstance(gn, nn.GroupNorm) and _gn_train_shape_ok(gn, x.shape[0])
            and conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1) and conv.dilation == (1, 1)
            and conv.groups == 1 and conv.padding_mode == "zeros" and conv.in_channels % 128 == 0 and conv.out_channels % 128 == 0
            and x.shape[1] == conv.in_channels and gn.num_channels == conv.out_channels and _exact_gelu_or_none(act)
            and conv.weight.is_cuda and conv.weight.dtype == torch.float32 and x.shape[0] * x.shape[2] * x.shape[3] < (1 << 31) - 4096)


class Conv3x3GnAct(torch.autograd.Function):
    """The head's [Conv2d 3x3/1/1, GroupNorm(, GELU)] with its backward on HIP kernels (csrc/conv_gn_bwd.hip).  x (N,Cin,H,W)
    channels_last -> y (N,Cout,H,W) channels_last.  The forward runs the fp32-MFMA convolution (``gdrnpp_conv_bias_act_f32``: the six-product kernel is
    past the gradient tests' bar at this depth), the GroupNorm statistics and the apply pass; saved are x, the convolution's output z and the statistics' partial sums — y and the pre-activation are recomputed."""

    @staticmethod
    def forward(ctx, x, weight, bias, gn_weight, gn_bias, groups, eps, gelu):
        z = hip_lib.conv3x3_f32_mfma(x, hip_lib.conv3x3_weight_kn(weight), bias)      # operand made per forward: the weight changes every step
        y, part = hip_lib.groupnorm_act_train(z, gn_weight, gn_bias, groups, eps, gelu)
        ctx.save_for_backward(x, z, part, weight, gn_weight, gn_bias)
        ctx.gn = (groups, eps, gelu)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, z, part, weight, gn_weight, gn_bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx = dw = db = dg = dbeta = None
        if any(need[:5]):
            dz, dg, dbeta = hip_lib.groupnorm_act_backward(z, part, gn_weight, gn_bias, *ctx.gn, _cl(grad_y), want=(any(need[:3]), need[3], need[4]))
            if any(need[:3]):
                dx, dw, db = hip_lib.conv3x3_backward(x, weight, dz, want=need[:3])
        return dx, dw, db, dg, dbeta, None, None, None


class GroupNormAct(torch.autograd.Function):
    """GroupNorm(, GELU) alone with its backward on ``gdrnpp_groupnorm_act_backward``: the norm behind the head's ConvTranspose2d and
    behind a convolution outside ``Conv3x3GnAct``.  Saved: the input and the statistics' partial sums."""

    @staticmethod
    def forward(ctx, z, gn_weight, gn_bias, groups, eps, gelu):
        y, part = hip_lib.groupnorm_act_train(z, gn_weight, gn_bias, groups, eps, gelu)
        ctx.save_for_backward(z, part, gn_weight, gn_bias)
        ctx.gn = (groups, eps, gelu)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        z, part, gn_weight, gn_bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = (None,) * 3
        if any(need[:3]):
            grads = hip_lib.groupnorm_act_backward(z, part, gn_weight, gn_bias, *ctx.gn, _cl(grad_y), want=need[:3])
        return (*grads, None, None, None)


class ConvTranspose2dGn(torch.autograd.Function):
    """The head's [ConvTranspose2d, GroupNorm(, GELU)] with its backward on HIP kernels: the im2col gather, the exact-f32 product for dx,
    the TN GEMM for the weight gradient, ``gdrnpp_groupnorm_act_backward`` for the norm.  Saved: x, the transposed convolution's
    output z and the statistics' partial sums (left by the forward's col2im gather)."""

    @staticmethod
    def forward(ctx, x, weight, bias, gn_weight, gn_bias, geom, groups, eps, gelu):
        z, part = hip_lib.conv_transpose2d_train(x, weight, bias, *geom, groups)
        ctx.save_for_backward(x, z, part, weight, gn_weight, gn_bias)
        ctx.geom, ctx.gn = geom, (groups, eps, gelu)
        return hip_lib.groupnorm_apply(z, part, gn_weight, gn_bias, groups, eps, gelu)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, z, part, weight, gn_weight, gn_bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx = dw = db = dg = dbeta = None
        if any(need[:5]):
            dz, dg, dbeta = hip_lib.groupnorm_act_backward(z, part, gn_weight, gn_bias, *ctx.gn, _cl(grad_y), want=(any(need[:3]), need[3], need[4]))
            if any(need[:3]):
                dx, dw, db = hip_lib.conv_transpose2d_backward(x, weight, dz, *ctx.geom, want=need[:3])
        return dx, dw, db, dg, dbeta, None, None, None, None


def _deconv_gn_train_ok(deconv: nn.ConvTranspose2d, gn: nn.GroupNorm, act, x: torch.Tensor) -> bool:
    ks = deconv.kernel_size[0] if isinstance(deconv, nn.ConvTranspose2d) else 0
    return (_train_ok(x) and isinstance(deconv, nn.ConvTranspose2d) and isinstance(gn, nn.GroupNorm) and _gn_train_shape_ok(gn, x.shape[0])
            and deconv.kernel_size[0] == deconv.kernel_size[1] and deconv.stride[0] == deconv.stride[1]
            and deconv.padding[0] == deconv.padding[1] and deconv.output_padding[0] == deconv.output_padding[1]
            and deconv.output_padding[0] < deconv.stride[0] and deconv.dilation == (1, 1) and deconv.groups == 1
            and x.shape[1] == deconv.in_channels and deconv.in_channels % 128 == 0 and (ks * ks * deconv.out_channels) % 128 == 0
            and gn.num_channels == deconv.out_channels and _exact_gelu_or_none(act) and deconv.weight.is_cuda
            and deconv.weight.dtype == torch.float32 and x.shape[0] * x.shape[2] * x.shape[3] * ks * ks * deconv.out_channels < (1 << 31))


class Upsample2x(torch.autograd.Function):
    """nn.UpsamplingBilinear2d(2) with its adjoint on ``gdrnpp_upsample_bilinear2x_backward_nhwc``; nothing is saved."""

    @staticmethod
    def forward(ctx, x):
        return hip_lib.upsample_bilinear2x(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        return hip_lib.upsample_bilinear2x_backward(_cl(grad_y))


_HEAD_TAIL_MAX_DEPTH = 256     # the depth to which the six-product kernel of the forward is measured inside the gradient tests' bar


class HeadTail(torch.autograd.Function):
    """The geometry head's tail with its backward on HIP kernels (csrc/head_tail_bwd.hip): the class-sliced 1x1 output layer, the class
    gather folded into it, the region softmax, the xyz de-normalisation and the concatenation that forms Patch-PnP's input.
    feat2d f32[B hw, K] (the NHWC rows of the trunk's result), weight / bias = the output layer's own parameters, cls_rows i64[C, n]
    (the rows of slice c), sel i32[B], coord2d f32[B,2,H,W], extents f32[B,3] -> (out2d f32[B hw, 128], pnp_in f32[B, hw, 96],
    planes f32[P, B, hw]) — the two launches of the inference tail, bit for bit, with the sliced, 128-row padded six-product pack built
    per call (the weights change every step).  Saved: feat2d, out2d, the sliced weight and the small tables; pnp_in is not saved (the
    backward rebuilds the softmax from out2d) and no copy of feat is made.  The backward runs the tail's adjoint, then the data gradient and the weight / bias gradient as ``needs_input_grad`` asks:
    a frozen output layer launches no weight-gradient kernel, a feat without gradient no data-gradient kernel."""

    @staticmethod
    def forward(ctx, feat2d, weight, bias, cls_rows, sel, coord2d, extents, double_mask):
        w = weight.detach().view(weight.shape[0], -1)[cls_rows].contiguous()      # [C, n, K]
        b = bias.detach()[cls_rows]                                               # [C, n]
        C, n, k = w.shape
        w128 = torch.zeros((C, 128, k), dtype=w.dtype, device=w.device)
        w128[:, :n] = w
        b128 = torch.zeros((C, 128), dtype=b.dtype, device=b.device)
        b128[:, :n] = b
        hw = coord2d.shape[2] * coord2d.shape[3]
        out2d = hip_lib.linear_f32_split_grouped(feat2d, hip_lib.pack_weight_bf16x3(w128.view(C * 128, k)), b128, sel, hw, n_store=(n + 3) // 4 * 4)
        pnp_in, planes = hip_lib.head_tail_nhwc(out2d, coord2d, extents, double_mask)
        ctx.save_for_backward(feat2d, out2d, w, cls_rows, sel, extents)
        ctx.layer = (tuple(weight.shape), hw, bool(double_mask))
        ctx.set_materialize_grads(False)      # an output the loss does not use arrives as None, not as a tensor of zeros
        return out2d, pnp_in, planes

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_out, g_pnp_in, g_planes):
        feat2d, out2d, w, cls_rows, sel, extents = ctx.saved_tensors
        w_shape, hw, double_mask = ctx.layer
        need = ctx.needs_input_grad
        dfeat = dw = db = None
        if any(need[:3]) and not (g_out is None and g_pnp_in is None and g_planes is None):
            g_out, g_pnp_in, g_planes = (None if g is None else g.contiguous() for g in (g_out, g_pnp_in, g_planes))
            d_out = hip_lib.head_tail_backward(out2d, extents, double_mask, g_pnp_in, g_planes, g_out)
            if need[0]:
                dfeat = hip_lib.grouped_linear_dinput(d_out, w, sel, hw)
            if need[1] or need[2]:
                dw, db = hip_lib.grouped_linear_wgrad(d_out, feat2d, sel, cls_rows, w.shape[0], w_shape[0], hw, want=(need[1], need[2]))
                dw = None if dw is None else dw.view(w_shape)
        return dfeat, dw, db, None, None, None, None, None


def head_tail_train_ok(feat: torch.Tensor, out_layer: nn.Module) -> bool:
    """Shapes and state ``HeadTail`` takes: switch on, gradients enabled, an fp32 device tensor [B,K,H,W] with K a multiple of 128 up
    to 256 and H W a multiple of 256, the 1x1 output layer with a bias on the device.  The head's configuration is the caller's to
    check (GDRN_DoubleMask._tail_config_ok)."""
    k = feat.shape[1] if feat.dim() == 4 else 0
    return (_train_ok(feat) and _MLP_GEMM == "split" and isinstance(out_layer, nn.Conv2d) and out_layer.kernel_size == (1, 1)
            and out_layer.bias is not None and out_layer.in_channels == k and k % 128 == 0 and k <= _HEAD_TAIL_MAX_DEPTH
            and (feat.shape[2] * feat.shape[3]) % 256 == 0 and 0 < feat.shape[0] <= 65535
            and feat.shape[0] * feat.shape[2] * feat.shape[3] < (1 << 31) - 128
            and out_layer.weight.is_cuda and out_layer.weight.dtype == torch.float32)


def head_tail(out_layer: nn.Conv2d, cls_rows: torch.Tensor, feat: torch.Tensor, sel: torch.Tensor, coord2d: torch.Tensor,
              extents: torch.Tensor, double_mask: bool):
    """``HeadTail`` on the trunk's result feat [B,K,H,W] -> (out2d, pnp_in, planes); after ``head_tail_train_ok``."""
    bs, ch, h, wd = feat.shape
    x2d = _cl(feat).permute(0, 2, 3, 1).reshape(bs * h * wd, ch)      # a view of the NHWC memory
    return HeadTail.apply(x2d, out_layer.weight, out_layer.bias, cls_rows, sel.to(torch.int32).contiguous(), coord2d.contiguous().float(),
                          extents.contiguous().float(), bool(double_mask))


class Conv3x3S2GnAct(torch.autograd.Function):
    """Patch-PnP's [Conv2d 3x3/2/1 without bias, GroupNorm, GELU] with its backward on HIP kernels (csrc/pnp_bwd.hip).  x (N,ld,H,W)
    channels_last whose first ``cin`` channels are the layer's input (the 96-pitch prepared input for the first layer, ld = cin
    behind it) -> y (N,Cout,H/2,W/2) channels_last.  The forward is the fp32-MFMA convolution (``gdrnpp_conv_bias_act_f32``, stride 2),
    the GroupNorm statistics and the apply pass: not the bits of the inference forward's six-product convolution, as in
    ``Conv3x3GnAct``.  Saved: x, the convolution's output z and the statistics' partial sums.  dx has x's channels and pitch, zero from ``cin`` on."""

    @staticmethod
    def forward(ctx, x, cin, weight, gn_weight, gn_bias, groups, eps, gelu):
        z = hip_lib.conv3x3s2_f32_mfma(x, hip_lib.conv3x3s2_weight_kn(weight))      # operand made per forward: the weight changes every step
        y, part = hip_lib.groupnorm_act_train(z, gn_weight, gn_bias, groups, eps, gelu)
        ctx.save_for_backward(x, z, part, weight, gn_weight, gn_bias)
        ctx.cin, ctx.gn = cin, (groups, eps, gelu)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, z, part, weight, gn_weight, gn_bias = ctx.saved_tensors
        need = ctx.needs_input_grad
        conv = (need[0], need[2])
        dx = dw = dg = dbeta = None
        if any(conv) or need[3] or need[4]:
            dz, dg, dbeta = hip_lib.groupnorm_act_backward(z, part, gn_weight, gn_bias, *ctx.gn, _cl(grad_y), want=(any(conv), need[3], need[4]))
            if any(conv):
                dx, dw = hip_lib.conv3x3s2_backward(x, ctx.cin, weight, dz, want=conv)
        return dx, None, dw, dg, dbeta, None, None, None


class FlattenNCHW(torch.autograd.Function):
    """``x.flatten(1)`` of a channels_last tensor in NCHW order (the order Patch-PnP's fc1 was trained in) on
    ``gdrnpp_nhwc_flatten_nchw``, and its inverse for the gradient; nothing is saved."""

    @staticmethod
    def forward(ctx, x):
        ctx.chw = tuple(x.shape[1:])
        return hip_lib.nhwc_flatten_nchw(x)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        return hip_lib.nhwc_unflatten_nchw(grad_y.contiguous(), *ctx.chw)


class LinearGelu(torch.autograd.Function):
    """gelu(x W^T + b) on [M,K] rows with few rows and a long K (Patch-PnP's fc1 and fc2): ``linear_f32_exact`` + ``gelu_f32`` forward;
    backward ``mlp_bwd_act_`` (dpre and the bias gradient), ``gemm_tn_f32`` (dW, its slot tiles in the persistent workspace) and
    ``linear_f32_exact`` on the weight as it lies (dx).  Saved: x, the pre-activation and the weight."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        pre = hip_lib.linear_f32_exact(x, weight, bias)
        ctx.save_for_backward(x, pre, weight)
        return hip_lib.gelu_f32(pre)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, pre, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx = dw = db = None
        if any(need[:3]):
            dpre = torch.empty_like(pre)      # autograd's grad_y may be somebody else's too: the activation pass works in place on a copy
            hip_lib.copy_d2d(dpre.data_ptr(), grad_y.contiguous())
            _, db = hip_lib.mlp_bwd_act_(pre, dpre, want_h=False, want_db1=need[2])
            if need[0]:
                dx = hip_lib.linear_f32_exact(dpre, weight, weight_kn=True)
            if need[1]:
                dw = hip_lib.gemm_tn_f32(dpre, x, persistent_ws=True)
        return dx, dw, db


class PnPHeads(torch.autograd.Function):
    """(fc_r(x), fc_t(x)) of Patch-PnP: ``gdrnpp_pnp_fc_heads`` forward, ``gdrnpp_pnp_fc_heads_backward`` backward.  A head the loss
    does not use arrives as None and contributes nothing.  Saved: x and the two weights."""

    @staticmethod
    def forward(ctx, x, w_r, b_r, w_t, b_t):
        ctx.save_for_backward(x, w_r, w_t)
        ctx.set_materialize_grads(False)
        return hip_lib.pnp_fc_heads(x, w_r.detach(), b_r.detach(), w_t.detach(), b_t.detach())

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_r, g_t):
        x, w_r, w_t = ctx.saved_tensors
        need = ctx.needs_input_grad
        if not any(need[:5]) or (g_r is None and g_t is None):
            return (None,) * 5
        g_r, g_t = (None if g is None else g.contiguous() for g in (g_r, g_t))
        return hip_lib.pnp_fc_heads_backward(g_r, g_t, x, w_r, w_t, want=need[:5])


def _param_ok(*tensors) -> bool:
    return all(t is not None and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)


def _pnp_train_ok(net: nn.Module, x96_cl: torch.Tensor) -> bool:
    """Shapes and state ``pnp_train`` takes: ``_train_ok`` plus the shipped ConvNeXt configuration of ConvPnPNet — the prepared 96-pitch
    channels_last input, three [Conv2d 3x3/2/1 without bias, GroupNorm, exact GELU] to featdim % 128 == 0 channels, H and W
    multiples of 8 that end at fc1's width, exact GELU behind fc1 and fc2, no mask attention, heads of at most 9 and of 3 rows."""
    f = getattr(net, "features", ())
    if not (_train_ok(x96_cl) and _MLP_GEMM == "split" and x96_cl.shape[1] == 96 and x96_cl.is_contiguous(memory_format=torch.channels_last)
            and len(f) == 9 and net.mask_attention_type == "none" and net.accepts_prepared_input() and _exact_gelu_or_none(net.act)
            and net.act is not None and x96_cl.shape[2] % 8 == 0 and x96_cl.shape[3] % 8 == 0):
        return False
    n, _, h, w = x96_cl.shape
    cin = 69
    for i in range(0, 9, 3):
        conv, gn, act = f[i], f[i + 1], f[i + 2]
        if not (isinstance(conv, nn.Conv2d) and isinstance(gn, nn.GroupNorm) and isinstance(act, nn.GELU) and _exact_gelu_or_none(act)
                and conv.kernel_size == (3, 3) and conv.stride == (2, 2) and conv.padding == (1, 1) and conv.dilation == (1, 1)
                and conv.groups == 1 and conv.padding_mode == "zeros" and conv.bias is None and conv.in_channels == cin
                and conv.out_channels % 128 == 0 and gn.num_channels == conv.out_channels and _gn_train_shape_ok(gn, n)
                and conv.weight.is_cuda and conv.weight.dtype == torch.float32      # any memory format: the operands are formed per call
                and _param_ok(gn.weight, gn.bias) and n * h * w < (1 << 31) - 4096):
            return False
        cin, h, w = conv.out_channels, h // 2, w // 2
    fc1, fc2, fc_r, fc_t = net.fc1, net.fc2, net.fc_r, net.fc_t
    return (fc1.in_features == cin * h * w and fc1.out_features % 128 == 0 and fc2.in_features == fc1.out_features
            and fc2.out_features % 128 == 0 and fc_r.in_features == fc_t.in_features == fc2.out_features <= 1024
            and fc_r.out_features <= 9 and fc_t.out_features == 3
            and _param_ok(fc1.weight, fc1.bias, fc2.weight, fc2.bias, fc_r.weight, fc_r.bias, fc_t.weight, fc_t.bias))


def pnp_train(net: nn.Module, x96_cl: torch.Tensor):
    """ConvPnPNet on the prepared input under autograd, every layer on this library's kernels forward and backward; after
    ``_pnp_train_ok``.  -> (rot, t) as ``forward_prepared`` returns them."""
    x, cin = x96_cl, 69
    for i in range(0, 9, 3):
        conv, gn = net.features[i], net.features[i + 1]
        x = Conv3x3S2GnAct.apply(x, cin, conv.weight, gn.weight, gn.bias, gn.num_groups, gn.eps, True)
        cin = conv.out_channels
    x = LinearGelu.apply(FlattenNCHW.apply(x), net.fc1.weight, net.fc1.bias)
    x = LinearGelu.apply(x, net.fc2.weight, net.fc2.bias)
    return PnPHeads.apply(x, net.fc_r.weight, net.fc_r.bias, net.fc_t.weight, net.fc_t.bias)


class StemConvLN(torch.autograd.Function):
    """The ConvNeXt stem [Conv2d(3 -> 128, 4x4/4), LayerNorm2d] with its backward on a HIP kernel (csrc/backbone_bwd.hip).  x (N,3,H,W)
    NCHW without a gradient of its own -> y (N,128,H/4,W/4) channels_last, the bits of the inference forward.  The backward recomputes
    the pre-norm activation and the statistics from x; saved are x and the parameters (the weight as the [co][ci][ky][kx] copy the
    forward read)."""

    @staticmethod
    def forward(ctx, x, weight, bias, ln_weight, ln_bias, eps):
        w = weight.detach().contiguous()      # the module may hold the weight channels_last; made per forward: the weight changes every step
        ctx.save_for_backward(x, w, bias, ln_weight)
        ctx.eps = eps
        return hip_lib.stem_conv4x4_ln(x, w, bias, ln_weight, ln_bias, eps)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, w, bias, ln_weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        grads = (None,) * 4
        if any(need[1:5]):
            grads = hip_lib.stem_conv4x4_ln_backward(x, w, bias, ln_weight, ctx.eps, _cl(grad_y), want=need[1:5])
        return (None, *grads, None)


class DownsampleLNConv(torch.autograd.Function):
    """A ConvNeXt stage entry [LayerNorm2d(C), Conv2d(C -> Cout, 2x2/2)] with its backward on this library's kernels.  x (N,C,H,W)
    channels_last -> z (N,Cout,H/2,W/2) channels_last.  The forward writes the LayerNorm's result in patch order (``layernorm_patch2x2``:
    the bits of the inference LayerNorm) and runs the convolution as A Wp^T + b on ``linear_f32_exact`` (a depth of 4 C >= 512: past
    the six-product kernel's accuracy) — not the bits of the inference forward's three-product convolution, as in
    ``Conv3x3GnAct``.  Saved: x, the LayerNorm's weight, the convolution's weight and, when that weight takes a gradient, A (the
    weight gradient's operand; kept, not recomputed: it is x's size and the forward has it in hand)."""

    @staticmethod
    def forward(ctx, x, ln_weight, ln_bias, eps, weight, bias):
        n, _, h, w = x.shape
        a = hip_lib.layernorm_patch2x2(x, ln_weight, ln_bias, eps)
        z = hip_lib.linear_f32_exact(a, hip_lib.downsample_weight_nk(weight), bias)      # operand made per forward: the weight changes every step
        ctx.save_for_backward(x, a if ctx.needs_input_grad[4] else None, ln_weight, weight)
        ctx.eps = eps
        return z.view(n, h // 2, w // 2, weight.shape[0]).permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_z):
        x, a, ln_weight, weight = ctx.saved_tensors
        need = ctx.needs_input_grad
        want = (need[0], need[1], need[2], need[4], need[5])
        dx = dg = dbeta = dw = db = None
        if any(want):
            dx, dg, dbeta, dw, db = hip_lib.downsample_backward(x, a, ln_weight, ctx.eps, weight, _cl(grad_z), want=want)
        return dx, dg, dbeta, None, dw, db


def _downsample_train_ok(ln: nn.Module, conv: nn.Module, x: torch.Tensor) -> bool:
    """Shapes and state ``DownsampleLNConv`` takes: ``_train_ok``, no autocast, LayerNorm with weight and bias over C = 128, 256, 512 or
    1024 channels, a dense 2x2 / stride 2 convolution without padding to a multiple of 128 channels, even H and W."""
    if not (_train_ok(x) and not torch.is_autocast_enabled() and isinstance(ln, nn.LayerNorm) and isinstance(conv, nn.Conv2d)):
        return False
    c = x.shape[1]
    return (ln.elementwise_affine and tuple(ln.normalized_shape) == (c,) and _param_ok(ln.weight, ln.bias) and c in (128, 256, 512, 1024)
            and conv.in_channels == c and conv.out_channels % 128 == 0 and conv.kernel_size == (2, 2) and conv.stride == (2, 2)
            and conv.padding == (0, 0) and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros"
            and conv.weight.is_cuda and conv.weight.dtype == torch.float32 and (conv.bias is None or _param_ok(conv.bias))
            and x.shape[2] % 2 == 0 and x.shape[3] % 2 == 0 and 0 < x.shape[0] * x.shape[2] * x.shape[3] < (1 << 31) - 4096)


def downsample(ln: nn.LayerNorm, conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """A ConvNeXt stage entry: LayerNorm2d, then the 2x2 / stride 2 convolution — ``conv2d(conv, ln(x))``, the inference kernels or the
    module path as those two decide.  With gradients enabled and ``set_train_kernels(True)`` the pair is ``DownsampleLNConv``."""
    if _downsample_train_ok(ln, conv, x):
        return DownsampleLNConv.apply(_cl(x), ln.weight, ln.bias, ln.eps, conv.weight, conv.bias)
    if _TRAIN_KERNELS and _ENABLED and torch.is_grad_enabled() and x.is_cuda:
        note_foreign_launch("downsample: under autograd outside DownsampleLNConv (odd size, another kernel, no affine LayerNorm, AMP)")
    return conv2d(conv, ln(x))


def _dwconv_train_ok(conv: nn.Conv2d, ln: nn.LayerNorm, x: torch.Tensor) -> bool:
    c = conv.in_channels
    q = c // 4
    return (_TRAIN_KERNELS and _ENABLED and torch.is_grad_enabled() and x.is_cuda and x.dtype == torch.float32 and x.dim() == 4
            and conv.kernel_size == (7, 7) and conv.stride == (1, 1) and conv.padding == (3, 3) and conv.dilation == (1, 1)
            and conv.groups == c == conv.out_channels and c % 4 == 0 and q <= 256 and 256 % q == 0 and conv.bias is not None
            and ln.elementwise_affine and ln.bias is not None and tuple(ln.normalized_shape) == (c,))


def dwconv_ln(conv: nn.Conv2d, ln: nn.LayerNorm, x: torch.Tensor, cache: dict, y_rows: bool = False) -> torch.Tensor:
    """ConvNeXt block head: depthwise 7x7 then LayerNorm over C.  Returns the NHWC *view* [N,H,W,C].  ``y_rows``: as an "f16x2
    rows" tensor for ``convnext_mlp(..., a_rows=True)`` (HIP path only; ``mlp_takes_rows`` says when).  With gradients enabled
    and ``set_train_kernels(True)`` the layer is ``DwConvLN``: the inference kernel forward, HIP kernels backward."""
    c = conv.in_channels
    if not y_rows and _dwconv_train_ok(conv, ln, x):
        # tap-major [49, C], made per forward: the weight changes every step, and a refill of ``cache`` waits for the device twice
        w49c = conv.weight.detach().reshape(c, 49).t().contiguous()
        y = DwConvLN.apply(_cl(x), conv.weight, w49c, conv.bias, ln.weight, ln.bias, ln.eps)
        return y.permute(0, 2, 3, 1)
    if _dwconv_hip_ok(conv, x):
        hit = cached(cache, "w49c", weight_tag(conv.weight), lambda: (conv.weight.detach().reshape(c, 49).t().contiguous(),),
                     conv.weight)  # tap-major [49, C]
        y = hip_lib.dwconv7x7_ln(_cl(x), hit[1], conv.bias, ln.weight, ln.bias, ln.eps, y_rows=y_rows)
        return y.permute(0, 2, 3, 1)
    if y_rows:
        raise RuntimeError("dwconv_ln: an f16x2-rows result exists on the HIP path only")
    _fallback("dwconv_ln: depthwise kernel / channel count outside the HIP kernel", x)
    y = conv(x).permute(0, 2, 3, 1)
    return F.layer_norm(y, ln.normalized_shape, ln.weight, ln.bias, ln.eps)


# GEMM engine of the ConvNeXt MLPs / head convolutions:
#   "split" (default) gdrnpp_linear_f32_split / gdrnpp_conv2d_f32_split: bf16 matrix cores, exact 3-way operand split, six
#                     partial products, fp32 accumulate — error vs fp64 at or below an fp32 fma chain, ~1.4x the fp32-MFMA rate;
#   "torch"           hipBLASLt / MIOpen fp32 + separate elementwise kernels everywhere (A/B measurements).
_MLP_GEMM = "split"
_SPLITK_BELOW_TILES = 512
_LIBRARY_BELOW_TILES = 0    # A/B switch: blocks whose fc2 has fewer 128x128 output tiles than this go to hipBLASLt + elementwise
                            # kernels.  Round 2 shipped 128 (the register-staged split-K kernel lost to the library's small-tile
                            # kernels at 8 ROIs); since round 3 gdrnpp_linear_f32_splitk runs such shapes on the pipelined kernel
                            # with a modelled number of K chunks and no block leaves this library


def set_mlp_gemm(mode: str) -> None:
    global _MLP_GEMM
    if mode not in ("split", "torch"):
        raise ValueError(f"unknown MLP GEMM mode {mode!r}")
    _MLP_GEMM = mode


def mlp_gemm() -> str:
    """Current GEMM engine of the network layers: "split" (HIP, bf16x6) or "torch" (hipBLASLt / MIOpen)."""
    return _MLP_GEMM


def set_library_below_tiles(n: int) -> None:
    """ConvNeXt blocks whose fc2 result has fewer than ``n`` 128x128 tiles run on hipBLASLt + elementwise kernels instead
    of the split GEMM (one image's worth of ROIs leaves the deep stages with a handful of tiles)."""
    global _LIBRARY_BELOW_TILES
    _LIBRARY_BELOW_TILES = int(n)


_FUSED_MLP = True
_FUSED_MLP_MAX_C = 256              # widest block that takes the fused kernel (it exists for C = 128 and C = 256)
_FUSED_MLP_MIN_ROWS = 128 * 256     # one 128-pixel workgroup per CU at least (8 ROIs at stage 0, 32 at stage 1; measured: profiles/r04e)


def set_fused_mlp_x3(flag: bool, max_c: int = 256, min_rows: int | None = None) -> None:
    """A/B switch: False runs the stage-0 / stage-1 ConvNeXt MLPs as two three-product launches again; ``max_c`` = 128 keeps the
    fused form to stage 0; ``min_rows``: fewest pixels a block must have to take it."""
    global _FUSED_MLP, _FUSED_MLP_MAX_C, _FUSED_MLP_MIN_ROWS
    _FUSED_MLP = bool(flag)
    _FUSED_MLP_MAX_C = int(max_c)
    if min_rows is not None:
        _FUSED_MLP_MIN_ROWS = int(min_rows)


def _fused_mlp_weights(mlp, cache: dict, m: int, c: int):
    """-> (packed image, fc1 slot, fc2 slot) when this block can run ``hip_lib.convnext_mlp_f32_fused``: the shape the kernel exists
    for, enough rows to fill the chip, both layers eligible for the three-product form (not demoted, weight rows in range)."""
    if not (_FUSED_MLP and c <= _FUSED_MLP_MAX_C and gemm_products() == 3 and m >= _FUSED_MLP_MIN_ROWS and hip_lib.mlp_fused_supported(c, 4 * c)
            and m * c * 4 < (1 << 32)):
        return None
    s1, s2 = x3_slot(cache, "fc1"), x3_slot(cache, "fc2")
    if is_demoted(s1) or is_demoted(s2):
        return None
    def build():
        packed = hip_lib.pack_mlp_fused_f16x2(mlp.fc1.weight.detach().contiguous(), mlp.fc2.weight.detach().contiguous())
        return packed, all(hip_lib.mlp_fused_rows_in_range(packed))

    hit = cached(cache, "mlp_fused_pk", weight_tag(mlp.fc1.weight, mlp.fc2.weight), build, mlp.fc1.weight)
    if hit[2]:
        note_launch(s1, s2)
    return (hit[1], s1, s2) if hit[2] else None


# "f16x2 rows" hand-over between the kernels of a ConvNeXt block (include/gdrnpp_hip.h: gdrnpp_linear_f32_split2_rows): the
# depthwise conv + LayerNorm kernel writes fc1's operand already split, fc1's GELU epilogue writes fc2's.  Bit-identical results;
# the k-loops lose their split arithmetic (32 of ~90 VALU operations per k-tile).  False: fp32 tensors between the kernels (A/B).
_F16X2_ROWS = True


def set_f16x2_rows(flag: bool) -> None:
    global _F16X2_ROWS
    _F16X2_ROWS = bool(flag)


def _mlp_split_ok(x_nhwc: torch.Tensor, shortcut_nhwc: torch.Tensor, m: int, c: int) -> bool:
    return (_MLP_GEMM == "split" and enabled_for(x_nhwc) and x_nhwc.is_contiguous() and shortcut_nhwc.is_contiguous() and c % 128 == 0
            and hip_lib.split_gemm_tiles(m, c) >= _LIBRARY_BELOW_TILES)


def mlp_takes_rows(mlp, conv_dw: nn.Conv2d, x_nchw: torch.Tensor, cache: dict) -> bool:
    """Will ``convnext_mlp`` of this block read its input through the three-product fc1 kernel (so that ``dwconv_ln`` may hand it
    an f16x2-rows tensor)?  Same tests, same state (demotions, forced products) as ``convnext_mlp`` itself applies a moment later."""
    c = x_nchw.shape[1]
    m = x_nchw.numel() // c
    nhwc = x_nchw.permute(0, 2, 3, 1)
    if not (_F16X2_ROWS and _dwconv_hip_ok(conv_dw, x_nchw) and c % 8 == 0 and _mlp_split_ok(nhwc, nhwc, m, c)):
        return False
    if _fused_mlp_weights(mlp, cache, m, c) is not None:
        return False
    return x3_for(cache, "fc1", mlp.fc1.weight, hip_lib.pack_weight_f16x2, m, 4 * c, c)[0] is not None


class ConvNeXtMlp(torch.autograd.Function):
    """ConvNeXt block tail y = resid + gamma * fc2(gelu(fc1(x))) on [M,C] rows with its backward on HIP kernels (csrc/mlp_bwd.hip +
    the six-product split GEMM for products up to a depth of 256).  Saved: x, the pre-activation and the parameters — neither h nor the MLP's output.  The shortcut's
    gradient is grad_y itself."""

    @staticmethod
    def forward(ctx, x2d, w1, b1, w2, b2, gamma, resid):
        y, pre = hip_lib.convnext_mlp_forward_train(x2d, w1, b1, w2, b2, gamma, resid)
        ctx.save_for_backward(x2d, pre, w1, w2, b2, gamma)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x2d, pre, w1, w2, b2, gamma = ctx.saved_tensors
        need = ctx.needs_input_grad
        grad_y = grad_y.contiguous()
        grads = (None,) * 6
        if any(need[:6]):
            grads = hip_lib.convnext_mlp_backward(x2d, pre, w1, w2, b2, gamma, grad_y, want=need[:6])
        return (*grads, grad_y if need[6] else None)


def _mlp_train_ok(mlp, gamma: torch.Tensor, x_nhwc: torch.Tensor, shortcut_nhwc: torch.Tensor, m: int, c: int) -> bool:
    fc1, fc2 = getattr(mlp, "fc1", None), getattr(mlp, "fc2", None)
    act = getattr(mlp, "act", None)
    if not (_TRAIN_KERNELS and _ENABLED and torch.is_grad_enabled() and isinstance(fc1, nn.Linear) and isinstance(fc2, nn.Linear)):
        return False
    tensors = (x_nhwc, shortcut_nhwc, gamma, fc1.weight, fc1.bias, fc2.weight, fc2.bias)
    return (all(t is not None and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous() for t in tensors)
            and c % 128 == 0 and tuple(fc1.weight.shape) == (4 * c, c) and tuple(fc2.weight.shape) == (c, 4 * c) and gamma.numel() == c
            and shortcut_nhwc.shape == x_nhwc.shape and isinstance(act, nn.GELU) and getattr(act, "approximate", "none") == "none"
            and 0 < m and m * 4 * c < (1 << 31))      # the GEMMs index rows with int, the split GEMM's A image below 4 GiB


def convnext_mlp(mlp, gamma: torch.Tensor, x_nhwc: torch.Tensor, shortcut_nhwc: torch.Tensor, cache: dict, a_rows: bool = False) -> torch.Tensor:
    """timm ConvNeXtBlock tail on NHWC tensors: shortcut + gamma * fc2(gelu(fc1(x))).  On the GPU both Linear layers
    run in the library's own GEMM with the exact-erf GELU and the layer-scale/residual fused into the epilogues
    (two HBM passes over the hidden tensor saved); otherwise plain PyTorch.  ``a_rows``: x_nhwc is an f16x2-rows tensor
    (``dwconv_ln(..., y_rows=True)`` after ``mlp_takes_rows`` said yes).  With gradients enabled and ``set_train_kernels(True)`` the
    tail is ``ConvNeXtMlp``: this library's kernels forward and backward (six-product GEMMs up to a depth of 256, exact-f32 beyond)."""
    c = x_nhwc.shape[-1]
    m = x_nhwc.numel() // c
    if not a_rows and _mlp_train_ok(mlp, gamma, x_nhwc, shortcut_nhwc, m, c):
        y = ConvNeXtMlp.apply(x_nhwc.view(m, c), mlp.fc1.weight, mlp.fc1.bias, mlp.fc2.weight, mlp.fc2.bias, gamma, shortcut_nhwc.reshape(m, c))
        return y.view(x_nhwc.shape)
    if _MLP_GEMM != "torch" and _mlp_split_ok(x_nhwc, shortcut_nhwc, m, c):
        fused = None if a_rows else _fused_mlp_weights(mlp, cache, m, c)
        if fused is not None:     # stage 0 (C = 128): fc1 + GELU + fc2 + layer scale + residual in one launch, no hidden tensor in HBM
            y = hip_lib.convnext_mlp_f32_fused(x_nhwc.view(m, c), fused[0], mlp.fc1.bias, mlp.fc2.bias, gamma, shortcut_nhwc.view(m, c),
                                               fused[1], fused[2])
            return y.view(x_nhwc.shape)
        w31, slot1 = x3_for(cache, "fc1", mlp.fc1.weight, hip_lib.pack_weight_f16x2, m, 4 * c, c)
        w32, slot2 = x3_for(cache, "fc2", mlp.fc2.weight, hip_lib.pack_weight_f16x2, m, c, 4 * c)
        if a_rows and w31 is None:
            raise RuntimeError("convnext_mlp: f16x2-rows input, but fc1 is not on the three-product kernel (mlp_takes_rows decides)")
        h_rows = _F16X2_ROWS and w31 is not None and w32 is not None     # fc1's GELU epilogue writes fc2's operand already split
        if w31 is not None:
            h = hip_lib.linear_f32_split(x_nhwc.view(m, c), w31, mlp.fc1.bias, "gelu", x3_slot=slot1, a_rows=a_rows, c_rows=h_rows)
        else:
            # fewer than two output tiles per CU (small ROI counts at the deep stages): split K as well, or most of the chip idles
            f1 = hip_lib.linear_f32_splitk if hip_lib.split_gemm_tiles(m, 4 * c) < _SPLITK_BELOW_TILES else hip_lib.linear_f32_split
            h = f1(x_nhwc.view(m, c), six_product_weight(cache, "fc1_pk", mlp.fc1.weight, hip_lib.pack_weight_bf16x3), mlp.fc1.bias, "gelu")
        if w32 is not None:
            y = hip_lib.linear_f32_split(h, w32, mlp.fc2.bias, "scale_res", gamma, shortcut_nhwc.view(m, c), x3_slot=slot2, a_rows=h_rows)
        else:
            f2 = hip_lib.linear_f32_splitk if hip_lib.split_gemm_tiles(m, c) < _SPLITK_BELOW_TILES else hip_lib.linear_f32_split
            y = f2(h, six_product_weight(cache, "fc2_pk", mlp.fc2.weight, hip_lib.pack_weight_bf16x3), mlp.fc2.bias, "scale_res", gamma, shortcut_nhwc.view(m, c))
        return y.view(x_nhwc.shape)
    if a_rows:
        raise RuntimeError("convnext_mlp: f16x2-rows input outside the split-GEMM path")
    _fallback("convnext_mlp: block outside the split GEMM (C % 128 != 0, non-contiguous, or mlp_gemm == 'torch')", x_nhwc)
    return torch.addcmul(shortcut_nhwc, mlp(x_nhwc), gamma)


_CONV_SPLIT = True


def set_conv_split(flag: bool) -> None:
    """3x3 convolutions of the geometry head: True = implicit-GEMM split kernel, False = MIOpen."""
    global _CONV_SPLIT
    _CONV_SPLIT = bool(flag)


def _conv_split_ok(conv, x) -> bool:
    """Shapes ``gdrnpp_conv2d_f32_split`` takes: dense, square kernel / stride / zero padding, Cin % 32 == 0, Cout % 128 == 0."""
    return (_CONV_SPLIT and _MLP_GEMM == "split" and isinstance(conv, nn.Conv2d) and enabled_for(x)
            and conv.kernel_size[0] == conv.kernel_size[1] and conv.stride[0] == conv.stride[1]
            and conv.padding[0] == conv.padding[1] and isinstance(conv.padding[0], int) and conv.padding[0] < conv.kernel_size[0]
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros" and conv.in_channels % 32 == 0
            and conv.out_channels % 128 == 0
            and (x.shape[2] + 2 * conv.padding[0] - conv.kernel_size[0]) // conv.stride[0] * conv.stride[0] < x.shape[2])


def conv2d(conv: nn.Conv2d, x: torch.Tensor) -> torch.Tensor:
    """nn.Conv2d forward; dense convolutions with square kernel / stride / padding, Cin % 32 == 0 and Cout % 128 == 0 (the
    head's 3x3/1, ConvNeXt's 2x2/2 downsamples, Patch-PnP's 3x3/2) run as an implicit GEMM in ``gdrnpp_conv2d_f32_split``
    (bf16 matrix cores, fp32-accurate), everything else in MIOpen."""
    if _conv_split_ok(conv, x):
        cache = module_cache(conv)
        is3x3 = conv.kernel_size == (3, 3) and conv.stride == (1, 1) and conv.padding == (1, 1)
        ks, st, pd = conv.kernel_size[0], conv.stride[0], conv.padding[0]
        oh, ow = (x.shape[2] + 2 * pd - ks) // st + 1, (x.shape[3] + 2 * pd - ks) // st + 1
        w_pk, slot = split_weight(cache, "conv", "w_pk", conv.weight, hip_lib.pack_conv_weight_f16x2, hip_lib.pack_conv_weight_bf16x3,
                                  x.shape[0] * oh * ow, conv.out_channels, allow3=ks * ks <= 32)
        if is3x3:
            return hip_lib.conv3x3_f32_split(_cl(x), w_pk, conv.bias, x3_slot=slot)
        return hip_lib.conv2d_f32_split(_cl(x), w_pk, conv.bias, conv.kernel_size[0], conv.kernel_size[1], conv.stride[0],
                                       conv.padding[0], x3_slot=slot)
    _fallback("conv2d: convolution outside the split implicit GEMM (MIOpen)", x)
    return conv(x)


def folded_conv_bn(conv: nn.Conv2d, bn: nn.BatchNorm2d):
    """(weight, bias) of the convolution that equals ``bn(conv(x))`` in inference mode: w * s and beta - mean * s with
    s = gamma / sqrt(var + eps) per output channel, formed in float64, cached on the conv module until a parameter or a
    running statistic changes."""
    cache = module_cache(conv)
    def build():
        with torch.no_grad():
            s = bn.weight.double() / torch.sqrt(bn.running_var.double() + bn.eps)
            w = (conv.weight.double() * s.view(-1, 1, 1, 1)).float().contiguous(memory_format=torch.channels_last)
            b0 = conv.bias.double() if conv.bias is not None else 0.0
            b = (bn.bias.double() + (b0 - bn.running_mean.double()) * s).float().contiguous()
        return w, b

    hit = cached(cache, "bn_fold", weight_tag(conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean, bn.running_var), build, conv.weight)
    return hit[1], hit[2]


_BN_SPLIT_MIN_TILES = 256   # 128x128 output tiles from which the split implicit GEMM beats MIOpen's fp32 kernels on the ResNet
                            # layers (config 1, 32 ROIs: 6.06 ms per step all-MIOpen, 5.91 at 256, 6.30 at 128, 7.2 at 64 and below)


def folded_conv(conv: nn.Conv2d, bn: nn.BatchNorm2d, x: torch.Tensor) -> torch.Tensor:
    """conv(x) with the BatchNorm scale folded into the weights and no bias: the split implicit GEMM when the layer fits it
    and gives the chip enough output tiles, else MIOpen."""
    w, _ = folded_conv_bn(conv, bn)
    k, st, pd = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    if _conv_split_ok(conv, x):
        oh, ow = (x.shape[2] + 2 * pd - k) // st + 1, (x.shape[3] + 2 * pd - k) // st + 1
        if hip_lib.split_gemm_tiles(x.shape[0] * oh * ow, conv.out_channels) >= _BN_SPLIT_MIN_TILES:
            cache = conv.__dict__["_gdrnpp_cache"]
            hit = cached(cache, "bn_fold_pk", weight_tag(w), lambda: (hip_lib.pack_conv_weight_bf16x3(w),), w)
            return hip_lib.conv2d_f32_split(_cl(x), hit[1], None, k, k, st, pd)
    _fallback("folded_conv: ResNet convolution on MIOpen", x)
    return F.conv2d(_cl(x), w, None, conv.stride, conv.padding, conv.dilation, conv.groups)


def conv_bn_act(conv: nn.Conv2d, bn: nn.BatchNorm2d, x: torch.Tensor, relu: bool, resid: torch.Tensor | None = None,
                extra_bias: torch.Tensor | None = None) -> torch.Tensor:
    """[Conv2d, BatchNorm2d (inference), (+ resid), (ReLU)] of a ResNet block as the folded convolution + ONE elementwise
    kernel (``gdrnpp_bias_act_nhwc``) instead of BatchNorm, add and ReLU kernels.  ``extra_bias`` is added to the folded
    bias (the folded bias of a downsample branch whose convolution output arrives as ``resid``)."""
    if (enabled_for(x) and not bn.training and bn.affine and bn.track_running_stats and conv.out_channels % 4 == 0
            and x.dtype == torch.float32):
        w, b = folded_conv_bn(conv, bn)
        if extra_bias is not None:
            b = b + extra_bias
        y = folded_conv(conv, bn, x)
        return hip_lib.bias_act_nhwc_(_cl(y), b, None if resid is None else _cl(resid), relu)
    _fallback("conv_bn_act: BatchNorm in training mode / without statistics", x)
    y = bn(conv(x))
    if extra_bias is not None:
        y = y + extra_bias.view(1, -1, 1, 1)
    if resid is not None:
        y = y + resid
    return torch.relu_(y) if relu else y


def _deconv_split_ok(deconv, x) -> bool:
    ks = deconv.kernel_size[0]
    return (_CONV_SPLIT and _MLP_GEMM == "split" and isinstance(deconv, nn.ConvTranspose2d) and enabled_for(x)
            and deconv.kernel_size[0] == deconv.kernel_size[1]
            and deconv.stride[0] == deconv.stride[1] and deconv.padding[0] == deconv.padding[1]
            and deconv.output_padding[0] == deconv.output_padding[1] and deconv.output_padding[0] < deconv.stride[0]
            and deconv.dilation == (1, 1) and deconv.groups == 1 and deconv.in_channels % 32 == 0
            and deconv.out_channels % 4 == 0 and (ks * ks * deconv.out_channels) % 128 == 0)


def _deconv_weight(deconv, x):
    """-> (packed GEMM weight of the transposed convolution in the three- or six-product format, range-word slot)."""
    ks = deconv.kernel_size[0]
    return split_weight(module_cache(deconv), "deconv", "w_pk", deconv.weight, hip_lib.pack_deconv_weight_f16x2,
                        hip_lib.pack_deconv_weight_bf16x3, x.shape[0] * x.shape[2] * x.shape[3], ks * ks * deconv.out_channels,
                        deconv.in_channels)


def conv_transpose2d(deconv: nn.ConvTranspose2d, x: torch.Tensor) -> torch.Tensor:
    """nn.ConvTranspose2d forward; the head's square-kernel / stride-2 form with Cin % 32 == 0 and KS*KS*Cout % 128 == 0
    runs as split GEMM + col2im gather (``hip_lib.conv_transpose2d_f32_split``), everything else in MIOpen."""
    if _deconv_split_ok(deconv, x):
        w_pk, slot = _deconv_weight(deconv, x)
        return hip_lib.conv_transpose2d_f32_split(_cl(x), w_pk, deconv.bias, deconv.kernel_size[0], deconv.stride[0], deconv.padding[0],
                                                  deconv.output_padding[0], x3_slot=slot)
    _fallback("conv_transpose2d: transposed convolution outside the split GEMM + col2im form (MIOpen)", x)
    return deconv(x)


def conv_transpose2d_groupnorm_act(deconv: nn.ConvTranspose2d, gn: nn.GroupNorm, act: nn.Module | None, x: torch.Tensor):
    """The head's [ConvTranspose2d, GroupNorm(, GELU)] triple with the GroupNorm statistics taken by the col2im gather
    (``hip_lib.conv_transpose2d_groupnorm_act``).  Returns None when the layers are outside that form; the caller then runs them
    one by one.  With gradients enabled and ``set_train_kernels(True)`` the triple is ``ConvTranspose2dGn``."""
    if _deconv_gn_train_ok(deconv, gn, act, x):
        geom = (deconv.kernel_size[0], deconv.stride[0], deconv.padding[0], deconv.output_padding[0])
        return ConvTranspose2dGn.apply(_cl(x), deconv.weight, deconv.bias, gn.weight, gn.bias, geom, gn.num_groups, gn.eps, act is not None)
    if not (_CONV_GN_FUSED and _deconv_split_ok(deconv, x) and isinstance(gn, nn.GroupNorm) and gn.num_channels == deconv.out_channels
            and _gn_ok(gn, x) and _exact_gelu_or_none(act)):
        return None
    w_pk, slot = _deconv_weight(deconv, x)
    return hip_lib.conv_transpose2d_groupnorm_act(_cl(x), w_pk, deconv.bias, deconv.kernel_size[0], deconv.stride[0], deconv.padding[0],
                                                  deconv.output_padding[0], gn.weight, gn.bias, gn.num_groups, gn.eps,
                                                  gelu=act is not None, x3_slot=slot)


_CONV_GN_FUSED = True


def set_conv_gn_fused(flag: bool) -> None:
    """A/B switch: False runs conv3x3 and GroupNorm as two layers (statistics pass + apply pass) again."""
    global _CONV_GN_FUSED
    _CONV_GN_FUSED = bool(flag)


def conv3x3_groupnorm_act(conv: nn.Conv2d, gn: nn.GroupNorm, act: nn.Module | None, x: torch.Tensor):
    """The head's [Conv2d 3x3/1/1, GroupNorm(, GELU)] triple with the GroupNorm statistics taken in the convolution's
    epilogue (``hip_lib.conv3x3_groupnorm_act``).  Returns None when the layers or the shape are outside that form; the
    caller then runs them one by one.  With gradients enabled and ``set_train_kernels(True)`` the triple is ``Conv3x3GnAct``."""
    if _conv_gn_train_ok(conv, gn, act, x):
        return Conv3x3GnAct.apply(_cl(x), conv.weight, conv.bias, gn.weight, gn.bias, gn.num_groups, gn.eps, act is not None)
    if not (_CONV_GN_FUSED and _CONV_SPLIT and _MLP_GEMM == "split" and enabled_for(x) and conv.kernel_size == (3, 3) and conv.stride == (1, 1)
            and conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros"
            and conv.in_channels % 32 == 0 and conv.out_channels % 128 == 0 and gn.affine
            and gn.num_channels == conv.out_channels and conv.out_channels == 8 * gn.num_groups
            and _exact_gelu_or_none(act)):
        return None
    cache = module_cache(conv)
    w_pk, slot = split_weight(cache, "conv", "w_pk", conv.weight, hip_lib.pack_conv_weight_f16x2, hip_lib.pack_conv_weight_bf16x3,
                              x.shape[0] * x.shape[2] * x.shape[3], conv.out_channels)
    return hip_lib.conv3x3_groupnorm_act(_cl(x), w_pk, conv.bias, gn.weight, gn.bias, gn.num_groups, gn.eps,
                                         gelu=act is not None, x3_slot=slot)


# [UpsamplingBilinear2d(2), ConvModule 3x3] of the geometry head at the low resolution (hip_lib.upsample2x_conv3x3_groupnorm_act):
# the library option "upconv_lowres" (default 1) is the switch, 0 = the upsampling and the convolution as two layers.
_UPCONV_MIN_PIXELS = 32768     # high-resolution pixels of the launch (8 ROIs at 64 x 64, 32 at 32 x 32) from which the pair takes the
                               # low-resolution form: where the convolution it replaces runs its 256-row tiles (conv3x3_groupnorm_act)
_UPCONV_CHUNK_ROWS = 32768     # low-resolution pixels per tap GEMM (32 ROIs at 32 x 32): its [rows, 9 * Cout] result is the workspace,
                               # 302 MB at Cout = 256 whatever the batch (profiles/upconv_lowres.md)


def set_upconv_lowres(min_pixels: int | None = None, chunk_rows: int | None = None) -> None:
    """A/B and test knobs of the low-resolution form: fewest high-resolution pixels that take it, low-resolution pixels per chunk."""
    global _UPCONV_MIN_PIXELS, _UPCONV_CHUNK_ROWS
    if min_pixels is not None:
        _UPCONV_MIN_PIXELS = int(min_pixels)
    if chunk_rows is not None:
        _UPCONV_CHUNK_ROWS = int(chunk_rows)


def upsample2x_conv3x3_groupnorm_act(conv: nn.Conv2d, gn: nn.GroupNorm, act: nn.Module | None, x: torch.Tensor):
    """[UpsamplingBilinear2d(2), Conv2d 3x3/1/1, GroupNorm(, GELU)] on the low-resolution input ``x``: the nine tap products at
    the low resolution (a quarter of the convolution's matrix work), then a gather that interpolates and sums them and takes
    the GroupNorm statistics.  Returns None outside the form of ``conv3x3_groupnorm_act`` (or with the library option
    "upconv_lowres" at 0, or below the minimum size); the caller then runs the layers one by one.  Under autograd too (``enabled_for``
    is false there): with ``set_train_kernels(True)`` the two layers are then ``Upsample2x`` and ``Conv3x3GnAct``."""
    if not (_CONV_GN_FUSED and _CONV_SPLIT and _MLP_GEMM == "split" and enabled_for(x) and isinstance(conv, nn.Conv2d)
            and isinstance(gn, nn.GroupNorm) and conv.kernel_size == (3, 3) and conv.stride == (1, 1)
            and conv.padding == (1, 1) and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros"
            and conv.in_channels % 32 == 0 and conv.out_channels % 128 == 0 and gn.affine
            and gn.num_channels == conv.out_channels and conv.out_channels == 8 * gn.num_groups and gn.num_groups <= 64
            and conv.out_channels <= 1024 and 256 % (conv.out_channels // 4) == 0 and _exact_gelu_or_none(act)
            and x.dim() == 4 and x.shape[1] == conv.in_channels and 0 < x.shape[0] <= 65535
            and 4 * x.shape[0] * x.shape[2] * x.shape[3] >= _UPCONV_MIN_PIXELS and hip_lib.get_option("upconv_lowres")):
        return None
    n, _, h, w = x.shape
    chunk = max(1, _UPCONV_CHUNK_ROWS // (h * w))
    w_pk, slot = split_weight(module_cache(conv), "upconv", "w_upconv_pk", conv.weight, hip_lib.pack_upconv_weight_f16x2,
                              hip_lib.pack_upconv_weight_bf16x3, min(n, chunk) * h * w, 9 * conv.out_channels, conv.in_channels,
                              slot_key="conv")
    return hip_lib.upsample2x_conv3x3_groupnorm_act(_cl(x), w_pk, conv.bias, gn.weight, gn.bias, gn.num_groups, gn.eps,
                                                    gelu=act is not None, x3_slot=slot, chunk=chunk)


def linear(fc: nn.Linear, x: torch.Tensor, gelu: bool = False) -> torch.Tensor:
    """nn.Linear on a [M, K] activation with few rows and a long K (Patch-PnP fc1: 8192 -> 1024 on one row per ROI):
    hipBLASLt picks a 256x16 macro-tile for it and streams the 33 MB weight at ~70 GB/s (0.49 ms at 128 ROIs); the split-K
    form of the split GEMM spreads K over 64 workgroups per output tile."""
    if (_MLP_GEMM == "split" and enabled_for(x) and x.dim() == 2 and x.is_contiguous() and fc.out_features % 128 == 0
            and fc.in_features % 32 == 0 and fc.in_features >= 1024 and x.shape[0] <= 1024):
        cache = module_cache(fc)
        return hip_lib.linear_f32_splitk(x, six_product_weight(cache, "w_pk", fc.weight, hip_lib.pack_weight_bf16x3), fc.bias, "gelu" if gelu else "none")
    _fallback("linear: nn.Linear outside the split-K form (hipBLASLt)", x)
    return F.gelu(fc(x)) if gelu else fc(x)


def _heads_with_pose(feat, w_r, b_r, w_t, b_t, pose: dict | None):
    """The two pose heads in one launch; with ``pose`` and a rotation head of that mode's width the same launch also leaves
    ``pose["result"] = (R_ego, trans)``."""
    if pose is not None and w_r.shape[0] == hip_lib.ROT_DIMS[pose["rot_mode"]]:
        kw = {k: v for k, v in pose.items() if k != "result"}
        rot_, t_, R, trans = hip_lib.pnp_fc_heads_pose(feat, w_r, b_r, w_t, b_t, **kw)
        pose["result"] = (R, trans)
        return rot_, t_
    return hip_lib.pnp_fc_heads(feat, w_r, b_r, w_t, b_t)


def pnp_fc_heads(fc_r: nn.Linear, fc_t: nn.Linear, x: torch.Tensor, pose: dict | None = None):
    """(fc_r(x), fc_t(x)) of Patch-PnP in one HIP launch instead of two library GEMMs (conv_pnp_net.py:99-101,178-182).
    ``pose`` (the keyword arguments of ``hip_lib.pose_from_pred`` after its two head tensors): the same launch also turns them
    into the pose and leaves ``pose["result"] = (R_ego, trans)``."""
    if (enabled_for(x) and _MLP_GEMM == "split" and x.dim() == 2 and x.is_contiguous() and fc_r.in_features == fc_t.in_features <= 1024
            and fc_r.out_features <= 9 and fc_t.out_features == 3):
        w_r, w_t = fc_r.weight.detach().contiguous(), fc_t.weight.detach().contiguous()
        return _heads_with_pose(x, w_r, fc_r.bias, w_t, fc_t.bias, pose)
    _fallback("pnp_fc_heads: pose heads outside the one-launch kernel (hipBLASLt)", x)
    return fc_r(x), fc_t(x)


def point_pnp(head: nn.Module, x2d: torch.Tensor, b: int, hw: int, pose: dict | None = None):
    """SimplePointPnPNet on a prepared NHWC input ``x2d`` f32[b*hw, pitch] whose first ``head.conv1.in_channels`` channels are
    the head's own concatenation: three launches — point-wise MLP + max over the points (``gdrnpp_point_pnp_pool``), fc1 / fc2
    (``gdrnpp_point_pnp_fc``), fc_pose as the two row slices of its weight through ``pnp_fc_heads`` (which also leaves the pose
    in ``pose["result"]``).  Outside the kernels (CPU tensor, HIP layers off, hw not a multiple of the point tile, more than 128
    input channels) the same layers run as PyTorch operators, counted as a fallback."""
    cin = head.conv1.in_channels
    if (enabled_for(x2d) and x2d.dim() == 2 and x2d.is_contiguous() and hw % hip_lib.POINT_PNP_TILE == 0 and x2d.shape[1] % 32 == 0
            and cin <= min(128, x2d.shape[1]) and not head.use_softpool):
        _, ws = hip_lib.point_pnp_pool(x2d, cin, head.conv1.weight.detach(), head.conv1.bias.detach(), head.conv2.weight.detach(),
                                       head.conv2.bias.detach(), head.conv3.weight.detach(), head.conv3.bias.detach(), b, hw,
                                       want_pooled=False)
        feat = hip_lib.point_pnp_fc(ws, head.fc1.weight.detach(), head.fc1.bias.detach(), head.fc2.weight.detach(),
                                    head.fc2.bias.detach(), b, hw)
        rd = head.rot_dim
        w, bias = head.fc_pose.weight.detach(), head.fc_pose.bias.detach()      # row slices of a contiguous matrix are contiguous
        w_r, w_t, b_r, b_t = w[:rd], w[rd:rd + 3], bias[:rd], bias[rd:rd + 3]
        return _heads_with_pose(feat, w_r, b_r, w_t, b_t, pose)
    _fallback("point_pnp: SimplePointPnPNet outside the fused point-MLP kernel (PyTorch operators)", x2d)
    return head.mlp_tail(x2d.view(b, hw, x2d.shape[1])[:, :, :cin].transpose(1, 2))
