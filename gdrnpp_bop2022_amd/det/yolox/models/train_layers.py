"""Training YOLOX's ``BaseConv`` — Conv2d, BatchNorm2d with batch statistics, SiLU — on this library's kernels
(csrc/conv_bn_bwd.hip and the fp32-MFMA convolution of csrc/yolox_net.hip), behind ``hip_layers.set_train_kernels(True)``.

``conv_bn_silu(conv, bn, x)`` is what ``BaseConv.forward`` asks first in training mode; it answers ``None`` for everything outside the
kernels and the caller then runs the module path unchanged.  With the switch off (the default) it always answers ``None``.

What stays on PyTorch's operators, on the channels_last tensors these layers return: the concatenations, the Bottleneck's ``y + x``,
the SPP max pools, the nearest upsampling, ``space_to_depth`` and the head's bias-only prediction layers (widths 4, 1 and
``num_classes`` are outside the kernels).  AMP, depthwise blocks and training on the inference path's slice buffers are not taken."""
import torch
import torch.nn as nn

from .... import hip_lib
from ....gdrn_modeling import hip_layers


class ConvBnSilu(torch.autograd.Function):
    """[Conv2d k x k / stride / pad (k - 1) // 2, BatchNorm2d in training mode, SiLU] with its backward on HIP kernels.  x (N,Cin,H,W)
    channels_last -> y (N,Cout,OH,OW) channels_last.  The forward runs the fp32-MFMA convolution, the batch statistics (which
    update ``stats`` = (running_mean, running_var, num_batches_tracked) in place, as the module does) and the apply pass; saved are x,
    the convolution's output z, the batch mean and 1 / std and the parameters — y and the pre-activation are recomputed."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, stats, stride, eps, momentum):
        running_mean, running_var, num_batches_tracked = stats
        z = hip_lib.conv_train_f32(x, weight, bias, stride)
        mean, invstd = hip_lib.bn_train_stats(z, eps, running_mean, running_var, momentum)
        num_batches_tracked.add_(1)
        ctx.save_for_backward(x, z, mean, invstd, weight, gamma, beta)
        ctx.stride = stride
        return hip_lib.bn_silu_apply(z, mean, invstd, gamma, beta)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_y):
        x, z, mean, invstd, weight, gamma, beta = ctx.saved_tensors
        need = ctx.needs_input_grad
        dx = dw = db = dgamma = dbeta = None
        if any(need[:5]):
            dz, dgamma, dbeta = hip_lib.bn_silu_backward(hip_layers._cl(grad_y), z, mean, invstd, gamma, beta, want=(any(need[:3]), need[3], need[4]))
            if need[0] or need[1]:
                dx, dw = hip_lib.conv_backward(x, weight, ctx.stride, dz, want=need[:2])
            if need[2]:
                n, cout, oh, ow = dz.shape
                db = hip_lib.colsum_f32(dz.permute(0, 2, 3, 1).reshape(n * oh * ow, cout))[1]
        return dx, dw, db, dgamma, dbeta, None, None, None, None


def _param_ok(*params) -> bool:
    return all(p is not None and p.is_cuda and p.dtype == torch.float32 for p in params)


def _layer_ok(conv: nn.Module, bn: nn.Module, x: torch.Tensor) -> bool:
    """The layers and the shape ``ConvBnSilu`` takes, whatever the device: what the kernels of csrc/conv_bn_bwd.hip accept."""
    if not (isinstance(conv, nn.Conv2d) and isinstance(bn, nn.BatchNorm2d) and x.dim() == 4):
        return False
    if not (bn.training and bn.affine and bn.track_running_stats and isinstance(bn.momentum, float) and bn.running_mean is not None):
        return False
    k, s = conv.kernel_size[0], conv.stride[0]
    if not (conv.kernel_size in ((1, 1), (3, 3)) and conv.stride in ((1, 1), (2, 2)) and conv.padding == ((k - 1) // 2,) * 2
            and conv.dilation == (1, 1) and conv.groups == 1 and conv.padding_mode == "zeros"):
        return False
    n, cin, h, w = x.shape
    if not (cin == conv.in_channels and cin % 4 == 0 and conv.out_channels % 4 == 0 and conv.out_channels == bn.num_features <= 4096):
        return False
    if s == 2 and (h % 2 or w % 2):
        return False
    pad = (k - 1) // 2
    m = n * ((h + 2 * pad - k) // s + 1) * ((w + 2 * pad - k) // s + 1)      # values per channel: batch statistics need two
    return n > 0 and m >= 2 and n * h * w < (1 << 31) - 4096


def _on_device(conv: nn.Conv2d, bn: nn.BatchNorm2d) -> bool:
    return (_param_ok(conv.weight, bn.weight, bn.bias, bn.running_mean, bn.running_var) and (conv.bias is None or _param_ok(conv.bias))
            and bn.num_batches_tracked.is_cuda)


def conv_bn_silu(conv: nn.Module, bn: nn.Module, x: torch.Tensor):
    """``silu(bn(conv(x)))`` of a training-mode ``BaseConv`` as ``ConvBnSilu``, or None: the caller then runs the three modules.  Taken
    when the HIP layers and the training switch are on, gradients are enabled, there is no autocast, x is a 4-D fp32 device tensor,
    the BatchNorm is in training mode, affine, tracks running statistics with a float momentum, and the convolution is dense, 1x1 or
    3x3 at stride 1 or 2 with padding (k - 1) // 2, both widths multiples of 4, even sizes at stride 2 and at least two values per
    channel.  A layer refused while the switch is on is counted as a launch outside this library."""
    if not hip_layers._train_ok(x):
        return None
    if torch.is_autocast_enabled() or not (_layer_ok(conv, bn, x) and _on_device(conv, bn)):
        hip_layers.note_foreign_launch("conv_bn_silu: under autograd outside ConvBnSilu (AMP, eval-mode or non-affine BatchNorm, a kernel, "
                                       "stride, padding, groups, width or size outside csrc/conv_bn_bwd.hip)")
        return None
    stats = (bn.running_mean, bn.running_var, bn.num_batches_tracked)
    return ConvBnSilu.apply(hip_layers._cl(x), conv.weight, conv.bias, bn.weight, bn.bias, stats, conv.stride[0], bn.eps, bn.momentum)
