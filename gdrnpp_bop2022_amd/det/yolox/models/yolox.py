"""The YOLOX detector: PAFPN over CSPDarknet, decoupled head.

``forward(x)`` on an eval-mode model returns ``{"det_preds": f32[B, A, 5 + num_classes]}`` — the tensor
``det.yolox.utils.boxes.postprocess`` takes.  On the GPU with the HIP layers enabled the whole forward runs on
csrc/yolox_net.hip (``hip_forward``); everywhere else it is the plain-PyTorch module path.

``forward(x, targets)`` on a train-mode model returns the reference's ``(out_dict, loss_dict)`` with ``loss_iou``, ``loss_conf``,
``loss_l1`` and ``loss_cls``; ``targets`` f32[B,G,5] = (class, cx, cy, w, h) in pixels of ``x``, zero rows behind an image's gts.  The
SimOTA assignment and the losses run on csrc/yolox_loss.hip (``losses.yolox_losses``).  With ``hip_layers.set_train_kernels(True)`` every
``BaseConv`` under the loss (convolution, BatchNorm with batch statistics, SiLU) runs forward and backward on csrc/conv_bn_bwd.hip
(``train_layers.ConvBnSilu``): bit-reproducible, every sum in a fixed order.  The concatenations, the Bottleneck's ``y + x``, the SPP
max pools, the nearest upsampling, ``space_to_depth`` and the head's bias-only prediction layers (widths 4, 1 and ``num_classes``)
stay on PyTorch's operators, on channels_last tensors.  With the switch off, the default, the whole graph is PyTorch's."""
import torch.nn as nn

from ....gdrn_modeling import hip_layers
from . import hip_forward
from .yolo_head import YOLOXHead
from .yolo_pafpn import YOLOPAFPN


class YOLOX(nn.Module):
    def __init__(self, backbone=None, head=None):
        super().__init__()
        self.backbone = YOLOPAFPN() if backbone is None else backbone
        self.head = YOLOXHead(80) if head is None else head
        self.init_yolo()

    def init_yolo(self):
        for m in self.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.eps = 1e-3
                m.momentum = 0.03
        self.head.initialize_biases(prior_prob=0.01)

    def forward(self, x, targets=None, augment=False, cfg=None):
        if augment:
            raise NotImplementedError("augment=True (multi-scale test: needs scale_img's interpolation) is not implemented")
        if self.training and targets is None:
            raise NotImplementedError("training mode needs targets: model(x, targets) returns (out_dict, loss_dict)")
        if targets is not None and not self.training:
            raise NotImplementedError("targets are only taken in training mode (model.train()); eval mode returns det_preds")
        if self.training:
            return self.head(self.backbone(x), targets, x)
        if hip_layers.enabled_for(x) and hip_forward.supported(self, x):
            return hip_forward.forward(self, x)
        hip_layers.foreign("YOLOX: forward outside the HIP path (PyTorch operators)", x)
        return self.head(self.backbone(x))


def build_yolox(depth: float = 1.33, width: float = 1.25, num_classes: int = 21, act: str = "silu") -> YOLOX:
    """YOLOX of the given size (s: 0.33 / 0.50, m: 0.67 / 0.75, l: 1.0 / 1.0, x: 1.33 / 1.25) in eval mode."""
    in_channels = [256, 512, 1024]
    model = YOLOX(YOLOPAFPN(depth, width, in_channels=in_channels, act=act), YOLOXHead(num_classes, width, in_channels=in_channels, act=act))
    return model.eval()
