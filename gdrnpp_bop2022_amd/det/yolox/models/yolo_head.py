"""Decoupled YOLOX head: per level a 1x1 stem, two 3x3 BaseConvs on each of the class and the box branch, and the 1x1 prediction
layers (classes | box | objectness).  The output row of an anchor is (cx, cy, w, h, obj, class scores), the levels' anchors
concatenated in level order, each level row-major.

Training mode: ``forward(xin, labels, imgs)`` returns the reference's ``(out_dict, loss_dict)``: the same rows undecoded and with
logits go to ``losses.yolox_losses`` (SimOTA assignment and the four losses; HIP kernels on fp32 device tensors).  The layers under
the loss, convolutions and BatchNorm with batch statistics, stay on PyTorch's graph in training mode."""
import math

import torch
import torch.nn as nn

from . import losses
from .network_blocks import BaseConv, _no_depthwise


class YOLOXHead(nn.Module):
    def __init__(self, num_classes, width=1.0, strides=(8, 16, 32), in_channels=(256, 512, 1024), act="silu", depthwise=False,
                 iou_loss_type="iou", cls_loss_type="bce", obj_loss_type="bce", fl_alpha=0.25, fl_gamma=2.0, **_unused):
        super().__init__()
        _no_depthwise(depthwise)
        self.use_l1 = False
        self.iou_loss_type, self.cls_loss_type, self.obj_loss_type = iou_loss_type, cls_loss_type, obj_loss_type
        self.fl_alpha, self.fl_gamma = fl_alpha, fl_gamma
        self.n_anchors = 1
        self.num_classes = num_classes
        self.decode_in_inference = True
        self.strides = list(strides)
        c = int(256 * width)
        self.cls_convs, self.reg_convs = nn.ModuleList(), nn.ModuleList()
        self.cls_preds, self.reg_preds, self.obj_preds = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        self.stems = nn.ModuleList()
        for cin in in_channels:
            self.stems.append(BaseConv(int(cin * width), c, 1, 1, act=act))
            self.cls_convs.append(nn.Sequential(BaseConv(c, c, 3, 1, act=act), BaseConv(c, c, 3, 1, act=act)))
            self.reg_convs.append(nn.Sequential(BaseConv(c, c, 3, 1, act=act), BaseConv(c, c, 3, 1, act=act)))
            self.cls_preds.append(nn.Conv2d(c, self.n_anchors * num_classes, 1, 1, 0))
            self.reg_preds.append(nn.Conv2d(c, 4, 1, 1, 0))
            self.obj_preds.append(nn.Conv2d(c, self.n_anchors, 1, 1, 0))
        self.hw = []

    def initialize_biases(self, prior_prob):
        """Class and objectness biases such that every initial score is ``prior_prob``."""
        b = -math.log((1 - prior_prob) / prior_prob)
        for conv in list(self.cls_preds) + list(self.obj_preds):
            with torch.no_grad():
                conv.bias.fill_(b)

    def forward(self, xin, labels=None, imgs=None):
        if self.training and labels is None:
            raise NotImplementedError("training mode needs labels: forward(xin, labels, imgs) returns (out_dict, loss_dict)")
        if labels is not None and not self.training:
            raise NotImplementedError("labels are only taken in training mode (model.train()); eval mode returns det_preds")
        outs = []
        for k, x in enumerate(xin):
            x = self.stems[k](x)
            cls_feat, reg_feat = self.cls_convs[k](x), self.reg_convs[k](x)
            obj, cls = self.obj_preds[k](reg_feat), self.cls_preds[k](cls_feat)
            outs.append(torch.cat([self.reg_preds[k](reg_feat), obj, cls] if self.training else
                                  [self.reg_preds[k](reg_feat), obj.sigmoid(), cls.sigmoid()], 1))
        self.hw = [tuple(o.shape[-2:]) for o in outs]
        out = torch.cat([o.flatten(start_dim=2) for o in outs], 2).permute(0, 2, 1)
        if self.training:
            return self.get_losses(out, labels)
        if not self.decode_in_inference:
            return out
        return {"det_preds": self.decode_outputs(out, out.dtype)}

    def get_losses(self, raw, labels):
        """raw [B,A,5+C]: the undecoded rows with logits of the last forward; labels [B,G,5] = (class, cx, cy, w, h) -> (out_dict,
        loss_dict) of the reference's ``get_losses``; ``out_dict["num_fg"]`` = max(num_fg, 1) / max(num_gts, 1) as a 0-d tensor."""
        grids, strides = self.grids_and_strides(raw.dtype, raw.device)
        anchors = torch.cat([grids[0], strides[0]], 1)
        labels = labels.to(device=raw.device, dtype=torch.float64 if raw.dtype == torch.float64 else torch.float32)     # never fp16 pixels
        loss_dict, info = losses.yolox_losses(raw, anchors, labels, iou_loss_type=self.iou_loss_type,
                                              cls_loss_type=self.cls_loss_type, obj_loss_type=self.obj_loss_type, fl_alpha=self.fl_alpha,
                                              fl_gamma=self.fl_gamma, use_l1=self.use_l1)
        return {"num_fg": info["num_fg_ratio"]}, loss_dict

    def grids_and_strides(self, dtype, device=None):
        """([1,A,2] anchor cell (x, y), [1,A,1] stride) of the levels of the last forward."""
        grids, strides = [], []
        for (h, w), s in zip(self.hw, self.strides):
            yv, xv = torch.meshgrid([torch.arange(h), torch.arange(w)], indexing="ij")
            grids.append(torch.stack((xv, yv), 2).view(1, -1, 2))
            strides.append(torch.full((1, h * w, 1), s))
        return torch.cat(grids, 1).to(device=device, dtype=dtype), torch.cat(strides, 1).to(device=device, dtype=dtype)

    def decode_outputs(self, outputs, dtype):
        grids, strides = self.grids_and_strides(dtype, outputs.device)
        outputs = outputs.contiguous()
        outputs[..., :2] = (outputs[..., :2] + grids) * strides
        outputs[..., 2:4] = torch.exp(outputs[..., 2:4]) * strides
        return outputs
