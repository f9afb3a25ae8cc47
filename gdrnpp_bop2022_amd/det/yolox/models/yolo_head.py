"""Decoupled YOLOX head, inference only: per level a 1x1 stem, two 3x3 BaseConvs on each of the class and the box branch, and
the 1x1 prediction layers (classes | box | objectness).  The output row of an anchor is (cx, cy, w, h, obj, class scores), the
levels' anchors concatenated in level order, each level row-major."""
import math

import torch
import torch.nn as nn

from .network_blocks import BaseConv, _no_depthwise


class YOLOXHead(nn.Module):
    def __init__(self, num_classes, width=1.0, strides=(8, 16, 32), in_channels=(256, 512, 1024), act="silu", depthwise=False, **_unused):
        super().__init__()
        _no_depthwise(depthwise)
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
        if labels is not None or self.training:
            raise NotImplementedError("training mode (labels / self.training: the SimOTA assignment and losses) is not implemented")
        outs = []
        for k, x in enumerate(xin):
            x = self.stems[k](x)
            cls_feat, reg_feat = self.cls_convs[k](x), self.reg_convs[k](x)
            outs.append(torch.cat([self.reg_preds[k](reg_feat), self.obj_preds[k](reg_feat).sigmoid(),
                                   self.cls_preds[k](cls_feat).sigmoid()], 1))
        self.hw = [tuple(o.shape[-2:]) for o in outs]
        out = torch.cat([o.flatten(start_dim=2) for o in outs], 2).permute(0, 2, 1)
        if not self.decode_in_inference:
            return out
        return {"det_preds": self.decode_outputs(out, out.dtype)}

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
