"""YOLOX's training losses: ``IOUloss`` and ``yolox_losses`` = SimOTA label assignment + the four detection losses of the reference's
``YOLOXHead.get_losses``, for the whole batch at once.

On fp32 device tensors with the HIP layers enabled, ``yolox_losses`` is one ``autograd.Function`` over csrc/yolox_loss.hip
(``hip_lib.yolox_assign``, ``yolox_losses``, ``yolox_losses_backward``): nothing is read back to the host.  CPU tensors, disabled HIP
layers and other dtypes (AMP's fp16 among them) take the torch-operator path below, which has the same arithmetic written batch-wise;
on a GPU that path is counted through ``hip_layers.foreign``.

Differences from the reference, in both paths: a gt without any candidate anchor gets no foreground (the reference's ``topk`` raises), a
class outside [0, C) has no positive class term (the reference's ``one_hot`` raises), ``loss_l1`` without ``use_l1`` is a zero tensor
(the reference: the float 0.0), and ``num_fg`` stays a device tensor."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .... import hip_lib
from ....gdrn_modeling import hip_layers

LOSS_KEYS = hip_lib.YOLOX_LOSS_KEYS
REG_WEIGHT = 5.0
CENTER_RADIUS = 2.5
N_CANDIDATE_K = 10


def _corners(box):
    half = box[..., 2:4] / 2
    return box[..., :2] - half, box[..., :2] + half


def iou_loss(pred, target, loss_type: str = "iou"):
    """The per-box loss of ``IOUloss`` for cxcywh boxes [..., 4]: "iou" = 1 - iou^2, "giou" = 1 - clamp(giou, -1, 1)."""
    if loss_type not in ("iou", "giou"):
        raise NotImplementedError(f"IOUloss: unknown loss_type {loss_type!r} (iou | giou)")
    p_tl, p_br = _corners(pred)
    t_tl, t_br = _corners(target)
    tl, br = torch.max(p_tl, t_tl), torch.min(p_br, t_br)
    overlap = (tl < br).to(pred.dtype).prod(-1)
    area_i = (br - tl).prod(-1) * overlap
    area_u = pred[..., 2:4].prod(-1) + target[..., 2:4].prod(-1) - area_i
    iou = area_i / (area_u + 1e-16)
    if loss_type == "iou":
        return 1 - iou ** 2
    area_c = (torch.max(p_br, t_br) - torch.min(p_tl, t_tl)).prod(-1)
    giou = iou - (area_c - area_u) / area_c.clamp(1e-16)
    return 1 - giou.clamp(min=-1.0, max=1.0)


class IOUloss(nn.Module):
    """``IOUloss(reduction="none" | "mean" | "sum", loss_type="iou" | "giou")`` over cxcywh boxes [N, 4]."""

    def __init__(self, reduction="none", loss_type="iou"):
        super().__init__()
        self.reduction = reduction
        self.loss_type = loss_type

    def forward(self, pred, target):
        assert pred.shape[0] == target.shape[0]
        loss = iou_loss(pred.view(-1, 4), target.view(-1, 4), self.loss_type)
        if self.reduction == "mean":
            return loss.mean()
        if self.reduction == "sum":
            return loss.sum()
        return loss


def sigmoid_focal_loss(logits, targets, alpha: float = 0.25, gamma: float = 2.0):
    """fvcore's ``sigmoid_focal_loss(..., reduction="none")``: alpha_t (1 - p_t)^gamma BCEWithLogits; alpha < 0 = no alpha_t."""
    p = torch.sigmoid(logits)
    ce = F.binary_cross_entropy_with_logits(logits, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce * (1 - p_t) ** gamma
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss


def decode_boxes(raw, anchors):
    """raw [B,A,>=4], anchors [A,3] -> cxcywh [B,A,4]: xy = (raw + shift) stride, wh = exp(raw) stride."""
    stride = anchors[:, 2:3]
    return torch.cat([(raw[..., :2] + anchors[:, :2]) * stride, torch.exp(raw[..., 2:4]) * stride], -1)


@torch.no_grad()
def simota_assign_torch(raw, anchors, labels):
    """SimOTA for the whole batch in torch operators, one [B,G,A] IoU and cost tensor, no [G,A,C] tensor and no per-image loop.
    Exact ties go to the lowest index, as in csrc/yolox_loss.hip: equal costs of one gt to the lowest anchor (a stable sort;
    ``topk`` promises no order among equal values), equal costs of one anchor to the lowest label row (``argmin`` returns the first).
    -> (matched_gt i32[B,A] with -1 = background, matched_iou [B,A], num_fg i32[B], num_gt i32[B])."""
    B, A, S = raw.shape
    C, G = S - 5, labels.shape[1]
    dev = raw.device
    num_gt = (labels.sum(2) > 0).sum(1)
    if G == 0:
        return (torch.full((B, A), -1, dtype=torch.int32, device=dev), raw.new_zeros((B, A)), torch.zeros(B, dtype=torch.int32, device=dev),
                num_gt.to(torch.int32))
    valid = (torch.arange(G, device=dev)[None] < num_gt[:, None])[:, :, None]                    # [B,G,1]
    box = decode_boxes(raw, anchors)
    gt = labels[..., 1:5][:, :, None, :]                                                         # [B,G,1,4]
    stride = anchors[:, 2]
    centre = torch.stack([anchors[:, 0] * stride + 0.5 * stride, anchors[:, 1] * stride + 0.5 * stride], -1)      # [A,2]

    def inside(lo, hi):
        return torch.minimum((centre - lo).amin(-1), (hi - centre).amin(-1)) > 0.0

    in_box = inside(gt[..., :2] - 0.5 * gt[..., 2:4], gt[..., :2] + 0.5 * gt[..., 2:4]) & valid
    radius = (CENTER_RADIUS * stride)[:, None]
    in_centre = inside(gt[..., :2] - radius, gt[..., :2] + radius) & valid
    use = (in_box | in_centre).any(1, keepdim=True) & valid                                      # [B,G,A]: candidate anchor, real gt

    g_tl, g_br = _corners(gt)
    p_tl, p_br = _corners(box[:, None])
    tl, br = torch.max(g_tl, p_tl), torch.min(g_br, p_br)
    area_i = (br - tl).prod(-1) * (tl < br).to(raw.dtype).prod(-1)
    iou = area_i / (gt[..., 2:4].prod(-1) + box[:, None, :, 2:4].prod(-1) - area_i)              # [B,G,A]

    p = (raw[..., 5:].sigmoid() * raw[..., 4:5].sigmoid()).sqrt()
    neg = -torch.log(1 - p).clamp_min(-100.0)
    pos_minus_neg = -torch.log(p).clamp_min(-100.0) - neg                                         # [B,A,C]
    cls = labels[..., 0].long()
    in_range = ((cls >= 0) & (cls < C))[:, :, None]
    at_cls = pos_minus_neg.gather(2, cls.clamp(0, C - 1)[:, None, :].expand(B, A, G)).permute(0, 2, 1)
    cost_cls = neg.sum(-1)[:, None, :] + torch.where(in_range, at_cls, torch.zeros_like(at_cls))
    cost = cost_cls + 3.0 * (-torch.log(iou + 1e-8)) + 100000.0 * (~(in_box & in_centre)).to(raw.dtype)

    k = min(N_CANDIDATE_K, A)
    top_iou = torch.where(use, iou, torch.zeros_like(iou)).topk(k, dim=2).values.sum(2)           # zeros pad an image with < 10 candidates
    dynamic_k = top_iou.int().clamp(min=1)
    cost = torch.where(use, cost, torch.full_like(cost, float("inf")))
    low_idx = cost.argsort(dim=2, stable=True)[..., :k]                                           # equal costs: the lowest anchor first
    low = cost.gather(2, low_idx)
    chosen = (torch.arange(k, device=dev) < dynamic_k[..., None]) & torch.isfinite(low)
    matching = torch.zeros((B, G, A), dtype=torch.bool, device=dev).scatter_(2, low_idx, chosen)
    n_chosen = matching.sum(1)
    matched = torch.where(n_chosen > 1, cost.argmin(1), matching.int().argmax(1))                 # argmin over ALL gts of the image
    fg = n_chosen > 0
    matched_iou = iou.gather(1, matched[:, None, :]).squeeze(1) * fg
    matched = torch.where(fg, matched, torch.full_like(matched, -1))
    return matched.to(torch.int32), matched_iou, fg.sum(1).to(torch.int32), num_gt.to(torch.int32)


def yolox_losses_torch(raw, anchors, labels, *, iou_loss_type="iou", cls_loss_type="bce", fl_alpha=0.25, fl_gamma=2.0, use_l1=False):
    """The torch-operator path of ``yolox_losses``; computes in fp64 for fp64 inputs, in fp32 for everything else."""
    dtype = torch.float64 if raw.dtype == torch.float64 else torch.float32
    raw, anchors, labels = raw.to(dtype), anchors.to(dtype), labels.to(dtype)
    matched_gt, matched_iou, num_fg, num_gt = simota_assign_torch(raw.detach(), anchors, labels)
    B, A, S = raw.shape
    C = S - 5
    fg = matched_gt >= 0
    den = num_fg.sum().clamp(min=1).to(dtype)
    row = matched_gt.clamp(min=0).long()
    if labels.shape[1] == 0:
        labels = labels.new_zeros((B, 1, 5))
    matched = labels.gather(1, row[..., None].expand(B, A, 5))                                   # [B,A,5]; row 0 on background, masked below
    zero = raw.new_zeros(())
    loss_iou = torch.where(fg, iou_loss(decode_boxes(raw, anchors), matched[..., 1:5], iou_loss_type), zero).sum() / den
    loss_conf = F.binary_cross_entropy_with_logits(raw[..., 4], fg.to(dtype), reduction="sum") / den
    cls_target = F.one_hot(matched[..., 0].long().clamp(0, C), C + 1)[..., :C].to(dtype) * matched_iou[..., None]
    cls_in_range = ((matched[..., 0].long() >= 0) & (matched[..., 0].long() < C))[..., None]
    cls_target = torch.where(cls_in_range, cls_target, torch.zeros_like(cls_target))
    if cls_loss_type == "bce":
        per_class = F.binary_cross_entropy_with_logits(raw[..., 5:], cls_target, reduction="none")
    elif cls_loss_type == "focal":
        per_class = sigmoid_focal_loss(raw[..., 5:], cls_target, fl_alpha, fl_gamma)
    else:
        raise NotImplementedError(f"Unknown cls_loss_type: {cls_loss_type}")
    loss_cls = torch.where(fg[..., None], per_class, zero).sum() / den
    if use_l1:
        stride = anchors[:, 2:3]
        l1_target = torch.cat([matched[..., 1:3] / stride - anchors[:, :2], torch.log(matched[..., 3:5] / stride + 1e-8)], -1)
        loss_l1 = torch.where(fg[..., None], (raw[..., :4] - l1_target).abs(), zero).sum() / den
    else:
        loss_l1 = raw.new_zeros(())
    losses = {"loss_iou": REG_WEIGHT * loss_iou, "loss_conf": loss_conf, "loss_l1": loss_l1, "loss_cls": loss_cls}
    info = {"matched_gt": matched_gt, "matched_iou": matched_iou, "num_fg": num_fg, "num_gt": num_gt,
            "num_fg_ratio": den / num_gt.sum().clamp(min=1).to(dtype)}
    return losses, info


class YoloxLosses(torch.autograd.Function):
    """forward(raw, anchors, labels, opts) -> (losses f32[4] in the order of ``LOSS_KEYS``, out f64[6], matched_gt, matched_iou, num_fg,
    num_gt) on csrc/yolox_loss.hip.  Only ``losses`` carries a gradient, and only to ``raw``: the backward kernel recomputes from the saved
    inputs with the assignment, its IoUs and num_fg as constants."""

    @staticmethod
    def forward(ctx, raw, anchors, labels, opts):
        raw = raw.detach().contiguous()
        matched_gt, matched_iou, num_fg, num_gt = hip_lib.yolox_assign(raw, anchors, labels)
        out = hip_lib.yolox_losses(raw, anchors, labels, matched_gt, num_fg, num_gt, **opts)
        ctx.save_for_backward(raw, anchors, labels, matched_gt, out)
        ctx.opts = opts
        ctx.mark_non_differentiable(out, matched_gt, matched_iou, num_fg, num_gt)
        return out[:4].float(), out, matched_gt, matched_iou, num_fg, num_gt

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad_losses, *_unused):
        raw, anchors, labels, matched_gt, out = ctx.saved_tensors
        grad = hip_lib.yolox_losses_backward(raw, anchors, labels, matched_gt, out, grad_losses.float().contiguous(), **ctx.opts)
        return grad, None, None, None


def kernel_path(raw, anchors, labels) -> bool:
    """Whether ``yolox_losses`` takes the HIP kernels: layers enabled, fp32 device tensors."""
    return hip_layers.is_enabled() and all(t.is_cuda and t.dtype == torch.float32 for t in (raw, anchors, labels))


def yolox_losses(raw, anchors, labels, *, iou_loss_type="iou", cls_loss_type="bce", obj_loss_type="bce", fl_alpha=0.25, fl_gamma=2.0,
                 use_l1=False):
    """SimOTA assignment + detection losses of a batch.  raw [B,A,5+C]: the head's undecoded rows (reg 4, objectness logit, class
    logits; levels in level order, each row-major), anchors [A,3] = (x_shift, y_shift, stride), labels [B,G,5] = (class, cx, cy, w, h)
    with zero rows behind the gts of an image.  -> (loss_dict with the reference's keys loss_iou (times 5), loss_conf, loss_l1,
    loss_cls, all divided by max(num_fg, 1); info: matched_gt i32[B,A] (-1 = background), matched_iou [B,A], num_fg i32[B], num_gt
    i32[B], num_fg_ratio = max(num_fg, 1) / max(num_gts, 1))."""
    if obj_loss_type != "bce":
        raise NotImplementedError(f"Unknown obj_loss_type: {obj_loss_type}")
    if iou_loss_type not in hip_lib.YOLOX_IOU_LOSSES:
        raise NotImplementedError(f"Unknown iou_loss_type: {iou_loss_type}")
    if cls_loss_type not in hip_lib.YOLOX_CLS_LOSSES:
        raise NotImplementedError(f"Unknown cls_loss_type: {cls_loss_type}")
    opts = dict(iou_loss_type=iou_loss_type, cls_loss_type=cls_loss_type, fl_alpha=float(fl_alpha), fl_gamma=float(fl_gamma), use_l1=bool(use_l1))
    if kernel_path(raw, anchors, labels):
        if labels.shape[1] == 0:        # no label rows at all: one empty row, the kernels take no null pointer
            labels = labels.new_zeros((labels.shape[0], 1, 5))
        losses, out, matched_gt, matched_iou, num_fg, num_gt = YoloxLosses.apply(raw, anchors.contiguous(), labels.contiguous(), opts)
        info = {"matched_gt": matched_gt, "matched_iou": matched_iou, "num_fg": num_fg, "num_gt": num_gt,
                "num_fg_ratio": (out[4] / out[5].clamp(min=1.0)).float()}
        return dict(zip(LOSS_KEYS, losses.unbind(0))), info
    if raw.is_cuda:
        with torch.no_grad():       # the counter takes fp32 tensors outside autograd: an empty one stands for this launch
            hip_layers.foreign("yolox_losses: SimOTA and losses outside the HIP path (PyTorch operators)", raw.detach()[:0].float())
    return yolox_losses_torch(raw, anchors, labels, **opts)
