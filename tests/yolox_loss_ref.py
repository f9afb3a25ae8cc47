"""Restatement of the reference's YOLOX training losses (det/yolox/models/yolo_head.py: get_losses, get_assignments, get_in_boxes_info,
dynamic_k_matching, get_l1_target; det/yolox/models/losses.py: IOUloss) in plain torch, one image at a time with dense [num_gt, A]
matrices, in the dtype of its inputs: the tests run it in fp64.  Independent of the package's batch-wise torch path and of the kernels.

``assign_image`` also returns the margin of every selection it makes; tests/golden/make_golden_yolox_loss.py asserts them."""
import math

import torch
import torch.nn.functional as F

KEYS = ("loss_iou", "loss_conf", "loss_l1", "loss_cls")


def anchor_table(hw, strides, dtype=torch.float64):
    """[(h, w)] per level, strides -> [A,3] rows (x_shift, y_shift, stride), levels in order, each row-major."""
    rows = []
    for (h, w), s in zip(hw, strides):
        ys, xs = torch.meshgrid(torch.arange(h), torch.arange(w), indexing="ij")
        rows.append(torch.stack([xs.reshape(-1), ys.reshape(-1), torch.full((h * w,), s)], 1))
    return torch.cat(rows, 0).to(dtype)


def decode(raw, anchors):
    s = anchors[:, 2:3]
    return torch.cat([(raw[..., :2] + anchors[:, :2]) * s, torch.exp(raw[..., 2:4]) * s], -1)


def pair_iou(gt, box):
    """cxcywh [n,4] x [A,4] -> [n,A], the xyxy=False form of bboxes_iou."""
    tl = torch.max(gt[:, None, :2] - gt[:, None, 2:] / 2, box[:, :2] - box[:, 2:] / 2)
    br = torch.min(gt[:, None, :2] + gt[:, None, 2:] / 2, box[:, :2] + box[:, 2:] / 2)
    en = (tl < br).to(gt.dtype).prod(2)
    area_i = (br - tl).prod(2) * en
    return area_i / (gt[:, 2:].prod(1)[:, None] + box[:, 2:].prod(1) - area_i)


def scaled_gap(lo, hi):
    """Gap of two costs in units of 1 + 1e-3 |cost|: the penalised costs (1e5) carry an fp32 rounding of 8e-3."""
    return float((hi - lo) / (1 + 1e-3 * abs(hi)))


def assign_image(raw, anchors, gts):
    """raw [A,5+C], anchors [A,3], gts [n,5] (n >= 1) -> dict: matched_gt i64[A] (-1 background), matched_iou [A], cand bool[A],
    in_box / in_centre bool[n,A], iou / cost [n,A] (cost inf off the candidates), dynamic_k, chosen bool[n,A] before the conflicts are
    resolved, margins {name: smallest margin of that kind of decision}."""
    n, A, C = gts.shape[0], raw.shape[0], raw.shape[1] - 5
    xs, ys, s = anchors[:, 0], anchors[:, 1], anchors[:, 2]
    xc, yc = xs * s + 0.5 * s, ys * s + 0.5 * s
    g = gts[:, 1:5]
    box_d = torch.stack([xc - (g[:, 0:1] - 0.5 * g[:, 2:3]), yc - (g[:, 1:2] - 0.5 * g[:, 3:4]),
                         (g[:, 0:1] + 0.5 * g[:, 2:3]) - xc, (g[:, 1:2] + 0.5 * g[:, 3:4]) - yc], 2)
    r = 2.5 * s
    ctr_d = torch.stack([xc - (g[:, 0:1] - r), yc - (g[:, 1:2] - r), (g[:, 0:1] + r) - xc, (g[:, 1:2] + r) - yc], 2)
    in_box, in_ctr = box_d.min(2).values > 0, ctr_d.min(2).values > 0
    cand = (in_box | in_ctr).any(0)
    margins = {"geometry": float(torch.cat([box_d, ctr_d], 2).abs().min())}
    iou = pair_iou(g, decode(raw, anchors))
    p = (raw[:, 5:].sigmoid() * raw[:, 4:5].sigmoid()).sqrt()
    onehot = F.one_hot(gts[:, 0].long(), C).to(raw.dtype)
    bce = -(onehot[:, None, :] * torch.log(p).clamp_min(-100.0) + (1 - onehot[:, None, :]) * torch.log(1 - p).clamp_min(-100.0))
    cost = bce.sum(2) + 3.0 * (-torch.log(iou + 1e-8)) + 100000.0 * (~(in_box & in_ctr)).to(raw.dtype)
    cost = torch.where(cand[None], cost, torch.full_like(cost, math.inf))
    n_cand = int(cand.sum())
    chosen = torch.zeros((n, A), dtype=torch.bool)
    dynamic_k = []
    margins.update(iou10=math.inf, dynamic_k=math.inf, cost_k=math.inf, conflict=math.inf)
    for j in range(n):
        ious = iou[j][cand].sort(descending=True).values
        total = float(ious[:10].sum())
        if n_cand > 10 and ious[9] > 0:
            margins["iou10"] = min(margins["iou10"], float(ious[9] - ious[10]))
        k = max(1, int(total))
        margins["dynamic_k"] = min(margins["dynamic_k"], min(abs(total - m) for m in range(2, 12)))
        dynamic_k.append(k)
        order = cost[j].argsort(stable=True)
        k = min(k, n_cand)
        chosen[j, order[:k]] = True
        if n_cand > k:
            margins["cost_k"] = min(margins["cost_k"], scaled_gap(cost[j, order[k - 1]], cost[j, order[k]]))
    times = chosen.sum(0)
    matched = torch.where(times > 0, chosen.int().argmax(0), torch.full((A,), -1))
    unchosen_argmin = 0
    for a in torch.nonzero(times > 1).flatten().tolist():
        low = cost[:, a].sort(stable=True)
        margins["conflict"] = min(margins["conflict"], scaled_gap(low.values[0], low.values[1]))
        matched[a] = low.indices[0]
        unchosen_argmin += int(not chosen[low.indices[0], a])
    matched_iou = torch.where(matched >= 0, iou.gather(0, matched.clamp(min=0)[None])[0], torch.zeros_like(iou[0]))
    return dict(matched_gt=matched, matched_iou=matched_iou, cand=cand, in_box=in_box, in_centre=in_ctr, iou=iou, cost=cost,
                dynamic_k=dynamic_k, chosen=chosen, times=times, unchosen_argmin=unchosen_argmin, margins=margins)


def iou_loss(pred, target, loss_type):
    tl = torch.max(pred[:, :2] - pred[:, 2:] / 2, target[:, :2] - target[:, 2:] / 2)
    br = torch.min(pred[:, :2] + pred[:, 2:] / 2, target[:, :2] + target[:, 2:] / 2)
    area_p, area_g = pred[:, 2:].prod(1), target[:, 2:].prod(1)
    area_i = (br - tl).prod(1) * (tl < br).to(pred.dtype).prod(1)
    area_u = area_p + area_g - area_i
    iou = area_i / (area_u + 1e-16)
    if loss_type == "iou":
        return 1 - iou ** 2
    c_tl = torch.min(pred[:, :2] - pred[:, 2:] / 2, target[:, :2] - target[:, 2:] / 2)
    c_br = torch.max(pred[:, :2] + pred[:, 2:] / 2, target[:, :2] + target[:, 2:] / 2)
    area_c = (c_br - c_tl).prod(1)
    return 1 - (iou - (area_c - area_u) / area_c.clamp(1e-16)).clamp(min=-1.0, max=1.0)


def focal(x, t, alpha, gamma):
    p = torch.sigmoid(x)
    ce = F.binary_cross_entropy_with_logits(x, t, reduction="none")
    loss = ce * (1 - (p * t + (1 - p) * (1 - t))) ** gamma
    return (alpha * t + (1 - alpha) * (1 - t)) * loss if alpha >= 0 else loss


def losses(raw, anchors, labels, iou_loss_type="iou", cls_loss_type="bce", fl_alpha=0.25, fl_gamma=2.0, use_l1=False, assignment=None):
    """raw [B,A,5+C] (may require grad), anchors [A,3], labels [B,G,5] -> (loss dict, info: matched_gt i64[B,A], matched_iou [B,A],
    num_fg [B], num_gt [B], per_image: the ``assign_image`` dicts or None).  ``assignment`` = (matched_gt, matched_iou) replaces the
    restatement's own (the losses of a given assignment)."""
    B, A, S = raw.shape
    C = S - 5
    num_gt = (labels.sum(2) > 0).sum(1).tolist()
    per_image, mg, mi = [], [], []
    with torch.no_grad():
        for b in range(B):
            res = assign_image(raw[b].detach(), anchors, labels[b, :num_gt[b]]) if num_gt[b] else None
            per_image.append(res)
            mg.append(res["matched_gt"] if res else torch.full((A,), -1))
            mi.append(res["matched_iou"] if res else raw.new_zeros(A))
    matched_gt, matched_iou = (torch.stack(mg), torch.stack(mi)) if assignment is None else assignment
    fg = matched_gt >= 0
    num_fg = max(int(fg.sum()), 1)
    box = decode(raw, anchors)
    s = anchors[:, 2]
    total = dict.fromkeys(KEYS, raw.new_zeros(()))
    total["loss_conf"] = F.binary_cross_entropy_with_logits(raw[..., 4], fg.to(raw.dtype), reduction="sum")
    for b in range(B):
        idx = torch.nonzero(fg[b]).flatten()
        if idx.numel() == 0:
            continue
        gt = labels[b, matched_gt[b, idx].long()]
        total["loss_iou"] = total["loss_iou"] + iou_loss(box[b, idx], gt[:, 1:5], iou_loss_type).sum()
        target = F.one_hot(gt[:, 0].long(), C).to(raw.dtype) * matched_iou[b, idx, None]
        x = raw[b, idx, 5:]
        per = F.binary_cross_entropy_with_logits(x, target, reduction="none") if cls_loss_type == "bce" else focal(x, target, fl_alpha, fl_gamma)
        total["loss_cls"] = total["loss_cls"] + per.sum()
        if use_l1:
            st = s[idx]
            l1t = torch.stack([gt[:, 1] / st - anchors[idx, 0], gt[:, 2] / st - anchors[idx, 1], torch.log(gt[:, 3] / st + 1e-8),
                               torch.log(gt[:, 4] / st + 1e-8)], 1)
            total["loss_l1"] = total["loss_l1"] + (raw[b, idx, :4] - l1t).abs().sum()
    out = {k: v / num_fg for k, v in total.items()}
    out["loss_iou"] = 5.0 * out["loss_iou"]
    info = dict(matched_gt=matched_gt, matched_iou=matched_iou, num_fg=fg.sum(1), num_gt=torch.tensor(num_gt), per_image=per_image)
    return out, info
