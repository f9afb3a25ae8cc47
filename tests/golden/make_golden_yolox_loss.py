"""Golden vectors of YOLOX's training losses from the reference's own ``YOLOXHead.get_losses`` (authoring container only: needs the
reference checkout that tests/golden/_refimport.py imports from).

What runs here is the reference's det/yolox/models/yolo_head.py (get_losses, get_assignments, get_in_boxes_info, dynamic_k_matching,
get_l1_target) and det/yolox/models/losses.py (IOUloss), imported from their files, in fp32 on the CPU; ``bboxes_iou`` is loaded from
the reference's det/yolox/utils/boxes.py (torchvision / cv2 are inert stand-ins, nothing of them runs).  fvcore is not installed: its
``sigmoid_focal_loss`` is served by the few lines below (the published formula).  The head is given constructed rows instead of a
network's: the decode ``get_output_and_grid`` applies is applied here with the same torch operators, on an autograd leaf, so that
the gradient of the summed losses by the RAW rows can be recorded.

Inputs are constructed, and searched over seeds, so that every selection has a margin on the fp64 restatement
(tests/yolox_loss_ref.py) — log / exp / sqrt differ in their last bits between host and device, and the tests demand EXACT equality of
the assignment.  Asserted per case, stored as ``margin_<kind>`` and ``margin_min``:
  geometry    every in-box and in-centre delta against 0 (pixels)
  iou10       10th against 11th IoU of every gt with a 10th IoU above 0 (a 10th IoU of exactly 0 is 0 in every precision:
              the pair does not overlap, and the sum does not depend on which zero is taken)
  dynamic_k   sum of the top-10 IoUs against the integers 2 .. 11 (below 2 the clamp makes dynamic_k 1 either way)
  cost_k      k-th against (k+1)-th cost of every gt, in units of 1 + 1e-3 |cost| (penalised costs of 1e5 round to 8e-3 in fp32)
  conflict    the two lowest costs over all gts of every multiply-chosen anchor, same units
The dense case (448 x 448, A = 4116: 16 - 17 anchors per lane of the assignment kernel's 256) takes its images from
tests/yolox_loss_edge_cases.py::dense_image: large gts with good predictions scattered over the whole box.  Asserted of its crowded
image, as ``lane_facts`` counts them: >= 128 lanes (anchor % 256) hold more than 10 candidates, >= 5 chosen anchors and >= 5 of the
anchors that form some gt's 10 largest IoUs are the 11th or a later candidate of their lane's walk.
``e_cost`` is the largest distance, in the same units, of the fp32 restatement's candidate costs from fp64: MARGIN is 1e-3, and
asserted to exceed 16 e_cost.

Per case yolox_loss_golden_<case>.npz: hw, strides, options; raw f32[B,A,5+C], labels f32[B,G,5]; the reference's fg_mask, matched_gt
(matched_gt_inds scattered to [B,A], -1 = background), matched_iou (pred_ious_this_matching, likewise), num_fg per image, num_gt, the
four losses, num_fg_ratio and grad = d (sum of the losses) / d raw; e_ref_<loss>, e_ref_grad, e_ref_iou = the distance of those fp32
results from the fp64 restatement: the unit of the GPU tests' bars.
"""
import importlib.util
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.dirname(HERE))

import _refimport  # noqa: E402

_refimport.install()


def sigmoid_focal_loss(inputs, targets, alpha=0.25, gamma=2.0, reduction="none"):
    """fvcore.nn.focal_loss.sigmoid_focal_loss as published (RetinaNet's focal loss on logits)."""
    p = torch.sigmoid(inputs)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(inputs, targets, reduction="none")
    p_t = p * targets + (1 - p) * (1 - targets)
    loss = ce * ((1 - p_t) ** gamma)
    if alpha >= 0:
        loss = (alpha * targets + (1 - alpha) * (1 - targets)) * loss
    return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss


import fvcore.nn.focal_loss as _ffl  # noqa: E402  (the stand-in module)

_ffl.sigmoid_focal_loss = sigmoid_focal_loss
_spec = importlib.util.spec_from_file_location("_ref_yolox_boxes", os.path.join(_refimport.REF, "det/yolox/utils/boxes.py"))
_boxes = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_boxes)
for name in ("det.yolox.utils", "det.yolox.utils.model_utils"):
    sys.modules[name] = _refimport._StubModule(name)
    sys.modules[name].__path__ = []
sys.modules["det.yolox.utils"].bboxes_iou = _boxes.bboxes_iou

import yolox_loss_edge_cases as E  # noqa: E402
import yolox_loss_ref as R  # noqa: E402
from det.yolox.models.yolo_head import YOLOXHead  # noqa: E402

MARGIN = 1e-3
STRIDES = (8, 16, 32)
# name: image (H, W), classes, images, label rows, the head's options
CASES = {
    "a_iou_bce": dict(size=(64, 96), C=3, layout="a", G=7, opts=dict(iou_loss_type="iou", cls_loss_type="bce", use_l1=False)),
    "a_giou_focal_l1": dict(size=(64, 96), C=3, layout="a", G=7, opts=dict(iou_loss_type="giou", cls_loss_type="focal", use_l1=True)),
    "b_iou_bce_l1": dict(size=(160, 160), C=3, layout="b", G=8, opts=dict(iou_loss_type="iou", cls_loss_type="bce", use_l1=True)),
    "b21_giou_focal": dict(size=(160, 160), C=21, layout="b", G=8, opts=dict(iou_loss_type="giou", cls_loss_type="focal", use_l1=False)),
    "dense_giou_focal_l1": dict(size=(E.DENSE_SIZE, E.DENSE_SIZE), C=E.DENSE_C, layout="dense", G=E.DENSE_G,
                                opts=dict(iou_loss_type="giou", cls_loss_type="focal", use_l1=True)),
}
FL_ALPHA, FL_GAMMA = 0.25, 2.0


def off_lattice(v):
    """Two decimals, never within 0.1 px of the anchor centres (multiples of 4 px)."""
    return np.round(v) + 0.37


def build_inputs(case, seed):
    c = CASES[case]
    H, W = c["size"]
    C, G = c["C"], c["G"]
    hw = [(H // s, W // s) for s in STRIDES]
    anchors = R.anchor_table(hw, STRIDES, torch.float32)
    A = anchors.shape[0]
    if c["layout"] == "dense":                               # no gt, one gt, a crowd of seven with the twin pair
        raw, labels = E.dense_batch(seed)
        return hw, anchors, torch.from_numpy(raw.copy()), torch.from_numpy(labels.copy())
    rng = np.random.default_rng(seed)

    def rand_gt(scale_lo=0.2, scale_hi=0.5):
        w, h = rng.uniform(scale_lo, scale_hi, 2) * (W, H)
        return [rng.integers(0, C), off_lattice(rng.uniform(0.25, 0.75) * W), off_lattice(rng.uniform(0.25, 0.75) * H), off_lattice(w), off_lattice(h)]

    crowd = [rand_gt() for _ in range(5)]
    twin = list(crowd[0])                                    # heavily overlapping pair: the same box moved by 2 - 3 px, another class
    twin[0] = (twin[0] + 1) % C
    twin[1], twin[2] = twin[1] + 2.0, twin[2] + 3.0
    crowd.insert(1, twin)
    clipped = [1, -14.63, -14.63, 40.37, 40.37]              # a box mostly outside the image: fewer than 10 candidate anchors
    if c["layout"] == "a":
        images = [[], [clipped], crowd, [rand_gt(), rand_gt(0.1, 0.2)]]
        good = {(2, 0), (2, 1), (2, 3), (3, 0)}
    else:
        images = [[], [rand_gt()], crowd + [rand_gt(0.08, 0.15)]]
        good = {(1, 0), (2, 0), (2, 1), (2, 2), (2, 4)}
    B = len(images)
    labels = np.zeros((B, G, 5), np.float32)
    raw = np.concatenate([rng.normal(0, 0.5, (B, A, 4)), rng.normal(-1.0, 1.5, (B, A, 1 + C))], 2).astype(np.float32)
    an = anchors.numpy()
    for b, gts in enumerate(images):
        assert len(gts) < G                                   # zero rows follow the valid ones
        for j, gt in enumerate(gts):
            labels[b, j] = gt
            if (b, j) not in good:
                continue
            # predictions near this gt are close to it: high IoUs, dynamic_k >= 3
            k, cx, cy, w, h = gt
            xc, yc = an[:, 0] * an[:, 2] + 0.5 * an[:, 2], an[:, 1] * an[:, 2] + 0.5 * an[:, 2]
            near = (np.abs(xc - cx) < 2.5 * an[:, 2]) & (np.abs(yc - cy) < 2.5 * an[:, 2]) & (rng.uniform(size=A) < 0.7)
            n = int(near.sum())
            raw[b, near, 0] = cx / an[near, 2] - an[near, 0] + rng.normal(0, 0.12, n)
            raw[b, near, 1] = cy / an[near, 2] - an[near, 1] + rng.normal(0, 0.12, n)
            raw[b, near, 2] = np.log(w / an[near, 2]) + rng.normal(0, 0.15, n)
            raw[b, near, 3] = np.log(h / an[near, 2]) + rng.normal(0, 0.15, n)
            raw[b, near, 4] += 2.0
            raw[b, near, 5 + int(k)] += 3.0
    return hw, anchors, torch.from_numpy(raw), torch.from_numpy(labels)


def check_margins(anchors, raw, labels):
    """The fp64 restatement's margins and coverage facts, and e_cost against its fp32 run."""
    _, info = R.losses(raw.double(), anchors.double(), labels.double())
    _, info32 = R.losses(raw, anchors, labels)
    margins, facts, e_cost = {}, dict(n_cand=[], dynamic_k=[], sums=[], conflicts=0, unchosen_argmin=0, box_only=0, centre_only=0), 0.0
    for res, res32 in zip(info["per_image"], info32["per_image"]):
        if res is None:
            continue
        for k, v in res["margins"].items():
            margins[k] = min(margins.get(k, np.inf), v)
        finite = torch.isfinite(res["cost"])
        e_cost = max(e_cost, float(((res32["cost"].double() - res["cost"])[finite].abs() / (1 + 1e-3 * res["cost"][finite].abs())).max()))
        facts["n_cand"].append(int(res["cand"].sum()))
        facts["dynamic_k"] += res["dynamic_k"]
        facts["conflicts"] += int((res["times"] > 1).sum())
        facts["unchosen_argmin"] += res["unchosen_argmin"]
        facts["box_only"] += int((res["in_box"] & ~res["in_centre"]).any(0).sum())
        facts["centre_only"] += int((res["in_centre"] & ~res["in_box"]).any(0).sum())
        facts["sums"] += [float(res["iou"][j][res["cand"]].sort(descending=True).values[:10].sum()) for j in range(res["iou"].shape[0])]
    return margins, facts, e_cost, info


def run_reference(case, anchors, raw, labels):
    c = CASES[case]
    head = YOLOXHead(c["C"], width=0.125, fl_alpha=FL_ALPHA, fl_gamma=FL_GAMMA,
                     **{k: v for k, v in c["opts"].items() if k != "use_l1"})
    head.use_l1 = c["opts"]["use_l1"]
    head.train()
    captured = {}
    inner = head.get_assignments

    def spy(*args, **kwargs):
        captured[args[0]] = inner(*args, **kwargs)
        return captured[args[0]]

    head.get_assignments = spy
    leaf = raw.clone().requires_grad_(True)
    grid, stride = anchors[:, :2][None], anchors[:, 2][None, :, None]
    outputs = torch.cat([(leaf[..., :2] + grid) * stride, torch.exp(leaf[..., 2:4]) * stride, leaf[..., 4:]], -1)
    out_dict, loss_dict = head.get_losses(None, [anchors[:, 0][None]], [anchors[:, 1][None]], [anchors[:, 2][None]], labels, outputs,
                                          [leaf[..., :4].clone()], dtype=torch.float32)
    sum(loss_dict.values()).backward()
    B, A = raw.shape[:2]
    matched_gt, matched_iou = np.full((B, A), -1, np.int32), np.zeros((B, A), np.float32)
    for b, (_cls, fg_mask, ious, inds, _n) in captured.items():
        matched_gt[b, fg_mask.numpy()] = inds.numpy()
        matched_iou[b, fg_mask.numpy()] = ious.numpy()
    losses = {k: np.float32(float(v.detach()) if isinstance(v, torch.Tensor) else v) for k, v in loss_dict.items()}
    return losses, np.float32(out_dict["num_fg"]), matched_gt, matched_iou, leaf.grad.numpy().copy()


def main():
    seen = dict(few_candidates=False, k3=False, k1_clamp=False, conflict=False, unchosen_argmin=False, box_only=False, centre_only=False,
                no_gt=False, one_gt=False, five_gt=False)
    for case, c in CASES.items():
        for seed in range(200):
            hw, anchors, raw, labels = build_inputs(case, seed)
            margins, facts, e_cost, info64 = check_margins(anchors, raw, labels)
            lanes = E.lane_facts(info64["per_image"][-1]) if c["layout"] == "dense" else None
            if (min(margins.values()) > MARGIN > 16 * e_cost and facts["conflicts"] > 0 and max(facts["dynamic_k"]) >= 3
                    and (lanes is None or (lanes["full_lanes"] >= 128 and min(lanes["late_chosen"], lanes["late_top_iou"]) >= 5))):
                break
        else:
            raise AssertionError(f"{case}: no seed with every margin above {MARGIN}")
        assert min(margins.values()) > MARGIN > 16 * e_cost, (margins, e_cost)
        if lanes is not None:
            assert lanes["full_lanes"] >= 128 and lanes["late_chosen"] >= 5 and lanes["late_top_iou"] >= 5 and lanes["max_per_lane"] > E.TOPK, lanes
            print(f"{case}: lanes of the crowded image {lanes}")
        losses, ratio, matched_gt, matched_iou, grad = run_reference(case, anchors, raw, labels)
        # the restatement in fp64: its assignment must be the reference's, and its distance from the reference's fp32 is e_ref
        leaf = raw.double().requires_grad_(True)
        l64, info64 = R.losses(leaf, anchors.double(), labels.double(), fl_alpha=FL_ALPHA, fl_gamma=FL_GAMMA, **c["opts"])
        sum(l64.values()).backward()
        assert np.array_equal(info64["matched_gt"].numpy(), matched_gt), case
        fg = matched_gt >= 0
        num_gt = info64["num_gt"].numpy()
        out = dict(hw=np.array(hw, np.int32), strides=np.array(STRIDES, np.int32), num_classes=np.int32(c["C"]), seed=np.int32(seed),
                   iou_loss_type=np.array(c["opts"]["iou_loss_type"]), cls_loss_type=np.array(c["opts"]["cls_loss_type"]),
                   use_l1=np.bool_(c["opts"]["use_l1"]), fl_alpha=np.float64(FL_ALPHA), fl_gamma=np.float64(FL_GAMMA),
                   raw=raw.numpy(), labels=labels.numpy(), fg_mask=fg, matched_gt=matched_gt, matched_iou=matched_iou,
                   num_fg=fg.sum(1).astype(np.int32), num_gt=num_gt.astype(np.int32), num_fg_ratio=ratio, grad=grad,
                   e_cost=np.float64(e_cost), margin_min=np.float64(min(margins.values())),
                   e_ref_grad=np.float64(np.abs(grad.astype(np.float64) - leaf.grad.numpy()).max()),
                   e_ref_iou=np.float64(np.abs(matched_iou.astype(np.float64) - info64["matched_iou"].numpy()).max()))
        for k, v in margins.items():
            out[f"margin_{k}"] = np.float64(v)
        for k in R.KEYS:
            out[k] = losses[k]
            out[f"e_ref_{k}"] = np.float64(abs(float(losses[k]) - float(l64[k].detach())))
        seen["few_candidates"] |= any(n < 10 for n in facts["n_cand"])
        seen["k3"] |= max(facts["dynamic_k"]) >= 3
        seen["k1_clamp"] |= any(s < 1.0 for s in facts["sums"])
        seen["conflict"] |= facts["conflicts"] > 0
        seen["unchosen_argmin"] |= facts["unchosen_argmin"] > 0
        seen["box_only"] |= facts["box_only"] > 0
        seen["centre_only"] |= facts["centre_only"] > 0
        seen["no_gt"] |= bool((num_gt == 0).any())
        seen["one_gt"] |= bool((num_gt == 1).any())
        seen["five_gt"] |= bool((num_gt >= 5).any())
        assert (labels.numpy()[np.arange(len(num_gt)), num_gt].sum(-1) == 0).all()        # zero rows after the valid ones
        path = os.path.join(HERE, f"yolox_loss_golden_{case}.npz")
        np.savez_compressed(path, **out)
        print(f"{case}: seed {seed} A {raw.shape[1]} num_gt {num_gt.tolist()} num_fg {fg.sum(1).tolist()} dynamic_k {facts['dynamic_k']} "
              f"conflicts {facts['conflicts']} (argmin unchosen {facts['unchosen_argmin']}) candidates {facts['n_cand']}")
        print("   margins", {k: f"{v:.3g}" for k, v in margins.items()}, f"e_cost {e_cost:.3g}")
        print("   losses", {k: float(losses[k]) for k in R.KEYS}, "e_ref", {k: float(out[f'e_ref_{k}']) for k in R.KEYS},
              f"grad {float(out['e_ref_grad']):.3g} iou {float(out['e_ref_iou']):.3g}")
        print("   wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)
    # unchosen_argmin: an anchor whose argmin over all gts is a gt that did not choose it; the crowded image of b_iou_bce_l1 has two
    print("coverage", seen)
    assert all(seen.values()), seen


if __name__ == "__main__":
    main()
