"""YOLOX training on the CPU: the fp64 restatement (tests/yolox_loss_ref.py) and the package's batch-wise torch path
(det/yolox/models/losses.py) against the reference's own get_losses as recorded by tests/golden/make_golden_yolox_loss.py, and the
model's training-mode forward end to end.

Bars.  The fixture is the reference's fp32 run.  A loss is a sum of at most A (5 + C) <= 13650 fp32 terms per image (32928 in the dense
case, 448 x 448 with A = 4116, where most of the 256 lanes of the assignment kernel hold more than 10 candidates) divided by num_fg;
each term and each partial sum carries a relative rounding of 2^-24 = 6e-8 and torch sums pairwise, so 1e-5 of max(|loss|, 1) bounds
the fp32 run's distance from exact arithmetic with a factor > 10 to spare (measured e_ref: <= 1e-6, dense loss_conf = 161: 8e-6,
stored in the fixture).  Gradient elements are single terms divided
by num_fg: 1e-5 absolute + 1e-5 relative.  The assignment is compared exactly: the fixture's inputs have asserted selection margins."""
import glob
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import yolox_loss_ref as R  # noqa: E402

from gdrnpp_bop2022_amd.det.yolox import models as M  # noqa: E402
from gdrnpp_bop2022_amd.det.yolox.models import losses as L  # noqa: E402

CASES = ("a_iou_bce", "a_giou_focal_l1", "b_iou_bce_l1", "b21_giou_focal", "dense_giou_focal_l1")


def load_case(case):
    z = np.load(os.path.join(HERE, "golden", f"yolox_loss_golden_{case}.npz"))
    opts = dict(iou_loss_type=str(z["iou_loss_type"]), cls_loss_type=str(z["cls_loss_type"]), use_l1=bool(z["use_l1"]),
                fl_alpha=float(z["fl_alpha"]), fl_gamma=float(z["fl_gamma"]))
    anchors = R.anchor_table([tuple(r) for r in z["hw"].tolist()], z["strides"].tolist())
    return z, opts, anchors


def test_every_fixture_case_is_listed():
    found = sorted(os.path.basename(p)[len("yolox_loss_golden_"):-4] for p in glob.glob(os.path.join(HERE, "golden", "yolox_loss_golden_*.npz")))
    assert found == sorted(CASES)
    seen = set()
    for case in CASES:
        z, opts, anchors = load_case(case)
        assert float(z["margin_min"]) > 1e-3 > 16 * float(z["e_cost"])
        assert anchors.shape[0] == z["raw"].shape[1] and z["raw"].shape[2] == 5 + int(z["num_classes"])
        seen |= {opts["iou_loss_type"], opts["cls_loss_type"], "l1" if opts["use_l1"] else "no_l1", f"A{anchors.shape[0]}", f"C{int(z['num_classes'])}"}
        assert (z["num_gt"] == 0).any() and (z["num_gt"] == 1).any() and (z["num_gt"] >= 5).any()
    assert seen == {"iou", "giou", "bce", "focal", "l1", "no_l1", "A126", "A525", "A4116", "C3", "C21"}


def close(value, want, what):
    value, want = (v.detach() if isinstance(v, torch.Tensor) else v for v in (value, want))
    assert abs(float(value) - float(want)) <= 1e-5 * max(abs(float(want)), 1.0), (what, float(value), float(want))


@pytest.mark.parametrize("case", CASES)
def test_restatement_matches_the_reference_fixture(case):
    z, opts, anchors = load_case(case)
    raw = torch.from_numpy(z["raw"]).double().requires_grad_(True)
    losses, info = R.losses(raw, anchors, torch.from_numpy(z["labels"]).double(), **opts)
    sum(losses.values()).backward()
    assert np.array_equal(info["matched_gt"].numpy(), z["matched_gt"])
    assert np.array_equal(info["num_fg"].numpy(), z["num_fg"]) and np.array_equal(info["num_gt"].numpy(), z["num_gt"])
    assert np.array_equal(info["matched_gt"].numpy() >= 0, z["fg_mask"])
    assert np.abs(info["matched_iou"].numpy() - z["matched_iou"]).max() <= 1e-5
    for k in R.KEYS:
        close(losses[k], z[k], k)
        assert abs(abs(float(losses[k].detach()) - float(z[k])) - float(z[f"e_ref_{k}"])) <= 1e-12      # e_ref is this very distance
    g = raw.grad.numpy()
    assert np.all(np.abs(g - z["grad"]) <= 1e-5 + 1e-5 * np.abs(g))
    assert abs(np.abs(g - z["grad"]).max() - float(z["e_ref_grad"])) <= 1e-12


@pytest.mark.parametrize("case", CASES)
def test_torch_path_matches_the_reference_fixture(case):
    z, opts, anchors = load_case(case)
    raw = torch.from_numpy(z["raw"]).requires_grad_(True)
    losses, info = L.yolox_losses(raw, anchors.float(), torch.from_numpy(z["labels"]), **opts)
    assert list(losses) == ["loss_iou", "loss_conf", "loss_l1", "loss_cls"]
    sum(losses.values()).backward()
    assert info["matched_gt"].dtype == torch.int32 and np.array_equal(info["matched_gt"].numpy(), z["matched_gt"])
    assert np.array_equal(info["num_fg"].numpy(), z["num_fg"]) and np.array_equal(info["num_gt"].numpy(), z["num_gt"])
    assert np.abs(info["matched_iou"].numpy() - z["matched_iou"]).max() <= 1e-5
    for k in R.KEYS:
        close(losses[k], z[k], k)
    close(info["num_fg_ratio"], z["num_fg_ratio"], "num_fg_ratio")
    g = raw.grad.numpy().astype(np.float64)
    assert np.all(np.abs(g - z["grad"]) <= 1e-5 + 1e-5 * np.abs(g))
    assert np.abs(g[z["fg_mask"]]).max() > 1e-3


@pytest.mark.parametrize("case", CASES)
def test_torch_path_in_fp64_is_the_restatement(case):
    z, opts, anchors = load_case(case)
    raw = torch.from_numpy(z["raw"]).double()
    labels = torch.from_numpy(z["labels"]).double()
    a, b = raw.clone().requires_grad_(True), raw.clone().requires_grad_(True)
    mine, info = L.yolox_losses(a, anchors, labels, **opts)
    ref, ref_info = R.losses(b, anchors, labels, **opts)
    sum(mine.values()).backward()
    sum(ref.values()).backward()
    assert mine["loss_iou"].dtype == torch.float64
    assert np.array_equal(info["matched_gt"].numpy(), ref_info["matched_gt"].numpy())
    for k in R.KEYS:
        assert abs(float(mine[k].detach()) - float(ref[k].detach())) <= 1e-12 * max(abs(float(ref[k].detach())), 1.0), k
    assert torch.allclose(a.grad, b.grad, rtol=1e-10, atol=1e-13)


def test_edge_inputs_of_the_torch_path():
    z, opts, anchors = load_case("a_iou_bce")
    raw = torch.from_numpy(z["raw"])
    # no label rows at all, and only empty rows: every anchor is background, the only loss is objectness over num_fg = 1
    for labels in (torch.zeros(raw.shape[0], 0, 5), torch.zeros(raw.shape[0], 3, 5)):
        losses, info = L.yolox_losses(raw, anchors.float(), labels)
        assert int((info["matched_gt"] >= 0).sum()) == 0 and float(losses["loss_iou"]) == 0.0 and float(losses["loss_cls"]) == 0.0
        want = torch.nn.functional.binary_cross_entropy_with_logits(raw[..., 4], torch.zeros_like(raw[..., 4]), reduction="sum")
        close(losses["loss_conf"], want, "loss_conf")
    # a gt no anchor centre falls into has no foreground (the reference raises there)
    labels = torch.zeros(raw.shape[0], 1, 5)
    labels[0, 0] = torch.tensor([1.0, 2000.0, 2000.0, 4.0, 4.0])
    losses, info = L.yolox_losses(raw, anchors.float(), labels)
    assert info["num_gt"].tolist()[0] == 1 and int(info["num_fg"].sum()) == 0
    # the reference's rule for an empty row BETWEEN valid ones: num_gt counts the rows with sum > 0, the gts are the FIRST num_gt rows —
    # here the valid row 0 and the empty row 1 (a zero-size gt at the origin); the valid row 2 is not a gt
    labels = torch.from_numpy(z["labels"]).double()
    first, second = labels[3, 0].clone(), labels[3, 1].clone()
    labels[3] = 0.0
    labels[3, 0], labels[3, 2] = first, second
    mine, info = L.yolox_losses(raw.double(), anchors, labels, use_l1=True)
    ref, ref_info = R.losses(raw.double(), anchors, labels, use_l1=True)
    assert info["num_gt"].tolist() == [0, 1, 6, 2] and np.array_equal(info["matched_gt"].numpy(), ref_info["matched_gt"].numpy())
    assert int((info["matched_gt"][3] == 1).sum()) >= 1 and int((info["matched_gt"][3] == 2).sum()) == 0
    for k in R.KEYS:
        assert abs(float(mine[k]) - float(ref[k])) <= 1e-12 * max(abs(float(ref[k])), 1.0), k
    with pytest.raises(NotImplementedError, match="obj_loss_type"):
        L.yolox_losses(raw, anchors.float(), labels, obj_loss_type="focal")
    with pytest.raises(NotImplementedError, match="cls_loss_type"):
        L.yolox_losses(raw, anchors.float(), labels, cls_loss_type="ce")


def test_iouloss_module_reductions():
    pred = torch.tensor([[10.0, 10.0, 8.0, 6.0], [30.0, 12.0, 4.0, 4.0]])
    target = torch.tensor([[11.0, 9.0, 8.0, 8.0], [10.0, 10.0, 4.0, 4.0]])
    none = L.IOUloss()(pred, target)
    inter, union = 7.0 * 6.0, 48.0 + 64.0 - 42.0
    assert torch.allclose(none, torch.tensor([1 - (inter / union) ** 2, 1.0]))
    assert torch.allclose(L.IOUloss(reduction="mean")(pred, target), none.mean()) and torch.allclose(L.IOUloss("sum")(pred, target), none.sum())
    giou = L.IOUloss(loss_type="giou")(pred, target)
    hull = 9.0 * 8.0
    assert torch.allclose(giou[0], torch.tensor(1 - (inter / union - (hull - union) / hull)))
    assert 1.0 < float(giou[1]) <= 2.0


def test_model_trains_end_to_end_on_the_torch_path():
    from gdrnpp_bop2022_amd.gdrn_modeling.solver import Ranger

    torch.manual_seed(0)
    net = M.build_yolox(0.33, 0.5, 3)
    keys = list(net.state_dict())
    net.train()
    assert net.head.use_l1 is False and (net.head.iou_loss_type, net.head.cls_loss_type, net.head.obj_loss_type) == ("iou", "bce", "bce")
    assert (net.head.fl_alpha, net.head.fl_gamma) == (0.25, 2.0) and list(net.state_dict()) == keys
    x = torch.randn(2, 3, 64, 64)
    targets = torch.zeros(2, 4, 5)
    targets[0, 0] = torch.tensor([1.0, 30.4, 28.3, 24.2, 30.1])
    targets[0, 1] = torch.tensor([2.0, 45.4, 40.3, 20.2, 18.1])
    targets[1, 0] = torch.tensor([0.0, 20.4, 40.3, 30.2, 22.1])
    net.head.use_l1 = True
    out_dict, loss_dict = net(x, targets)
    assert list(loss_dict) == ["loss_iou", "loss_conf", "loss_l1", "loss_cls"]
    assert all(torch.isfinite(v) and v.dim() == 0 for v in loss_dict.values()) and float(loss_dict["loss_l1"]) > 0
    assert 0 < float(out_dict["num_fg"]) <= 10.0
    opt = Ranger(net.parameters(), lr=1e-3)
    sum(loss_dict.values()).backward()
    missing = [n for n, p in net.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing, missing
    assert sum(float(p.grad.abs().sum()) for p in net.parameters()) > 0
    before = [p.detach().clone() for p in net.parameters()]
    opt.step()
    assert any(not torch.equal(a, p.detach()) for a, p in zip(before, net.parameters()))
    assert all(torch.isfinite(p).all() for p in net.parameters())
    # the head alone: the same pair through forward(xin, labels, imgs)
    feats = net.backbone(x)
    out2, loss2 = net.head(feats, targets, x)
    assert set(loss2) == set(loss_dict) and "num_fg" in out2
