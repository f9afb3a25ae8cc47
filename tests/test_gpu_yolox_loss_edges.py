"""-m gpu: csrc/yolox_loss.hip (``gdrnpp_yolox_assign``, ``gdrnpp_yolox_losses``, ``gdrnpp_yolox_losses_backward``) on the cases of
tests/yolox_loss_edge_cases.py: full per-lane lists and evictions, more partial sums than threads, exact ties between lanes, waves, list
entries and label rows, A = 7 and A = 257, the non-smooth points of the IoU losses through a hand-made assignment, and uneven weights
of the four losses in the backward.  The yardstick is tests/yolox_loss_ref.py in fp64 on the CPU;
tests/test_yolox_loss_edge_cases_cpu.py asserts what each case is built to hold.

Bars.  The assignment (matched_gt, the matched_iou > 0 pattern, num_fg, num_gt) is EQUAL to the restatement's: every decision has a
margin of 1e-3 against 16 e_cost, or is an exact tie of equal bits, which goes to the lowest index.  Each loss and each gradient element:
|ours - ref64| <= 2 e_ref + one fp32 ulp of the value, e_ref = the restatement's own fp32 run's distance from its fp64 run on the same
inputs (per loss; for the gradient the largest element distance), the form and the factor of tests/test_gpu_yolox_loss.py.  The
hand-made assignment is handed to ``hip_lib.yolox_losses`` / ``yolox_losses_backward`` directly; its losses are the kernel's f64.  With
``use_l1`` its pairs of equal width or height sit on the kink of the L1 loss: the target is log(1 + 1e-8), which is 0 in fp32 and 1e-8
in fp64 against a size logit of 0, so the fp32 restatement's sign there is 0 and e_ref of those twelve elements is 1 / num_fg.  For this
case e_ref of the gradient is therefore taken per element, never above the largest one, and loss_iou is also run alone.

Measured on an MI355X, largest |ours - ref64| / bar (losses, gradient): 16 images 0.13, 0.03; ties lane 0.14, 0.05, wave 0.14, 0.05, list
0.17, 0.12; duplicate rows 0.19, 0.03; A = 7 0.22, 0.03; A = 257 0.12, 0.02; hand-made pairs, all options: losses 3e-9 (the kernel's f64),
gradient 0.10 - 0.25 with e_ref per element, loss_iou alone 0.10 (iou) and 0.19 (giou); weighted backward of the A = 126 fixture 0.12,
0.05 - 0.25 over the five weight vectors; of the pairs 3e-9, 0.13 - 0.25."""
import numpy as np
import pytest
import torch

import yolox_loss_edge_cases as C
import yolox_loss_ref as R

from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd.det.yolox.models import losses as L
from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers

pytestmark = pytest.mark.gpu
DEV = "cuda"
ONES = (1.0, 1.0, 1.0, 1.0)


def run_device(case, weights=ONES):
    raw = C.T(case["raw"]).to(DEV).requires_grad_(True)
    before = hip_layers.fallback_launches()
    losses, info = L.yolox_losses(raw, C.anchors_of(case, torch.float32).to(DEV), C.T(case["labels"]).to(DEV), **case["opts"])
    sum(w * losses[k] for w, k in zip(weights, R.KEYS)).backward()
    assert hip_layers.fallback_launches() == before        # nothing of it ran on PyTorch operators
    return {k: float(v.detach()) for k, v in losses.items()}, info, raw.grad.cpu().numpy().astype(np.float64)


def assert_assignment(info, y):
    matched_gt, matched_iou = info["matched_gt"].cpu().numpy(), info["matched_iou"].cpu().numpy()
    wrong = np.argwhere(matched_gt != y["matched_gt"])
    assert wrong.size == 0, (len(wrong), [(int(b), int(a), int(matched_gt[b, a]), int(y["matched_gt"][b, a])) for b, a in wrong[:8]])
    assert np.array_equal(matched_iou > 0, y["matched_iou"] > 0)
    assert np.array_equal(info["num_fg"].cpu().numpy(), y["num_fg"]) and np.array_equal(info["num_gt"].cpu().numpy(), y["num_gt"])
    return matched_gt, matched_iou


def assert_values(what, losses, grad, y, each=False):
    """``each``: e_ref of the gradient per element instead of the largest one (nowhere a wider bar)."""
    worst = 0.0
    for k in R.KEYS:
        d, bar = abs(losses[k] - y["l64"][k]), 2 * y["e_loss"][k] + float(C.ulp32(y["l64"][k]))
        print(f"{what}: {k} = {losses[k]:.8g}, |ours - ref64| = {d:.3g}, bar {bar:.3g} (e_ref {y['e_loss'][k]:.3g})")
        assert d <= bar, (what, k, d, bar)
        worst = max(worst, d / bar)
    d, bar = np.abs(grad - y["g64"]), 2 * (y["e_grad_each"] if each else y["e_grad"]) + C.ulp32(y["g64"])
    print(f"{what}: gradient max |ours - ref64| = {d.max():.3g} (e_ref {y['e_grad']:.3g}); largest distance / bar: losses {worst:.3g}, gradient {np.max(d / bar):.3g}")
    assert np.all(d <= bar), (what, float((d - bar).max()), np.argwhere(d > bar)[:8].tolist())


def check_case(case):
    y = C.yardstick(case)
    losses, info, grad = run_device(case)
    matched = assert_assignment(info, y)
    assert_values(case["name"], losses, grad, y)
    return matched


def test_sixteen_images_with_full_lane_lists_and_258_partial_sums():
    check_case(C.partials_case())


@pytest.mark.parametrize("variant", sorted(C.TIE_VARIANTS))
def test_twelve_equal_costs_go_to_the_lowest_anchors(variant):
    matched_gt, matched_iou = check_case(C.tie_case(variant))
    want = C.tie_members(variant)[:C.TIE_VARIANTS[variant]["k"]]
    assert np.flatnonzero(matched_gt[0] >= 0).tolist() == want
    assert len(set(matched_iou[0, want].tolist())) == 1          # one box, one IoU


def test_a_label_row_written_twice_resolves_to_the_lower_row():
    matched_gt, _ = check_case(C.duplicate_case())
    for b, (row, copy) in C.DUPLICATE_ROWS.items():
        assert (matched_gt[b] != copy).all() and (matched_gt[b] == row).any()


@pytest.mark.parametrize("kind", sorted(C.SMALL_LAYOUT))
def test_seven_anchors_and_one_anchor_past_a_workgroup(kind):
    matched_gt, _ = check_case(C.small_case(kind))
    if kind == "ragged":
        assert matched_gt[0, -1] == 0 and matched_gt[1, -1] == 0


def run_given_assignment(case, opts, weights):
    raw, anchors, labels = C.T(case["raw"]).to(DEV), C.anchors_of(case, torch.float32).to(DEV), C.T(case["labels"]).to(DEV)
    y = C.yardstick(case, weights, opts, case["matched_gt"])
    matched = C.T(case["matched_gt"]).to(DEV)
    out = hip_lib.yolox_losses(raw, anchors, labels, matched, C.T(y["num_fg"]).to(DEV), C.T(y["num_gt"]).to(DEV), **C.FL, **opts)
    scale = torch.tensor(weights, dtype=torch.float32, device=DEV)
    grad = hip_lib.yolox_losses_backward(raw, anchors, labels, matched, out, scale, **C.FL, **opts)
    out = out.cpu().tolist()
    assert out[4] == max(int(y["num_fg"].sum()), 1) and out[5] == int(y["num_gt"].sum())
    return dict(zip(R.KEYS, out[:4])), grad.cpu().numpy().astype(np.float64), y


@pytest.mark.parametrize("opts", C.PAIR_OPTIONS, ids=lambda o: f"{o['iou_loss_type']}-{o['cls_loss_type']}-{'l1' if o['use_l1'] else 'no_l1'}")
def test_hand_made_pairs_on_equal_edges_touching_and_disjoint(opts):
    case = C.pair_case()
    losses, grad, y = run_given_assignment(case, opts, ONES)
    assert_values(f"pairs {opts}", losses, grad, y, each=True)
    # loss_iou alone: what iou_loss<kGrad> gives at its non-smooth points, against that loss's own fp32 distance
    losses, grad, y = run_given_assignment(case, opts, (1.0, 0.0, 0.0, 0.0))
    assert_values(f"pairs {opts}, loss_iou alone", losses, grad, y)


@pytest.mark.parametrize("weights", C.WEIGHTS, ids=lambda w: "_".join(f"{v:g}" for v in w))
def test_weighted_backward_of_the_small_fixture(weights):
    case = C.fixture_case("a_giou_focal_l1")
    y = C.yardstick(case, weights)
    losses, info, grad = run_device(case, weights)
    assert_assignment(info, y)
    assert_values(f"fixture weights {weights}", losses, grad, y)


@pytest.mark.parametrize("weights", C.WEIGHTS, ids=lambda w: "_".join(f"{v:g}" for v in w))
def test_weighted_backward_of_the_hand_made_pairs(weights):
    opts = C.PAIR_OPTIONS[-1]          # giou, focal, l1
    losses, grad, y = run_given_assignment(C.pair_case(), opts, weights)
    assert_values(f"pairs weights {weights}", losses, grad, y, each=True)
