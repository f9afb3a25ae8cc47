"""The builders of tests/yolox_loss_edge_cases.py without a GPU: every property that makes a case of tests/test_gpu_yolox_loss_edges.py
prove something is asserted here on the fp64 restatement (tests/yolox_loss_ref.py), and the package's torch path
(det/yolox/models/losses.py) runs on the same cases: its assignment is the restatement's, at the exact ties too.

Every decision that is no exact tie has a margin above 1e-3 against an fp32 cost distance e_cost with 16 e_cost < 1e-3, as in
tests/golden/make_golden_yolox_loss.py; the ties are equal bits in fp32 and fp64, and the restatement's stable sorts give them to the
lowest index."""
import numpy as np
import pytest
import torch

import yolox_loss_edge_cases as C
import yolox_loss_ref as R

from gdrnpp_bop2022_amd.det.yolox.models import losses as L

MARGIN = C.MARGIN
ASSIGNED = [("partials", ()), ("tie", ("lane",)), ("tie", ("wave",)), ("tie", ("list",)), ("duplicate", ()), ("small", ("tiny",)), ("small", ("ragged",))]


def build(kind, args):
    return getattr(C, f"{kind}_case")(*args)


def images_of(case, skip_rows=None):
    """(image, its gts f32[n,5]) of the images with a gt; ``skip_rows`` {image: (row, copy)}: without the copy."""
    for b in range(case["raw"].shape[0]):
        lab = case["labels"][b]
        n = int((lab.sum(1) > 0).sum())
        rows = [j for j in range(n) if not (skip_rows and b in skip_rows and j == skip_rows[b][1])]
        if rows:
            yield b, lab[rows]


def assert_margins(case, skip_rows=None):
    out = {}
    for b, gts in images_of(case, skip_rows):
        res, e_cost = C.image_margins(case["raw"][b], C.anchors_of(case), gts)
        assert min(res["margins"].values()) > MARGIN > 16 * e_cost, (case["name"], b, res["margins"], e_cost)
        out[b] = res
    return out


# ------------------------------------------------------------------------------------------------------------------ dense images
def test_dense_fixture_is_the_builders_batch_and_its_lanes_are_full():
    z = np.load(f"{C.HERE}/golden/yolox_loss_golden_dense_giou_focal_l1.npz")
    raw, labels = C.dense_batch(int(z["seed"]))
    assert np.array_equal(raw, z["raw"]) and np.array_equal(labels, z["labels"]) and raw.shape == (3, 4116, 8)
    assert z["num_gt"].tolist() == [0, 1, 7] and (str(z["iou_loss_type"]), str(z["cls_loss_type"]), bool(z["use_l1"])) == ("giou", "focal", True)
    boxes = labels[2, :7, 3:5] / C.DENSE_SIZE
    assert (boxes[:6] > 0.6).all() and (boxes[:6] < 0.91).all() and (boxes[6] < 0.16).all()          # six large (the twin pair first), one small
    assert np.array_equal(labels[2, 1, 3:5], labels[2, 0, 3:5]) and labels[2, 1, 0] != labels[2, 0, 0]
    for kind in ("single", "crowd"):
        ok, res, e_cost, facts = C.dense_ok(*C.dense_image(kind, int(z["seed"])))
        assert ok, (kind, res["margins"], e_cost, facts)
    print("dense fixture, crowded image:", facts)
    assert facts["full_lanes"] >= 128 and facts["late_chosen"] >= 5 and facts["late_top_iou"] >= 5 and facts["max_per_lane"] >= 13
    assert facts["dynamic_k"] >= 8 and facts["conflicts"] >= 5
    # the chosen anchors of the fixture are the restatement's, so the late ones are among what the kernel must find
    assert np.array_equal(res["matched_gt"].numpy(), z["matched_gt"][2])


def test_partials_case_has_more_partials_than_threads_and_four_dense_images():
    case = C.partials_case()
    B, A, _ = case["raw"].shape
    assert (B, A) == (16, 4116) and -(-B * A // C.LANES) == 258 > C.LANES
    assert ((case["labels"].sum(2) > 0).sum(1) == np.array([7] * 4 + [0] * 12)).all()
    assert len(set(C.PARTIALS_SEEDS)) == 4
    for seed in C.PARTIALS_SEEDS:
        ok, res, e_cost, facts = C.dense_ok(*C.dense_image("crowd", seed))
        assert ok and facts["full_lanes"] >= 128 and facts["late_chosen"] >= 5 and facts["late_top_iou"] >= 5, (seed, res["margins"], e_cost, facts)
    y = C.yardstick(case)
    assert (y["num_fg"][:4] >= 20).all() and (y["num_fg"][4:] == 0).all()
    # partials 256 and 257, the second step of threads 0 and 1, hold a share of the objectness loss that is far above the bar
    tail = C.T(case["raw"].reshape(-1, 8)[256 * C.LANES:, 4], torch.float64)
    share = float(torch.nn.functional.softplus(tail).sum()) / max(int(y["num_fg"].sum()), 1)
    assert share > 1e3 * (2 * y["e_loss"]["loss_conf"] + C.ulp32(y["l64"]["loss_conf"])), share


# ------------------------------------------------------------------------------------------------------------------- exact ties
@pytest.mark.parametrize("variant", sorted(C.TIE_VARIANTS))
def test_tie_case_has_twelve_equal_costs_and_the_lowest_indices_win(variant):
    case, v, D = C.tie_case(variant), C.TIE_VARIANTS[variant], C.tie_members(variant)
    k = v["k"]
    assert case["raw"].shape == (1, 4096, 8) and len(D) == 12 == len(set(D))
    lane, wave = [d % C.LANES for d in D], [d % C.LANES // 64 for d in D]
    if variant == "lane":
        assert D[k] - D[k - 1] == 1 and wave[k] == wave[k - 1]
    elif variant == "wave":
        assert D[k] - D[k - 1] == 64 and wave[k] != wave[k - 1] and lane[k] % 64 == lane[k - 1] % 64
    else:
        assert D[k - 1] + 256 in D and D[k] - D[k - 1] < 256 and lane.count(lane[k - 1]) == 2
    gts = case["labels"][0, :1]
    res, e_cost = C.image_margins(case["raw"][0], C.anchors_of(case), gts)
    res32 = R.assign_image(C.T(case["raw"][0]), C.anchors_of(case, torch.float32), C.T(gts))
    member = torch.zeros(4096, dtype=torch.bool)
    member[D] = True
    assert bool((res["in_box"][0] & res["in_centre"][0])[D].all()) and int(res["in_centre"][0].sum()) == 25
    for r in (res, res32):          # equal bits, costs and IoUs, and the same decoded box
        assert len(set(r["cost"][0, D].tolist())) == 1 and len(set(r["iou"][0, D].tolist())) == 1
    box32 = R.decode(C.T(case["raw"][0]), C.anchors_of(case, torch.float32))[D]
    assert bool((box32 == box32[0]).all()) and box32[0, :2].tolist() == [260.0, 188.0]
    others = res["cand"] & ~member
    assert R.scaled_gap(res["cost"][0, D[0]], res["cost"][0, others].min()) > MARGIN > 16 * e_cost
    assert float(res["iou"][0, D[0]] - res["iou"][0, others].max()) > MARGIN           # the ten largest IoUs are members': 10 times one value
    assert res["margins"]["geometry"] > MARGIN and res["margins"]["dynamic_k"] > 0.4 and res["dynamic_k"] == [k]
    assert abs(10 * float(res["iou"][0, D[0]]) - (k + 0.5)) < 0.05
    assert torch.nonzero(res["matched_gt"] >= 0).flatten().tolist() == D[:k] == torch.nonzero(res32["matched_gt"] >= 0).flatten().tolist()


def test_duplicate_rows_resolve_to_the_lower_row_and_count_once():
    case = C.duplicate_case()
    unique = assert_margins(case, C.DUPLICATE_ROWS)
    y = C.yardstick(case)
    labels = case["labels"]
    for b, (row, copy) in C.DUPLICATE_ROWS.items():
        assert np.array_equal(labels[b, row], labels[b, copy]) and labels[b, row].sum() > 0
        res = unique[b]
        both = torch.nonzero(res["chosen"][row]).flatten().tolist()
        assert len(both) >= 5
        # with the copy every one of them is chosen more than once: the argmin over the DIFFERENT gts has a margin, the copy ties
        for a in both:
            low = res["cost"][:, a].sort().values
            assert low.numel() < 2 or R.scaled_gap(low[0], low[1]) > MARGIN
        m = y["matched_gt"][b]
        assert (m != copy).all() and int((m == row).sum()) >= 5
        # the same foreground as without the copy, each anchor counted once; rows behind the copy moved up by one
        want = res["matched_gt"].numpy()
        assert np.array_equal(m >= 0, want >= 0) and int(y["num_fg"][b]) == int((want >= 0).sum())
        assert np.array_equal(np.where(m > copy, m - 1, m), want)
    assert int((unique[0]["times"] > 1).sum()) >= 1          # and an anchor that two different gts choose


@pytest.mark.parametrize("kind", sorted(C.SMALL_LAYOUT))
def test_small_cases_have_their_anchor_counts_and_margins(kind):
    case = C.small_case(kind)
    res = assert_margins(case)
    A = case["raw"].shape[1]
    y = C.yardstick(case)
    assert y["num_gt"].tolist() == [1, 2, 0]
    if kind == "tiny":
        assert case["hw"] == [(2, 3), (1, 1)] and A == 7
        assert all(int(r["cand"].sum()) < C.TOPK for r in res.values()) and max(res[0]["dynamic_k"]) >= 2
    else:
        assert A % C.LANES == 1 and A > C.LANES
        assert y["matched_gt"][0, -1] == 0 and y["matched_gt"][1, -1] == 0          # the lone anchor of the second workgroup is foreground
    assert (y["num_fg"][:2] >= 1).all() and y["num_fg"][2] == 0


# ----------------------------------------------------------------------------------------------------------- hand-made assignment
def test_pair_case_is_exact_and_sits_on_the_non_smooth_points():
    case = C.pair_case()
    assert case["raw"].shape == (2, 336, 8) and len(case["pairs"]) == 21
    a32, a64 = C.anchors_of(case, torch.float32), C.anchors_of(case)
    box32, box64 = R.decode(C.T(case["raw"]), a32), R.decode(C.T(case["raw"], torch.float64), a64)
    m = case["matched_gt"]
    assert int((m >= 0).sum()) == 21 and (m[:, ::2] == -1).all()          # background in between
    seen = set()
    for kind, b, a, row in case["pairs"]:
        assert m[b, a] == row and torch.equal(box32[b, a].double(), box64[b, a])
        s = float(a64[a, 2])
        p, g = box64[b, a].numpy(), case["labels"][b, row, 1:5].astype(np.float64)
        assert p[2] == p[3] == s and np.array_equal(4 * p / s, np.round(4 * p / s)) and np.array_equal(4 * g / s, np.round(4 * g / s))
        pl, pt, pr, pb = p[0] - p[2] / 2, p[1] - p[3] / 2, p[0] + p[2] / 2, p[1] + p[3] / 2
        gl, gt, gr, gb = g[0] - g[2] / 2, g[1] - g[3] / 2, g[0] + g[2] / 2, g[1] + g[3] / 2
        iou = float(R.pair_iou(torch.from_numpy(g)[None], box64[b, a][None]))
        assert {"identical": (pl, pt, pr, pb) == (gl, gt, gr, gb) and iou == 1.0,
                "left_edge": pl == gl and gt < pt and pb < gb and pr < gr and 0 < iou < 1,
                "top_edge_inside": pt == gt and gl < pl and pr < gr and pb < gb and 0 < iou < 1,
                "touching": pr == gl and gt < pb and pt < gb and iou == 0,
                "corner_touch": pr == gl and pb == gt and iou == 0,
                "disjoint": pr < gl and gb < pt and iou == 0,
                "same_centre": (p[0], p[1]) == (g[0], g[1]) and gl < pl and pt < gt and 0 < iou < 1}[kind], (kind, p, g)
        seen.add((kind, s))
    assert seen == {(k, float(s)) for k in C.PAIR_KINDS for s in C.STRIDES}
    # GIoU has a gradient where the boxes do not overlap, IoU has none; equal edges split the gradient of max / min evenly
    for opts in C.PAIR_OPTIONS:
        y = C.yardstick(case, (1.0, 0.0, 0.0, 0.0), opts, m)
        for kind, b, a, _ in case["pairs"]:
            g = y["g64"][b, a, :4]
            if kind in ("touching", "corner_touch", "disjoint"):
                assert (np.abs(g).max() > 1e-3) == (opts["iou_loss_type"] == "giou"), (kind, opts, g)
            if kind == "identical":
                assert np.abs(g).max() < 1e-12          # the maximum of the IoU
            if kind == "left_edge" and opts["iou_loss_type"] == "iou":
                assert g[0] < -1e-3          # half of the left edge's pull is missing: moving right loses nothing at the shared edge


def test_torch_iou_loss_has_the_restatements_gradient_on_the_pairs():
    case = C.pair_case()
    box = R.decode(C.T(case["raw"], torch.float64), C.anchors_of(case))
    rows = [(b, a, row) for _, b, a, row in case["pairs"]]
    pred = torch.stack([box[b, a] for b, a, _ in rows])
    target = torch.stack([C.T(case["labels"][b, row, 1:5], torch.float64) for b, _, row in rows])
    for kind in ("iou", "giou"):
        p1, p2 = pred.clone().requires_grad_(True), pred.clone().requires_grad_(True)
        mine, ref = L.iou_loss(p1, target, kind), R.iou_loss(p2, target, kind)
        mine.sum().backward()
        ref.sum().backward()
        assert float((mine - ref).abs().max()) <= 1e-15 and float((p1.grad - p2.grad).abs().max()) <= 1e-15          # another order of the products


# ------------------------------------------------------------------------------------------------------------------ weighted sums
@pytest.mark.parametrize("which", ("fixture", "pairs"))
def test_weighted_gradients_tell_the_four_losses_apart(which):
    case = C.fixture_case("a_giou_focal_l1") if which == "fixture" else C.pair_case()
    kw = dict(opts=None, matched_gt=None) if which == "fixture" else dict(opts=C.PAIR_OPTIONS[-1], matched_gt=C.pair_case()["matched_gt"])
    assert (kw["opts"] or case["opts"])["use_l1"]
    ys = [C.yardstick(case, w, **kw) for w in C.WEIGHTS]
    units = [y["g64"] for y in ys[1:]]
    assert np.abs(ys[0]["g64"] - sum(w * g for w, g in zip(C.WEIGHTS[0], units))).max() < 1e-12
    # every loss reaches the gradient, the L1 and the class loss in different columns: exchanged weights cannot go unseen
    assert all(np.abs(g).max() > 1e-3 for g in units)
    assert np.abs(units[2][..., 4:]).max() == 0 and np.abs(units[3][..., :5]).max() == 0 and np.abs(units[1][..., :4]).max() == 0
    assert len({abs(w) for w in C.WEIGHTS[0]}) == 4
    kinks = np.argwhere(ys[3]["e_grad_each"] > 1e-6)          # where the fp32 restatement's L1 gradient leaves fp64
    if which == "fixture":
        assert kinks.size == 0
    else:
        # a gt side of one stride against a size logit of 0: the L1 target log(1 + 1e-8) is 0 in fp32, its sign too.  Everywhere else
        # the per-element e_ref of the GPU test is at rounding level
        square = {(b, a) for kind, b, a, _ in case["pairs"] if kind in ("identical", "corner_touch")}
        assert len(kinks) == 12 and {(b, a) for b, a, _ in kinks.tolist()} == square and set(kinks[:, 2].tolist()) == {2, 3}
        assert all(abs(ys[3]["e_grad_each"][b, a, c] - 1 / 21) < 1e-6 for b, a, c in kinks.tolist())


# ------------------------------------------------------------------------------------------------------------------ the torch path
@pytest.mark.parametrize("kind,args", ASSIGNED, ids=lambda v: "_".join(v) if isinstance(v, tuple) else v)
@pytest.mark.parametrize("dtype", (torch.float32, torch.float64), ids=("fp32", "fp64"))
def test_torch_path_gives_the_restatements_assignment_and_losses(kind, args, dtype):
    case = build(kind, args)
    y = C.yardstick(case)
    # no case sits on a kink of the losses by accident: the fp32 restatement stays near fp64, which keeps the GPU tests' bars tight
    assert y["e_grad"] <= 1e-6 and all(y["e_loss"][k] <= 1e-5 * max(abs(y["l64"][k]), 1.0) for k in R.KEYS), (y["e_grad"], y["e_loss"])
    raw = C.T(case["raw"], dtype).requires_grad_(True)
    losses, info = L.yolox_losses(raw, C.anchors_of(case, dtype), C.T(case["labels"], dtype), **case["opts"])
    sum(losses.values()).backward()
    assert np.array_equal(info["matched_gt"].numpy(), y["matched_gt"])
    assert np.array_equal(info["num_fg"].numpy(), y["num_fg"]) and np.array_equal(info["num_gt"].numpy(), y["num_gt"])
    # fp64: the restatement's arithmetic in another order of summation; fp32: the bars of tests/test_yolox_loss_cpu.py
    rel, g_abs = (1e-12, 1e-13) if dtype == torch.float64 else (1e-5, 1e-5)
    for k in R.KEYS:
        assert abs(float(losses[k].detach()) - y["l64"][k]) <= rel * max(abs(y["l64"][k]), 1.0), k
    g = raw.grad.double().numpy()
    assert np.all(np.abs(g - y["g64"]) <= g_abs + (1e-10 if dtype == torch.float64 else 1e-5) * np.abs(y["g64"]))
