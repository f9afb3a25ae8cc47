"""Case builders for csrc/yolox_loss.hip (SimOTA assignment, detection losses, their gradient) at the inputs its four small fixtures
never reach, shared by tests/test_gpu_yolox_loss_edges.py (the kernels against tests/yolox_loss_ref.py in fp64),
tests/test_yolox_loss_edge_cases_cpu.py (the preconditions that make each case prove something, and the package's torch path on the
same cases) and tests/golden/make_golden_yolox_loss.py (the dense image of the A = 4116 fixture).  Plain helper module: no fixtures;
builders are cached and their arrays are read-only.  Seeds were searched when the cases were written and are fixed here; the CPU test
asserts the margins they were searched for.

What the cases are placed on (kThreads = 256 lanes, kTopK = 10):

    match_kernel     lane t walks anchors t, t + 256, ...; per lane the 10 largest IoUs and the 10 lowest (cost, anchor) pairs by
                     insertion, the tail evicted once a list is full.  ``dense_image``: 448 x 448, A = 4116, 16 - 17 anchors per lane,
                     large gts, good predictions scattered over the whole box: most lanes hold more than 10 candidates and winners come
                     late in a lane's walk.
    ties             "the lowest index wins": ``better()`` across lanes and waves, the strict ``>`` of one lane's cost list, the strict
                     ``<`` of resolve_kernel.  ``tie_case``: tied anchors one lane, one wave and one list position apart;
                     ``duplicate_case``: a label row written twice.
    block_best       lanes without any candidate, fewer candidates than 10: ``small_case`` with A = 7 and A = 257.
    finish_kernel    partial j of thread t: j = t, t + 256, ...: ``partials_case`` has 258 partials.
    iou_loss<kGrad>  equal edges (0.5 / 0.5), no overlap (only GIoU has a gradient), through a given assignment: ``pair_case``.
    scale[4]         ``WEIGHTS``: one uneven weight vector and the four unit vectors.
"""
import os
import sys
from functools import lru_cache

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import yolox_loss_ref as R  # noqa: E402

MARGIN = 1e-3
LANES = 256            # kThreads of csrc/yolox_loss.hip
TOPK = 10              # kTopK
STRIDES = (8, 16, 32)
FL = dict(fl_alpha=0.25, fl_gamma=2.0)
# loss_iou, loss_conf, loss_l1, loss_cls: uneven and of both signs, then every loss alone
WEIGHTS = ((0.5, 2.0, -1.5, 3.0), (1.0, 0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 0.0), (0.0, 0.0, 1.0, 0.0), (0.0, 0.0, 0.0, 1.0))


def _frozen(a):
    a.setflags(write=False)
    return a


def off_lattice(v):
    """Two decimals, never within 0.1 px of an anchor centre (multiples of 4 px)."""
    return np.round(v) + 0.37


def T(a, dtype=None):
    """A read-only array as a tensor of its own."""
    t = torch.tensor(np.asarray(a))
    return t if dtype is None else t.to(dtype)


def anchors_of(case, dtype=torch.float64):
    return R.anchor_table(case["hw"], case["strides"], dtype)


def _case(name, hw, strides, raw, labels, **opts):
    full = dict(iou_loss_type="iou", cls_loss_type="bce", use_l1=False, **FL)
    full.update(opts)
    return dict(name=name, hw=[tuple(r) for r in hw], strides=tuple(strides), raw=_frozen(np.ascontiguousarray(raw, np.float32)),
                labels=_frozen(np.ascontiguousarray(labels, np.float32)), opts=full)


def _random_rows(rng, A, C):
    return np.concatenate([rng.normal(0, 0.5, (A, 4)), rng.normal(-1.0, 1.5, (A, 1 + C))], 1).astype(np.float32)


def _good_rows(raw, an, where, gt, rng):
    """The rows ``where`` predict ``gt`` well: centre within 0.12 strides, size within 15 %, objectness + 2, the gt's class + 3."""
    k, cx, cy, w, h = gt
    n = int(where.sum())
    raw[where, 0] = cx / an[where, 2] - an[where, 0] + rng.normal(0, 0.12, n)
    raw[where, 1] = cy / an[where, 2] - an[where, 1] + rng.normal(0, 0.12, n)
    raw[where, 2] = np.log(w / an[where, 2]) + rng.normal(0, 0.15, n)
    raw[where, 3] = np.log(h / an[where, 2]) + rng.normal(0, 0.15, n)
    raw[where, 4] += 2.0
    raw[where, 5 + int(k)] += 3.0


def _labels(images, G):
    labels = np.zeros((len(images), G, 5), np.float32)
    for b, gts in enumerate(images):
        assert len(gts) <= G
        for j, gt in enumerate(gts):
            labels[b, j] = gt
    return labels


# --------------------------------------------------------------------------------------------------------- margins and lane facts
def image_margins(raw, anchors, gts):
    """One image, ``gts`` [n >= 1, 5]: (the fp64 restatement's ``assign_image`` result with its margins, e_cost = the largest distance
    of the fp32 restatement's candidate costs from it in units of 1 + 1e-3 |cost|)."""
    raw, anchors, gts = (T(t) for t in (raw, anchors, gts))
    res = R.assign_image(raw.double(), anchors.double(), gts.double())
    res32 = R.assign_image(raw.float(), anchors.float(), gts.float())
    finite = torch.isfinite(res["cost"])
    e_cost = float(((res32["cost"].double() - res["cost"])[finite].abs() / (1 + 1e-3 * res["cost"][finite].abs())).max()) if finite.any() else 0.0
    return res, e_cost


def lane_facts(res):
    """What one workgroup of match_kernel meets in an image (``res`` of ``assign_image``): full_lanes = lanes (anchor % 256) holding more
    than 10 candidates, max_per_lane, late_chosen = chosen anchors that are the 11th or a later candidate of their lane's walk,
    late_top_iou = the same among the anchors that form some gt's 10 largest IoUs."""
    cand = res["cand"].numpy()
    rank, seen = np.zeros(cand.shape[0], np.int64), np.zeros(LANES, np.int64)
    for a in np.flatnonzero(cand):
        rank[a] = seen[a % LANES]
        seen[a % LANES] += 1
    late = cand & (rank >= TOPK)
    chosen = res["chosen"].any(0).numpy()
    top = np.zeros_like(cand)
    for j in range(res["iou"].shape[0]):
        iou = torch.where(res["cand"], res["iou"][j], torch.full_like(res["iou"][j], -1.0))
        top[iou.topk(min(TOPK, int(cand.sum()))).indices.numpy()] = True
    return dict(full_lanes=int((seen > TOPK).sum()), max_per_lane=int(seen.max()), late_chosen=int((chosen & late).sum()),
                late_top_iou=int((top & late).sum()), dynamic_k=max(res["dynamic_k"]), conflicts=int((res["times"] > 1).sum()))


# ------------------------------------------------------------------------------------------------------------- the dense image
DENSE_SIZE, DENSE_C, DENSE_G = 448, 3, 8
DENSE_HW = [(DENSE_SIZE // s, DENSE_SIZE // s) for s in STRIDES]          # 56^2 + 28^2 + 14^2 = 4116 anchors
DENSE_KINDS = ("empty", "single", "crowd")
DENSE_SCATTER = 0.03


@lru_cache(maxsize=None)
def dense_image(kind, seed):
    """One 448 x 448 image with C = 3 -> (raw f32[4116,8], gts f32[n,5]).  "empty": no gt.  "single": one large gt.  "crowd": five large
    gts (0.6 - 0.9 of the image), the first one's twin (moved by 2 - 3 px, another class) behind it, and a small one.  Every anchor
    inside a large gt predicts it well with probability 0.03, wherever in the box it lies; levels 1 and 2 start at anchor 3136, behind
    12 or more level-0 anchors of every lane, so such winners come late in a lane's walk."""
    rng = np.random.default_rng([seed, DENSE_KINDS.index(kind)])
    an = R.anchor_table(DENSE_HW, STRIDES, torch.float32).numpy()
    A, S = an.shape[0], DENSE_SIZE

    def gt(lo, hi):
        w, h = rng.uniform(lo, hi, 2) * S
        return [rng.integers(0, DENSE_C), off_lattice(rng.uniform(0.35, 0.65) * S), off_lattice(rng.uniform(0.35, 0.65) * S), off_lattice(w), off_lattice(h)]

    gts, good = [], []
    if kind == "single":
        gts, good = [gt(0.6, 0.9)], [0]
    elif kind == "crowd":
        gts = [gt(0.6, 0.9) for _ in range(5)]
        twin = list(gts[0])
        twin[0] = (twin[0] + 1) % DENSE_C
        twin[1], twin[2] = twin[1] + 2.0, twin[2] + 3.0
        gts.insert(1, twin)
        gts.append(gt(0.08, 0.15))
        good = [0, 1, 2, 3, 4, 5]
    raw = _random_rows(rng, A, DENSE_C)
    xc, yc = an[:, 0] * an[:, 2] + 0.5 * an[:, 2], an[:, 1] * an[:, 2] + 0.5 * an[:, 2]
    for j in good:
        _, cx, cy, w, h = gts[j]
        inside = (np.abs(xc - cx) < 0.5 * w) & (np.abs(yc - cy) < 0.5 * h) & (rng.uniform(size=A) < DENSE_SCATTER)
        _good_rows(raw, an, inside, gts[j], rng)
    return _frozen(raw), _frozen(np.array(gts, np.float32).reshape(-1, 5))


def dense_batch(seed):
    """The three kinds of one seed as a batch: (raw f32[3,4116,8], labels f32[3,8,5])."""
    images = [dense_image(kind, seed) for kind in DENSE_KINDS]
    return np.stack([raw for raw, _ in images]), _labels([gts for _, gts in images], DENSE_G)


def dense_ok(raw, gts):
    """Whether a dense image has every margin above MARGIN > 16 e_cost and the lane facts the dense cases are there for."""
    res, e_cost = image_margins(raw, R.anchor_table(DENSE_HW, STRIDES), gts)
    facts = lane_facts(res)
    ok = min(res["margins"].values()) > MARGIN > 16 * e_cost
    if len(gts) > 1:
        ok = ok and facts["full_lanes"] >= 128 and facts["late_chosen"] >= 5 and facts["late_top_iou"] >= 5 and facts["conflicts"] > 0
    return ok, res, e_cost, facts


# ----------------------------------------------------------------------------------------------- more partials than threads
PARTIALS_SEEDS = (16, 25, 37, 41)         # crowd images that pass ``dense_ok``
PARTIALS_B = 16


@lru_cache(maxsize=None)
def partials_case():
    """B = 16 at A = 4116: 258 partial sums for finish_kernel's 256 threads.  Images 0 - 3 are dense crowds, the other twelve have no
    label and random rows (objectness alone)."""
    rng = np.random.default_rng(77)
    crowd = [dense_image("crowd", s) for s in PARTIALS_SEEDS]
    raw = np.stack([r for r, _ in crowd] + [_random_rows(rng, crowd[0][0].shape[0], DENSE_C) for _ in range(PARTIALS_B - len(crowd))])
    labels = _labels([g for _, g in crowd] + [[]] * (PARTIALS_B - len(crowd)), DENSE_G)
    return _case("partials", DENSE_HW, STRIDES, raw, labels, iou_loss_type="iou", cls_loss_type="bce", use_l1=True)


# ------------------------------------------------------------------------------------------------------------------ exact ties
TIE_GRID, TIE_STRIDE, TIE_C = 64, 8, 3
TIE_BLOCK = (21, 30)          # row, column of the centre block's first anchor
TIE_GT = (1.0, 8 * 32 + 4 + 0.37, 8 * 23 + 4 + 0.37, 100.37, 100.37)
# The gt's centre block is 5 x 5 anchors; anchor (r, c) of it has index (21 + r) 64 + 30 + c, lane (index % 256) and wave ((21 + r) % 4).
# members: the twelve tied anchors; k: dynamic_k, so that the k-th and (k + 1)-th lowest members straddle the decision; iou: of the
# shared box, 10 iou = k + 0.5.  "lane": the pair is one lane apart.  "wave": 64 apart, the same lane position of the next wave.
# "list": two anchors share a lane only in rows 0 and 4 of the block, 256 apart, so at most five members are not above the lower one:
# it is the 3rd, and a lane list that held the pair in the other order would hand the 4th out in its place.
TIE_VARIANTS = {
    "lane": dict(members=[(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (1, 1), (1, 2), (1, 3), (2, 1), (3, 3), (4, 0)], k=7, gap=1),
    "wave": dict(members=[(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 0), (1, 1), (2, 1), (2, 2), (2, 3), (3, 0), (4, 2)], k=7, gap=64),
    "list": dict(members=[(0, 0), (0, 1), (0, 2), (0, 3), (0, 4), (1, 1), (1, 3), (2, 0), (2, 4), (3, 2), (4, 2), (4, 4)], k=3, gap=256),
}


def tie_members(variant):
    return sorted((TIE_BLOCK[0] + r) * TIE_GRID + TIE_BLOCK[1] + c for r, c in TIE_VARIANTS[variant]["members"])


@lru_cache(maxsize=None)
def tie_case(variant):
    """One level of 64 x 64 anchors at stride 8 (A = 4096: 16 per lane), one gt.  Twelve anchors of its centre block decode to the same
    box bit for bit (raw + shift is the same half-integer, the size logits are shared) and share objectness and class logits: twelve
    equal costs, the lowest of the image.  The box lies inside the gt and has (k + 0.5) / 10 of its area."""
    v = TIE_VARIANTS[variant]
    rng = np.random.default_rng([5, sorted(TIE_VARIANTS).index(variant)])
    hw = [(TIE_GRID, TIE_GRID)]
    an = R.anchor_table(hw, [TIE_STRIDE], torch.float32).numpy()
    raw = _random_rows(rng, an.shape[0], TIE_C)
    side = np.float32(np.log(np.sqrt((v["k"] + 0.5) / TOPK) * TIE_GT[3] / TIE_STRIDE))
    for a in tie_members(variant):
        raw[a] = [32.5 - an[a, 0], 23.5 - an[a, 1], side, side, 3.0, -3.0, 3.0, -3.0]
    return _case(f"tie_{variant}", hw, [TIE_STRIDE], raw[None], _labels([[TIE_GT]], 2), iou_loss_type="giou", cls_loss_type="bce", use_l1=True)


# ---------------------------------------------------------------------------------------------- scenes with predictions near the gts
def _near_scene(size, strides, C, images, good, rng, force_last=False):
    """Random rows; the anchors within 2.5 strides of a ``good`` (image, row) gt predict it well with probability 0.7."""
    H, W = size
    hw = [(max(H // s, 1), max(W // s, 1)) for s in strides]
    an = R.anchor_table(hw, strides, torch.float32).numpy()
    A = an.shape[0]
    raw = np.stack([_random_rows(rng, A, C) for _ in images])
    xc, yc = an[:, 0] * an[:, 2] + 0.5 * an[:, 2], an[:, 1] * an[:, 2] + 0.5 * an[:, 2]
    for b, j in good:
        _, cx, cy, w, h = images[b][j]
        near = (np.abs(xc - cx) < 2.5 * an[:, 2]) & (np.abs(yc - cy) < 2.5 * an[:, 2]) & (rng.uniform(size=A) < 0.7)
        if force_last:
            near[-1] = True
        _good_rows(raw[b], an, near, images[b][j], rng)
        if force_last:         # the last anchor predicts the gt within 3 %, not exactly (|x| of the L1 loss has no gradient at 0)
            k, cx, cy, w, h = images[b][j]
            raw[b, -1, :4] = [cx / an[-1, 2] - an[-1, 0] + 0.02, cy / an[-1, 2] - an[-1, 1] - 0.02, np.log(w / an[-1, 2]) + 0.03, np.log(h / an[-1, 2]) - 0.03]
    return hw, raw


def _rand_gt(rng, size, C, lo, hi, c_lo=0.3, c_hi=0.7):
    H, W = size
    w, h = rng.uniform(lo, hi, 2) * (W, H)
    return [float(rng.integers(0, C)), off_lattice(rng.uniform(c_lo, c_hi) * W), off_lattice(rng.uniform(c_lo, c_hi) * H), off_lattice(w), off_lattice(h)]


DUPLICATE_SEED = 0
DUPLICATE_ROWS = {0: (0, 2), 1: (0, 1)}        # image: (the row, its copy)


@lru_cache(maxsize=None)
def duplicate_case(seed=None):
    """160 x 160, A = 525.  Image 0: rows g0, g1, g0 again, g2.  Image 1: one gt, written twice.  Every anchor the first copy chooses the
    second chooses too, at equal cost."""
    rng = np.random.default_rng([6, DUPLICATE_SEED if seed is None else seed])
    size, C = (160, 160), 3
    g = [_rand_gt(rng, size, C, 0.2, 0.5) for _ in range(4)]
    g[2][1:3] = [g[0][1] + 6.0, g[0][2] - 5.0]           # g2 overlaps g0: anchors that more than one DIFFERENT gt chooses
    images = [[g[0], g[1], g[0], g[2]], [g[3], g[3]]]
    hw, raw = _near_scene(size, STRIDES, C, images, [(0, 0), (0, 1), (0, 3), (1, 0)], rng)
    return _case("duplicate", hw, STRIDES, raw, _labels(images, 5), iou_loss_type="giou", cls_loss_type="focal", use_l1=True)


SMALL_SEEDS = {"tiny": 0, "ragged": 0}
SMALL_LAYOUT = {"tiny": dict(size=(16, 24), strides=(8, 16)),          # hw (2, 3), (1, 1): A = 7
                "ragged": dict(size=(128, 128), strides=(8, 128))}     # hw (16, 16), (1, 1): A = 257, anchor 256 alone in its workgroup


@lru_cache(maxsize=None)
def small_case(kind, seed=None):
    """"tiny": A = 7, 249 lanes without an anchor, fewer candidates than 10.  "ragged": A = 257 = 256 + 1; the last anchor, the only one
    of lane 0's second step and of the second workgroup of the per-anchor kernels, predicts the first gt of both images well."""
    lay = SMALL_LAYOUT[kind]
    rng = np.random.default_rng([7, sorted(SMALL_LAYOUT).index(kind), SMALL_SEEDS[kind] if seed is None else seed])
    size, C = lay["size"], 3
    images = [[_rand_gt(rng, size, C, 0.5, 0.9, 0.4, 0.6)], [_rand_gt(rng, size, C, 0.5, 0.9, 0.4, 0.6), _rand_gt(rng, size, C, 0.3, 0.5)], []]
    hw, raw = _near_scene(size, lay["strides"], C, images, [(0, 0), (1, 0)], rng, force_last=kind == "ragged")
    return _case(kind, hw, lay["strides"], raw, _labels(images, 3), iou_loss_type="iou", cls_loss_type="focal", use_l1=True)


# ------------------------------------------------------------------------------------------------------- a hand-made assignment
PAIR_HW = [(16, 16), (8, 8), (4, 4)]
PAIR_C = 3
# name: the gt (dx, dy, w, h) in strides against a prediction of one stride squared at the origin.  Every value is a multiple of 1/4
# stride: exact in fp32 and fp64.
PAIR_KINDS = {
    "identical": (0.0, 0.0, 1.0, 1.0),
    "left_edge": (0.5, 0.25, 2.0, 2.5),          # gl == pl, the prediction inside otherwise
    "top_edge_inside": (0.25, 0.5, 2.5, 2.0),    # gt == pt, the prediction inside otherwise
    "touching": (1.5, 0.25, 2.0, 1.5),           # pr == gl: no overlap
    "corner_touch": (1.0, 1.0, 1.0, 1.0),        # pr == gl and pb == gt
    "disjoint": (3.0, -2.0, 1.5, 2.0),
    "same_centre": (0.0, 0.0, 2.0, 0.5),         # same centre, other size: neither contains the other
}
PAIR_OPTIONS = [dict(iou_loss_type=i, cls_loss_type=c, use_l1=l) for i in ("iou", "giou") for c in ("bce", "focal") for l in (False, True)]


@lru_cache(maxsize=None)
def pair_case():
    """B = 2, A = 336 on three strides.  Every pair of PAIR_KINDS once per stride, alternating between the images, on every second anchor
    of a level's first rows (background in between and behind). Foreground rows have size logits 0 (w = h = stride) and centre offsets of +- 0.5: lattice values, which
    fp32 and fp64 decode exactly.  -> case with ``matched_gt`` i32[2,336], ``pairs`` [(kind, image, anchor, row)]."""
    rng = np.random.default_rng(8)
    an = R.anchor_table(PAIR_HW, STRIDES, torch.float32).numpy()
    A = an.shape[0]
    raw = np.stack([_random_rows(rng, A, PAIR_C) for _ in range(2)])
    matched = np.full((2, A), -1, np.int32)
    level_start = np.cumsum([0] + [h * w for h, w in PAIR_HW])
    images, pairs = [[], []], []
    for lvl, s in enumerate(STRIDES):
        for n, (kind, (dx, dy, w, h)) in enumerate(PAIR_KINDS.items()):
            b, a = (n + lvl) % 2, level_start[lvl] + 1 + 2 * n
            off = (0.5, -0.5) if n % 2 else (-0.5, 0.5)
            raw[b, a, :4] = [off[0], off[1], 0.0, 0.0]
            px, py = (an[a, 0] + off[0]) * s, (an[a, 1] + off[1]) * s
            matched[b, a] = len(images[b])
            pairs.append((kind, b, int(a), len(images[b])))
            images[b].append([float(n % PAIR_C), px + dx * s, py + dy * s, w * s, h * s])
    case = _case("pairs", PAIR_HW, STRIDES, raw, _labels(images, max(len(i) for i in images)))
    case.update(matched_gt=_frozen(matched), pairs=pairs)
    return case


# ------------------------------------------------------------------------------------------------------------------- yardstick
def restatement(case, dtype, weights=(1.0, 1.0, 1.0, 1.0), opts=None, matched_gt=None):
    """tests/yolox_loss_ref.py on a case in ``dtype`` -> (losses {key: float}, gradient of sum_k weights[k] loss_k by raw as f64
    ndarray, info).  ``matched_gt``: a given assignment, whose class targets are ``pair_iou`` of the matched pairs in ``dtype``."""
    anchors = anchors_of(case, dtype)
    leaf = T(case["raw"], dtype).requires_grad_(True)
    labels = T(case["labels"], dtype)
    assignment = None
    if matched_gt is not None:
        m = T(matched_gt).long()
        box = R.decode(leaf.detach(), anchors)
        iou = torch.stack([R.pair_iou(labels[b, :, 1:5], box[b]).gather(0, m[b].clamp(min=0)[None])[0] for b in range(m.shape[0])])
        assignment = (m, torch.where(m >= 0, iou, torch.zeros_like(iou)))
    losses, info = R.losses(leaf, anchors, labels, assignment=assignment, **(case["opts"] if opts is None else dict(FL, **opts)))
    sum(w * losses[k] for w, k in zip(weights, R.KEYS)).backward()
    return {k: float(v.detach()) for k, v in losses.items()}, leaf.grad.double().numpy().copy(), info


_YARD = {}


def yardstick(case, weights=(1.0, 1.0, 1.0, 1.0), opts=None, matched_gt=None):
    """The fp64 restatement of a case and the fp32 restatement's distance from it, computed once per (case, weights, options) and never
    changed -> dict l64 {key: float}, g64 f64[B,A,5+C], e_loss {key: float}, e_grad (largest element distance), e_grad_each (per
    element), matched_gt, matched_iou, num_fg, num_gt of the fp64 run."""
    key = (case["name"], tuple(weights), None if opts is None else tuple(sorted(opts.items())))
    if key not in _YARD:
        l64, g64, info = restatement(case, torch.float64, weights, opts, matched_gt)
        l32, g32, info32 = restatement(case, torch.float32, weights, opts, matched_gt)
        assert torch.equal(info["matched_gt"], info32["matched_gt"]), case["name"]
        _YARD[key] = dict(l64=l64, g64=_frozen(g64), e_loss={k: abs(l32[k] - l64[k]) for k in R.KEYS}, e_grad=float(np.abs(g32 - g64).max()), e_grad_each=_frozen(np.abs(g32 - g64)),
                          matched_gt=_frozen(info["matched_gt"].numpy().astype(np.int32)), matched_iou=_frozen(info["matched_iou"].numpy().copy()),
                          num_fg=_frozen(info["num_fg"].numpy().astype(np.int32)), num_gt=_frozen(info["num_gt"].numpy().astype(np.int32)))
    return _YARD[key]


def ulp32(v):
    return np.spacing(np.abs(np.asarray(v, np.float64)).astype(np.float32)).astype(np.float64)


def fixture_case(name):
    """A fixture of tests/golden/make_golden_yolox_loss.py in the form of the cases above."""
    z = np.load(os.path.join(HERE, "golden", f"yolox_loss_golden_{name}.npz"))
    return _case(f"fixture_{name}", z["hw"].tolist(), z["strides"].tolist(), z["raw"], z["labels"], iou_loss_type=str(z["iou_loss_type"]),
                 cls_loss_type=str(z["cls_loss_type"]), use_l1=bool(z["use_l1"]), fl_alpha=float(z["fl_alpha"]), fl_gamma=float(z["fl_gamma"]))
