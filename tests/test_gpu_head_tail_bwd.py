"""The backward of the geometry head's tail on the HIP kernels (csrc/head_tail_bwd.hip, hip_layers.HeadTail) against fp64 autograd on
the CPU (tests/head_tail_bwd_ref.py).

The bar, per tensor: max|hip - ref64| <= 2 max|torch fp32 on the CPU - ref64| + 1 ulp of max|ref64| (tests/mlp_bwd_ref.py); every test
prints its worst ratio to that bar.  The data gradient and the weight / bias gradient are also held EXACT on integer lattices and
one-hot locator probes.

Measured on an MI355X, error / bar:
    case (B, hw, K, classes, mask)    d_out   dfeat   dW      db      |  forward, printed only:  out     pnp_in  planes
        (1, 256, 128, 1, single)      0.38    0.44    0.40    0.15    |                          0.22    1.00    0.41
        (2, 512, 256, 2, double)      0.68    0.43    0.28    0.15    |                          0.72    0.52    0.98
        (5, 256, 128, 3, double)      0.16    0.30    0.33    0.10    |                          0.41    0.23    0.41
        (3, 512, 128, 3, single)      0.52    0.48    0.35    0.11    |                          0.46    0.28    0.20
        (2, 768, 256, 2, double)      0.90    0.45    0.36    0.14    |                          1.06    0.79    1.09
    each gradient source alone (g_pnp_in, g_planes, g_out), worst                 0.78
    the small GDRN_DoubleMask through forward_loss + backward: loss 0.16, out_layer.weight 0.49, out_layer.bias 0.27, the trunk's and
    the backbone's parameters 0.15 .. 0.47, Patch-PnP's (PyTorch's graph behind the tail) 0.36 .. 0.90
The forward columns are the inference kernels' results, which HeadTail returns bit for bit (tested below): gdrnpp_linear_f32_split_grouped
at a depth of 256 sits at the bar itself on these operands (1.06 / 1.09 in the last case, eight pixels per ROI four times further out), as
DESIGN.md's figures for the six-product kernel per depth say.  The bar is asserted on the backward, which is what this file tests.
"""
import copy
import itertools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_tail_bwd_ref as R  # noqa: E402
from mlp_bwd_ref import bar, ratio_to_bar  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN = float("nan")
PITCH = 128


def _tail(t, pad=4096):
    """``t`` as the head of a flat device allocation with NaN behind its end: a read past the tensor poisons the result."""
    t = t.contiguous()
    buf = torch.full((t.numel() + pad,), NAN, device=DEV, dtype=t.dtype) if t.is_floating_point() else torch.zeros(t.numel() + pad, device=DEV, dtype=t.dtype)
    buf[:t.numel()] = t.reshape(-1).to(DEV)
    return buf[:t.numel()].view(t.shape)


def _pitched(d, pitch=PITCH, fill=NAN):
    """[B,hw,n] -> device f32[B hw, pitch] with ``fill`` in the padding columns and NaN behind the end."""
    B, hw, n = d.shape
    full = torch.full((B * hw, pitch), fill)
    full[:, :n] = d.reshape(B * hw, n)
    return _tail(full)


def _dev_case(case):
    t = R.make_inputs(case)
    sel32 = t["sel"].to(torch.int32)
    return t, {k: (_tail(v) if isinstance(v, torch.Tensor) else v) for k, v in dict(t, sel=sel32).items()}


def _hip_forward(hip_layers, d, grad=()):
    """HeadTail on a device case -> (leaves feat, weight, bias, out2d, pnp_in, planes)."""
    B, hw, K = d["feat"].shape
    leaves = [d[k].detach().clone().requires_grad_(k in grad) for k in ("feat", "weight", "bias")]
    side = int(hw ** 0.5) if int(hw ** 0.5) ** 2 == hw else 16
    coord = d["coord2d"].view(B, 2, side, hw // side)
    out = hip_layers.HeadTail.apply(leaves[0].view(B * hw, K), leaves[1].view(-1, K, 1, 1), leaves[2], d["cls_rows"], d["sel"], coord,
                                    d["extents"], d["double_mask"])
    return leaves, out


def _loss(d, out2d, pnp_in, planes):
    n = d["g_out"].shape[-1]
    B, hw, _ = d["feat"].shape
    return (pnp_in * d["g_pnp"]).sum() + (planes * d["g_planes"]).sum() + (out2d[:, :n] * d["g_out"].view(B * hw, n)).sum()


@pytest.fixture
def train_kernels():
    from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers

    hip_layers.set_train_kernels(True)
    yield hip_layers
    hip_layers.set_train_kernels(False)


# ---- the two products, exact ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_products_are_exact_on_integer_operands(hip, case):
    B, hw, K, C, double, sel = case
    rows = R.class_rows(C, double)
    n, out_rows = rows.shape[1], rows.numel()
    slots, _ = R.wgrad_slots(B, hw, K)
    assert hip.load().gdrnpp_grouped_linear_wgrad_f32_workspace_bytes(B, hw, K, n) == B * slots * (n * K + 128) * 8
    assert hip.load().gdrnpp_grouped_linear_wgrad_f32_workspace_bytes(B, hw + 64, K, n) == 0
    assert hip.load().gdrnpp_grouped_linear_wgrad_f32_workspace_bytes(B, hw, K + 32, n) == 0
    sel_t = torch.tensor(sel)
    sel_d, rows_d = _tail(sel_t.to(torch.int32)), _tail(rows)
    for kind, (d_out, feat, w) in (("lattice", R.lattice(case)), ("locator", R.locator(case))):
        dd, fd, wd = _pitched(d_out), _tail(feat.view(B * hw, K)), _tail(w)
        want = R.restated_dinput(d_out, w, sel_t)
        got = hip.grouped_linear_dinput(dd, wd, sel_d, hw).cpu().double().view(B, hw, K)
        assert torch.equal(got, want), f"{kind} dinput: {(got != want).sum().item()} wrong of {got.numel()}, first {(got != want).nonzero()[:4].tolist()}"
        if kind == "locator":      # dfeat[b, r] IS row r % n of the slice of its ROI
            assert torch.equal(got[:, :n], w.double()[sel_t])
        want_w, want_b = R.restated_wgrad(d_out, feat, sel_t, rows, out_rows)
        assert float(want_w.abs().max()) < 2 ** 24
        dw, db = hip.grouped_linear_wgrad(dd, fd, sel_d, rows_d, C, out_rows, hw)
        bad = (dw.cpu().double() != want_w).nonzero()
        assert len(bad) == 0, f"{kind} dW: {len(bad)} wrong of {dw.numel()}, first {bad[:4].tolist()}"
        assert torch.equal(db.cpu().double(), want_b), kind
        for c in set(range(C)) - set(sel):      # a class without a ROI: exactly zero, written (the gradients are torch.empty)
            assert not dw[rows[c].to(DEV)].any() and not db[rows[c].to(DEV)].any()
        # either alone: the same bits; neither: nothing
        only_w, none_b = hip.grouped_linear_wgrad(dd, fd, sel_d, rows_d, C, out_rows, hw, want=(True, False))
        none_w, only_b = hip.grouped_linear_wgrad(dd, fd, sel_d, rows_d, C, out_rows, hw, want=(False, True))
        assert none_b is None and none_w is None and torch.equal(only_w, dw) and torch.equal(only_b, db)
        assert hip.grouped_linear_wgrad(dd, fd, sel_d, rows_d, C, out_rows, hw, want=(False, False)) == (None, None)


def test_selector_out_of_range_poisons_its_roi_only(hip):
    case = R.CASES[2]
    B, hw, K, C, double, _ = case
    rows = R.class_rows(C, double)
    n, out_rows = rows.shape[1], rows.numel()
    d_out, feat, w = R.lattice(case, seed=9)
    sel = torch.tensor([2, C, 0, -1, 2])
    keep = (sel >= 0) & (sel < C)
    sel_d, rows_d, dd = _tail(sel.to(torch.int32)), _tail(rows), _pitched(d_out)
    got = hip.grouped_linear_dinput(dd, _tail(w), sel_d, hw).cpu().view(B, hw, K)
    assert torch.isnan(got[~keep]).all()
    assert torch.equal(got[keep].double(), R.restated_dinput(d_out[keep], w, sel[keep]))
    dw, db = hip.grouped_linear_wgrad(dd, _tail(feat.view(B * hw, K)), sel_d, rows_d, C, out_rows, hw)
    want_w, want_b = R.restated_wgrad(d_out[keep], feat[keep], sel[keep], rows, out_rows)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    assert torch.equal(dw.cpu().double(), want_w) and torch.equal(db.cpu().double(), want_b)


# ---- random operands -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_gradients_meet_the_bar(hip, train_kernels, case):
    t, d = _dev_case(case)
    ref64, ref32 = R.references(case)
    B, hw, K = t["feat"].shape
    n = t["g_out"].shape[-1]
    (feat, weight, bias), (out2d, pnp_in, planes) = _hip_forward(train_kernels, d, grad=("feat", "weight", "bias"))
    assert out2d.shape == (B * hw, PITCH) and pnp_in.shape == (B, hw, 96) and planes.shape == (n - 65, B, hw)
    _loss(d, out2d, pnp_in, planes).backward()
    d_out = hip.head_tail_backward(out2d.detach(), d["extents"], d["double_mask"], d["g_pnp"], d["g_planes"], _pitched(t["g_out"]))
    assert not d_out[:, n:].any()                       # the padding columns are written 0, whatever g_out holds there
    got = dict(out=out2d.detach()[:, :n], pnp_in=pnp_in.detach()[..., :69], planes=planes.detach(), d_out=d_out[:, :n], dfeat=feat.grad,
               dW=weight.grad, db=bias.grad)
    assert not pnp_in.detach()[..., 69:].any()
    ratios = {k: ratio_to_bar(v, ref64[k], ref32[k]) for k, v in got.items()}
    print("head_tail_bwd", R.case_id(case), " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert all(torch.isfinite(v).all() for v in got.values())
    # the bar holds the backward.  out, pnp_in and planes are the inference kernels' results, bit for bit (the test below): their ratios
    # are printed, not asserted — the six-product GEMM at a depth of 256 sits at the bar itself (the docstring has the figures)
    assert max(ratios[k] for k in ("d_out", "dfeat", "dW", "db")) <= 1.0, ratios
    # the softmax saturates somewhere: a probability above 0.999, and gradients that vanish with it
    assert float(pnp_in.detach()[..., 5:69].max()) > 0.999
    # the d_out autograd's backward formed is the one of the direct call: two calls, equal bits
    w_sliced = d["weight"][d["cls_rows"]].contiguous()
    assert torch.equal(hip.grouped_linear_dinput(d_out, w_sliced, d["sel"], hw).view(B, hw, K), feat.grad)
    again = hip.head_tail_backward(out2d.detach(), d["extents"], d["double_mask"], d["g_pnp"], d["g_planes"], _pitched(t["g_out"], fill=0.0))
    assert torch.equal(again, d_out)


def test_tail_adjoint_sources_and_null_inputs(hip, train_kernels):
    """Each gradient source alone meets the bar of its own autograd run; an absent source is not read (its place holds NaN)."""
    case = R.CASES[1]
    t, d = _dev_case(case)
    with torch.no_grad():
        _, (out2d, _, _) = _hip_forward(train_kernels, d)
    n = t["g_out"].shape[-1]
    zeros = {k: torch.zeros_like(t[k]) for k in ("g_pnp", "g_planes", "g_out")}
    worst = 0.0
    for keep in ("g_pnp", "g_planes", "g_out"):
        only = dict(t, **{k: v for k, v in zeros.items() if k != keep})
        r64, r32 = R.autograd_tail(only, torch.float64)["d_out"], R.autograd_tail(only, torch.float32)["d_out"]
        kw = {"g_pnp_in" if keep == "g_pnp" else keep: _pitched(t[keep]) if keep == "g_out" else d[keep]}
        got = hip.head_tail_backward(out2d, d["extents"], d["double_mask"], **kw)
        assert torch.isfinite(got).all() and not got[:, n:].any()
        worst = max(worst, ratio_to_bar(got[:, :n], r64, r32))
    print("head_tail_bwd sources alone: worst ratio %.3f" % worst)
    assert worst <= 1.0
    # g_planes / g_out alone do not read the forward's result: NaN in its place changes nothing
    poison = torch.full_like(out2d, NAN)
    a = hip.head_tail_backward(poison, d["extents"], d["double_mask"], g_planes=d["g_planes"], g_out=_pitched(t["g_out"]))
    b = hip.head_tail_backward(out2d, d["extents"], d["double_mask"], g_planes=d["g_planes"], g_out=_pitched(t["g_out"]))
    assert torch.equal(a, b)
    none = hip.head_tail_backward(out2d, d["extents"], d["double_mask"])
    assert not none.any()


# ---- determinism -----------------------------------------------------------------------------------------------------------------
def test_class_rows_do_not_depend_on_other_classes_rois(hip):
    B, hw, K, C = 2, 512, 128, 2
    rows = R.class_rows(C, True)
    n, out_rows = rows.shape[1], rows.numel()
    gen = torch.Generator().manual_seed(77)
    d_out, feat = torch.randn(3, hw, n, generator=gen), torch.randn(3, hw, K, generator=gen)
    rows_d = _tail(rows)

    def run(idx, sel):
        return hip.grouped_linear_wgrad(_pitched(d_out[idx]), _tail(feat[idx].reshape(-1, K)), _tail(torch.tensor(sel, dtype=torch.int32)), rows_d, C,
                                        out_rows, hw)

    dw2, db2 = run([0, 2], [0, 0])
    dw3, db3 = run([0, 1, 2], [0, 1, 0])
    again = run([0, 1, 2], [0, 1, 0])
    assert torch.equal(dw3, again[0]) and torch.equal(db3, again[1])
    r0 = rows[0].to(DEV)
    assert torch.equal(dw2[r0], dw3[r0]) and torch.equal(db2[r0], db3[r0])
    assert dw3[rows[1].to(DEV)].any() and not dw2[rows[1].to(DEV)].any()


# ---- gradient subsets ----------------------------------------------------------------------------------------------------------------
def test_gradient_subsets_keep_bits_and_skip_launches(hip, train_kernels):
    case = R.CASES[1]
    _, d = _dev_case(case)
    names = ("feat", "weight", "bias")

    def run(grad):
        timer = hip.LaunchTimer()
        hip.set_launch_timer(timer)
        try:
            leaves, out = _hip_forward(train_kernels, d, grad=grad)
            _loss(d, *out).backward()
        finally:
            hip.set_launch_timer(None)
        return {k: leaf.grad for k, leaf in zip(names, leaves)}, [r[0] for r in timer.records]

    full, kinds = run(names)
    assert kinds.count("mfma_f32:grouped_wgrad") == 1 and kinds.count("mfma_f32:grouped_dinput") == 1 and kinds.count("hbm:head_tail_bwd") == 1
    for r in range(1, 3):
        for grad in itertools.combinations(names, r):
            part, kinds = run(grad)
            for k in names:
                assert (part[k] is None) == (k not in grad), (grad, k)
                if k in grad:
                    assert torch.equal(part[k], full[k]), (grad, k)
            assert kinds.count("mfma_f32:grouped_wgrad") == (0 if grad == ("feat",) else 1), (grad, kinds)      # a frozen layer: no weight-gradient kernel
            assert kinds.count("mfma_f32:grouped_dinput") == (1 if "feat" in grad else 0), (grad, kinds)


# ---- the model -----------------------------------------------------------------------------------------------------------------------
class TinyBackbone(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.conv = torch.nn.Conv2d(3, 128, 4, stride=4)

    def forward(self, x):
        return torch.nn.functional.gelu(self.conv(x))


def _tiny_model():
    """GDRN_DoubleMask, class-aware with 3 classes, double mask: 32 x 32 crops, a 16 x 16 output (hw = 256), a 128-channel head."""
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from gdrnpp_bop2022_amd.gdrn_modeling.GDRN_double_mask import GDRN_DoubleMask
    from gdrnpp_bop2022_amd.gdrn_modeling.heads import ConvPnPNet, TopDownDoubleMaskXyzRegionHead

    cfg = get_cfg("tudl_convnext_a6", ["MODEL.POSE_NET.OUTPUT_RES=16", "MODEL.POSE_NET.INPUT_RES=32", "MODEL.POSE_NET.LOSS_CFG.FULL_MASK_LW=1.0"])
    assert cfg.MODEL.POSE_NET.NUM_CLASSES == 3
    torch.manual_seed(5)
    head = TopDownDoubleMaskXyzRegionHead(128, feat_dim=128, up_types=("bilinear",), num_conv_per_block=1, mask_num_classes=3,
                                          xyz_num_classes=3, region_num_classes=3, mask_out_dim=2)
    pnp = ConvPnPNet(nIn=69, num_regions=64, featdim=128, rot_dim=6, norm="GN", act="gelu", final_spatial_size=(2, 2))
    model = GDRN_DoubleMask(cfg, TinyBackbone(), head, pnp_net=pnp)
    with torch.no_grad():       # the heads' own initial values (std 0.001) would leave every map at its bias
        for name, p in model.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * (p[0].numel() ** -0.5))
            elif name.endswith("bias"):
                p.copy_(torch.randn_like(p) * 0.1)
    return cfg, model.eval()


def _tiny_batch(cfg, B, dev, dtype=torch.float32):
    from gdrnpp_bop2022_amd import synthetic as S
    from gdrnpp_bop2022_amd.gdrn_modeling import losses as L
    from tests.test_gpu_losses import dense_inputs, rot

    rng = np.random.default_rng(20221019 + 29)
    net = cfg.MODEL.POSE_NET
    C, o = net.NUM_CLASSES, net.OUTPUT_RES

    def T(a):
        a = torch.from_numpy(np.ascontiguousarray(a))
        return a.to(dev, dtype if a.is_floating_point() else None)

    ext = (rng.random((C, 3)) * 0.1 + 0.05).astype(np.float32)
    det = S.make_detections(B, C, ext, rng, out_res=o)
    det["roi_cls"][:] = np.array([2, 0, 2, 1, 0])[:B]
    det["roi_extent"] = ext[det["roi_cls"]]
    dn = dense_inputs(B, o, 1, net.GEO_HEAD.NUM_REGIONS + 1, seed=C)
    syms = [None if c % 2 else np.stack([np.eye(3), rot([0, 0, 1], 180)]).astype(np.float32) for c in range(C)]
    batch = dict(roi_classes=T(det["roi_cls"]), roi_cams=T(det["roi_cam"]), roi_whs=T(det["roi_wh"]), roi_centers=T(det["roi_center"]),
                 resize_ratios=T(det["resize_ratio"]), roi_coord_2d=T(S.coord2d_roi(det["roi_center"], det["scale"], out_res=o)),
                 roi_extents=T(det["roi_extent"]), gt_xyz=T(dn["gt_xyz"]), gt_xyz_bin=T(dn["gt_xyz_bin"]), gt_region=T(dn["gt_region"]),
                 gt_ego_rot=T(det["R_gt"]), gt_trans=T(det["t_gt"]),
                 gt_trans_ratio=T((rng.standard_normal((B, 3)) * [0.1, 0.1, 0.2] + [0, 0, 1.0]).astype(np.float32)),
                 **{k: T(dn[k]) for k in ("gt_mask_trunc", "gt_mask_visib", "gt_mask_obj", "gt_mask_full")})
    points = ((rng.random((C, 200, 3)) - 0.5) * ext[:, None]).astype(np.float32)
    x = T(rng.random((B, 3, net.INPUT_RES, net.INPUT_RES)).astype(np.float32))
    per_roi = dict(gt_points=points[det["roi_cls"]], sym_infos=[syms[c] for c in det["roi_cls"]], extents=det["roi_extent"])
    tables = (lambda: dict(points=T(points), sym=L.sym_tables(syms, dev), extents=T(ext)))
    return x, batch, tables, per_roi


def _cpu_reference(cfg, model, dtype):
    """forward_maps + the losses of tests/losses_ref.py + backward on the CPU in ``dtype`` -> (total loss, {parameter: gradient})."""
    from gdrnpp_bop2022_amd.gdrn_modeling import losses as L
    from tests import losses_ref as LR

    m = copy.deepcopy(model).cpu().to(dtype)
    x, batch, _, per_roi = _tiny_batch(cfg, 5, "cpu", dtype)
    pred_rot_, pred_t_, maps = m.forward_maps(x, batch["roi_classes"], batch["roi_coord_2d"], None, batch["roi_extents"], None)
    Rm, tr = L.pose_from_pred_train(pred_rot_, pred_t_, batch["roi_cams"], batch["roi_centers"], batch["roi_whs"], batch["resize_ratios"],
                                    z_type="REL", is_allo=True)
    loss, _ = LR.gdrn_loss_ref(L.loss_cfg(cfg), out_mask_vis=maps["mask"], out_mask_full=maps["full_mask"], out_x=maps["coor_x"],
                               out_y=maps["coor_y"], out_z=maps["coor_z"], out_region=maps["region"], out_rot=Rm, out_trans=tr,
                               out_centroid=pred_t_[:, :2], out_trans_z=pred_t_[:, 2], gt_rot=batch["gt_ego_rot"],
                               gt_points=torch.from_numpy(per_roi["gt_points"]).to(dtype), sym_infos=per_roi["sym_infos"],
                               extents=torch.from_numpy(per_roi["extents"]).to(dtype),
                               **{k: batch[k] for k in ("gt_mask_trunc", "gt_mask_visib", "gt_mask_obj", "gt_mask_full", "gt_xyz", "gt_xyz_bin",
                                                        "gt_region", "gt_trans", "gt_trans_ratio")})
    total = sum(loss.values())
    total.backward()
    return total.detach(), {n: p.grad for n, p in m.named_parameters()}


@pytest.fixture(scope="module")
def tiny():
    cfg, model = _tiny_model()
    return dict(cfg=cfg, model=model, ref64=_cpu_reference(cfg, model, torch.float64), ref32=_cpu_reference(cfg, model, torch.float32))


def _graph_nodes(y):
    seen, todo = set(), [y.grad_fn]
    while todo:
        fn = todo.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        todo.extend(f for f, _ in fn.next_functions)
    return {type(fn).__name__ for fn in seen}


def test_forward_is_the_inference_tail_bit_for_bit(hip, train_kernels, tiny):
    model = copy.deepcopy(tiny["model"]).to(DEV)
    _, batch, _, _ = _tiny_batch(tiny["cfg"], 5, DEV)
    gen = torch.Generator().manual_seed(3)
    feat = torch.randn(5, 128, 16, 16, generator=gen).to(DEV).contiguous(memory_format=torch.channels_last)
    sel, coord, ext = batch["roi_classes"], batch["roi_coord_2d"], batch["roi_extents"]
    model.pnp_net.forward_prepared = lambda x96, pose=None: (x96, x96)       # hand the prepared input back instead of running Patch-PnP
    with torch.no_grad():
        assert model._fused_tail_ok(feat, feat, sel, coord, ext)
        x96, _, maps = model._fused_tail(feat, sel, coord, ext)
        out2d, pnp_in, planes = train_kernels.head_tail(model.geo_head_net.out_layer, model._cls_rows, feat, sel, coord, ext, True)
    assert torch.equal(x96.permute(0, 2, 3, 1).reshape(5, 256, 96), pnp_in)
    planes = planes.view(5, 5, 1, 16, 16)
    for k, name in enumerate(("mask", "full_mask", "coor_x", "coor_y", "coor_z")):
        assert torch.equal(maps[name], planes[k]), name
    assert torch.equal(maps["region"], out2d.view(5, 16, 16, PITCH)[..., 5:70].permute(0, 3, 1, 2))


def test_model_trains_through_the_tail(hip, train_kernels, tiny):
    hip_layers = train_kernels
    cfg = tiny["cfg"]
    model = copy.deepcopy(tiny["model"]).to(DEV).to(memory_format=torch.channels_last)
    x, batch, tables, _ = _tiny_batch(cfg, 5, DEV)
    _, loss = model(x, do_loss=True, gt_tables=tables(), **batch)
    total = sum(loss.values())
    nodes = _graph_nodes(total)
    assert "HeadTailBackward" in nodes and "BaddbmmBackward0" not in nodes, nodes
    total.backward()
    (t64, g64), (t32, g32) = tiny["ref64"], tiny["ref32"]
    ratios = {"loss": abs(float(total.detach()) - float(t64)) / bar(t64.reshape(1), t32.reshape(1))}
    for n, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
        ratios[n] = ratio_to_bar(p.grad, g64[n], g32[n])
    print("head_tail_bwd model", " ".join(f"{k}={v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    # switch off: the module path, as before — PyTorch's graph, and the maps are those of _sliced_out_layer on the trunk's result
    hip_layers.set_train_kernels(False)
    seen = {}
    trunk = model.geo_head_net.trunk
    model.geo_head_net.trunk = lambda f: seen.setdefault("feat", trunk(f))
    try:
        _, _, maps = model.forward_maps(x, batch["roi_classes"], batch["roi_coord_2d"], None, batch["roi_extents"], None)
    finally:
        del model.geo_head_net.trunk
    nodes = _graph_nodes(maps["region"])
    assert "BaddbmmBackward0" in nodes and "HeadTailBackward" not in nodes, nodes
    want = model._sliced_out_layer(seen["feat"], batch["roi_classes"])
    for name, w in zip(("mask", "full_mask", "coor_x", "coor_y", "coor_z", "region"), want):
        assert torch.equal(maps[name], w), name


def test_inference_is_untouched(hip, train_kernels, tiny):
    model = copy.deepcopy(tiny["model"]).to(DEV).to(memory_format=torch.channels_last)
    x, batch, _, _ = _tiny_batch(tiny["cfg"], 5, DEV)
    args = (x, batch["roi_classes"], batch["roi_coord_2d"], None, batch["roi_extents"], None)
    with torch.no_grad():
        on = model.forward_maps(*args)
        train_kernels.set_train_kernels(False)
        off = model.forward_maps(*args)
    assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]) and all(torch.equal(on[2][k], off[2][k]) for k in off[2])
    assert on[0].grad_fn is None
