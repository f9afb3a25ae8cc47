"""The restated backward of the geometry head's tail (tests/head_tail_bwd_ref.py) against fp64 autograd, and the sliced form of the
output layer against the reference's full-width layer followed by the class gather.  CPU only, no HIP library."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import head_tail_bwd_ref as R  # noqa: E402


def _rel(a, b):
    return float((a.double() - b.double()).abs().max()) / max(float(b.double().abs().max()), 1e-300)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_restated_formulas_equal_fp64_autograd(case):
    t = R.make_inputs(case)
    ref64, _ = R.references(case)
    d_out = R.restated_tail_backward(ref64["out"], t["extents"], t["double_mask"], t["g_pnp"], t["g_planes"], t["g_out"])
    w_sliced = t["weight"][t["cls_rows"]]
    dfeat = R.restated_dinput(d_out, w_sliced, t["sel"])
    dW, db = R.restated_wgrad(d_out, t["feat"], t["sel"], t["cls_rows"], t["weight"].shape[0])
    errs = dict(d_out=_rel(d_out, ref64["d_out"]), dfeat=_rel(dfeat, ref64["dfeat"]), dW=_rel(dW, ref64["dW"]), db=_rel(db, ref64["db"]))
    print("head_tail restated", R.case_id(case), " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    assert max(errs.values()) <= 1e-12, errs
    p = ref64["pnp_in"][..., 5:]
    assert float(p.max()) > 0.999 and float(p.min()) < 1e-12       # the cases hold saturated pixels
    # a class without a ROI has exactly zero rows, in the formulas and under autograd
    for c in set(range(case[3])) - set(case[5]):
        rows = t["cls_rows"][c]
        assert not dW[rows].any() and not db[rows].any() and not ref64["dW"][rows].any() and not ref64["db"][rows].any()


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_each_gradient_source_alone(case):
    """The three sources add: each alone equals autograd with the other two loss terms dropped."""
    t = dict(R.make_inputs(case))
    for keep in ("g_pnp", "g_planes", "g_out"):
        only = dict(t, **{k: torch.zeros_like(t[k]) for k in ("g_pnp", "g_planes", "g_out") if k != keep})
        ref = R.autograd_tail(only, torch.float64)
        got = R.restated_tail_backward(ref["out"], t["extents"], t["double_mask"], **{keep: t[keep]})
        assert _rel(got, ref["d_out"]) <= 1e-12, keep
    kx = 2 if t["double_mask"] else 1
    got = R.restated_tail_backward(R.references(case)[0]["out"], t["extents"], t["double_mask"], g_pnp=t["g_pnp"])
    assert not got[..., :kx].any() and not got[..., kx + 3].any()      # masks and the background logit get nothing from Patch-PnP's input


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_sliced_form_equals_full_width_then_gather(case):
    t = R.make_inputs(case)
    ref64, _ = R.references(case)
    full = R.autograd_tail(t, torch.float64, full_width=True)
    for k in ("out", "pnp_in", "planes", "d_out", "dfeat", "dW", "db"):
        assert full[k].shape == ref64[k].shape and _rel(full[k], ref64[k]) <= 1e-12, k


def test_class_rows_are_the_heads_row_table():
    from gdrnpp_bop2022_amd.gdrn_modeling.heads import TopDownDoubleMaskXyzRegionHead, TopDownMaskXyzRegionHead

    for cls, double, C in ((TopDownDoubleMaskXyzRegionHead, True, 3), (TopDownMaskXyzRegionHead, False, 2)):
        head = cls(128, feat_dim=128, up_types=("bilinear",), num_conv_per_block=1, mask_num_classes=C, xyz_num_classes=C,
                   region_num_classes=C, mask_out_dim=2 if double else 1)
        assert torch.equal(head.class_channel_index(C), R.class_rows(C, double))


def test_slot_plan():
    assert R.wgrad_slots(1, 256, 128) == (1, 512) and R.wgrad_slots(2, 768, 256) == (2, 512)
    assert R.wgrad_slots(48, 4096, 256) == (8, 512) and R.wgrad_slots(128, 4096, 256) == (4, 1024)
