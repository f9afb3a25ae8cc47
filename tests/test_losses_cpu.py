"""tests/losses_ref.py, the yardstick of the GPU loss tests, against values and gradients recorded from the reference's own ``gdrn_loss``
(tests/golden/losses_golden.npz, written by tests/golden/make_golden_losses.py).  CPU only."""
import json
import os

import numpy as np
import pytest
import torch

from tests.losses_ref import VARIANTS, closest_rots, gdrn_loss_ref, variant_inputs

HERE = os.path.dirname(os.path.abspath(__file__))
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(HERE, "golden", "losses_golden.npz"))
    return z, json.loads(str(z["meta"]))


def test_fixture_holds_the_variants(golden):
    z, meta = golden
    assert tuple(meta) == VARIANTS
    assert meta["single"]["model"] == "GDRN" and "loss_mask_full" not in meta["single"]["keys"]
    assert "loss_PM_RT" in meta["pm_rt"]["keys"] and "loss_bind" in meta["fallback"]["keys"]
    assert z["sym_0"].shape == (2, 3, 3) and z["sym_1"].shape == (315, 3, 3) and "sym_2" not in z.files


def test_loss_defaults_are_the_references_block(golden):
    from gdrnpp_bop2022_amd.gdrn_modeling.losses import LOSS_DEFAULTS

    assert LOSS_DEFAULTS == json.loads(str(golden[0]["loss_defaults"]))


@pytest.mark.parametrize("name", VARIANTS)
def test_restatement_matches_the_recorded_fp64_run(golden, name):
    z, meta = golden
    lc, kw, z_type = variant_inputs(z, meta, name)
    loss, R_sel = gdrn_loss_ref(lc, z_type=z_type, **kw)
    assert list(loss) == meta[name]["keys"]
    for k, v in loss.items():
        ref = float(z[f"{name}/loss64/{k}"])
        assert abs(float(v.detach()) - ref) <= 1e-12 * abs(ref), (k, float(v.detach()), ref)
    sum(loss.values()).backward()
    assert meta[name]["grads"]
    for k in meta[name]["grads"]:
        g, ref = kw[k].grad.numpy(), z[f"{name}/grad64/{k}"]
        assert np.abs(g - ref).max() <= 1e-12 * np.abs(ref).max(), (k, np.abs(g - ref).max(), np.abs(ref).max())
    if lc["PM_LOSS_SYM"]:
        ref = z[f"{name}/gt_rot_closest"]
        assert np.abs(R_sel - ref).max() <= 1e-12
        # ROI 1 sits 0.05 degrees from step 100 of its 315 rotations, ROI 0 near its flipped ground truth, ROI 2 is asymmetric
        gt = z[f"{name}/in/gt_rot"].astype(np.float64)
        assert np.abs(R_sel[0] - gt[0] @ z["sym_0"][1].astype(np.float64)).max() < 1e-12
        assert np.abs(R_sel[1] - gt[1] @ z["sym_1"][100].astype(np.float64)).max() < 1e-12
        assert np.array_equal(R_sel[2], gt[2])


@pytest.mark.parametrize("name", VARIANTS)
def test_recorded_fp32_values_lie_within_their_rounding(golden, name):
    """The reference's fp32 run against its fp64 run.  A term is a mean of n values, each formed with a handful of fp32 roundings and summed
    in fp32 by torch's pairwise reduction: about (8 + log2 n) eps relative.  The point-matching terms subtract transformed points of size
    |p| ~ 0.05 (times w) that differ by ~|p| sin(10 degrees), which magnifies the rounding of the products by up to |p| / |d| ~ 10.  256 eps
    (3e-5) covers both with room; what it must exclude is a different symmetry candidate or a dropped term, which move a value by percents."""
    z, meta = golden
    for k in meta[name]["keys"]:
        l32, l64 = float(z[f"{name}/loss32/{k}"]), float(z[f"{name}/loss64/{k}"])
        assert abs(l32 - l64) <= 256 * EPS32 * abs(l64), (k, l32, l64)


def test_closest_rotation_keeps_the_first_of_equal_candidates():
    """The identity among the symmetries, and a duplicated symmetry: the strict < of the reference keeps the earlier candidate."""
    from scipy.spatial.transform import Rotation

    gt = torch.from_numpy(Rotation.random(2, random_state=5).as_matrix())
    flip = Rotation.from_rotvec([0, 0, np.pi]).as_matrix()
    pred = torch.from_numpy(np.stack([gt[0].numpy() @ Rotation.from_rotvec([0.02, 0, 0]).as_matrix(),
                                      gt[1].numpy() @ flip @ Rotation.from_rotvec([0, 0.03, 0]).as_matrix()]))
    sel = closest_rots(pred, gt, [np.stack([np.eye(3), flip]), np.stack([flip, np.eye(3), flip])])
    assert np.array_equal(sel[0], gt[0].numpy())            # the identity does not displace R_gt
    assert np.abs(sel[1] - gt[1].numpy() @ flip).max() < 1e-15
    assert np.array_equal(closest_rots(pred, gt, [None, None]), gt.numpy())


def test_loss_plan_names_where_every_term_runs():
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from gdrnpp_bop2022_amd.gdrn_modeling.losses import loss_cfg, loss_plan

    cfg = get_cfg("ycbv_convnext_a6", ["MODEL.POSE_NET.LOSS_CFG.PM_LOSS_SYM=True", "MODEL.POSE_NET.LOSS_CFG.FULL_MASK_LW=1.0"])
    assert loss_cfg(cfg)["FULL_MASK_LOSS_TYPE"] == "L1" and loss_cfg(cfg)["REGION_LOSS_MASK_GT"] == "visib"      # the config's keys over the defaults
    plan = loss_plan(cfg)
    assert list(plan["terms"]) == ["loss_coor_x", "loss_coor_y", "loss_coor_z", "loss_mask", "loss_mask_full", "loss_region", "loss_PM_R",
                                   "loss_centroid", "loss_z"]
    assert set(plan["terms"].values()) == {"kernel"} and plan["dense_kernel"] and plan["pose_kernel"]
    # the single-mask model has no full-mask term; a frozen head has no dense term
    assert "loss_mask_full" not in loss_plan(get_cfg("lmo_resnet34_ape", ["MODEL.POSE_NET.LOSS_CFG.FULL_MASK_LW=1.0"]))["terms"]
    frozen = loss_plan(get_cfg("ycbv_convnext_a6", ["MODEL.POSE_NET.GEO_HEAD.FREEZE=True"]))
    assert list(frozen["terms"]) == ["loss_PM_R", "loss_centroid", "loss_z"] and not frozen["dense_kernel"]
    opts = [f"MODEL.POSE_NET.LOSS_CFG.{k}" for k in ("MASK_LOSS_TYPE=dice", "PM_LOSS_TYPE=L2", "ROT_LW=1.0", "TRANS_LW=1.0", "BIND_LW=1.0", "Z_LOSS_TYPE=MSE")]
    terms = loss_plan(get_cfg("ycbv_convnext_a6", opts))["terms"]
    on_torch = {k for k, v in terms.items() if v == "torch"}
    assert on_torch == {"loss_mask", "loss_PM_R", "loss_rot", "loss_centroid", "loss_z", "loss_trans_xy", "loss_trans_z", "loss_bind"}
    for opt, key in (("MODEL.POSE_NET.LOSS_CFG.PM_DISENTANGLE_T=True", "PM_DISENTANGLE_T"), ("MODEL.POSE_NET.LOSS_CFG.PM_DISENTANGLE_Z=True", "PM_DISENTANGLE_Z"),
                     ("MODEL.POSE_NET.USE_MTL=True", "USE_MTL")):
        with pytest.raises(NotImplementedError, match=key):
            loss_plan(get_cfg("ycbv_convnext_a6", [opt]))
