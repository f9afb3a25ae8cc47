"""Golden training losses from the reference's OWN ``gdrn_loss`` (authoring container only: needs /root/reference).

Cut out of the reference files with ``ast`` and executed UNMODIFIED:

    gdrn_loss                                            core/gdrn_modeling/models/GDRN_double_mask.py and models/GDRN.py (methods; ``self`` is
                                                         read only under USE_MTL, which is off)
    PyPMLoss                                             core/gdrn_modeling/losses/pm_loss.py
    L2Loss, l2_loss                                      core/gdrn_modeling/losses/l2_loss.py
    CrossEntropyHeatmapLoss, _assert_no_grad             core/gdrn_modeling/losses/coor_cross_entropy.py
    weighted_ex_loss_probs, soft_dice_loss               core/gdrn_modeling/losses/mask_losses.py
    angular_distance(_rot, _quat), rot_l2_loss           core/gdrn_modeling/losses/rot_loss.py
    get_closest_rot_batch, get_closest_rot               core/utils/pose_utils.py
    re                                                   lib/pysixd/pose_error.py
    transform_pts_batch                                  lib/pysixd/misc.py

Served by stand-ins, because the packages are not installed: ``fvcore.nn.smooth_l1_loss`` (its published definition: |d| below beta
is 0.5 d^2 / beta, else |d| - 0.5 beta; plain L1 for beta < 1e-5), ``detectron2``'s ``log_first_n`` (silent) and ``quat2mat_torch`` (never
reached: every rotation is a matrix).  ``cfg`` is this project's ``Config`` over the reference's own LOSS_CFG block, which is read from
configs/_base_/gdrn_base.py and recorded as ``loss_defaults``.

Every variant runs on seeded inputs in fp32 and again in fp64 on the same values cast up; both runs are differentiated by autograd with
respect to every network-side input.  Recorded in losses_golden.npz: the inputs, both sets of loss values, the fp64 gradients of the sum
of the losses, per tensor the largest distance of the fp32 gradient from the fp64 one (``grad32_err``: the reference's own fp32 error, the
measure for terms that run in fp32 here too) and the ground-truth rotations ``get_closest_rot_batch`` chose.  B = 3 ROIs, 8 x 8 maps, 50 model points; ROI 0 is an object
with 2 discrete symmetries, ROI 1 one with the 0.01-step discretisation of a continuous symmetry (315 rotations), ROI 2 is asymmetric.

The reference selects the closest rotation on float32 ``arccos`` values, which near 0 degrees resolve no better than about 0.02 degrees:
candidates closer than that are decided by its rounding noise.  The inputs are therefore built so that, per ROI, the best and the
runner-up candidate differ by at least 1 degree or are bit-equal duplicates, and that is asserted here, on the fp32 and the fp64 values."""
import ast
import json
import logging
import os
import sys
from functools import partial

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
from scipy.spatial.transform import Rotation

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
from gdrnpp_bop2022_amd.gdrn_modeling.config import Config  # noqa: E402

REF = "/root/reference"
SEED = 20221019 + 7
B, O, P, NBIN = 3, 8, 50, 64

# name -> (model file, region channels, Z_TYPE, LOSS_CFG overrides)
VARIANTS = {
    "shipped": ("GDRN_double_mask", 65, "REL", dict(XYZ_LOSS_TYPE="L1", MASK_LOSS_TYPE="L1", FULL_MASK_LOSS_TYPE="L1", FULL_MASK_LW=1.0,
                                                    PM_LOSS_SYM=True, PM_R_ONLY=True)),
    "ce_bce": ("GDRN_double_mask", 5, "REL", dict(XYZ_LOSS_TYPE="CE_coor", XYZ_LOSS_MASK_GT="obj", MASK_LOSS_TYPE="BCE", MASK_LOSS_GT="visib",
                                                  FULL_MASK_LOSS_TYPE="BCE", FULL_MASK_LW=0.5, REGION_LOSS_MASK_GT="trunc", XYZ_LW=0.7,
                                                  REGION_LW=0.1, PM_LOSS_SYM=True)),
    "pm_rt": ("GDRN_double_mask", 65, "ABS", dict(PM_LOSS_TYPE="Smooth_L1", PM_SMOOTH_L1_BETA=0.2, PM_NORM_BY_EXTENT=True, PM_R_ONLY=False,
                                                  PM_LOSS_SYM=True, PM_LW=2.0, FULL_MASK_LW=1.0, FULL_MASK_LOSS_TYPE="L1", CENTROID_LW=0.3,
                                                  Z_LW=1.7, MASK_LW=0.9)),
    "fallback": ("GDRN_double_mask", 5, "REL", dict(MASK_LOSS_TYPE="RW_BCE", FULL_MASK_LOSS_TYPE="dice", FULL_MASK_LW=1.0, PM_LOSS_TYPE="L2",
                                                    PM_LOSS_SYM=True, ROT_LW=0.5, ROT_LOSS_TYPE="angular", TRANS_LW=0.25, TRANS_LOSS_TYPE="L2",
                                                    TRANS_LOSS_DISENTANGLE=True, BIND_LW=0.75, BIND_LOSS_TYPE="L1", CENTROID_LOSS_TYPE="L2",
                                                    Z_LOSS_TYPE="MSE")),
    "fallback_ce": ("GDRN_double_mask", 5, "ABS", dict(MASK_LOSS_TYPE="CE", FULL_MASK_LOSS_TYPE="RW_BCE", FULL_MASK_LW=2.0, PM_LOSS_TYPE="MSE",
                                                       PM_LOSS_SYM=False, ROT_LW=1.5, ROT_LOSS_TYPE="L2", TRANS_LW=0.5, TRANS_LOSS_TYPE="MSE",
                                                       TRANS_LOSS_DISENTANGLE=False, BIND_LW=0.2, BIND_LOSS_TYPE="L2", CENTROID_LOSS_TYPE="MSE",
                                                       Z_LOSS_TYPE="L2")),
    "single": ("GDRN", 65, "REL", dict(MASK_LOSS_TYPE="BCE", PM_LOSS_SYM=True)),
}
NET_INPUTS = ("out_mask_vis", "out_mask_full", "out_x", "out_y", "out_z", "out_region", "out_rot", "out_trans", "out_centroid", "out_trans_z")


def cut_def(path, name):
    """Source text of the function, method or class ``name`` in the reference file, dedented."""
    src = open(os.path.join(REF, path)).read()
    for node in ast.walk(ast.parse(src)):
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name == name:
            lines = src.splitlines()[node.lineno - 1:node.end_lineno]
            indent = len(lines[0]) - len(lines[0].lstrip())
            return "\n".join(l[indent:] for l in lines) + "\n"
    raise KeyError(name)


def smooth_l1_loss(input, target, beta, reduction="none"):
    if beta < 1e-5:
        loss = torch.abs(input - target)
    else:
        n = torch.abs(input - target)
        loss = torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta)
    return loss.mean() if reduction == "mean" else loss.sum() if reduction == "sum" else loss


def reference_namespace(model_file):
    ns = dict(torch=torch, nn=nn, F=F, np=np, partial=partial, logging=logging, smooth_l1_loss=smooth_l1_loss,
              log_first_n=lambda *a, **k: None, quat2mat_torch=None)
    for path, names in (("lib/pysixd/pose_error.py", ["re"]), ("lib/pysixd/misc.py", ["transform_pts_batch"]),
                        ("core/utils/pose_utils.py", ["get_closest_rot", "get_closest_rot_batch"]),
                        ("core/gdrn_modeling/losses/l2_loss.py", ["l2_loss", "L2Loss"]),
                        ("core/gdrn_modeling/losses/coor_cross_entropy.py", ["_assert_no_grad", "CrossEntropyHeatmapLoss"]),
                        ("core/gdrn_modeling/losses/mask_losses.py", ["weighted_ex_loss_probs", "soft_dice_loss"]),
                        ("core/gdrn_modeling/losses/rot_loss.py", ["angular_distance_quat", "angular_distance_rot", "angular_distance", "rot_l2_loss"]),
                        ("core/gdrn_modeling/losses/pm_loss.py", ["PyPMLoss"]),
                        (f"core/gdrn_modeling/models/{model_file}.py", ["gdrn_loss"])):
        for name in names:
            exec(compile(cut_def(path, name), os.path.join(REF, path), "exec"), ns)
    return ns


def reference_loss_defaults():
    ns = {}
    exec(compile(open(os.path.join(REF, "configs/_base_/gdrn_base.py")).read(), "gdrn_base.py", "exec"), ns)
    return dict(ns["MODEL"]["POSE_NET"]["LOSS_CFG"])


def rot(axis, deg):
    return Rotation.from_rotvec(np.asarray(axis, np.float64) / np.linalg.norm(axis) * np.deg2rad(deg)).as_matrix()


def symmetries():
    """Per ROI the reference's ``sym_infos`` entry, float32 as data_loader builds it: [I, Rz(180)], the 315 rotations about z that
    misc.get_symmetry_transformations makes of a continuous symmetry at max_sym_disc_step = 0.01 (ceil(pi / 0.01) steps), None."""
    two = np.stack([np.eye(3), rot([0, 0, 1], 180.0)]).astype(np.float32)
    n = int(np.ceil(np.pi / 0.01))
    cont = np.stack([rot([0, 0, 1], 360.0 * k / n) for k in range(n)]).astype(np.float32)
    return [two, cont, None]


def make_inputs(rng, region_c, mask_c, xyz_ce):
    """Seeded float32 inputs: nested masks (trunc in visib in obj in full), targets as roi_train_targets forms them (background bin n_bin,
    background region 0) with a few non-zero targets left on masked-out pixels, and poses near a symmetric copy of the ground truth."""
    d = {}
    obj = rng.random((B, O, O)) < 0.55
    visib = obj & (rng.random((B, O, O)) < 0.8)
    trunc = visib & (rng.random((B, O, O)) < 0.8)
    full = obj | (rng.random((B, O, O)) < 0.15)
    for k, m in (("obj", obj), ("visib", visib), ("trunc", trunc), ("full", full)):
        d[f"gt_mask_{k}"] = m.astype(np.float32)
    xyz = rng.random((B, 3, O, O)).astype(np.float32)
    d["gt_xyz"] = xyz * obj[:, None]
    bins = np.minimum((xyz * NBIN).astype(np.int64), NBIN - 1)
    d["gt_xyz_bin"] = np.where(obj[:, None], bins, NBIN).astype(np.uint8)
    region = rng.integers(1, region_c, (B, O, O))
    stray = rng.random((B, O, O)) < 0.1            # targets that the mask must switch off
    d["gt_region"] = np.where(obj | stray, region, 0).astype(np.int32)
    cx = NBIN + 1 if xyz_ce else 1
    for k in ("x", "y", "z"):
        d[f"out_{k}"] = (rng.standard_normal((B, cx, O, O)) * (2.0 if xyz_ce else 0.5) + (0.0 if xyz_ce else 0.5)).astype(np.float32)
    d["out_mask_vis"] = rng.standard_normal((B, mask_c, O, O)).astype(np.float32)
    d["out_mask_full"] = rng.standard_normal((B, mask_c, O, O)).astype(np.float32)
    d["out_region"] = (rng.standard_normal((B, region_c, O, O)) * 2.0).astype(np.float32)
    # L1 pixels where out == gt exactly
    if not xyz_ce:
        d["out_x"][0, 0, :2] = d["gt_xyz"][0, 0, :2]
    gt_rot = Rotation.random(B, random_state=int(rng.integers(1 << 30))).as_matrix()
    n = int(np.ceil(np.pi / 0.01))
    near = [rot([0, 0, 1], 180.0) @ rot([1, 2, 3], 9.0),                 # ROI 0: 9 degrees from the flipped ground truth
            rot([0, 0, 1], 360.0 * 100 / n + 0.02) @ rot([1, 0, 0], 0.05),   # ROI 1: 0.05 degrees from step 100 of 315
            rot([3, 1, 2], 14.0)]                                      # ROI 2: asymmetric
    d["gt_rot"] = gt_rot.astype(np.float32)
    d["out_rot"] = np.stack([gt_rot[i] @ near[i] for i in range(B)]).astype(np.float32)
    d["gt_trans"] = (rng.random((B, 3)) * [0.2, 0.2, 0.5] + [-0.1, -0.1, 0.6]).astype(np.float32)
    d["out_trans"] = (d["gt_trans"] + rng.standard_normal((B, 3)) * 0.02).astype(np.float32)
    d["gt_trans_ratio"] = (rng.standard_normal((B, 3)) * [0.1, 0.1, 0.3] + [0, 0, 1.0]).astype(np.float32)
    d["out_centroid"] = (d["gt_trans_ratio"][:, :2] + rng.standard_normal((B, 2)) * 0.05).astype(np.float32)
    d["out_trans_z"] = (d["gt_trans_ratio"][:, 2] + rng.standard_normal(B) * 0.1).astype(np.float32)
    d["extents"] = (rng.random((B, 3)) * 0.1 + 0.05).astype(np.float32)
    d["gt_points"] = ((rng.random((B, P, 3)) - 0.5) * d["extents"][:, None]).astype(np.float32)
    return d


def check_candidates(ns, d, syms, dtype):
    """The condition on the inputs: per ROI, best and runner-up re differ by >= 1 degree or are bit-equal duplicates."""
    for i, sym in enumerate(syms):
        if sym is None:
            continue
        Rp, Rg = d["out_rot"][i].astype(dtype), d["gt_rot"][i].astype(dtype)
        cands = [Rg] + [Rg.dot(s.astype(dtype)) for s in sym]
        res = np.array([ns["re"](Rp, c) for c in cands], np.float64)
        order = np.argsort(res, kind="stable")
        best, second = order[0], order[1]
        assert res[second] - res[best] >= 1.0 or np.array_equal(cands[best], cands[second]), (i, res[best], res[second])


def run(ns, cfg, d, syms, dtype, single, want_grad):
    t = {}
    for k, v in d.items():
        if v.dtype == np.float32:
            t[k] = torch.from_numpy(v.astype(np.float64 if dtype == torch.float64 else np.float32))
            if want_grad and k in NET_INPUTS:
                t[k].requires_grad_(True)
        else:
            t[k] = torch.from_numpy(v)
    kw = dict(cfg=cfg, gt_mask_trunc=t["gt_mask_trunc"], gt_mask_visib=t["gt_mask_visib"], gt_mask_obj=t["gt_mask_obj"], out_x=t["out_x"],
              out_y=t["out_y"], out_z=t["out_z"], gt_xyz=t["gt_xyz"], gt_xyz_bin=t["gt_xyz_bin"], out_region=t["out_region"],
              gt_region=t["gt_region"], out_rot=t["out_rot"], gt_rot=t["gt_rot"], out_trans=t["out_trans"], gt_trans=t["gt_trans"],
              out_centroid=t["out_centroid"], out_trans_z=t["out_trans_z"], gt_trans_ratio=t["gt_trans_ratio"], gt_points=t["gt_points"],
              sym_infos=[None if s is None else s.astype(np.float64 if dtype == torch.float64 else np.float32) for s in syms],
              extents=t["extents"])
    if single:
        kw["out_mask"] = t["out_mask_vis"]
    else:
        kw.update(out_mask_vis=t["out_mask_vis"], out_mask_full=t["out_mask_full"], gt_mask_full=t["gt_mask_full"])
    chosen = {}
    orig = ns["get_closest_rot_batch"]

    def spy(*a, **k):
        chosen["R"] = orig(*a, **k)
        return chosen["R"]

    ns["get_closest_rot_batch"] = spy
    try:
        loss = ns["gdrn_loss"](None, **kw)
    finally:
        ns["get_closest_rot_batch"] = orig
    grads = {}
    if want_grad:
        sum(loss.values()).backward()
        grads = {k: t[k].grad.numpy() for k in NET_INPUTS if k in t and t[k].grad is not None}
    return {k: v.detach().numpy() for k, v in loss.items()}, grads, chosen.get("R")


def main():
    out = {"loss_defaults": json.dumps(reference_loss_defaults())}
    meta = {}
    syms = symmetries()
    for j, s in enumerate(syms):
        if s is not None:
            out[f"sym_{j}"] = s
    for vi, (name, (model_file, region_c, z_type, over)) in enumerate(VARIANTS.items()):
        rng = np.random.default_rng(SEED + vi)
        ns = reference_namespace(model_file)
        lc = reference_loss_defaults()
        lc.update(over)
        single = model_file == "GDRN"
        cfg = Config(dict(MODEL=dict(POSE_NET=dict(USE_MTL=False, GEO_HEAD=dict(FREEZE=False), PNP_NET=dict(TRANS_TYPE="centroid_z", Z_TYPE=z_type),
                                                   LOSS_CFG=lc))))
        mask_c = 2 if "CE" in (lc["MASK_LOSS_TYPE"], lc["FULL_MASK_LOSS_TYPE"]) else 1
        d = make_inputs(rng, region_c, mask_c, lc["XYZ_LOSS_TYPE"] == "CE_coor")
        if lc["PM_LOSS_SYM"]:
            check_candidates(ns, d, syms, np.float32)
            check_candidates(ns, d, syms, np.float64)
        l32, g32, R32 = run(ns, cfg, d, syms, torch.float32, single, True)
        l64, g64, R64 = run(ns, cfg, d, syms, torch.float64, single, True)
        assert list(l32) == list(l64) and list(g32) == list(g64)
        if R64 is not None:
            assert np.abs(R32.numpy().astype(np.float64) - R64.numpy()).max() < 1e-5, name      # the same candidates in both precisions
            out[f"{name}/gt_rot_closest"] = R64.numpy()
        for k, v in d.items():
            out[f"{name}/in/{k}"] = v
        for k in l64:
            out[f"{name}/loss32/{k}"] = np.float32(l32[k])
            out[f"{name}/loss64/{k}"] = np.float64(l64[k])
        for k, v in g64.items():
            out[f"{name}/grad64/{k}"] = v
            # of the fp32 gradients only their distance from the fp64 ones is used (the bar of terms that run in fp32): one number per tensor
            out[f"{name}/grad32_err/{k}"] = np.float64(np.abs(g32[k].astype(np.float64) - v).max())
        meta[name] = dict(model=model_file, region_channels=region_c, z_type=z_type, loss_cfg=over, keys=list(l64), grads=list(g64))
        print(name, {k: float(v) for k, v in l64.items()})
    out["meta"] = json.dumps(meta)
    path = os.path.join(HERE, "losses_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
