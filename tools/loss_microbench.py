"""Microbenchmark of GDRN's training losses on one MI355X: ``gdrn_modeling.losses.gdrn_loss`` (the HIP kernels of csrc/gdrn_loss.hip behind
their autograd Functions) against the same losses on torch operators (tests/losses_ref.py in fp32 on the same GPU, its closest-rotation
step done the reference's way: both rotation batches copied to the host, a NumPy loop over the ROIs, the result copied back).

Shapes: ``--rois`` 36 and 48 (the IMS_PER_BATCH of the shipped configs), 64 x 64 maps, 65 region channels, 3000 model points, 21 objects of
which 17 are symmetric (5 with the 315 rotations of a discretised continuous symmetry, 12 with 2 or 4 discrete ones); the shipped loss
configuration: L1 xyz and masks with the full mask on, region CE, symmetric PM_R, L1 centroid and z.

Measured per variant: forward + backward of the loss alone (the maps and the pose are leaves that require grad) by the host clock around
``--reps`` steps that end in a device synchronise, the two variants alternating within each of ``--rounds`` rounds, after a warm-up of
both; median / min / max over the rounds.  The kernel path's table form (per-object points, symmetries and extents indexed by
roi_classes) is what a training loop would pass; the torch path takes the reference's per-ROI form.  The launch count comes from a
separate profiled step of each variant (torch.profiler device events); when the profiler is unavailable it is reported as not measured.
Nothing here is gated.

    python tools/loss_microbench.py [--out profiles/loss_microbench.json] [--rois 36 48] [--reps 20] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

O, CR, P, N_OBJ, N_CONT = 64, 65, 3000, 21, 315
LOSS_CFG = dict(XYZ_LOSS_TYPE="L1", MASK_LOSS_TYPE="L1", FULL_MASK_LOSS_TYPE="L1", FULL_MASK_LW=1.0, PM_LOSS_SYM=True, PM_R_ONLY=True)
LEAVES = ("out_x", "out_y", "out_z", "out_mask_vis", "out_mask_full", "out_region", "out_rot", "pred_t_")


def rot(axis, deg):
    from scipy.spatial.transform import Rotation

    return Rotation.from_rotvec(np.asarray(axis, np.float64) / np.linalg.norm(axis) * np.deg2rad(deg)).as_matrix()


def object_symmetries():
    syms = []
    for o in range(N_OBJ):
        if o < 5:
            syms.append(np.stack([rot([0, 0, 1], 360.0 * k / N_CONT) for k in range(N_CONT)]).astype(np.float32))
        elif o < 11:
            syms.append(np.stack([np.eye(3), rot([0, 0, 1], 180)]).astype(np.float32))
        elif o < 17:
            syms.append(np.stack([np.eye(3), rot([0, 0, 1], 90), rot([0, 0, 1], 180), rot([0, 0, 1], 270)]).astype(np.float32))
        else:
            syms.append(None)
    return syms


def build(rng, B, dev):
    import torch
    from scipy.spatial.transform import Rotation

    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    obj_m = rng.random((B, O, O)) < 0.45
    visib = obj_m & (rng.random((B, O, O)) < 0.85)
    d = {"gt_mask_obj": obj_m, "gt_mask_visib": visib, "gt_mask_trunc": visib & (rng.random((B, O, O)) < 0.9), "gt_mask_full": obj_m}
    t = {k: T(v.astype(np.float32)) for k, v in d.items()}
    t["gt_xyz"] = T((rng.random((B, 3, O, O)) * obj_m[:, None]).astype(np.float32))
    t["gt_region"] = T(np.where(obj_m, rng.integers(1, CR, (B, O, O)), 0).astype(np.int32))
    for k in ("out_x", "out_y", "out_z", "out_mask_vis", "out_mask_full"):
        t[k] = T(rng.standard_normal((B, 1, O, O)).astype(np.float32))
    t["out_region"] = T((rng.standard_normal((B, CR, O, O)) * 2).astype(np.float32))
    cls = rng.integers(0, N_OBJ, B)
    gt = Rotation.random(B, random_state=int(rng.integers(1 << 30))).as_matrix()
    t["gt_rot"] = T(gt.astype(np.float32))
    t["out_rot"] = T(np.stack([gt[i] @ rot(rng.standard_normal(3), 25.0) for i in range(B)]).astype(np.float32))
    t["gt_trans"] = T((rng.random((B, 3)) + [0, 0, 0.5]).astype(np.float32))
    t["gt_trans_ratio"] = T(rng.standard_normal((B, 3)).astype(np.float32))
    t["pred_t_"] = T(rng.standard_normal((B, 3)).astype(np.float32))
    ext = (rng.random((N_OBJ, 3)) * 0.1 + 0.05).astype(np.float32)
    pts = ((rng.random((N_OBJ, P, 3)) - 0.5) * ext[:, None]).astype(np.float32)
    return t, cls, ext, pts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_microbench.json"))
    ap.add_argument("--rois", type=int, nargs="+", default=[36, 48])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd.gdrn_modeling import losses as L
    from gdrnpp_bop2022_amd.gdrn_modeling.config import Config
    from tests import losses_ref as LR

    assert torch.cuda.is_available(), "loss_microbench needs the GPU"
    dev = torch.device("cuda")
    lc = dict(L.LOSS_DEFAULTS)
    lc.update(LOSS_CFG)
    cfg = Config(dict(MODEL=dict(POSE_NET=dict(NAME="GDRN_double_mask", USE_MTL=False, GEO_HEAD=dict(FREEZE=False),
                                               PNP_NET=dict(TRANS_TYPE="centroid_z", Z_TYPE="REL"), LOSS_CFG=LOSS_CFG))))
    syms = object_symmetries()
    result = {"device": torch.cuda.get_device_name(0), "shapes": dict(o=O, region_channels=CR, points=P, objects=N_OBJ, symmetric=17),
              "loss_cfg": LOSS_CFG, "reps": args.reps, "rounds": args.rounds, "cases": []}
    for B in args.rois:
        rng = np.random.default_rng(20221019 + B)
        t, cls, ext, pts = build(rng, B, dev)
        for k in LEAVES:
            t[k].requires_grad_(True)
        common = {k: t[k] for k in ("out_mask_vis", "out_mask_full", "gt_mask_trunc", "gt_mask_visib", "gt_mask_obj", "gt_mask_full", "out_x", "out_y",
                                    "out_z", "gt_xyz", "out_region", "gt_region", "out_rot", "gt_rot", "gt_trans", "gt_trans_ratio")}
        tables = dict(gt_points=torch.from_numpy(pts).to(dev), sym_infos=L.sym_tables(syms, dev), extents=torch.from_numpy(ext).to(dev),
                      roi_classes=torch.from_numpy(cls).to(dev))
        per_roi = dict(gt_points=torch.from_numpy(pts[cls]).to(dev), sym_infos=[syms[c] for c in cls], extents=torch.from_numpy(ext[cls]).to(dev))

        def clear():
            for k in LEAVES:
                t[k].grad = None

        def step_kernels():
            clear()
            loss = L.gdrn_loss(cfg, out_centroid=t["pred_t_"][:, :2], out_trans_z=t["pred_t_"][:, 2], **common, **tables)
            sum(loss.values()).backward()
            return loss

        def step_torch():
            clear()
            loss, _ = LR.gdrn_loss_ref(lc, out_centroid=t["pred_t_"][:, :2], out_trans_z=t["pred_t_"][:, 2], **common, **per_roi)
            sum(loss.values()).backward()
            return loss

        # the two paths compute the same thing
        a, b = step_kernels(), step_torch()
        agree = {k: abs(float(a[k]) - float(b[k])) / abs(float(b[k])) for k in b}
        for fn in (step_kernels, step_torch):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {"kernels": [], "torch": []}
        for _ in range(args.rounds):
            for name, fn in (("kernels", step_kernels), ("torch", step_torch)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.reps * 1e3)
        launches = {}
        for name, fn in (("kernels", step_kernels), ("torch", step_torch)):
            try:
                from torch.autograd import DeviceType
                from torch.profiler import ProfilerActivity, profile

                with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                    fn()
                    torch.cuda.synchronize()
                ev = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
                launches[name] = {"device_events": len(ev), "copies": sum("emcpy" in e.name for e in ev)}
            except Exception as exc:      # noqa: BLE001
                launches[name] = {"not_measured": repr(exc)[:200]}
        case = {"rois": B, "max_relative_difference_of_the_losses": max(agree.values()), "launches": launches}
        for name, v in times.items():
            case[f"{name}_ms_per_step"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        result["cases"].append(case)
        print(json.dumps(case))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
