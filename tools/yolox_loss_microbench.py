"""Microbenchmark of YOLOX's training losses on one MI355X: ``det.yolox.models.losses.yolox_losses`` on the HIP kernels of
csrc/yolox_loss.hip (SimOTA assignment + losses + backward, nothing read back) against the package's own batch-wise torch-operator path
(``yolox_losses_torch``) on the same GPU and the same inputs.

Shape: the detector's real one — 640 x 640 images, 8400 anchors (80 x 80, 40 x 40, 20 x 20), 21 classes, batch 16, 1 .. 30 gts per
image in 32 label rows; predictions near two thirds of the gts are close to them, so dynamic_k spans 1 .. 10 and anchors are contested.
Both loss configurations of the tests: iou + bce and giou + focal + l1.

A transcription of the reference's per-image Python loop is not timed: this repository carries none of the reference's program text,
and tests/yolox_loss_ref.py, the per-image restatement of the tests, also computes selection margins with extra host round trips, so
its time would say nothing about the reference's.

Measured per variant: forward + backward of the loss alone (the raw rows are a leaf that requires grad) by the host clock around
``--reps`` steps that end in a device synchronise, the variants alternating within each of ``--rounds`` rounds, after a warm-up of
both; median / min / max over the rounds.  Nothing here is gated.

    python tools/yolox_loss_microbench.py [--out profiles/yolox_loss_microbench.json] [--batch 16] [--reps 20] [--rounds 9]
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

SIZE, STRIDES, C, G = 640, (8, 16, 32), 21, 32
CONFIGS = {"iou_bce": dict(iou_loss_type="iou", cls_loss_type="bce", use_l1=False),
           "giou_focal_l1": dict(iou_loss_type="giou", cls_loss_type="focal", use_l1=True)}


def build(rng, B):
    an = []
    for s in STRIDES:
        n = SIZE // s
        ys, xs = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
        an.append(np.stack([xs.ravel(), ys.ravel(), np.full(n * n, s)], 1))
    an = np.concatenate(an).astype(np.float32)
    A = len(an)
    raw = np.concatenate([rng.normal(0, 0.5, (B, A, 4)), rng.normal(-2.0, 1.5, (B, A, 1 + C))], 2).astype(np.float32)
    labels = np.zeros((B, G, 5), np.float32)
    xc, yc = an[:, 0] * an[:, 2] + 0.5 * an[:, 2], an[:, 1] * an[:, 2] + 0.5 * an[:, 2]
    for b in range(B):
        for j in range(int(rng.integers(1, 31))):
            w, h = rng.uniform(0.05, 0.5, 2) * SIZE
            k, cx, cy = int(rng.integers(0, C)), rng.uniform(0.1, 0.9) * SIZE, rng.uniform(0.1, 0.9) * SIZE
            labels[b, j] = (k, cx, cy, w, h)
            if rng.uniform() < 0.67:
                near = (np.abs(xc - cx) < 2.5 * an[:, 2]) & (np.abs(yc - cy) < 2.5 * an[:, 2]) & (rng.uniform(size=A) < 0.7)
                n = int(near.sum())
                raw[b, near, 0] = cx / an[near, 2] - an[near, 0] + rng.normal(0, 0.12, n)
                raw[b, near, 1] = cy / an[near, 2] - an[near, 1] + rng.normal(0, 0.12, n)
                raw[b, near, 2] = np.log(w / an[near, 2]) + rng.normal(0, 0.15, n)
                raw[b, near, 3] = np.log(h / an[near, 2]) + rng.normal(0, 0.15, n)
                raw[b, near, 4] += 2.0
                raw[b, near, 5 + k] += 3.0
    return an, raw, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolox_loss_microbench.json"))
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=9)
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd.det.yolox.models import losses as L

    assert torch.cuda.is_available(), "yolox_loss_microbench needs the GPU"
    dev = torch.device("cuda")
    an, raw_np, labels_np = build(np.random.default_rng(20221019), args.batch)
    anchors, labels = torch.from_numpy(an).to(dev), torch.from_numpy(labels_np).to(dev)
    raw = torch.from_numpy(raw_np).to(dev).requires_grad_(True)
    result = {"device": torch.cuda.get_device_name(0), "shape": dict(batch=args.batch, anchors=len(an), classes=C, label_rows=G, image=SIZE),
              "reps": args.reps, "rounds": args.rounds, "cases": []}
    for name, opts in CONFIGS.items():
        def step_kernels():
            raw.grad = None
            losses, info = L.yolox_losses(raw, anchors, labels, **opts)
            sum(losses.values()).backward()
            return losses, info

        def step_torch():
            raw.grad = None
            losses, info = L.yolox_losses_torch(raw, anchors, labels, **opts)
            sum(losses.values()).backward()
            return losses, info

        (a, ia), (b, ib) = step_kernels(), step_torch()
        a, b = ({k: float(v.detach()) for k, v in d.items()} for d in (a, b))
        agree = {k: abs(a[k] - b[k]) / abs(b[k]) for k in b if b[k] != 0.0}
        differing = int((ia["matched_gt"] != ib["matched_gt"]).sum())      # random inputs carry no selection margins: a few may differ
        for fn in (step_kernels, step_torch):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {"kernels": [], "torch": []}
        for _ in range(args.rounds):
            for variant, fn in (("kernels", step_kernels), ("torch", step_torch)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                times[variant].append((time.perf_counter() - t0) / args.reps * 1e3)
        case = {"config": name, "num_gt": int(ia["num_gt"].sum()), "num_fg": int(ia["num_fg"].sum()), "anchors_assigned_differently": differing,
                "max_relative_difference_of_the_losses": max(agree.values())}
        for variant, v in times.items():
            case[f"{variant}_ms_per_step"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        result["cases"].append(case)
        print(json.dumps(case))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
