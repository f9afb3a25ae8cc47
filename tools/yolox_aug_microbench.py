"""Microbenchmark of YOLOX's training-batch augmentation on one MI355X: one call of ``hip_lib.yolox_train_inputs`` (csrc/yolox_aug.hip: the
mosaic and mixup canvases, then warpAffine, the mixup blend, two HSV passes, mirror and preproc per output pixel) for a training batch.

Shapes: ``--images`` 64 (the batch of configs/yolox/bop_pbr/yolox_base.py) at 640 x 640 from a dataset of sixteen 640 x 480 images with
three boxes each; every item takes the heaviest branch — mosaic + mixup, HSV pass 1 and pass 2 — which the tool asserts of the plans.

Measured, by the host clock around ``--reps`` calls that end in a device synchronise, median / min / max over ``--rounds`` rounds after a
warm-up: (1) the device call with the sources already uploaded — the table check, the one staged copy and the two launches; its output
(315 MB) and workspace (524 MB) exceed the 256 MB last-level cache, so a call does not find the bytes of the call before; (2)
``MosaicDetectionHip.batch`` end to end: the host's draws and box arithmetic, the upload of every source image as ``pull_item`` returned
it (five per item, 295 MB a batch), and the call.  The first and last item are compared with the NumPy restatement
(tests/yolox_aug_ref.py) before anything is timed.

Reported beside them: the algorithmic bytes of (1) — every source read once, the canvases (4 bytes a pixel: 2H x 2W and H x W per item)
written once and read once, the f32 output written once — and the share of the 8.0 TB/s HBM peak they make of the measured time (a
whole-call rate: it includes the staged copy and the launch gaps, it is not a kernel's share of peak); and the YOLOX-x forward + backward
time per image already recorded in profiles/yolox_train_microbench.json, so the share of a training step shows.  Nothing here is gated.

    python tools/yolox_aug_microbench.py [--out profiles/yolox_aug_microbench.json] [--images 64] [--reps 20] [--rounds 7]
"""
import argparse
import json
import os
import random
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W = 640, 640
SRC_H, SRC_W, N_SRC = 480, 640, 16
HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolox_aug_microbench.json"))
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batch-rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.det.yolox.data import data_augment as DA
    from gdrnpp_bop2022_amd.det.yolox.data import mosaic as MZ
    from tests import yolox_aug_ref as R

    assert torch.cuda.is_available(), "yolox_aug_microbench needs the GPU"
    dev = torch.device("cuda")
    B = args.images
    dataset = R.StubDataset([(SRC_H, SRC_W)] * N_SRC, [3] * N_SRC, (H, W), 20221021, box_px=(40, 160))
    wrapper = MZ.MosaicDetectionHip(dataset, (H, W), hsv_prob=1.0, AUG_HSV_PROB=1.0, HSV_H=0.015, HSV_S=0.7, HSV_V=0.4, FORMAT="RGB")
    indices = [b % N_SRC for b in range(B)]
    py, npr = random.Random(0), np.random.RandomState(0)
    items = wrapper.plan(indices, py_random=py, np_random=npr)
    assert all(it["branch"] == "mixup" and it["hsv"] and it["hsv2"] for it in items), "every item takes mosaic + mixup + both HSV passes"

    # the pieces of launch_items, kept apart so that the sources are uploaded once
    images, rows, luts, off = [], [], [], 0
    for it in items:
        offsets = []
        for s in it["sources"]:
            offsets.append(off)
            images.append(np.ascontiguousarray(s["image"]).reshape(-1))
            off += images[-1].size
        row, lut = MZ.item_row(it, offsets)
        rows.append(row)
        luts.append(lut)
    src = torch.from_numpy(np.concatenate(images)).to(dev)
    lut = torch.from_numpy(np.stack(luts)).to(dev)
    table = hip_lib.yolox_aug_table(rows)
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)

    def call():
        return hip_lib.yolox_train_inputs(src, table, lut, H, W, out=out)

    _, flags = call()
    torch.cuda.synchronize()
    assert not flags.any().item()
    for b in (0, B - 1):
        assert (out[b].cpu().numpy() == R.run_item(items[b], DA.hsv_luts)).all(), b
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    call_ms = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            call()
        torch.cuda.synchronize()
        call_ms.append((time.perf_counter() - t0) / args.reps * 1e3)
    batch_ms = []
    wrapper.batch(indices, py_random=py, np_random=npr)
    for _ in range(args.batch_rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        wrapper.batch(indices, py_random=py, np_random=npr)
        torch.cuda.synchronize()
        batch_ms.append((time.perf_counter() - t0) * 1e3)
    summary = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}          # noqa: E731
    canvas_bytes = 4 * (2 * H * 2 * W + H * W)
    algorithmic_bytes = int(src.numel() + B * (2 * canvas_bytes + 12 * H * W))
    stats = summary(call_ms)
    result = {"device": torch.cuda.get_device_name(0), "images": B, "input": [H, W], "source_size": [SRC_W, SRC_H], "branch": "mosaic + mixup, HSV pass 1 and 2",
              "reps": args.reps, "rounds": args.rounds, "yolox_train_inputs_ms_per_batch": stats, "mosaic_batch_end_to_end_ms": summary(batch_ms),
              "uploaded_source_bytes_per_batch": int(src.numel()), "algorithmic_bytes": algorithmic_bytes,
              "algorithmic_bytes_per_second": algorithmic_bytes / (stats["median"] * 1e-3),
              "share_of_hbm_peak_8TBps_whole_call": algorithmic_bytes / (stats["median"] * 1e-3) / HBM_PEAK}
    recorded = os.path.join(ROOT, "profiles", "yolox_train_microbench.json")
    if os.path.exists(recorded):
        model = json.load(open(recorded))["model"]
        step = model["hip_fwd_bwd_ms"]["median"] / model["batch"]
        result["yolox_x_fwd_bwd_ms_per_image_recorded"] = step
        result["yolox_train_inputs_ms_per_image"] = stats["median"] / B
        result["share_of_a_yolox_x_step"] = (stats["median"] / B) / step
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
