"""Microbenchmark of background replacement on one MI355X: one call of ``hip_lib.replace_bg`` (csrc/replace_bg.hip: the mask extents, the
cut, the resize of the background and the composite) for a training batch against the same batch through the NumPy restatement of the
reference's per-sample host code (tests/replace_bg_ref.py ``replace_bg_ref``), image after image on one host core.

Shapes: ``--images`` 48 (the largest IMS_PER_BATCH of the shipped configs) of 640 x 480, a pool of eight backgrounds of 500 x 375 and
375 x 500 (the VOC sizes), every image replaced, the five branches of trunc_mask in turn, masks that are a filled ellipse of about a
sixth of the image.

Measured: the device call by the host clock around ``--reps`` calls that end in a device synchronise (so it includes the table check, the
one staged copy and the launches), median / min / max over ``--rounds`` rounds after a warm-up.  The calls walk round ``--copies`` copies
of the batch (images, masks and mask_trunc: 74 MB each), so that a call does not find its own bytes of the call before in the 256 MB
last-level cache — a training loop's batch arrives fresh too.  The host path by the host clock around one
pass over the batch, ``--host-rounds`` times.  The restatement is NumPy, not OpenCV: cv2's vectorised resize is faster than it, so the
host figure bounds the reference's cost from above and is not a measurement of it.  The first and last image of the batch are compared
with the restatement before anything is timed.  Nothing here is gated.

    python tools/replace_bg_microbench.py [--out profiles/replace_bg_microbench.json] [--images 48] [--copies 6] [--reps 300] [--rounds 7]
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

H, W = 480, 640
BG_SIZES = [(375, 500), (500, 375)] * 4


def build(rng, B):
    images = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    masks = np.zeros((B, H, W), np.uint8)
    for b in range(B):
        cy, cx, ry, rx = rng.uniform(150, 330), rng.uniform(200, 440), rng.uniform(80, 130), rng.uniform(100, 160)
        masks[b] = (((yy - cy) / ry) ** 2 + ((xx - cx) / rx) ** 2 <= 1.0)
    bgs = [rng.integers(0, 256, s + (3,), dtype=np.uint8) for s in BG_SIZES]
    spec = [(int(rng.integers(len(bgs))), b % 5, float(rng.random())) for b in range(B)]       # background, cut, u
    return images, masks, bgs, spec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "replace_bg_microbench.json"))
    ap.add_argument("--images", type=int, default=48)
    ap.add_argument("--copies", type=int, default=6)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--host-rounds", type=int, default=3)
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import train_inputs as TI
    from tests import replace_bg_ref as R

    assert torch.cuda.is_available(), "replace_bg_microbench needs the GPU"
    dev = torch.device("cuda")
    B = args.images
    images, masks, bgs, spec = build(np.random.default_rng(20221020), B)
    pool = TI.BgPool(bgs, dev)
    rows = [dict(do=1, bg_off=pool.offsets[i], bg_stride=pool.sizes[i][1], cut=cut, u=u, **TI.bg_geometry(*pool.sizes[i], H, W))
            for i, cut, u in spec]
    table = hip_lib.replace_bg_table(rows)
    sets = [(torch.from_numpy(images).to(dev), torch.from_numpy(masks).to(dev), torch.zeros((B, H, W), dtype=torch.uint8, device=dev))
            for _ in range(args.copies)]
    d_images, _, d_out = sets[0]
    calls = [0]

    def step():
        im, ma, out = sets[calls[0] % len(sets)]
        calls[0] += 1
        hip_lib.replace_bg(im, ma, pool.data, table, out_mask=out)

    for _ in sets:
        step()
    torch.cuda.synchronize()
    for b in (0, B - 1):
        ref, keep = R.replace_bg_ref(images[b], masks[b], bgs[spec[b][0]], spec[b][1], spec[b][2])
        assert (d_images[b].cpu().numpy() == ref).all() and ((d_out[b].cpu().numpy() != 0) == keep).all(), b
    for _ in range(3 * len(sets)):
        step()
    torch.cuda.synchronize()
    device_ms = []
    for _ in range(args.rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            step()
        torch.cuda.synchronize()
        device_ms.append((time.perf_counter() - t0) / args.reps * 1e3)
    host_ms = []
    for _ in range(args.host_rounds):
        t0 = time.perf_counter()
        for b in range(B):
            R.replace_bg_ref(images[b], masks[b], bgs[spec[b][0]], spec[b][1], spec[b][2])
        host_ms.append((time.perf_counter() - t0) * 1e3)
    summary = lambda v: {"median": statistics.median(v), "min": min(v), "max": max(v)}          # noqa: E731
    # the mask byte read (once; a cut reads it twice) and the mask_trunc byte written per pixel, three image bytes written per replaced pixel
    algorithmic_bytes = int(B * H * W * 2 + (masks == 0).sum() * 3)
    result = {"device": torch.cuda.get_device_name(0), "images": B, "image_size": [W, H], "backgrounds": BG_SIZES, "copies": args.copies, "reps": args.reps,
              "rounds": args.rounds, "replace_bg_ms_per_batch": summary(device_ms), "replace_bg_ref_one_core_ms_per_batch": summary(host_ms),
              "replaced_pixel_fraction": float((masks == 0).mean()), "algorithmic_bytes": algorithmic_bytes,
              "note": "replace_bg_ref is NumPy, not OpenCV: an upper bound of the reference's host cost, not a measurement of it"}
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
