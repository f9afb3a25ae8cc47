"""Microbenchmark of ``gdrnpp_roi_train_targets`` (csrc/roi_targets.hip) on one MI355X at the BOP image size: 640x480, ``--rois`` instances
(default 128) whose xyz crops are ~120 x 100 px float16 blobs, two masks each, 64 farthest-point-sampling points per object, 64 x 64 targets
with 64 bins: the shapes of one training batch of the shipped configs.

Measured: the entry point alone (every buffer allocated and every index uploaded beforehand), hipEvents around each call on a warmed
kernel, median / min / max of ``--reps``; the binding ``hip_lib.roi_train_targets`` end to end (host checks of the indices, one upload,
the launch, outputs preallocated) by wall clock around a synchronised call; and the NumPy restatement of the reference's per-instance
path (tests/roi_targets_ref.py: the crop pasted into a full image, full-image masks, five nearest-neighbour warps through the C oracle,
the fp64 distances, normalisation and bins) on the first ``--cpu-rois`` of the same ROIs on this machine's CPU, one thread, which also
serves as the check (every output equal).  The restatement is not the reference's own code: its warps are the oracle's C loops where the
reference calls OpenCV, and its distances are NumPy where the reference calls scipy.  Nothing here is gated.

    python tools/roi_targets_bench.py [--out profiles/roi_targets_bench.md] [--rois 128] [--reps 20] [--cpu-rois 8]
"""
import argparse
import os
import platform
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

W, H, OUT, F, N_BIN, N_OBJ = 640, 480, 64, 64, 64, 8
HBM_BYTES = 8e12                          # bytes/s, the MI355X's HBM3E rate the other benches here use


def build(rng, n):
    recs, masks = [], np.zeros((2 * n, H, W), np.uint8)
    for k in range(n):
        w, h = int(rng.integers(90, 150)), int(rng.integers(70, 130))
        x1, y1 = int(rng.integers(0, W - w)), int(rng.integers(0, H - h))
        yy, xx = np.mgrid[0:h, 0:w]
        inside = ((xx - w / 2) / (w / 2)) ** 2 + ((yy - h / 2) / (h / 2)) ** 2 <= 1.0
        crop = (rng.uniform(-0.05, 0.05, (h, w, 3)) * inside[:, :, None]).astype(np.float16)
        recs.append({"xyz_crop": crop, "xyxy": [x1, y1, x1 + w - 1, y1 + h - 1]})
        masks[2 * k, y1:y1 + h, x1:x1 + w] = inside & (xx > w // 5)              # visible: the object minus an occluded strip
        masks[2 * k + 1, y1:y1 + h, x1:x1 + w] = 1                                # full: the box
    centers = np.array([[0.5 * (r["xyxy"][0] + r["xyxy"][2]), 0.5 * (r["xyxy"][1] + r["xyxy"][3])] for r in recs]) + rng.uniform(-8, 8, (n, 2))
    scales = np.array([max(r["xyxy"][2] - r["xyxy"][0], r["xyxy"][3] - r["xyxy"][1]) for r in recs]) * rng.uniform(1.1, 1.9, n)
    return recs, masks, centers, np.minimum(scales, float(W))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "roi_targets_bench.md"))
    ap.add_argument("--rois", type=int, default=128)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-rois", type=int, default=8)
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import train_targets as TT
    from gdrnpp_bop2022_amd.hip_lib import abi
    from tests import roi_targets_ref as RR

    assert torch.cuda.is_available(), "roi_targets_bench needs the GPU"
    dev = torch.device("cuda")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rng = np.random.default_rng(105)
    n = args.rois
    recs, masks_h, centers_h, scales_h = build(rng, n)
    extents_h = rng.uniform(0.09, 0.11, (N_OBJ, 3)).astype(np.float32)
    fps_h = rng.uniform(-0.05, 0.05, (N_OBJ, F, 3))
    obj_h = np.arange(n) % N_OBJ
    vis_h, full_h, none_h = 2 * np.arange(n), 2 * np.arange(n) + 1, np.full((n,), -1)
    packed, table = TT.pack_records(recs, (W, H), dev)
    masks, centers, scales, extents, fps = T(masks_h), T(centers_h), T(scales_h), T(extents_h), T(fps_h)
    out = {k: torch.empty((n, OUT, OUT) if ch is None else (n, ch, OUT, OUT), dtype=dt, device=dev) for k, (dt, ch) in hip_lib.ROI_TARGET_KEYS.items()}
    kw = dict(masks=masks, visib_idx=vis_h, trunc_idx=none_h, full_idx=full_h, obj=obj_h, extents=extents, fps=fps, out_res=OUT, n_bin=N_BIN, bin_mask="visib")

    # ---- the entry point alone ---------------------------------------------------------------------------------------------------------
    off = T(table[:, 10].astype(np.int64))
    box = T(table[:, [6, 8, 7, 9]].astype(np.int32))
    cols = [T(c.astype(np.int32)) for c in (vis_h, none_h, full_h, obj_h)]

    def call():
        abi.launch("gdrnpp_roi_train_targets", packed.data_ptr(), packed.shape[0], off.data_ptr(), box.data_ptr(), masks.data_ptr(), 2 * n, cols[0].data_ptr(),
                   cols[1].data_ptr(), cols[2].data_ptr(), H, W, centers.data_ptr(), scales.data_ptr(), cols[3].data_ptr(), extents.data_ptr(), N_OBJ,
                   fps.data_ptr(), F, OUT, N_BIN, 1, *[out[k].data_ptr() for k in hip_lib.ROI_TARGET_KEYS], n)

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    evs = []
    for _ in range(args.reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(z) for a, z in evs]
    med, lo, hi = statistics.median(ms), min(ms), max(ms)
    alone = {k: v.cpu().numpy() for k, v in out.items()}
    written = n * OUT * OUT * (4 * 4 + 4 + 12 + 3)                             # four masks, region, xyz, bins: 35 bytes per output pixel
    print(f"gdrnpp_roi_train_targets, {n} ROIs, {W}x{H} -> {OUT}x{OUT}, F={F}, {N_BIN} bins: {med:.4f} ms (min {lo:.4f}, max {hi:.4f}) = "
          f"{med * 1e3 / n:.3f} us per ROI; {written / 1e6:.2f} MB written = {100 * written / HBM_BYTES / (med * 1e-3):.2f} % of the HBM write roofline", flush=True)

    # ---- the binding end to end ----------------------------------------------------------------------------------------------------------
    wall = []
    for k in range(3 + min(args.reps, 10)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        hip_lib.roi_train_targets(packed, table, centers, scales, (W, H), out=out, **kw)
        torch.cuda.synchronize()
        if k >= 3:
            wall.append(time.perf_counter() - t0)
    bmed = statistics.median(wall)
    bound = {k: v.cpu().numpy() for k, v in out.items()}
    same = all(np.array_equal(alone[k], bound[k]) for k in alone)
    print(f"hip_lib.roi_train_targets end to end (index checks, one upload, launch, synchronise): {bmed * 1e3:.3f} ms = {bmed * 1e6 / n:.2f} us per ROI; "
          f"equal to the entry point alone: {same}", flush=True)

    # ---- the restatement of the per-instance reference path on this machine's CPU --------------------------------------------------------
    m = min(args.cpu_rois, n)
    packed_h = packed.cpu().numpy()
    per = []
    equal = True
    for k in range(m):
        t0 = time.perf_counter()
        ref = RR.batch_ref(packed_h, table, centers_h[k:k + 1], scales_h[k:k + 1], (W, H), src=[k], masks=masks_h, visib_idx=vis_h[k:k + 1], trunc_idx=none_h[k:k + 1],
                           full_idx=full_h[k:k + 1], obj=obj_h[k:k + 1], extents=extents_h, fps=fps_h, out_res=OUT, n_bin=N_BIN, bin_mask="visib")
        per.append(time.perf_counter() - t0)
        equal &= all(np.array_equal(ref[key][0], bound[key][k]) for key in ref)
    cmed = statistics.median(per)
    print(f"tests/roi_targets_ref.py, per instance on the CPU: {cmed * 1e3:.2f} ms (min {min(per) * 1e3:.2f}, max {max(per) * 1e3:.2f}) over {m} ROIs; "
          f"equal to the device: {equal}", flush=True)

    cpu = platform.processor() or platform.machine()
    try:
        with open("/proc/cpuinfo") as f:
            cpu = next((line.split(":", 1)[1].strip() for line in f if line.startswith("model name")), cpu)
    except OSError:
        pass
    text = f"""# Per-ROI training targets on the device: `tools/roi_targets_bench.py` on one MI355X

Box: {torch.cuda.get_device_name(0)} (gfx950), ROCm PyTorch {torch.__version__}; host CPU {cpu}.  Workload: {W} x {H}, {n} instances with float16
crops of about 120 x 100 px, two masks each, {F} points per object, {OUT} x {OUT} targets, {N_BIN} bins under the visible mask: all seven outputs.
hipEvents around each call on a warmed kernel, median (min - max) of {args.reps}; wall clock for the other two rows.  Nothing is gated.

| what | time for the batch | per ROI |
|---|---|---|
| `gdrnpp_roi_train_targets`, entry point alone (buffers and indices on the device beforehand) | {med:.4f} ms ({lo:.4f} - {hi:.4f}) | {med * 1e3 / n:.3f} us |
| `hip_lib.roi_train_targets` end to end: host index checks, one upload, launch, synchronise (wall clock, {len(wall)} calls) | {bmed * 1e3:.3f} ms ({min(wall) * 1e3:.3f} - {max(wall) * 1e3:.3f}) | {bmed * 1e6 / n:.2f} us |
| `tests/roi_targets_ref.py`, the NumPy restatement of the per-instance reference path, one CPU thread ({m} ROIs, median) | {cmed * 1e3 * n:.1f} ms extrapolated to {n} | {cmed * 1e3:.2f} ms ({min(per) * 1e3:.2f} - {max(per) * 1e3:.2f}) |

The launch writes {written / 1e6:.2f} MB (35 bytes per output pixel) = {100 * written / HBM_BYTES / (med * 1e-3):.2f} % of the 8 TB/s HBM write roofline over the measured time: the call is
bound by launch latency and the per-workgroup prologue (one lane solves the ROI's affine map), not by traffic or arithmetic.  The restatement's
time is what this machine's CPU needs for the reference's recipe (a zeroed {H} x {W} x 3 float32 image, full-image float masks, five warps through
the C oracle, {OUT * OUT} x {F} fp64 distances in NumPy); it is not a measurement of the reference's own OpenCV / scipy calls.
Outputs: the entry point and the binding are equal ({same}); the first {m} ROIs equal the restatement on every output ({equal}).
"""
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
