"""Microbenchmark of ``gdrnpp_gt_xyz_crop`` (csrc/xyz_crop.hip) on one MI355X at the BOP image size: 640x480, an icosphere of subdivision 4
(2 562 vertices, 5 120 faces, ~100 mm across at 0.6 - 1.1 m: the scenes and poses of tools/vsd_bench.py), 4 images x 4 objects x 16 poses =
256 ground-truth poses in one launch.

Measured: the entry point alone (workspace, rows and packed buffer allocated beforehand, no read-back), hipEvents around each call on a
warmed kernel, median / min / max of ``--reps``; the binding ``hip_lib.gt_xyz_crops`` end to end (launch, one device-to-host copy, host
arrays) by wall clock around a synchronised call; and, as the nearest existing sibling, ``gdrnpp_gt_visibility`` with masks on the plain
image for the same poses.  Beside them the bytes the header of csrc/xyz_crop.hip counts per pose (6 B per box pixel written, 40 B per
staged vertex, 48 B of the row; 12 F + 12 V of the model read once) as a fraction of the HBM rate over the measured time, and the face
walk's L2 gathers and fp64 operations by tools/vsd_bench.py's per-item figures: which of them bounds the call.  The first ``--cpu-poses``
go through tests/xyz_crop_ref.py: the check (rows and float16 bits equal).  Nothing here is gated.

    python tools/xyz_crop_bench.py [--out profiles/xyz_crop_bench.json] [--reps 20] [--cpu-poses 2]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import vsd_bench as VB  # noqa: E402

W, H, TILE, K = VB.W, VB.H, VB.TILE, VB.K
Z_NEAR, Z_FAR = 1.0, 1e6                 # millimetres, as the scenes of vsd_bench.py
OPS_PIXEL = 40                           # csrc/xyz_crop.hip, header: fp32 operations per covered pixel


def timed(call, reps):
    import torch

    for _ in range(3):
        call()
    torch.cuda.synchronize()
    evs = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        call()
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(z) for a, z in evs]
    return dict(median=statistics.median(ms), min=min(ms), max=max(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "xyz_crop_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-poses", type=int, default=2)
    args = ap.parse_args()
    import torch

    import gt_info_bench as GB
    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.hip_lib import abi
    from tests import xyz_crop_ref as XR

    assert torch.cuda.is_available(), "xyz_crop_bench needs the GPU"
    lib = hip_lib.load()
    dev = torch.device("cuda")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    rng = np.random.default_rng(104)
    verts, faces, images, pairs = VB.build(rng, 4, n_im=4)
    poses = [(p[1], p[2]) for p in pairs]
    im_of = [p[0] for p in pairs]
    n = len(poses)
    assert n == 256 and len(faces) == 5120
    meshes = hip_lib.MeshSet([verts], [faces], dev)
    obj, im_idx = T(np.zeros(n, np.int32)), T(np.array(im_of, np.int32))
    R, t, Kd = T(np.stack([r.reshape(9) for r, _ in poses])), T(np.stack([x for _, x in poses])), T(np.repeat(K.reshape(1, 9), n, 0))

    # ---- the entry point alone -------------------------------------------------------------------------------------------------------------
    cap = 16 * H * W
    nbytes = lib.gdrnpp_gt_xyz_crop_workspace_bytes(meshes.c, n)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    out = torch.empty((3 * cap,), dtype=torch.float16, device=dev)
    rows = torch.empty((n, 12), dtype=torch.int32, device=dev)
    totals = torch.empty((2,), dtype=torch.int64, device=dev)

    def call():
        abi.launch("gdrnpp_gt_xyz_crop", meshes.c, obj.data_ptr(), R.data_ptr(), t.data_ptr(), Kd.data_ptr(), H, W, Z_NEAR, Z_FAR, out.data_ptr(), cap,
                   rows.data_ptr(), totals.data_ptr(), n, ws.data_ptr(), nbytes)

    ms = timed(call, args.reps)
    n_done, used = totals.tolist()
    got = rows.cpu().numpy()
    assert n_done == n and (got[:, 0] == 0).all(), "the bench's capacity must serve every pose in one launch"
    covered = int(got[:, 1].sum())
    sec = ms["median"] * 1e-3
    hbm_written = 6 * used + n * len(verts) * VB.B_VERTEX_STAGE + n * 48
    hbm = hbm_written + 12 * len(faces) + 12 * len(verts)
    alg = GB.algorithmic(verts, faces, poses, (0, 0), 0, False)            # the face walk's counts: vertices, faces x tiles, candidate centres
    l2, ops64 = alg["l2_bytes"], alg["fp64_ops"]
    least = {"hbm_write": hbm_written / VB.HBM_BYTES, "l2_gather": l2 / VB.L2_BYTES, "fp64_valu": ops64 / VB.F64_VALU_OPS,
             "fp32_valu_pixels": covered * OPS_PIXEL / (2 * VB.F64_VALU_OPS)}
    res = dict(device=torch.cuda.get_device_name(0), image=[W, H], vertices=len(verts), faces=len(faces), poses=n, reps=args.reps,
               workspace_bytes=int(nbytes), box_pixels=int(used), covered_pixels=covered,
               entry_point=dict(hip_ms=ms, poses_per_s=n / sec, us_per_pose=sec * 1e6 / n, hbm_bytes=int(hbm), hbm_bytes_written=int(hbm_written),
                                hbm_write_bytes_per_s=hbm_written / sec, fraction_of_hbm_write_roofline=hbm_written / VB.HBM_BYTES / sec,
                                l2_bytes=int(l2), fp64_ops=int(ops64), least_seconds=least, bound_by=max(least, key=least.get),
                                roofline_fraction=max(least.values()) / sec))
    print(f"gdrnpp_gt_xyz_crop, {n} poses, {len(faces)} faces, {W}x{H}: {ms['median']:.3f} ms (min {ms['min']:.3f}, max {ms['max']:.3f}) = "
          f"{n / sec:.0f} poses/s; {used} box px, {covered} covered; HBM written {hbm_written / 1e6:.2f} MB = "
          f"{100 * res['entry_point']['fraction_of_hbm_write_roofline']:.2f} % of the HBM write roofline; least time by "
          f"{res['entry_point']['bound_by']}: {100 * res['entry_point']['roofline_fraction']:.1f} % of the call", flush=True)

    # ---- the binding end to end ------------------------------------------------------------------------------------------------------------
    wall = []
    for k in range(3 + min(args.reps, 10)):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        packed, table = hip_lib.gt_xyz_crops(meshes, obj, R, t, Kd, (W, H), z_near=Z_NEAR, z_far=Z_FAR)
        if k >= 3:
            wall.append(time.perf_counter() - t0)
    med = statistics.median(wall)
    res["binding"] = dict(wall_ms=dict(median=med * 1e3, min=min(wall) * 1e3, max=max(wall) * 1e3), poses_per_s=n / med, packed_pixels=int(len(packed)))
    print(f"hip_lib.gt_xyz_crops end to end (launch + one copy + host arrays): {med * 1e3:.3f} ms = {n / med:.0f} poses/s", flush=True)

    # ---- the nearest sibling: gt_visibility with masks on the plain image ----------------------------------------------------------------
    imgs = T(images)
    info = torch.empty((n, 11), dtype=torch.int32, device=dev)
    mask = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    visib = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    nb2 = lib.gdrnpp_gt_visibility_workspace_bytes(meshes.c, n)
    ws2 = torch.empty((nb2,), dtype=torch.uint8, device=dev)

    def sibling():
        abi.launch("gdrnpp_gt_visibility", meshes.c, obj.data_ptr(), im_idx.data_ptr(), R.data_ptr(), t.data_ptr(), Kd.data_ptr(), imgs.data_ptr(),
                   len(images), H, W, 0, 0, VB.DELTA, Z_NEAR, Z_FAR, info.data_ptr(), mask.data_ptr(), visib.data_ptr(), n, ws2.data_ptr(), nb2)

    ms2 = timed(sibling, args.reps)
    res["gt_visibility_masks_plain_image"] = dict(hip_ms=ms2, poses_per_s=n / (ms2["median"] * 1e-3))
    assert np.array_equal(info.cpu().numpy()[:, 0], got[:, 1]), "both kernels render the same silhouettes"
    print(f"gdrnpp_gt_visibility(want_masks) on the same poses: {ms2['median']:.3f} ms = {n / (ms2['median'] * 1e-3):.0f} poses/s", flush=True)

    # ---- the check ---------------------------------------------------------------------------------------------------------------------------
    m = min(args.cpu_poses, n)
    if m:
        equal = True
        for k in range(m):
            r = XR.xyz_crop_ref(verts, faces, poses[k][0], poses[k][1], K, W, H, Z_NEAR, Z_FAR)
            b = XR.pose_box(verts, K, poses[k][0], poses[k][1], W, H, Z_NEAR, Z_FAR)
            row = table[k].tolist()
            box = packed[row[10]:row[10] + (b[1] - b[0] + 1) * (b[3] - b[2] + 1)].reshape(b[3] - b[2] + 1, b[1] - b[0] + 1, 3)
            want = r["full"][b[2]:b[3] + 1, b[0]:b[1] + 1]
            equal &= row[:10] == [0, r["count"]] + r["xyxy"] + b
            equal &= bool(((box.view(np.uint16) == want.view(np.uint16)) | ((box == 0) & (want == 0))).all())
        res["cpu_poses"], res["equal_to_restatement"] = m, bool(equal)
        print("equal to tests/xyz_crop_ref.py on", m, "poses:", bool(equal), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
