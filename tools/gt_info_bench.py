"""Microbenchmark of ``gdrnpp_gt_visibility`` (csrc/gt_visib.hip) on one MI355X at the BOP image size: 640x480 depth images, 8 of them with 4
objects each, 16 poses per object = 512 ground-truth poses (the scenes and poses of tools/vsd_bench.py: its ground truths and the estimates
around them), for icosphere subdivision 2 (162 vertices, 320 faces) and 4 (2 562 vertices, 5 120 faces), ~100 mm across at 0.6 - 1.1 m.

Three calls per model: calc_gt_info.py's 3W x 3H canvas without masks, the same with masks, and calc_gt_masks.py's plain image with masks.
Each is the entry point alone (workspace and outputs allocated beforehand, no read-back): hipEvents around each call on a warmed kernel,
median / min / max of ``--reps``; poses/s.  Beside it the least time the chip could take for the operations and bytes the algorithm needs,
counted here from the poses with the per-item figures of the kernel's header (fp64 vector rate, L2 gather bandwidth for the face walk, HBM
for the staged vertices, the depth image and the masks), and which bounds it.  The first ``--cpu-poses`` go through the NumPy restatement
tests/gt_info_ref.py on one core: the check (rows equal) and the CPU figure.

    python tools/gt_info_bench.py [--out profiles/gt_info_bench.json] [--reps 20] [--cpu-poses 2]
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

W, H, TILE, K, DELTA = VB.W, VB.H, VB.TILE, VB.K, VB.DELTA
# csrc/gt_visib.hip, header: fp64 operations per item (the face walk's are vsd_error.hip's)
OPS_PIXEL = 65


def algorithmic(verts, faces, poses, offset, visible, want_masks):
    """The header's operation and byte counts for this workload, from the poses: faces walked (per canvas tile under the pose's box), faces
    with a candidate centre, candidate centres; ``visible``: the covered window pixels (px_count_all on the plain image; on the canvas the
    larger of px_count_valid and px_count_visib, a lower bound: a covered pixel is valid or, over missing depth, visible)."""
    ox, oy = offset
    Wc, Hc = W + 2 * ox, H + 2 * oy
    Kc = K.copy()
    Kc[0, 2], Kc[1, 2] = K[0, 2] + ox, K[1, 2] + oy
    v = verts.astype(np.float64)
    n_walk = n_reach = n_centre = 0
    for R, t in poses:
        h = (v.dot(R.T) + t).dot(Kc.T)
        uv = h[:, :2] / h[:, 2:]
        lo, hi = np.maximum(np.ceil(uv.min(0) - 0.5), 0), np.minimum(np.floor(uv.max(0) - 0.5), [Wc - 1, Hc - 1])
        if (lo > hi).any():
            continue
        n_walk += len(faces) * int((hi[0] // TILE - lo[0] // TILE + 1) * (hi[1] // TILE - lo[1] // TILE + 1))
        fu = uv[faces]
        flo, fhi = np.maximum(np.ceil(fu.min(1) - 0.5), 0), np.minimum(np.floor(fu.max(1) - 0.5), [Wc - 1, Hc - 1])
        ext = np.maximum(fhi - flo + 1, 0)
        area = ext[:, 0] * ext[:, 1]
        n_reach += int((area > 0).sum())
        n_centre += int(area.sum())
    n_vert = len(poses) * len(verts)
    ops = n_vert * VB.OPS_VERTEX + n_walk * VB.OPS_FACE_TEST + n_reach * VB.OPS_FACE_SETUP + n_centre * VB.OPS_CENTRE + int(visible) * OPS_PIXEL
    l2 = n_walk * VB.B_FACE_TEST + n_reach * VB.B_FACE_SETUP
    hbm = n_vert * (VB.B_VERTEX_STAGE + 12) + int(visible) * 4 + len(poses) * 44 + (len(poses) * 2 * H * W + 2 * int(visible) if want_masks else 0)
    bounds = {"fp64_valu": ops / VB.F64_VALU_OPS, "l2_gather": l2 / VB.L2_BYTES, "hbm": hbm / VB.HBM_BYTES}
    return dict(vertices_projected=n_vert, faces_walked=n_walk, faces_with_candidates=n_reach, candidate_centres=n_centre, pixels_compared=int(visible),
                fp64_ops=ops, l2_bytes=l2, hbm_bytes=hbm, least_seconds=bounds, bound_by=max(bounds, key=bounds.get))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gt_info_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-poses", type=int, default=2)
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.hip_lib import abi
    from tests import gt_info_ref as G

    assert torch.cuda.is_available(), "gt_info_bench needs the GPU"
    lib = hip_lib.load()
    dev = torch.device("cuda")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    res = dict(device=torch.cuda.get_device_name(0), image=[W, H], reps=args.reps, delta=DELTA,
               peaks=dict(fp64_valu_ops_per_s=VB.F64_VALU_OPS, l2_gather_bytes_per_s=VB.L2_BYTES, hbm_bytes_per_s=VB.HBM_BYTES), models={})
    for subdiv in (2, 4):
        rng = np.random.default_rng(100 + subdiv)
        verts, faces, images, pairs = VB.build(rng, subdiv)
        poses = [(p[1], p[2]) for p in pairs]                      # vsd_bench's estimates: 16 poses around each of the 32 ground truths
        im_of = [p[0] for p in pairs]
        n = len(poses)
        meshes = hip_lib.MeshSet([verts], [faces], dev)
        d = [T(np.zeros(n, np.int32)), T(np.array(im_of, np.int32)), T(np.stack([R.reshape(9) for R, _ in poses])), T(np.stack([t for _, t in poses])),
             T(np.repeat(K.reshape(1, 9), n, 0)), T(images)]
        info = torch.empty((n, 11), dtype=torch.int32, device=dev)
        mask = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        visib = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
        nbytes = lib.gdrnpp_gt_visibility_workspace_bytes(meshes.c, n)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
        per_model = {}
        for name, offset, want_masks in (("info_3x_canvas", (W, H), False), ("info_and_masks_3x_canvas", (W, H), True), ("masks_plain_image", (0, 0), True)):
            def call():
                abi.launch("gdrnpp_gt_visibility", meshes.c, *[t.data_ptr() for t in d], len(images), H, W, offset[0], offset[1], DELTA, 1.0, 1e6,
                           info.data_ptr(), mask.data_ptr() if want_masks else None, visib.data_ptr() if want_masks else None, n, ws.data_ptr(), nbytes)

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
            med = statistics.median(ms)
            got = info.cpu().numpy()
            alg = algorithmic(verts, faces, poses, offset, got[:, 0].sum() if offset == (0, 0) else np.maximum(got[:, 1], got[:, 2]).sum(), want_masks)
            least = max(alg["least_seconds"].values())
            r = dict(poses=n, hip_ms=dict(median=med, min=min(ms), max=max(ms)), poses_per_s=n / (med * 1e-3), us_per_pose=med * 1e3 / n,
                     algorithmic=alg, fraction_of_bound={k: v / (med * 1e-3) for k, v in alg["least_seconds"].items()}, roofline_fraction=least / (med * 1e-3))
            m = min(args.cpu_poses, n)
            if m:
                t0 = time.perf_counter()
                cpu = [G.gt_visibility_ref(verts, faces, *poses[k], K, images[im_of[k]], DELTA, offset) for k in range(m)]
                r.update(cpu_poses=m, cpu_numpy_one_core_s_per_pose=(time.perf_counter() - t0) / m,
                         rows_equal=bool(np.array_equal(np.array([c[0] for c in cpu]), got[:m])))
                if want_masks:
                    r["masks_equal"] = bool(np.array_equal(np.array([c[1] for c in cpu]), mask[:m].cpu().numpy() == 255)
                                            and np.array_equal(np.array([c[2] for c in cpu]), visib[:m].cpu().numpy() == 255))
            per_model[name] = r
            print(f"{len(faces)} faces, {n} poses, {name}: hip {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) = {r['poses_per_s']:.0f} poses/s, "
                  f"{r['us_per_pose']:.2f} us per pose; least time by {alg['bound_by']}: {100 * r['roofline_fraction']:.1f} % of the call"
                  + (f"; rows equal: {r['rows_equal']}" + (f", masks equal: {r['masks_equal']}" if want_masks else "") if m else ""), flush=True)
        res["models"][f"icosphere_{subdiv}"] = dict(vertices=len(verts), faces=len(faces), images=len(images), workspace_bytes=int(nbytes), calls=per_model)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
