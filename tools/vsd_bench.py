"""Microbenchmark of ``gdrnpp_vsd_counts`` (csrc/vsd_error.hip) on one MI355X at the BOP image size: 640x480 depth images, 8 of them with 4
ground-truth objects each, 16 estimates per ground truth = 512 (estimate, ground truth) pairs, for the two model sizes of the synthetic set:
icosphere subdivision 2 (162 vertices, 320 faces) and 4 (2 562 vertices, 5 120 faces: the size the refine path quotes), ~100 mm across
at 0.6 - 1.1 m.

  (a) hip   one ``hip_lib.vsd_errors``-sized launch through the entry point alone (workspace allocated beforehand, no read-back): hipEvents
            around each call on a warmed kernel, median / min / max of ``--reps``; pairs/s.  Beside it the least time the chip could take for
            the operations and bytes the algorithm needs, counted here from the poses with the per-item figures of the kernel's header
            (fp64 vector rate, L2 gather bandwidth for the face walk, HBM for the staged vertices and the depth image), and which bounds it.
  (b) cpu   the same pairs (the first ``--cpu-pairs``) through the NumPy restatement tests/vsd_ref.py on one core (one Python thread, element-wise NumPy, no
            BLAS); also the check: counts equal.
  (c) per-kernel times come from a profiler run of their own:
            rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/vsd_bench.py --reps 5 --cpu-pairs 0 --out DIR/x.json
            python tools/vsd_bench.py --kernel-stats DIR          (merges the two kernels' average times into --out, no device needed)

    python tools/vsd_bench.py [--out profiles/vsd_bench.json] [--reps 20] [--cpu-pairs 4]
"""
import argparse
import csv
import glob
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F64_VALU_OPS = 78.6e12 / 2          # lane operations per second (the peak counts an fma as two)
L2_BYTES = 17e12                    # rows shared by many workgroups, gathered from the XCDs' L2
HBM_BYTES = 8.0e12
W, H, TILE = 640, 480, 64
K = np.array([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]]).astype(np.float32).astype(np.float64)
TAUS = list(np.arange(0.05, 0.51, 0.05))
DELTA = 15.0
# csrc/vsd_error.hip, header: fp64 operations per item
OPS_VERTEX, OPS_FACE_TEST, OPS_FACE_SETUP, OPS_CENTRE, OPS_PIXEL = 31 + 2 * 13, 20, 60, 18 + 3 + 13, 110
B_FACE_TEST, B_FACE_SETUP, B_VERTEX_STAGE = 12 + 72, 72, 40


def build(rng, subdiv, n_im=8, per_im=4, per_gt=16):
    from scipy.spatial.transform import Rotation

    from gdrnpp_bop2022_amd import synthetic as S
    from tests import vsd_ref as V

    v, f = S.icosphere(subdiv)
    verts, faces = (v * np.array([50.0, 38.0, 30.0])).astype(np.float32), f.astype(np.int32)
    images, pairs = [], []
    for im in range(n_im):
        d = np.full((H, W), 1500.0, np.float32)
        for k in range(per_im):
            z = rng.uniform(600, 1100)
            u, w = (k + 0.5) / per_im * W + rng.uniform(-30, 30), rng.uniform(120, 360)
            t = np.array([(u - K[0, 2]) / K[0, 0] * z, (w - K[1, 2]) / K[1, 1] * z, z])
            R = S.random_rotation(rng).astype(np.float32).astype(np.float64)        # float32 values: the scene is drawn by the C oracle
            r = V.render_oracle(verts, faces, K, R, t, W, H, 1.0, 1e6)
            d = np.where((r > 0) & (r < d), np.round(r), d).astype(np.float32)
            for _ in range(per_gt):
                Re = R.dot(Rotation.from_rotvec(rng.standard_normal(3) * 0.05).as_matrix())
                pairs.append((im, Re, t + rng.standard_normal(3) * 5.0, R, t))
        d[rng.integers(0, H, 200), rng.integers(0, W, 200)] = 0.0
        images.append(d)
    return verts, faces, np.stack(images), pairs


def algorithmic(verts, faces, pairs, union):
    """The header's operation and byte counts for this workload, from the poses: faces walked (per pose and tile under the pose's box),
    faces with a candidate centre, candidate centres; covered pixels taken as the visible ones (``union``)."""
    v = verts.astype(np.float64)
    n_walk = n_reach = n_centre = 0
    for _, Re, te, Rg, tg in pairs:
        for R, t in ((Re, te), (Rg, tg)):
            h = (v.dot(R.T) + t).dot(K.T)
            uv = h[:, :2] / h[:, 2:]
            lo, hi = np.ceil(uv.min(0) - 0.5), np.floor(uv.max(0) - 0.5)
            lo, hi = np.maximum(lo, 0), np.minimum(hi, [W - 1, H - 1])
            if (lo > hi).any():
                continue
            n_walk += len(faces) * int((hi[0] // TILE - lo[0] // TILE + 1) * (hi[1] // TILE - lo[1] // TILE + 1))
            fu = uv[faces]                                        # [F,3,2]
            flo, fhi = np.maximum(np.ceil(fu.min(1) - 0.5), 0), np.minimum(np.floor(fu.max(1) - 0.5), [W - 1, H - 1])
            ext = np.maximum(fhi - flo + 1, 0)
            area = ext[:, 0] * ext[:, 1]
            n_reach += int((area > 0).sum())
            n_centre += int(area.sum())
    n_vert = 2 * len(pairs) * len(verts)
    ops = n_vert * OPS_VERTEX + n_walk * OPS_FACE_TEST + n_reach * OPS_FACE_SETUP + n_centre * OPS_CENTRE + int(union) * OPS_PIXEL
    l2 = n_walk * B_FACE_TEST + n_reach * B_FACE_SETUP
    hbm = n_vert * (B_VERTEX_STAGE + 12) + int(union) * 4 + len(pairs) * 4 * (2 + len(TAUS))
    bounds = {"fp64_valu": ops / F64_VALU_OPS, "l2_gather": l2 / L2_BYTES, "hbm": hbm / HBM_BYTES}
    return dict(vertices_projected=n_vert, faces_walked=n_walk, faces_with_candidates=n_reach, candidate_centres=n_centre, pixels_compared=int(union),
                fp64_ops=ops, l2_bytes=l2, hbm_bytes=hbm, least_seconds=bounds, bound_by=max(bounds, key=bounds.get))


def merge_kernel_stats(stats_dir, out):
    rows = {}
    for path in glob.glob(os.path.join(stats_dir, "**", "*kernel_stats.csv"), recursive=True):
        for r in csv.DictReader(open(path)):
            for k in ("vsd_project", "vsd_tiles"):
                if k in r["Name"]:
                    rows[k] = dict(calls=int(r["Calls"]), average_ms=float(r["AverageNs"]) * 1e-6, min_ms=float(r["MinNs"]) * 1e-6, max_ms=float(r["MaxNs"]) * 1e-6)
    if not rows:
        raise SystemExit(f"no vsd kernel in {stats_dir}")
    res = json.load(open(out))
    res["kernel_stats"] = dict(source="rocprofv3 --kernel-trace --stats, a run of its own; both model sizes' launches averaged together", kernels=rows)
    json.dump(res, open(out, "w"), indent=1)
    print("merged", rows, "into", out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "vsd_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-pairs", type=int, default=4)
    ap.add_argument("--kernel-stats", default=None, help="directory of a rocprofv3 --kernel-trace --stats run of this tool: merge and exit")
    args = ap.parse_args()
    if args.kernel_stats:
        return merge_kernel_stats(args.kernel_stats, args.out)
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.hip_lib import abi
    from tests import vsd_ref as V

    assert torch.cuda.is_available(), "vsd_bench needs the GPU"
    lib = hip_lib.load()
    dev = torch.device("cuda")
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    res = dict(device=torch.cuda.get_device_name(0), image=[W, H], reps=args.reps, n_tau=len(TAUS), delta=DELTA,
               peaks=dict(fp64_valu_ops_per_s=F64_VALU_OPS, l2_gather_bytes_per_s=L2_BYTES, hbm_bytes_per_s=HBM_BYTES), models={})
    for subdiv in (2, 4):
        rng = np.random.default_rng(100 + subdiv)
        verts, faces, images, pairs = build(rng, subdiv)
        b = len(pairs)
        diam = float(np.linalg.norm(verts.max(0) - verts.min(0)))
        meshes = hip_lib.MeshSet([verts], [faces], dev)
        d = [T(np.zeros(b, np.int32)), T(np.array([p[0] for p in pairs], np.int32)), T(np.stack([p[1].reshape(9) for p in pairs])),
             T(np.stack([p[2] for p in pairs])), T(np.stack([p[3].reshape(9) for p in pairs])), T(np.stack([p[4] for p in pairs])),
             T(np.repeat(K.reshape(1, 9), b, 0)), T(np.full(b, diam)), T(images)]
        taus = T(np.array(TAUS))
        out = torch.empty((b, 2 + len(TAUS)), dtype=torch.int32, device=dev)
        nbytes = lib.gdrnpp_vsd_counts_workspace_bytes(meshes.c, b)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)

        def call():
            abi.launch("gdrnpp_vsd_counts", meshes.c, *[t.data_ptr() for t in d], len(images), H, W, taus.data_ptr(), len(TAUS), DELTA, 1.0, 1e6,
                       out.data_ptr(), b, ws.data_ptr(), nbytes)

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
        got = out.cpu().numpy()
        alg = algorithmic(verts, faces, pairs, got[:, 0].sum())
        least = max(alg["least_seconds"].values())
        r = dict(vertices=len(verts), faces=len(faces), pairs=b, images=len(images), hip_ms=dict(median=med, min=min(ms), max=max(ms)),
                 pairs_per_s=b / (med * 1e-3), workspace_bytes=int(nbytes), algorithmic=alg,
                 fraction_of_bound={k: v / (med * 1e-3) for k, v in alg["least_seconds"].items()}, roofline_fraction=least / (med * 1e-3))
        m = min(args.cpu_pairs, b)
        if m:
            V.vsd_counts_ref(verts, faces, *pairs[0][1:], K, images[pairs[0][0]], DELTA, TAUS, diam)      # warm
            t0 = time.perf_counter()
            cpu = np.array([V.vsd_counts_ref(verts, faces, *p[1:], K, images[p[0]], DELTA, TAUS, diam) for p in pairs[:m]])
            cpu_s = (time.perf_counter() - t0) / m
            r.update(cpu_pairs=m, cpu_numpy_one_core_s_per_pair=cpu_s, hip_over_cpu=cpu_s / (med * 1e-3 / b), counts_equal=bool(np.array_equal(cpu, got[:m])))
        res["models"][f"icosphere_{subdiv}"] = r
        print(f"{len(faces)} faces, {b} pairs on {len(images)} images {W}x{H}: hip {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) = {r['pairs_per_s']:.0f} pairs/s; "
              f"least time by {alg['bound_by']}: {100 * r['roofline_fraction']:.1f} % of the call"
              + (f";  NumPy one core {r['cpu_numpy_one_core_s_per_pair']:.3f} s per pair -> x{r['hip_over_cpu']:.0f}; counts equal: {r['counts_equal']}" if m else ""),
              flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
