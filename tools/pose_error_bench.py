"""Microbenchmark of ``gdrnpp_pose_errors`` (csrc/pose_error.hip) on one MI355X at synthetic eval-model sizes — 2 k, 8 k and 32 k
points — for 1 024 (estimate, ground truth) pairs, half of them of a symmetric class (ADI: the O(n^2) nearest-neighbour search):

  (a) hip   the entry point alone (workspace allocated beforehand, no wrapper, no read-back): hipEvents around each call on a
            warmed kernel, median of ``--reps``.  Reported with the (query, target) evaluations per second of the search and what
            that is of the fp32 VALU rate: 6.5 VALU operations per evaluation (3 sub, 3 fma, half a min3) against 157.3e12 / 2 lane
            operations per second (the peak counts an fma as two).
  (b) cpu   the reference-style loop on this machine: per pair te / re / add / arp_2d in NumPy, adi with a scipy cKDTree built and
            queried per pair, on min(16, cpus) threads (cKDTree releases the GIL).  Also the check: the largest |hip - cpu| of the
            ADI column in units of 2^-24 rho.

    python tools/pose_error_bench.py [--out profiles/pose_error_bench.json] [--reps 20] [--sizes 2048 8192 32768] [--pairs 1024]
"""
import argparse
import json
import os
import statistics
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch
from scipy import spatial

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gdrnpp_bop2022_amd import hip_lib, synthetic as S  # noqa: E402
from gdrnpp_bop2022_amd.hip_lib import abi  # noqa: E402

F32_VALU_TFLOPS = 157.3
VALU_OPS_PER_EVAL = 6.5
SYMS = np.stack([np.diag([-1.0, -1.0, 1.0]), np.diag([1.0, -1.0, -1.0])])


def rodrigues(w):
    angle = np.linalg.norm(w)
    a = w / angle
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx.dot(Kx)


def make_case(n, pairs, rng):
    """Two classes of n points on ellipsoids (class 1 symmetric, two symmetries); pairs alternate between them."""
    verts = []
    for _ in range(2):
        u = rng.standard_normal((n, 3))
        verts.append((u / np.linalg.norm(u, axis=1, keepdims=True) * rng.uniform(0.03, 0.12, 3)).astype(np.float32))
    obj = (np.arange(pairs) % 2).astype(np.int32)
    R_gt = np.stack([S.random_rotation(rng) for _ in range(pairs)])
    t_gt = np.stack([rng.uniform(-0.15, 0.15, pairs), rng.uniform(-0.1, 0.1, pairs), rng.uniform(0.45, 0.9, pairs)], 1)
    # every eighth estimate is unrelated to its ground truth, the others sit within a few degrees; float32 like a prediction
    R_est = np.stack([R_gt[i].dot(S.random_rotation(rng) if i % 8 == 0 else rodrigues(rng.standard_normal(3) * 0.03)) for i in range(pairs)])
    R_est = R_est.astype(np.float32).astype(np.float64)
    t_est = (t_gt + rng.standard_normal((pairs, 3)) * 0.01).astype(np.float32).astype(np.float64)
    K = np.repeat(S.YCBV_K.astype(np.float64)[None], pairs, 0)
    return verts, obj, R_est, t_est, R_gt, t_gt, K


def cpu_pair(pts, R_est, t_est, R_gt, t_gt, K, symmetric):
    def re(A, B):
        tr = min(np.trace(A.dot(B.T)), 3)
        return np.rad2deg(np.arccos(min(1.0, max(-1.0, 0.5 * (tr - 1.0)))))

    R_sym = R_gt
    if symmetric:
        best = re(R_est, R_gt)
        for s in SYMS:
            cur = re(R_est, R_gt.dot(s))
            if cur < best:
                best, R_sym = cur, R_gt.dot(s)
    est, gt = (R_est.dot(pts.T) + t_est[:, None]).T, (R_gt.dot(pts.T) + t_gt[:, None]).T
    if symmetric:
        ad = spatial.cKDTree(est).query(gt, k=1)[0].mean()
    else:
        ad = np.linalg.norm(est - gt, axis=1).mean()
    pe, pg = K.dot(est.T), K.dot(R_sym.dot(pts.T) + t_gt[:, None])
    proj = np.linalg.norm((pe[:2] / pe[2] - pg[:2] / pg[2]).T, axis=1).mean()
    return ad, re(R_est, R_sym), np.linalg.norm(t_gt - t_est), proj


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pose_error_bench.json"))
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sizes", type=int, nargs="*", default=[2048, 8192, 32768])
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--cpu-pairs", type=int, default=256, help="pairs the CPU loop runs (the first ones; its rate is per pair)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "pose_error_bench needs the GPU"
    hip_lib.load()
    dev = torch.device("cuda")
    threads = min(16, os.cpu_count() or 1)
    res = dict(device=torch.cuda.get_device_name(0), pairs=args.pairs, reps=args.reps, cpu_threads=threads, f32_valu_tflops=F32_VALU_TFLOPS,
               valu_ops_per_eval=VALU_OPS_PER_EVAL, sizes={})
    for n in args.sizes:
        rng = np.random.default_rng(n)
        verts, obj, R_est, t_est, R_gt, t_gt, K = make_case(n, args.pairs, rng)
        meshes = hip_lib.MeshSet(verts, [np.zeros((1, 3), np.int32)] * 2, dev)
        T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
        d = [T(obj), T(R_est.reshape(-1, 9)), T(t_est), T(R_gt.reshape(-1, 9)), T(t_gt), T(K.reshape(-1, 9)), T(SYMS.reshape(-1, 9)),
             T(np.array([0, 0, 2], np.int32)), T(np.array([0, 1], np.uint8))]
        out = torch.empty((args.pairs, 4), dtype=torch.float64, device=dev)
        nbytes = hip_lib.load().gdrnpp_pose_errors_workspace_bytes(meshes.c, args.pairs)
        ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)

        def call():
            abi.launch("gdrnpp_pose_errors", meshes.c, *[t.data_ptr() for t in d], out.data_ptr(), args.pairs, ws.data_ptr(), nbytes)

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
        ms = [a.elapsed_time(b) for a, b in evs]
        med = statistics.median(ms)
        n_sym = int((obj == 1).sum())
        evals = float(n_sym) * n * n
        evals_per_s = evals / (med * 1e-3)
        valu_fraction = evals_per_s * VALU_OPS_PER_EVAL / (F32_VALU_TFLOPS * 1e12 / 2)
        got = out.cpu().numpy()

        m = min(args.cpu_pairs, args.pairs)
        pts64 = [v.astype(np.float64) for v in verts]
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(lambda i: cpu_pair(pts64[obj[i]], R_est[i], t_est[i], R_gt[i], t_gt[i], K[i], obj[i] == 1), range(threads)))   # warm
            t0 = time.perf_counter()
            cpu = np.array(list(pool.map(lambda i: cpu_pair(pts64[obj[i]], R_est[i], t_est[i], R_gt[i], t_gt[i], K[i], obj[i] == 1), range(m))))
            cpu_s = time.perf_counter() - t0
        rho = max(np.linalg.norm(v, axis=1).max() for v in pts64) + np.linalg.norm(t_gt[:m] - t_est[:m], axis=1).max()
        sym = obj[:m] == 1
        adi_units = np.abs(got[:m][sym, 0] - cpu[sym, 0]).max() / (2.0 ** -24 * rho)
        rel = np.abs(got[:m] - cpu) / np.abs(cpu)
        res["sizes"][str(n)] = dict(
            hip_ms=dict(median=med, min=min(ms), max=max(ms)), symmetric_pairs=n_sym, evals=evals, evals_per_s=evals_per_s,
            fp32_valu_fraction=valu_fraction, pairs_per_s=args.pairs / (med * 1e-3), workspace_bytes=int(nbytes),
            cpu_pairs=m, cpu_s=cpu_s, cpu_pairs_per_s=m / cpu_s, hip_over_cpu=(args.pairs / (med * 1e-3)) / (m / cpu_s),
            adi_max_err_in_2pow_m24_rho=float(adi_units), add_max_rel=float(rel[~sym, 0].max()), re_max_abs_deg=float(np.abs(got[:m, 1] - cpu[:, 1]).max()),
            proj_max_rel=float(rel[:, 3].max()))
        print(f"n = {n:6d}: hip {med:.3f} ms for {args.pairs} pairs ({n_sym} symmetric) = {evals_per_s / 1e12:.2f} T evals/s = "
              f"{100 * valu_fraction:.1f} % of the fp32 VALU rate;  cpu ({threads} threads) {m / cpu_s:.1f} pairs/s  ->  x{res['sizes'][str(n)]['hip_over_cpu']:.0f};  "
              f"ADI err {adi_units:.3f} x 2^-24 rho", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
