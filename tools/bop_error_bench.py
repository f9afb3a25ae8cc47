"""Microbenchmark of ``gdrnpp_bop_errors`` (csrc/bop_error.hip) on one MI355X at a realistic BOP size: 1 000 (estimate, ground truth)
pairs of a 20 000-vertex eval model with one continuous symmetry axis (314 transformations), i.e. 6.28e9 (point, symmetry) evaluations.

  (a) hip   the entry point alone (workspace allocated beforehand, no wrapper, no read-back): hipEvents around each call on a warmed
            kernel, median / min / max of ``--reps``.  Reported with the evaluations per second and what that is of the fp64 vector
            rate: 45 fp64 VALU operations per evaluation (csrc/bop_error.hip header) against 78.6e12 / 2 lane operations per second
            (the peak counts an fma as two).
  (b) cpu   the BOP toolkit's arithmetic for one pair in NumPy on this machine, one Python thread, NumPy's BLAS threads as the
            environment sets them (per symmetry: pose all points, project, two row norms, two maxima), timed on ``--cpu-pairs`` pairs;
            also the check, the largest |hip - cpu| in mm / px.

    python tools/bop_error_bench.py [--out profiles/bop_error_bench.json] [--reps 10] [--pairs 1000] [--verts 20000]
                                    [--reference-one-core-s MSSD MSPD]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gdrnpp_bop2022_amd import hip_lib, synthetic as S  # noqa: E402
from gdrnpp_bop2022_amd.hip_lib import abi  # noqa: E402
from gdrnpp_bop2022_amd.lib.pysixd import misc  # noqa: E402

F64_VALU_TFLOPS = 78.6
VALU_OPS_PER_EVAL = 45
K = np.array([[1066.778, 0.0, 312.9869], [0.0, 1067.487, 241.3109], [0.0, 0.0, 1.0]])


def rodrigues(w):
    angle = np.linalg.norm(w)
    a = w / angle
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx.dot(Kx)


def cpu_pair(pts, R_est, t_est, R_gt, t_gt, syms):
    """pose_error.mssd / mspd of the BOP toolkit, restated: (mssd, mspd)."""
    def project(R, t):
        p = K.dot(np.hstack((R, t.reshape(3, 1)))).dot(np.hstack((pts, np.ones((len(pts), 1)))).T)
        return (p[:2] / p[2]).T

    est, est2 = (R_est.dot(pts.T) + t_est.reshape(3, 1)).T, project(R_est, t_est)
    e3, e2 = [], []
    for s in syms:
        R, t = R_gt.dot(s["R"]), R_gt.dot(s["t"]) + t_gt.reshape(3, 1)
        e3.append(np.linalg.norm(est - (R.dot(pts.T) + t).T, axis=1).max())
        e2.append(np.linalg.norm(est2 - project(R, t), axis=1).max())
    return min(e3), min(e2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bop_error_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--verts", type=int, default=20000)
    ap.add_argument("--cpu-pairs", type=int, default=2)
    ap.add_argument("--reference-one-core-s", type=float, nargs=2, metavar=("MSSD", "MSPD"), default=None,
                    help="seconds per pair of the BOP toolkit's own pose_error.mssd / mspd at this size on one CPU core, measured where that "
                         "code can be run (not on this host); recorded verbatim beside the figures measured here")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bop_error_bench needs the GPU"
    lib = hip_lib.load()
    dev = torch.device("cuda")
    rng = np.random.default_rng(314)
    n, b = args.verts, args.pairs
    u = rng.standard_normal((n, 3))
    verts = (u / np.linalg.norm(u, axis=1, keepdims=True) * np.array([40.0, 40.0, 90.0])).astype(np.float32)     # mm, symmetric about z
    syms = misc.get_symmetry_transformations({"symmetries_continuous": [{"axis": [0, 0, 1], "offset": [0, 0, 0]}]}, 0.01)
    sym_R, sym_t, sym_off = misc.flatten_symmetry_transformations([syms])
    R_gt = np.stack([S.random_rotation(rng) for _ in range(b)])
    t_gt = np.stack([rng.uniform(-150, 150, b), rng.uniform(-100, 100, b), rng.uniform(450, 900, b)], 1)
    R_est = np.stack([R_gt[i].dot(rodrigues(rng.standard_normal(3) * 0.05)) for i in range(b)]).astype(np.float32).astype(np.float64)
    t_est = (t_gt + rng.standard_normal((b, 3)) * 5.0).astype(np.float32).astype(np.float64)
    meshes = hip_lib.MeshSet([verts], [np.zeros((1, 3), np.int32)], dev)
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    d = [T(np.zeros(b, np.int32)), T(R_est.reshape(-1, 9)), T(t_est), T(R_gt.reshape(-1, 9)), T(t_gt), T(np.repeat(K.reshape(1, 9), b, 0)),
         T(sym_R), T(sym_t)]
    out = torch.empty((b, 2), dtype=torch.float64, device=dev)
    nbytes = lib.gdrnpp_bop_errors_workspace_bytes(meshes.c, sym_off.ctypes.data, b)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)

    def call():
        abi.launch("gdrnpp_bop_errors", meshes.c, *[t.data_ptr() for t in d], sym_off.ctypes.data, out.data_ptr(), b, ws.data_ptr(), nbytes)

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
    evals = float(b) * n * len(syms)
    evals_per_s = evals / (med * 1e-3)
    fraction = evals_per_s * VALU_OPS_PER_EVAL / (F64_VALU_TFLOPS * 1e12 / 2)
    got = out.cpu().numpy()

    m = min(args.cpu_pairs, b)
    pts = verts.astype(np.float64)
    cpu_pair(pts[:256], R_est[0], t_est[0], R_gt[0], t_gt[0], syms[:4])        # warm
    t0 = time.perf_counter()
    cpu = np.array([cpu_pair(pts, R_est[i], t_est[i], R_gt[i], t_gt[i], syms) for i in range(m)])
    cpu_s = (time.perf_counter() - t0) / m
    err = np.abs(got[:m] - cpu).max(0)
    res = dict(device=torch.cuda.get_device_name(0), pairs=b, verts=n, symmetries=len(syms), reps=args.reps, f64_valu_tflops=F64_VALU_TFLOPS,
               valu_ops_per_eval=VALU_OPS_PER_EVAL, hip_ms=dict(median=med, min=min(ms), max=max(ms)), evals=evals, evals_per_s=evals_per_s,
               fp64_valu_fraction=fraction, pairs_per_s=b / (med * 1e-3), workspace_bytes=int(nbytes), cpu_pairs=m,
               cpu_numpy_s_per_pair=cpu_s, hip_over_cpu=cpu_s / (med * 1e-3 / b), mssd_max_abs_mm=float(err[0]), mspd_max_abs_px=float(err[1]))
    if args.reference_one_core_s:
        res["reference_pose_error_one_core_s_per_pair"] = dict(mssd=args.reference_one_core_s[0], mspd=args.reference_one_core_s[1],
                                                               where="another machine's CPU, one core: not measured by this run")
    print(f"{b} pairs x {n} vertices x {len(syms)} symmetries: hip {med:.3f} ms (min {min(ms):.3f}, max {max(ms):.3f}) = {evals_per_s / 1e12:.3f} T evals/s = "
          f"{100 * fraction:.1f} % of the fp64 vector rate;  NumPy on this host {cpu_s:.3f} s per pair  ->  x{res['hip_over_cpu']:.0f};  "
          f"|hip - cpu| mssd {err[0]:.2e} mm, mspd {err[1]:.2e} px", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
