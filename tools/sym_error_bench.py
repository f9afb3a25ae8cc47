"""Microbenchmark of ``gdrnpp_sym_errors`` (csrc/sym_error.hip) on one MI355X at the size tools/bop_error_bench.py uses: 1 000 (estimate,
ground truth) pairs of a 20 000-vertex eval model with one continuous symmetry axis (314 transformations), i.e. 6.28e9 (point, symmetry)
evaluations for projS — and ``gdrnpp_bop_errors`` on the very same inputs in the same run, the three alternating, so that the two kernels
are compared on one device at one clock.

  sym_K     reS, teS and projS: the entry point alone (workspace allocated beforehand, no wrapper, no read-back), hipEvents around each
            call on a warmed kernel, median / min / max of ``--reps``.  Reported with the evaluations per second and what that is of the
            fp64 vector rate: 58 VALU operations per evaluation (csrc/sym_error.hip header) against 78.6e12 / 2 lane operations per second.
  sym_noK   K = NULL: reS and teS only, nothing over the points; O(pairs x symmetries).
  bop       gdrnpp_bop_errors (mssd, mspd; 45 operations per evaluation).
  cpu       the toolkit's arithmetic for one pair in NumPy on this machine (per symmetry: pose and project all points, one row norm, a
            mean), timed on ``--cpu-pairs`` pairs; also the check, the largest |hip - cpu| per column.

    python tools/sym_error_bench.py [--out profiles/sym_error_bench.json] [--reps 10] [--pairs 1000] [--verts 20000]
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
from tools.bop_error_bench import F64_VALU_TFLOPS, K, rodrigues  # noqa: E402
from tools.bop_error_bench import VALU_OPS_PER_EVAL as BOP_OPS_PER_EVAL  # noqa: E402

VALU_OPS_PER_EVAL = 58


def cpu_pair(pts, R_est, t_est, R_gt, t_gt, syms):
    """pose_error.re_sym / te_sym / arp_2d_sym of the reference's toolkit fork, restated: (reS deg, teS, projS px)."""
    def project(R, t):
        p = K.dot(R.dot(pts.T) + t.reshape(3, 1))
        return (p[:2] / p[2]).T

    est2 = project(R_est, t_est)
    re, te, pj = [], [], []
    for s in syms:
        R, t = R_gt.dot(s["R"]), R_gt.dot(s["t"]).reshape(3) + t_gt
        tr = min(np.trace(R_est.dot(R.T)), 3.0)
        re.append(np.rad2deg(np.arccos(min(1.0, max(-1.0, 0.5 * (tr - 1.0))))))
        te.append(np.linalg.norm(t - t_est))
        pj.append(np.linalg.norm(est2 - project(R, t), axis=1).mean())
    return min(re), min(te), min(pj)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sym_error_bench.json"))
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--pairs", type=int, default=1000)
    ap.add_argument("--verts", type=int, default=20000)
    ap.add_argument("--cpu-pairs", type=int, default=2)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sym_error_bench needs the GPU"
    lib = hip_lib.load()
    dev = torch.device("cuda")
    rng = np.random.default_rng(314)                           # the inputs of tools/bop_error_bench.py, drawn in its order
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
    ptrs = [t.data_ptr() for t in d]
    no_K = ptrs[:5] + [None] + ptrs[6:]
    out_sym = torch.empty((b, 3), dtype=torch.float64, device=dev)
    out_rt = torch.empty((b, 3), dtype=torch.float64, device=dev)
    out_bop = torch.empty((b, 2), dtype=torch.float64, device=dev)
    offp = sym_off.ctypes.data
    n_sym, n_bop = lib.gdrnpp_sym_errors_workspace_bytes(meshes.c, offp, b), lib.gdrnpp_bop_errors_workspace_bytes(meshes.c, offp, b)
    ws = torch.empty((max(n_sym, n_bop),), dtype=torch.uint8, device=dev)
    calls = {
        "sym_K": lambda: abi.launch("gdrnpp_sym_errors", meshes.c, *ptrs, offp, out_sym.data_ptr(), b, ws.data_ptr(), n_sym),
        "sym_noK": lambda: abi.launch("gdrnpp_sym_errors", meshes.c, *no_K, offp, out_rt.data_ptr(), b, ws.data_ptr(), n_sym),
        "bop": lambda: abi.launch("gdrnpp_bop_errors", meshes.c, *ptrs, offp, out_bop.data_ptr(), b, ws.data_ptr(), n_bop),
    }
    for _ in range(3):
        for call in calls.values():
            call()
    torch.cuda.synchronize()
    evs = {name: [] for name in calls}
    for _ in range(args.reps):                                 # alternating: one device, one clock
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            call()
            e1.record()
            evs[name].append((e0, e1))
    torch.cuda.synchronize()
    ms = {name: [a.elapsed_time(z) for a, z in v] for name, v in evs.items()}
    med = {name: statistics.median(v) for name, v in ms.items()}
    evals = float(b) * n * len(syms)
    rate = {name: evals / (med[name] * 1e-3) for name in ("sym_K", "bop")}
    fraction = {"sym_K": rate["sym_K"] * VALU_OPS_PER_EVAL / (F64_VALU_TFLOPS * 1e12 / 2),
                "bop": rate["bop"] * BOP_OPS_PER_EVAL / (F64_VALU_TFLOPS * 1e12 / 2)}
    got, got_rt = out_sym.cpu().numpy(), out_rt.cpu().numpy()
    assert got_rt[:, :2].tobytes() == got[:, :2].tobytes() and np.isnan(got_rt[:, 2]).all()

    m = min(args.cpu_pairs, b)
    pts = verts.astype(np.float64)
    cpu_pair(pts[:256], R_est[0], t_est[0], R_gt[0], t_gt[0], syms[:4])        # warm
    t0 = time.perf_counter()
    cpu = np.array([cpu_pair(pts, R_est[i], t_est[i], R_gt[i], t_gt[i], syms) for i in range(m)])
    cpu_s = (time.perf_counter() - t0) / m
    err = np.abs(got[:m] - cpu).max(0)
    res = dict(device=torch.cuda.get_device_name(0), pairs=b, verts=n, symmetries=len(syms), reps=args.reps, f64_valu_tflops=F64_VALU_TFLOPS,
               valu_ops_per_eval=dict(sym_K=VALU_OPS_PER_EVAL, bop=BOP_OPS_PER_EVAL),
               hip_ms={name: dict(median=med[name], min=min(v), max=max(v)) for name, v in ms.items()}, evals=evals, evals_per_s=rate,
               fp64_valu_fraction=fraction, sym_K_over_bop=med["sym_K"] / med["bop"], workspace_bytes=int(n_sym), cpu_pairs=m,
               cpu_numpy_s_per_pair=cpu_s, hip_over_cpu=cpu_s / (med["sym_K"] * 1e-3 / b), reS_max_abs_deg=float(err[0]),
               teS_max_abs_mm=float(err[1]), projS_max_abs_px=float(err[2]))
    print(f"{b} pairs x {n} vertices x {len(syms)} symmetries: sym_errors with K {med['sym_K']:.3f} ms (min {min(ms['sym_K']):.3f}, max {max(ms['sym_K']):.3f}) = "
          f"{rate['sym_K'] / 1e12:.3f} T evals/s = {100 * fraction['sym_K']:.1f} % of the fp64 vector rate;  without K {med['sym_noK']:.4f} ms;  "
          f"bop_errors {med['bop']:.3f} ms ({100 * fraction['bop']:.1f} %)  ->  sym / bop = {res['sym_K_over_bop']:.2f};  NumPy on this host "
          f"{cpu_s:.3f} s per pair  ->  x{res['hip_over_cpu']:.0f};  |hip - cpu| reS {err[0]:.2e} deg, teS {err[1]:.2e} mm, projS {err[2]:.2e} px", flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
