"""``add / adi / re / te / arp_2d`` with the signatures of the reference's lib/pysixd/pose_error.py (:256-296, :359-374, :406-417,
:440-445): NumPy arrays in, a float out.  Each call runs ``gdrnpp_pose_errors`` (csrc/pose_error.hip) with b = 1 on the current
device; ``mssd / mspd`` (:131-179) run ``gdrnpp_bop_errors`` (csrc/bop_error.hip) the same way, the entry point
``gdrn_modeling.bop_eval.bop19_scores`` runs once for a whole results file — the entry point ``GDRN_EvaluatorCustom`` runs once for a whole dataset; use ``hip_lib.pose_errors`` directly for more
than a handful of poses.  ``pts`` is taken as float32 (what a ``hip_lib.MeshSet`` holds); there is no CPU fallback."""
from __future__ import annotations

import numpy as np
import torch

_EYE = np.eye(3)
_ZERO = np.zeros(3)
_ONE_POINT = np.zeros((1, 3), np.float32)
_NO_FACES = np.zeros((1, 3), np.int32)


def _errors(R_est, t_est, R_gt, t_gt, pts=_ONE_POINT, K=_EYE, symmetric=False) -> np.ndarray:
    if not torch.cuda.is_available():
        raise RuntimeError("pysixd.pose_error: needs a HIP device (no CPU fallback)")
    from ... import hip_lib

    dev = torch.device("cuda", torch.cuda.current_device())
    pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 3))
    mesh = hip_lib.MeshSet([pts], [_NO_FACES], device=dev)

    def T(a, n):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).reshape(1, n))).to(dev)

    out = hip_lib.pose_errors(mesh, torch.zeros(1, dtype=torch.int32, device=dev), T(R_est, 9), T(t_est, 3), T(R_gt, 9), T(t_gt, 3),
                              T(K, 9), symmetric=torch.full((1,), 1 if symmetric else 0, dtype=torch.uint8, device=dev))
    return out.cpu().numpy()[0]


def add(R_est, t_est, R_gt, t_gt, pts):
    """Average distance of model points for objects with no indistinguishable views (Hinterstoisser et al., ACCV'12)."""
    return float(_errors(R_est, t_est, R_gt, t_gt, pts)[0])


def adi(R_est, t_est, R_gt, t_gt, pts):
    """Average distance to the nearest estimated-posed model point, for objects with indistinguishable views."""
    return float(_errors(R_est, t_est, R_gt, t_gt, pts, symmetric=True)[0])


def re(R_est, R_gt):
    """Rotational error in degrees."""
    R_est, R_gt = np.asarray(R_est), np.asarray(R_gt)
    assert R_est.shape == R_gt.shape == (3, 3)
    return float(_errors(R_est, _ZERO, R_gt, _ZERO)[1])


def te(t_est, t_gt):
    """Translational error."""
    t_est, t_gt = np.asarray(t_est).flatten(), np.asarray(t_gt).flatten()
    assert t_est.size == t_gt.size == 3
    return float(_errors(_EYE, t_est, _EYE, t_gt)[2])


def arp_2d(R_est, t_est, R_gt, t_gt, pts, K):
    """Average re-projection error in pixels."""
    return float(_errors(R_est, t_est, R_gt, t_gt, pts, K)[3])


def _bop_errors(R_est, t_est, R_gt, t_gt, K, pts, syms) -> np.ndarray:
    if not torch.cuda.is_available():
        raise RuntimeError("pysixd.pose_error: needs a HIP device (no CPU fallback)")
    from ... import hip_lib
    from .misc import flatten_symmetry_transformations

    dev = torch.device("cuda", torch.cuda.current_device())
    pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 3))
    mesh = hip_lib.MeshSet([pts], [_NO_FACES], device=dev)
    sym_R, sym_t, sym_off = flatten_symmetry_transformations([list(syms)])

    def T(a, n):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).reshape(-1, n))).to(dev)

    out = hip_lib.bop_errors(mesh, torch.zeros(1, dtype=torch.int32, device=dev), T(R_est, 9), T(t_est, 3), T(R_gt, 9), T(t_gt, 3),
                             T(K, 9), T(sym_R, 9), T(sym_t, 3), sym_off)
    return out.cpu().numpy()[0]


def mssd(R_est, t_est, R_gt, t_gt, pts, syms):
    """Maximum Symmetry-Aware Surface Distance: the smallest, over the symmetry transformations ``syms`` (``{"R", "t"}`` dicts), of
    the largest distance between a model point in the two poses."""
    return float(_bop_errors(R_est, t_est, R_gt, t_gt, _EYE, pts, syms)[0])


def mspd(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """Maximum Symmetry-Aware Projection Distance: as ``mssd``, between the projections by ``K``, in pixels."""
    return float(_bop_errors(R_est, t_est, R_gt, t_gt, K, pts, syms)[1])
