"""``add / adi / re / te / arp_2d`` with the signatures of the reference's lib/pysixd/pose_error.py (:256-296, :359-374, :406-417,
:440-445): NumPy arrays in, a float out.  Each call runs ``gdrnpp_pose_errors`` (csrc/pose_error.hip) with b = 1 on the current
device; ``mssd / mspd`` (:131-179) run ``gdrnpp_bop_errors`` (csrc/bop_error.hip) the same way, and ``re_sym / te_sym / arp_2d_sym /
proj_sym`` (:377-396, :420-437, :183-217) ``gdrnpp_sym_errors`` (csrc/sym_error.hip), the entry points
``gdrn_modeling.bop_eval.bop19_scores`` runs once each for a whole results file — the entry point ``GDRN_EvaluatorCustom`` runs once for a whole dataset; use ``hip_lib.pose_errors`` directly for more
than a handful of poses.  ``pts`` is taken as float32 (what a ``hip_lib.MeshSet`` holds); there is no CPU fallback.
``vsd`` (:22-128) runs ``gdrnpp_vsd_counts`` (csrc/vsd_error.hip) with b = 1; its ``renderer`` is a ``VsdRenderer``: the resident meshes
(with faces) that the kernel renders, in place of the toolkit's GL renderer."""
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


def _sym_pair(fn, R_est, t_est, R_gt, t_gt, K, pts, syms) -> np.ndarray:
    """One pair through ``hip_lib.bop_errors`` / ``hip_lib.sym_errors``: a one-object mesh set, ``syms`` flattened, b = 1."""
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

    out = getattr(hip_lib, fn)(mesh, torch.zeros(1, dtype=torch.int32, device=dev), T(R_est, 9), T(t_est, 3), T(R_gt, 9), T(t_gt, 3),
                               None if K is None else T(K, 9), T(sym_R, 9), T(sym_t, 3), sym_off)
    return out.cpu().numpy()[0]


def _bop_errors(R_est, t_est, R_gt, t_gt, K, pts, syms) -> np.ndarray:
    return _sym_pair("bop_errors", R_est, t_est, R_gt, t_gt, K, pts, syms)


def mssd(R_est, t_est, R_gt, t_gt, pts, syms):
    """Maximum Symmetry-Aware Surface Distance: the smallest, over the symmetry transformations ``syms`` (``{"R", "t"}`` dicts), of
    the largest distance between a model point in the two poses."""
    return float(_bop_errors(R_est, t_est, R_gt, t_gt, _EYE, pts, syms)[0])


def mspd(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """Maximum Symmetry-Aware Projection Distance: as ``mssd``, between the projections by ``K``, in pixels."""
    return float(_bop_errors(R_est, t_est, R_gt, t_gt, K, pts, syms)[1])


def re_sym(R_est, R_gt, syms):
    """Rotational error in degrees against the closest of the symmetric ground-truth rotations ``R_gt . sym["R"]``."""
    R_est, R_gt = np.asarray(R_est), np.asarray(R_gt)
    assert R_est.shape == R_gt.shape == (3, 3)
    return float(_sym_pair("sym_errors", R_est, _ZERO, R_gt, _ZERO, None, _ONE_POINT, syms)[0])


def te_sym(t_est, t_gt, R_gt, syms):
    """Translational error against the closest of the symmetric ground-truth translations ``R_gt . sym["t"] + t_gt``."""
    t_est, t_gt = np.asarray(t_est).flatten(), np.asarray(t_gt).flatten()
    assert t_est.size == t_gt.size == 3
    return float(_sym_pair("sym_errors", _EYE, t_est, R_gt, t_gt, None, _ONE_POINT, syms)[1])


def arp_2d_sym(R_est, t_est, R_gt, t_gt, pts, K, syms):
    """Average re-projection error in pixels, the smallest over the symmetry transformations (the same as ``proj_sym``)."""
    return float(_sym_pair("sym_errors", R_est, t_est, R_gt, t_gt, K, pts, syms)[2])


def proj_sym(R_est, t_est, R_gt, t_gt, K, pts, syms):
    """Average distance of the projections of the model points in pixels (Brachmann et al., CVPR'16), the smallest over ``syms``."""
    return float(_sym_pair("sym_errors", R_est, t_est, R_gt, t_gt, K, pts, syms)[2])


class VsdRenderer:
    """What ``vsd`` needs in place of the toolkit's renderer: the models as a ``hip_lib.MeshSet`` with faces, resident on the device,
    and the map from BOP object id to the index in that set."""

    def __init__(self, meshes, obj_index):
        self.meshes = meshes
        self.obj_index = {int(k): int(v) for k, v in obj_index.items()}


def vsd(R_est, t_est, R_gt, t_gt, depth_test, K, delta, taus, normalized_by_diameter, diameter, renderer, obj_id, cost_type="step"):
    """Visible Surface Discrepancy (Hodan, Michel et al., ECCV 2018), one error per misalignment tolerance in ``taus``: a list of floats.
    depth_test: hxw test depth image in the unit of the model (mm), 0 = missing; renderer: a ``VsdRenderer``."""
    if cost_type != "step":
        if cost_type == "tlinear":
            raise NotImplementedError("pysixd.pose_error.vsd: cost_type 'tlinear' is not computed here (the evaluation scripts use 'step')")
        raise ValueError("Unknown pixel matching cost.")
    if not torch.cuda.is_available():
        raise RuntimeError("pysixd.pose_error: needs a HIP device (no CPU fallback)")
    from ... import hip_lib

    dev = renderer.meshes.verts.device

    def T(a, n):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).reshape(1, n))).to(dev)

    depth = torch.from_numpy(np.ascontiguousarray(np.asarray(depth_test, np.float32))[None]).to(dev)
    out = hip_lib.vsd_errors(renderer.meshes, torch.full((1,), renderer.obj_index[int(obj_id)], dtype=torch.int32, device=dev),
                             torch.zeros(1, dtype=torch.int32, device=dev), T(R_est, 9), T(t_est, 3), T(R_gt, 9), T(t_gt, 3), T(K, 9),
                             T(diameter if normalized_by_diameter else 1.0, 1), depth, [float(t) for t in taus], float(delta))
    return [float(x) for x in out.cpu().numpy()[0]]
