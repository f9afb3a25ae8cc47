"""``get_symmetry_transformations`` with the signature and the result of the reference's lib/pysixd/misc.py:234-282: the set of rigid
transformations that map an object model onto itself, which MSSD and MSPD take their minimum over, and ``overlapping_sphere_projections`` (:1219-1241), the host test that spares VSD a render
(host code, NumPy)."""
from __future__ import annotations

import math

import numpy as np


def _axis_angle_matrix(angle: float, axis) -> np.ndarray:
    """Rotation by ``angle`` about ``axis`` (Rodrigues): cos a I + (1 - cos a) d d^T + sin a [d]x, d the unit axis."""
    d = np.array(axis, np.float64).reshape(3)
    d = d / math.sqrt(float(np.dot(d, d)))
    sin_a, cos_a = math.sin(angle), math.cos(angle)
    R = np.diag([cos_a, cos_a, cos_a])
    R = R + np.outer(d, d) * (1.0 - cos_a)
    s = d * sin_a
    return R + np.array([[0.0, -s[2], s[1]], [s[2], 0.0, -s[0]], [-s[1], s[0], 0.0]])


def get_symmetry_transformations(model_info: dict, max_sym_disc_step: float) -> list:
    """model_info: an entry of a BOP ``models_info.json`` -> list of ``{"R": f64[3,3], "t": f64[3,1]}``.

    * ``symmetries_discrete``: 4x4 matrices as flat lists of 16; the identity comes first.
    * ``symmetries_continuous``: ``{"axis", "offset"}``; each is discretised into n = ceil(pi / max_sym_disc_step) rotations by
      2 pi i / n, i = 1 .. n - 1, about the axis through ``offset``: t = -R offset + offset.
    * The result is every discrete one combined with every continuous one (R_c R_d, R_c t_d + t_c), discrete outer.  With a continuous
      symmetry the plain discrete transformations, the identity among them, are NOT part of the set; without one, the set is the discrete list."""
    discrete = [{"R": np.eye(3), "t": np.zeros((3, 1))}]
    for sym in model_info.get("symmetries_discrete", []):
        m = np.reshape(sym, (4, 4))
        discrete.append({"R": m[:3, :3], "t": m[:3, 3].reshape((3, 1))})

    continuous = []
    for sym in model_info.get("symmetries_continuous", []):
        offset = np.array(sym["offset"]).reshape((3, 1))
        steps = int(np.ceil(np.pi / max_sym_disc_step))
        step = 2.0 * np.pi / steps
        for i in range(1, steps):
            R = _axis_angle_matrix(i * step, sym["axis"])
            continuous.append({"R": R, "t": -(R.dot(offset)) + offset})

    if not continuous:
        return discrete
    return [{"R": c["R"].dot(d["R"]), "t": c["R"].dot(d["t"]) + c["t"]} for d in discrete for c in continuous]


def flatten_symmetry_transformations(per_object: list):
    """[[{"R","t"}, ...] per object] -> (sym_R f64[n,9], sym_t f64[n,3], sym_off i32[n_obj+1]): the layout of ``hip_lib.bop_errors``."""
    off = np.cumsum([0] + [len(s) for s in per_object]).astype(np.int32)
    R = np.stack([np.asarray(t["R"], np.float64).reshape(9) for s in per_object for t in s])
    t = np.stack([np.asarray(t["t"], np.float64).reshape(3) for s in per_object for t in s])
    return np.ascontiguousarray(R), np.ascontiguousarray(t), off


def overlapping_sphere_projections(radius, p1, p2) -> bool:
    """Whether the silhouettes of two spheres of ``radius`` centred at p1 and p2 overlap, approximately, with the result of the
    reference's misc.py:1219-1241: the test eval_calc_errors.py:363-378 makes before it renders a pair for VSD.  The centres are projected
    to the plane z = 1; a sphere at depth z has the radius ``radius / z`` there.  A centre in the camera plane never overlaps."""
    p1, p2 = np.asarray(p1, np.float64).reshape(3), np.asarray(p2, np.float64).reshape(3)
    z1, z2 = p1[2], p2[2]
    if z1 == 0 or z2 == 0:
        return False
    gap = np.linalg.norm((p1 / z1)[:2] - (p2 / z2)[:2])
    return bool(gap < radius * (1.0 / z1 + 1.0 / z2))
