"""Golden MSSD / MSPD values from the reference's own code (authoring container only: needs /root/reference).

Recorded in bop_error_golden.npz, through tests/golden/_refimport.py like make_golden_pose_error.py: ``lib/pysixd/pose_error.py``
``mssd / mspd`` and ``lib/pysixd/misc.py`` ``get_symmetry_transformations`` (``max_sym_disc_step`` = 0.01), unmodified, on every pair
-> ``errors`` f64[pairs,2], with ``models_info`` (JSON), the expanded transforms and the inputs.

Inputs: ellipsoid point clouds of gdrnpp_bop2022_amd.synthetic scaled to millimetres (float32).  Class c has COUNTS[c % 11] points and
symmetry KINDS[c % 9], 22 classes, so that every count and every kind occurs at least twice and in different company:
* point counts at the edges of csrc/bop_error.hip — 64 lanes per wave, 256 threads per workgroup (a thread's second point): 1, 63, 64,
  65, 255, 256, 257, 511, 512, 513, 1025;
* symmetries: none (1 transform), one discrete (2), six discrete (7), one continuous axis with a non-zero offset (314), continuous +
  one discrete (628), and 7 / 8 / 15 / 16 discrete (8, 9, 16, 17 transforms: the kernel's chunk of 8 symmetries +- 1, and two chunks
  +- 1).  Discrete symmetries carry a translation part.
Three pairs per class: rotation perturbations 1e-3 / 3e-2 / 1 rad with translation perturbations 0.1 / 3 / 100 mm, the estimate
starting from a randomly chosen symmetric equivalent of the ground truth; plus one exact-identity pair (a class without symmetries).

Conditions asserted here (conditions of the fixture, not measurements): every posed point has z >= 300 mm; every coordinate and
pixel magnitude is below 2e3; every normalised error (mssd / diameter, mspd at image width 640) is at least 1e-6 relative away from
every threshold of its type; the file is smaller than 1 MiB."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import _refimport  # noqa: E402

_refimport.install()

from gdrnpp_bop2022_amd import synthetic as S  # noqa: E402

COUNTS = [1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025]
KINDS = ["none", "d1", "d6", "cont", "cont_d1", "d7", "d8", "d15", "d16"]
N_TRANSFORMS = {"none": 1, "d1": 2, "d6": 7, "cont": 314, "cont_d1": 628, "d7": 8, "d8": 9, "d15": 16, "d16": 17}
N_CLS = 22
ROT_PERT = [1e-3, 3e-2, 1.0]
TRANS_PERT = [0.1, 3.0, 100.0]
STEP = 0.01
MSSD_THS = np.arange(0.05, 0.51, 0.05)
MSPD_THS = np.arange(5, 51, 5)


def rotvec(axis, angle):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(np.asarray(axis, np.float64) / np.linalg.norm(axis) * angle).as_matrix()


def rigid(R, t):
    m = np.eye(4)
    m[:3, :3], m[:3, 3] = R, t
    return m.reshape(-1).tolist()


def model_info(kind, diameter, rng):
    info = {"diameter": diameter}
    if kind == "d6":                                         # five about z and a flip about x, as make_golden_pose_error.py
        info["symmetries_discrete"] = [rigid(rotvec([0, 0, 1], 2 * np.pi * j / 6), rng.uniform(-3, 3, 3)) for j in range(1, 6)] + [
            rigid(rotvec([1, 0, 0], np.pi), rng.uniform(-3, 3, 3))]
    elif kind.startswith("d"):
        k = int(kind[1:])
        info["symmetries_discrete"] = [rigid(rotvec([0, 0, 1], 2 * np.pi * j / (k + 1)), rng.uniform(-3, 3, 3)) for j in range(1, k + 1)]
    if kind.startswith("cont"):
        info["symmetries_continuous"] = [{"axis": [0, 0, 1], "offset": [1.5, -2.0, 0.5]}]
        if kind == "cont_d1":
            info["symmetries_discrete"] = [rigid(rotvec([1, 0, 0], np.pi), [0.0, 0.0, 2.5])]
    return info


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def main():
    from lib.pysixd import misc as M
    from lib.pysixd import pose_error as PE

    rng = np.random.default_rng(20220925 + 47)
    verts_m, _, _ = S.make_models(N_CLS, rng, 4)
    verts = [(v[:COUNTS[c % len(COUNTS)]] * np.float32(1000.0)).astype(np.float32) for c, v in enumerate(verts_m)]
    kinds = [KINDS[c % len(KINDS)] for c in range(N_CLS)]
    diameters = [float(np.linalg.norm(v.max(0) - v.min(0))) * 1000.0 for v in verts_m]
    models_info = {c + 1: model_info(kinds[c], diameters[c], rng) for c in range(N_CLS)}       # obj_id = class + 1, as BOP ids
    syms = [M.get_symmetry_transformations(models_info[c + 1], STEP) for c in range(N_CLS)]
    assert [len(s) for s in syms] == [N_TRANSFORMS[k] for k in kinds]
    K0 = S.YCBV_K.astype(np.float64)

    obj, R_est, t_est, R_gt, t_gt, Ks = [], [], [], [], [], []
    for c in range(N_CLS):
        for rp, tp in zip(ROT_PERT, TRANS_PERT):
            Rg = S.random_rotation(rng)
            tg = np.array([rng.uniform(-150, 150), rng.uniform(-100, 100), rng.uniform(450, 900)])
            s = syms[c][rng.integers(len(syms[c]))]
            Re = Rg.dot(s["R"]).dot(rotvec(rng.standard_normal(3), rp * rng.uniform(0.7, 1.0)))
            d = rng.standard_normal(3)
            te = Rg.dot(s["t"]).reshape(3) + tg + d / np.linalg.norm(d) * tp * rng.uniform(0.7, 1.0)
            obj.append(c); R_est.append(f32(Re)); t_est.append(f32(te)); R_gt.append(Rg); t_gt.append(tg)    # estimates are float32
            Ks.append(K0 * np.array([[rng.uniform(0.98, 1.02)], [rng.uniform(0.98, 1.02)], [1.0]]))
    ident_cls = kinds.index("none")
    Rid = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    tid = f32([30.0, -20.0, 700.0])
    obj.append(ident_cls); R_est.append(Rid); t_est.append(tid); R_gt.append(Rid.copy()); t_gt.append(tid.copy()); Ks.append(K0)
    identity = len(obj) - 1
    obj = np.array(obj, np.int32)
    R_est, t_est, R_gt, t_gt, Ks = (np.stack(a) for a in (R_est, t_est, R_gt, t_gt, Ks))

    errors = np.empty((len(obj), 2))
    for i, c in enumerate(obj):
        pts = verts[c].astype(np.float64)
        a = (R_est[i], t_est[i].reshape(3, 1), R_gt[i], t_gt[i].reshape(3, 1))
        errors[i] = [PE.mssd(*a, pts, syms[c]), PE.mspd(*a, Ks[i], pts, syms[c])]
        # conditions on the inputs: depth and magnitudes, over the estimate and every symmetric ground truth
        for R, t in [(a[0], a[1])] + [(a[2].dot(s["R"]), a[2].dot(s["t"]) + a[3]) for s in syms[c]]:
            p3 = M.transform_pts_Rt(pts, R, t)
            assert p3[:, 2].min() >= 300.0, (i, p3[:, 2].min())
            assert np.abs(p3).max() < 2e3 and np.abs(M.project_pts(pts, Ks[i], R, t)).max() < 2e3, i
    assert errors[identity, 0] == 0.0 and errors[identity, 1] == 0.0

    def away(value, thresholds):
        return all(abs(value - th) >= 1e-6 * th for th in thresholds)

    for i, c in enumerate(obj):
        assert away(errors[i, 0] / diameters[c], MSSD_THS) and away(errors[i, 1] * (640.0 / 640.0), MSPD_THS), i

    sym_off = np.cumsum([0] + [len(s) for s in syms]).astype(np.int32)
    path = os.path.join(HERE, "bop_error_golden.npz")
    np.savez_compressed(
        path, models_info=json.dumps(models_info), kinds=json.dumps(kinds), max_sym_disc_step=STEP,
        verts=np.concatenate(verts).astype(np.float32), vert_off=np.cumsum([0] + [len(v) for v in verts]).astype(np.int32),
        sym_R=np.stack([t["R"].reshape(9) for s in syms for t in s]), sym_t=np.stack([t["t"].reshape(3) for s in syms for t in s]),
        sym_off=sym_off, obj=obj, identity=np.int64(identity), R_est=R_est.reshape(-1, 9), t_est=t_est, R_gt=R_gt.reshape(-1, 9),
        t_gt=t_gt, K=Ks.reshape(-1, 9), errors=errors)
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("wrote bop_error_golden.npz:", len(obj), "pairs,", int(sym_off[-1]), "transforms,", size, "bytes")
    print("mssd range", errors[:, 0].min(), errors[:, 0].max(), " mspd range", errors[:, 1].min(), errors[:, 1].max())


if __name__ == "__main__":
    main()
