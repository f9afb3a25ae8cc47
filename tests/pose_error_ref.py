"""NumPy fp64 restatement of the pose errors of the custom evaluator, used only by the tests: ``add / adi / re / te / arp_2d`` of
lib/pysixd/pose_error.py (:256-296, :359-374, :406-417, :440-445), ``get_closest_rot`` of core/utils/pose_utils.py:472-496 and the
per-pair rule of gdrn_custom_evaluator.py:684-724.  The nearest neighbour of ``adi`` is a brute-force search (no scipy).  It covers
the shapes that are too many to record; tests/test_pose_error_cpu.py shows that it reproduces every value recorded from the
reference's own functions (tests/golden/pose_error_golden.npz) to 1e-12 relative.

Also here, because the golden maker and the tests must build the same thing: the loader of the golden file and ``table_case``, the
(ground truths, predictions) of the recorded recall / precision tables."""
import json
import os
from collections import OrderedDict

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pose_error_golden.npz")


def transform_pts_Rt(pts, R, t):
    return (R.dot(pts.T) + t.reshape((3, 1))).T


def transform_pts_Rt_2d(pts, R, t, K):
    pts_c = K.dot(R.dot(pts.T) + t.reshape((3, 1)))
    return np.stack([pts_c[0] / pts_c[2], pts_c[1] / pts_c[2]], 1)


def add(R_est, t_est, R_gt, t_gt, pts):
    return np.linalg.norm(transform_pts_Rt(pts, R_est, t_est) - transform_pts_Rt(pts, R_gt, t_gt), axis=1).mean()


def nn_dists(queries, targets, chunk=256):
    """Distance from every query to its nearest target, brute force in fp64."""
    out = np.empty(len(queries))
    for i in range(0, len(queries), chunk):
        d = queries[i:i + chunk, None, :] - targets[None, :, :]
        out[i:i + chunk] = np.sqrt((d * d).sum(-1).min(1))
    return out


def adi(R_est, t_est, R_gt, t_gt, pts):
    return nn_dists(transform_pts_Rt(pts, R_gt, t_gt), transform_pts_Rt(pts, R_est, t_est)).mean()


def re(R_est, R_gt):
    trace = np.trace(np.dot(R_est, R_gt.T))
    trace = trace if trace <= 3 else 3
    return np.rad2deg(np.arccos(min(1.0, max(-1.0, 0.5 * (trace - 1.0)))))


def te(t_est, t_gt):
    return np.linalg.norm(t_gt.flatten() - t_est.flatten())


def arp_2d(R_est, t_est, R_gt, t_gt, pts, K):
    return np.linalg.norm(transform_pts_Rt_2d(pts, R_est, t_est, K) - transform_pts_Rt_2d(pts, R_gt, t_gt, K), axis=1).mean()


def get_closest_rot(rot_est, rot_gt, sym_info):
    if sym_info is None:
        return rot_gt
    sym_info = np.asarray(sym_info).reshape(-1, 3, 3)
    r_err, closest = re(rot_est, rot_gt), rot_gt
    for s in sym_info:
        rot_gt_sym = rot_gt.dot(s)
        cur = re(rot_est, rot_gt_sym)
        if cur < r_err:
            r_err, closest = cur, rot_gt_sym
    return closest


def pair_errors(pts, R_est, t_est, R_gt, t_gt, K, symmetric=False, sym_info=None):
    """One (estimate, ground truth) pair -> [ad, re, te, proj] by the rule of gdrn_custom_evaluator.py:684-724."""
    pts = np.asarray(pts, np.float64)
    if symmetric:
        R_sym = get_closest_rot(R_est, R_gt, sym_info)
        ad = adi(R_est, t_est, R_gt, t_gt, pts)         # the unmodified R_gt
    else:
        R_sym = R_gt
        ad = add(R_est, t_est, R_gt, t_gt, pts)
    return np.array([ad, re(R_est, R_sym), te(t_est, t_gt), arp_2d(R_est, t_est, R_sym, t_gt, pts, K)])


def pose_errors(verts, obj, R_est, t_est, R_gt, t_gt, K, symmetric=None, sym_infos=None):
    """The batch form of ``hip_lib.pose_errors`` -> f64[b,4]; ``verts``: list of [n,3] per class."""
    out = np.empty((len(obj), 4))
    for i, o in enumerate(obj):
        out[i] = pair_errors(verts[o], R_est[i].reshape(3, 3), t_est[i], R_gt[i].reshape(3, 3), t_gt[i], K[i].reshape(3, 3),
                             bool(symmetric[o]) if symmetric is not None else False, sym_infos[o] if sym_infos is not None else None)
    return out


def adi_bound(pts, R_est, t_est, R_gt, t_gt):
    """8 * 2^-24 * rho of the issue: rho = the largest norm among the model points and the queries in the estimate's model frame,
    q_j = R_est^T R_gt p_j + R_est^T (t_gt - t_est)."""
    pts = np.asarray(pts, np.float64)
    q = transform_pts_Rt(pts, R_est.T.dot(R_gt), R_est.T.dot(t_gt - t_est))
    return 8.0 * 2.0 ** -24 * max(np.linalg.norm(pts, axis=1).max(), np.linalg.norm(q, axis=1).max())


def load_golden():
    z = np.load(GOLDEN)
    g = {k: z[k] for k in z.files}
    g["names"] = json.loads(str(g["names"]))
    g["sym_objs"] = json.loads(str(g["sym_objs"]))
    for k in ("recall_table", "precision_table", "exp_id", "dataset_name"):
        g[k] = str(g[k])
    off = g["vert_off"]
    g["verts_list"] = [g["verts"][off[i]:off[i + 1]] for i in range(len(off) - 1)]
    so = g["sym_off"]
    g["sym_infos"] = [g["sym_rots"][so[i]:so[i + 1]].reshape(-1, 3, 3) if g["has_sym_info"][i] else None for i in range(len(so) - 1)]
    return g


def table_case(g):
    """The (gts, predictions) of the recorded tables, built from the golden pairs: pair i of class c is image ``img_<i>``.  Every
    third class has a ground-truth image that nobody predicted (recall counts it 0.0, precision skips it); class 1 has a second,
    later prediction for one image (the first counts); the last class has no prediction at all (the object is skipped) and one
    prediction names a class that has no ground truth.  -> (gts, predictions list, pair index of every counted prediction in the
    order of the evaluator's walk)."""
    names, obj = g["names"], g["obj"]
    gts, preds, walk = OrderedDict(), [], []
    last = len(names) - 1
    for c, name in enumerate(names):
        idx = [i for i in range(len(obj)) if obj[i] == c]
        gts[name] = OrderedDict()
        for i in idx:
            gts[name][f"img_{i}"] = {"R": g["R_gt"][i].reshape(3, 3), "t": g["t_gt"][i], "K": g["K"][i].reshape(3, 3)}
            if c != last:
                walk.append(i)
                preds.append({"cls_name": name, "file_name": f"img_{i}", "score": 0.5 + 0.001 * i,
                              "R": g["R_est"][i].reshape(3, 3).astype(np.float32), "t": g["t_est"][i].astype(np.float32), "time": 0.1})
        if c % 3 == 0:
            i = idx[0]
            gts[name][f"img_missed_{c}"] = {"R": g["R_gt"][i].reshape(3, 3), "t": g["t_gt"][i], "K": g["K"][i].reshape(3, 3)}
    i = [k for k in range(len(obj)) if obj[k] == 1][0]
    preds.append({"cls_name": names[1], "file_name": f"img_{i}", "score": 0.1, "R": np.eye(3, dtype=np.float32),
                  "t": np.array([0.0, 0.0, 1.0], np.float32), "time": 0.1})
    preds.append({"cls_name": "no_such_object", "file_name": "img_0", "score": 0.1, "R": np.eye(3, dtype=np.float32),
                  "t": np.array([0.0, 0.0, 1.0], np.float32), "time": 0.1})
    return gts, preds, walk
