"""-m gpu: ``gdrnpp_pose_errors`` (csrc/pose_error.hip) against the values the reference's own pose_error.py functions gave
(tests/golden/pose_error_golden.npz), at every point count at the kernel's edges — 64 points per wave, 256 per workgroup and per wave's
share of a tile, 1024 per tile — and ``GDRN_EvaluatorCustom`` end to end.

Tolerances, derived (not measured on a GPU):
  ADD, te, proj   1e-11 relative: fp64 sums of <= 4096 terms, n * 2^-53.
  re              1e-8 deg: the trace rounds at ~1e-15, divided by sin 0.01 deg, x30 margin; the identity pair < 1e-6 deg.
  ADI             8 * 2^-24 * rho, rho = the largest norm among the model points and the queries in the estimate's model frame: one
                  fp32 rounding of the query plus the fp32 evaluation of d^2 (pose_error_ref.adi_bound).
"""
import os
import pickle

import numpy as np
import pytest
import torch

from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd.gdrn_modeling import gdrn_custom_evaluator as CE
from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
from gdrnpp_bop2022_amd.gdrn_modeling.gdrn_evaluator import GDRN_Evaluator
from tests import evalgolden as EG
from tests import pose_error_ref as PR

pytestmark = pytest.mark.gpu
DEV = "cuda"
REL, RE_ABS = 1e-11, 1e-8
NO_FACE = np.zeros((1, 3), np.int32)


def T(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


@pytest.fixture(scope="module")
def g():
    return PR.load_golden()


@pytest.fixture(scope="module")
def meshes(g):
    return hip_lib.MeshSet(g["verts_list"], [NO_FACE] * len(g["verts_list"]), DEV)


def _sym_args(g):
    return dict(sym_rots=T(g["sym_rots"]), sym_off=T(g["sym_off"]), symmetric=T(g["symmetric"]))


def _run(meshes, g, order, **sym):
    return hip_lib.pose_errors(meshes, T(g["obj"][order]), T(g["R_est"][order]), T(g["t_est"][order]), T(g["R_gt"][order]),
                               T(g["t_gt"][order]), T(g["K"][order]), **sym).cpu().numpy()


def check_against(out, ref, verts, obj, R_est, t_est, R_gt, t_gt, symmetric, what):
    """Every row of ``out`` against ``ref`` within the derived tolerances; prints the figures before it asserts."""
    out, ref = np.asarray(out), np.asarray(ref)
    assert out.shape == ref.shape and np.isfinite(out).all(), what
    rel = np.abs(out - ref) / np.where(ref != 0, np.abs(ref), 1.0)
    sym = np.array([bool(symmetric[o]) for o in obj])
    adi_units = np.zeros(len(obj))
    for i in np.nonzero(sym)[0]:
        bound = PR.adi_bound(verts[obj[i]], R_est[i].reshape(3, 3), t_est[i], R_gt[i].reshape(3, 3), t_gt[i])
        adi_units[i] = abs(out[i, 0] - ref[i, 0]) / (bound / 8.0)
    add_rel = rel[~sym, 0].max() if (~sym).any() else 0.0
    re_abs = np.abs(out[:, 1] - ref[:, 1]).max()
    print(f"{what}: ADD rel {add_rel:.3e}  re abs {re_abs:.3e} deg  te rel {rel[:, 2].max():.3e}  proj rel {rel[:, 3].max():.3e}  "
          f"ADI {adi_units.max():.4f} x 2^-24 rho")
    assert add_rel <= REL and rel[:, 2].max() <= REL and rel[:, 3].max() <= REL, what
    assert re_abs <= RE_ABS, what
    assert adi_units.max() <= 8.0, what


def test_kernel_against_the_reference_values_mixed_and_reversed(hip, g, meshes):
    n = len(g["obj"])
    fwd = _run(meshes, g, np.arange(n), **_sym_args(g))
    args = (g["verts_list"], g["obj"], g["R_est"], g["t_est"], g["R_gt"], g["t_gt"], g["symmetric"])
    check_against(fwd, g["errors"], *args, "one launch, all classes mixed")
    i = int(g["identity"])
    assert fwd[i, 1] < 1e-6 and fwd[i, 0] == 0.0 and fwd[i, 2] == 0.0 and fwd[i, 3] == 0.0
    rev = _run(meshes, g, np.arange(n)[::-1].copy(), **_sym_args(g))
    check_against(rev[::-1], g["errors"], *args, "the same pairs in reversed order")
    assert np.array_equal(rev[::-1], fwd)                   # a pair's result does not depend on its place in the launch
    again = _run(meshes, g, np.arange(n), **_sym_args(g))
    assert again.tobytes() == fwd.tobytes()                 # fixed summation order: two runs are bit-equal


def test_more_pairs_than_a_grid_dimension(hip, g):
    """b = 65 537 pairs of the two 3-point models (ADD and ADI with its one symmetry) against the restatement."""
    cls = [1, 13]
    verts = [g["verts_list"][c] for c in cls]
    assert [len(v) for v in verts] == [3, 3] and g["sym_infos"][13] is not None
    small = hip_lib.MeshSet(verts, [NO_FACE] * 2, DEV)
    rng = np.random.default_rng(5)
    m = 251                                                  # distinct pairs; pair i of the launch is distinct pair (7 i) mod 251
    base = np.array([k for k in range(len(g["obj"])) if g["obj"][k] in cls])
    pick = base[rng.integers(len(base), size=m)]
    obj = np.array([cls.index(g["obj"][k]) for k in pick], np.int32)
    R_est, t_est, R_gt, K = g["R_est"][pick], g["t_est"][pick].copy(), g["R_gt"][pick], g["K"][pick]
    t_gt = g["t_gt"][pick] + rng.uniform(-1e-3, 1e-3, (m, 3))
    symmetric, sym_infos = np.array([0, 1], np.uint8), [None, g["sym_infos"][13]]
    ref = PR.pose_errors(verts, obj, R_est, t_est, R_gt, t_gt, K, symmetric, sym_infos)
    b = 65537
    idx = (7 * np.arange(b)) % m
    out = hip_lib.pose_errors(small, T(obj[idx]), T(R_est[idx]), T(t_est[idx]), T(R_gt[idx]), T(t_gt[idx]), T(K[idx]),
                              sym_rots=T(g["sym_infos"][13].reshape(-1, 9)), sym_off=T(np.array([0, 0, 1], np.int32)),
                              symmetric=T(symmetric)).cpu().numpy()
    first = np.array([np.nonzero(idx == k)[0][0] for k in range(m)])
    check_against(out[first], ref, verts, obj, R_est, t_est, R_gt, t_gt, symmetric, "b = 65537, distinct pairs")
    assert np.array_equal(out, out[first][idx])             # every copy of a pair, wherever it sits, gives the same bits
    assert np.isfinite(out[-1]).all()


def test_single_pair_and_symmetric_class_without_a_symmetry_table(hip, g, meshes):
    for k in (0, 40, len(g["obj"]) - 2):
        one = _run(meshes, g, np.array([k]), **_sym_args(g))
        check_against(one, g["errors"][[k]], g["verts_list"], g["obj"][[k]], g["R_est"][[k]], g["t_est"][[k]], g["R_gt"][[k]], g["t_gt"][[k]],
                      g["symmetric"], f"b = 1, pair {k}")
    # sym_rots=None: ADI for the flagged classes, R_gt kept for re and proj
    n = len(g["obj"])
    out = _run(meshes, g, np.arange(n), symmetric=T(g["symmetric"]))
    ref = PR.pose_errors(g["verts_list"], g["obj"], g["R_est"], g["t_est"], g["R_gt"], g["t_gt"], g["K"], g["symmetric"], None)
    check_against(out, ref, g["verts_list"], g["obj"], g["R_est"], g["t_est"], g["R_gt"], g["t_gt"], g["symmetric"], "sym_rots=None")
    none = [i for i in range(n) if g["symmetric"][g["obj"][i]] and g["sym_infos"][g["obj"][i]] is None]
    assert none and np.abs(out[none] - g["errors"][none])[:, 1].max() <= RE_ABS      # K = 0 classes: the recorded values
    # symmetric=None: every class takes ADD
    out = _run(meshes, g, np.arange(n))
    ref = PR.pose_errors(g["verts_list"], g["obj"], g["R_est"], g["t_est"], g["R_gt"], g["t_gt"], g["K"])
    check_against(out, ref, g["verts_list"], g["obj"], g["R_est"], g["t_est"], g["R_gt"], g["t_gt"], np.zeros(24, np.uint8), "symmetric=None")
    assert hip_lib.pose_errors(meshes, T(g["obj"][:0]), T(g["R_est"][:0]), T(g["t_est"][:0]), T(g["R_gt"][:0]), T(g["t_gt"][:0]),
                               T(g["K"][:0])).shape == (0, 4)


def test_argument_errors_return_a_status_and_launch_nothing(hip, g, meshes):
    lib = hip_lib.load()
    b = 4
    a = [T(g[k][:b]) for k in ("obj", "R_est", "t_est", "R_gt", "t_gt", "K")]
    out = torch.full((b, 4), -7.0, dtype=torch.float64, device=DEV)
    need = lib.gdrnpp_pose_errors_workspace_bytes(meshes.c, b)
    assert need == 8 * b * (24 + 2 * ((2100 + 255) // 256))
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p = [t.data_ptr() for t in a]

    def call(ptrs, nb, ws_ptr, ws_bytes, m=meshes.c):
        return lib.gdrnpp_pose_errors(m, *ptrs, None, None, None, out.data_ptr(), nb, ws_ptr, ws_bytes, None)

    assert call([None] + p[1:], b, ws.data_ptr(), need) == -1 and b"null pointer" in lib.gdrnpp_last_error()
    assert call(p, 0, ws.data_ptr(), need) == -1
    assert call(p, b, ws.data_ptr(), need - 1) == -1 and b"workspace" in lib.gdrnpp_last_error()
    assert call(p, b, None, need) == -1
    assert call(p, b, ws.data_ptr(), need, None) == -1 and b"no models" in lib.gdrnpp_last_error()
    empty = hip_lib.gdrnpp_meshes(meshes.verts.data_ptr(), None, meshes.vert_off.data_ptr(), None, 0, 2100, 0)
    import ctypes
    assert call(p, b, ws.data_ptr(), need, ctypes.byref(empty)) == -1
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (ws == 0).all()          # nothing ran
    bad = g["obj"][:b].copy()
    bad[2] = 24
    with pytest.raises(RuntimeError, match="obj must lie in"):
        hip_lib.pose_errors(meshes, T(bad), *a[1:])
    with pytest.raises(RuntimeError, match="dtype"):
        hip_lib.pose_errors(meshes, a[0], a[1].float(), *a[2:])
    assert call(p, b, ws.data_ptr(), need) == 0             # and the same arguments, complete, run
    torch.cuda.synchronize()
    assert (out != -7.0).all()


def test_pysixd_shims_run_the_entry_point(hip, g):
    from gdrnpp_bop2022_amd.lib.pysixd import pose_error as PE

    k = 40                                                   # a symmetric class
    c = g["obj"][k]
    Re, te, Rg, tg, K = g["R_est"][k].reshape(3, 3), g["t_est"][k], g["R_gt"][k].reshape(3, 3), g["t_gt"][k], g["K"][k].reshape(3, 3)
    pts = g["verts_list"][c].astype(np.float64)
    assert g["symmetric"][c]
    assert abs(PE.adi(Re, te, Rg, tg, pts) - g["errors"][k, 0]) <= PR.adi_bound(pts, Re, te, Rg, tg)
    assert abs(PE.add(Re, te, Rg, tg, pts) - PR.add(Re, te, Rg, tg, pts)) <= REL * PR.add(Re, te, Rg, tg, pts)
    assert abs(PE.re(Re, Rg) - PR.re(Re, Rg)) <= RE_ABS and isinstance(PE.re(Re, Rg), float)
    assert abs(PE.te(te, tg) - g["errors"][k, 2]) <= REL * g["errors"][k, 2]
    Rs = g["R_gt_sym"][k].reshape(3, 3)
    assert abs(PE.arp_2d(Re, te, Rs, tg, pts, K) - g["errors"][k, 3]) <= REL * g["errors"][k, 3]


# ---- the evaluator end to end --------------------------------------------------------------------------------------------------
SYM_B = np.stack([np.diag([-1.0, -1.0, 1.0]), np.diag([1.0, -1.0, -1.0])])


def _rot(axis, angle):
    axis = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    Kx = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + np.sin(angle) * Kx + (1 - np.cos(angle)) * Kx.dot(Kx)


def _evaluator_case(e):
    """Per-image inputs with ``file_name`` and synthetic ground truths around the recorded poses of the five ROIs (classes 0 1 1 | 0 0):
    obj_b is symmetric and has no prediction in the second image; obj_c has ground truths and no prediction at all."""
    files = ["scene48/000007.png", "scene48/000008.png"]
    rng = np.random.default_rng(11)
    gts = {n: {} for n in e["names"]}
    roi = 0
    for k, (lo, hi) in enumerate(e["split"]):
        for i in range(lo, hi):
            name = e["names"][int(e["roi_cls"][i])]
            R, t = e["R"][i].astype(np.float64), e["maps"]["t_init"][i].astype(np.float64)
            start = R.dot(SYM_B[1]) if name == "obj_b" else R
            d = rng.standard_normal(3)
            gts[name].setdefault(files[k], {"R": start.dot(_rot(rng.standard_normal(3), (0.02, 0.06, 0.3, 0.012, 0.15)[roi])),
                                            "t": t + d / np.linalg.norm(d) * (0.004, 0.03, 0.2, 0.001, 0.07)[roi],
                                            "K": e["roi_cam"][i].astype(np.float64)})
            roi += 1
    gts["obj_b"][files[1]] = dict(gts["obj_b"][files[0]])
    gts["obj_c"][files[0]] = dict(gts["obj_a"][files[0]])
    return files, gts


def test_custom_evaluator_end_to_end(hip, tmp_path):
    e = EG.load()
    files, gts = _evaluator_case(e)
    verts = [e["maps"]["verts"][i] for i in range(3)]
    models = hip_lib.MeshSet(verts, [e["maps"]["faces"][i] for i in range(3)], DEV)
    diameters = [float(np.linalg.norm(v.max(0) - v.min(0))) for v in verts]
    sym_infos = [None, SYM_B, None]
    cfg = get_cfg("ycbv_convnext_a6")
    cfg.EXP_ID = e["exp_id"]
    cfg.DATASETS = {"SYM_OBJS": ["obj_b"]}
    kw = dict(obj_names=e["names"], obj2id=e["obj2id"], models=models, diameters=diameters, gts=gts, sym_infos=sym_infos)
    ev = CE.build_evaluator(cfg, "ycbv_test", False, str(tmp_path), **kw)
    assert type(ev) is CE.GDRN_EvaluatorCustom
    cfg_bop = get_cfg("ycbv_convnext_a6")
    cfg_bop.VAL.USE_BOP = True
    assert type(CE.build_evaluator(cfg_bop, "ycbv_test", False, None, **kw)) is GDRN_Evaluator
    cfg_bop.VAL.USE_BOP = False
    assert type(CE.build_evaluator(cfg_bop, "ycbv_test", False, None, **kw)) is CE.GDRN_EvaluatorCustom

    ev.reset()
    inputs = EG.image_inputs(e, DEV)
    for k, (lo, hi) in enumerate(e["split"]):
        inputs[k]["file_name"] = [files[k]] * int(hi - lo)
    ev.process(inputs, [dict(time=float(t)) for t in e["fwd_time"]], EG.out_dict(e, DEV))       # both images in one call
    preds = list(ev._predictions)
    assert len(preds) == 5 and [p["cls_name"] for p in preds] == [e["names"][int(c)] for c in e["roi_cls"]]
    for i, p in enumerate(preds):                            # running ROI index; R 3x3, t in metres
        assert set(p) == {"cls_name", "file_name", "score", "R", "t", "time"} and p["R"].shape == (3, 3) and p["t"].shape == (3,)
        assert np.array_equal(p["R"], e["R"][i]) and np.array_equal(p["t"], e["maps"]["t_init"][i]) and p["file_name"] == files[i >= 3]
    assert ev.evaluate() == {}

    slots, pairs = CE.match_pairs(gts, CE.reorganize_preds(preds), e["names"])
    assert list(slots) == ["obj_a", "obj_b"] and slots["obj_b"][1] is None and len(pairs) == 3
    ref = np.stack([PR.pair_errors(verts[lb], np.asarray(Re, np.float64), np.asarray(te, np.float64), Rg, tg, K, lb == 1, sym_infos[lb])
                    for lb, Re, te, Rg, tg, K in pairs])
    for (lb, *_), row in zip(pairs, ref):                    # the case keeps clear of every threshold: the tables must agree
        for value, ths in zip(row, ([f * diameters[lb] for f in (0.02, 0.05, 0.1)], (2, 5, 10), (0.02, 0.05, 0.1), (2, 5, 10))):
            assert all(abs(value - th) > 1e-3 * th for th in ths), (row, ths)
    _, _, table = CE.summarize_errors(slots, ref, diameters, e["names"])
    stem = f"{e['exp_id'].replace('_', '-')}_ycbv_test"
    assert sorted(os.listdir(tmp_path)) == sorted([stem + "_tab.txt", stem + "_errors.pkl", stem + "_recalls.pkl"])
    assert open(tmp_path / (stem + "_tab.txt")).read() == table + "\n"
    errors = pickle.load(open(tmp_path / (stem + "_errors.pkl"), "rb"))
    got = np.array([[errors[n][k][j] for k in CE.ERROR_NAMES] for n in errors for j in range(len(errors[n]["ad"]))])
    lbs = np.array([p[0] for p in pairs])
    check_against(got, ref, verts, lbs, np.stack([np.asarray(p[1], np.float64).reshape(9) for p in pairs]),
                  np.stack([np.asarray(p[2], np.float64) for p in pairs]), np.stack([p[3].reshape(9) for p in pairs]),
                  np.stack([p[4] for p in pairs]), np.array([0, 1, 0]), "evaluator end to end")
    recalls = pickle.load(open(tmp_path / (stem + "_recalls.pkl"), "rb"))
    assert len(recalls["obj_b"]["ad_2"]) == 2 and recalls["obj_b"]["ad_2"][1] == 0.0
