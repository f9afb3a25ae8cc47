"""Host side of the custom evaluator's pose errors (no GPU): the NumPy restatement against the values recorded from the reference's own
functions, the ABI declaration, and the host-only table assembly against the reference's recorded table text."""
import os
import pickle
import re as regex
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tests import pose_error_ref as PR  # noqa: E402


@pytest.fixture(scope="module")
def g():
    return PR.load_golden()


def test_golden_covers_the_kernel_edges(g):
    counts = np.diff(g["vert_off"]).tolist()
    edges = [1, 3, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2100]
    assert counts == edges + edges
    assert g["symmetric"].tolist() == [0] * 12 + [1] * 12
    assert sorted({0 if s is None else len(s) for s in g["sym_infos"][12:]}) == [0, 1, 6]
    assert all(s is None for s in g["sym_infos"][:12])
    for c in range(24):                                           # every class, hence every point count, in ADD and in ADI
        assert (g["obj"] == c).sum() >= 3
    assert os.path.getsize(PR.GOLDEN) < 1 << 20


def test_restatement_reproduces_every_recorded_value(g):
    ours = PR.pose_errors(g["verts_list"], g["obj"], g["R_est"], g["t_est"], g["R_gt"], g["t_gt"], g["K"], g["symmetric"], g["sym_infos"])
    ref = g["errors"]
    worst = np.abs(ours - ref) / np.where(ref != 0, np.abs(ref), 1.0)
    print("restatement vs recorded, max relative difference per column:", worst.max(0))
    assert worst.max() <= 1e-12
    i = int(g["identity"])
    assert ours[i, 1] < 1e-6 and ours[i, 0] == 0.0 and ours[i, 2] == 0.0 and ours[i, 3] == 0.0
    for k in range(len(g["obj"])):
        c = g["obj"][k]
        R_sym = PR.get_closest_rot(g["R_est"][k].reshape(3, 3), g["R_gt"][k].reshape(3, 3), g["sym_infos"][c]) if g["symmetric"][c] else g["R_gt"][k].reshape(3, 3)
        assert np.array_equal(R_sym.reshape(9), g["R_gt_sym"][k])


def test_symbols_are_declared_in_the_header_and_in_signatures():
    from gdrnpp_bop2022_amd.hip_lib import abi

    header = open(os.path.join(ROOT, "include", "gdrnpp_hip.h")).read()
    assert regex.search(r"size_t\s+gdrnpp_pose_errors_workspace_bytes\(const gdrnpp_meshes\*\s*models,\s*int b\);", header)
    assert regex.search(r"int\s+gdrnpp_pose_errors\(const gdrnpp_meshes\*\s*models,", header)
    res, args = abi.SIGNATURES["gdrnpp_pose_errors"]
    assert res is abi.c_int and len(args) == 15 and args[-1] is abi.c_void_p and args[-2] is abi.c_size_t
    assert abi.SIGNATURES["gdrnpp_pose_errors_workspace_bytes"][0] is abi.c_size_t
    if os.path.exists(abi.LIB_PATH):
        lib = abi.load()
        assert lib.gdrnpp_pose_errors_workspace_bytes(None, 4) == 0
        assert lib.gdrnpp_pose_errors(None, None, None, None, None, None, None, None, None, None, None, 1, None, 0, None) == -1
        assert b"no models" in lib.gdrnpp_last_error()
    from gdrnpp_bop2022_amd import hip_lib
    assert hip_lib.pose_errors is hip_lib.pose.pose_errors


def _walk_errors(g):
    """The golden errors in the order ``match_pairs`` numbers the pairs of ``table_case``."""
    from gdrnpp_bop2022_amd.gdrn_modeling import gdrn_custom_evaluator as CE

    gts, preds, walk = PR.table_case(g)
    slots, pairs = CE.match_pairs(gts, CE.reorganize_preds(preds), g["names"])
    assert len(pairs) == len(walk)
    for k, i in enumerate(walk):                                # each pair is the golden pair the walk says it is
        label, R_est, t_est, R_gt, t_gt, K = pairs[k]
        assert label == g["obj"][i]
        assert np.array_equal(np.asarray(R_est, np.float64).reshape(9), g["R_est"][i]) and np.array_equal(np.asarray(t_est, np.float64), g["t_est"][i])
        assert np.array_equal(R_gt.reshape(9), g["R_gt"][i]) and np.array_equal(t_gt, g["t_gt"][i]) and np.array_equal(K.reshape(9), g["K"][i])
    return slots, g["errors"][walk]


@pytest.mark.parametrize("mode", ["recall", "precision"])
def test_table_assembly_reproduces_the_reference_text(g, mode):
    from gdrnpp_bop2022_amd.gdrn_modeling import gdrn_custom_evaluator as CE

    slots, errs = _walk_errors(g)
    assert any(s is None for v in slots.values() for s in v)     # images without a prediction: recall and precision differ
    assert g["names"][-1] not in slots and "no_such_object" not in slots
    errors, rates, table = CE.summarize_errors(slots, errs, g["diameters"].tolist(), g["names"], eval_precision=mode == "precision")
    assert table + "\n" == g[mode + "_table"]
    assert g["recall_table"] != g["precision_table"]
    assert list(errors[g["names"][0]]) == ["ad", "re", "te", "proj"] and list(rates[g["names"][0]]) == list(CE.METRIC_NAMES)
    n_gt, n_pred = len(slots[g["names"][0]]), sum(s is not None for s in slots[g["names"][0]])
    assert n_gt == n_pred + 1
    assert len(rates[g["names"][0]]["ad_2"]) == (n_pred if mode == "precision" else n_gt)
    assert len(errors[g["names"][0]]["ad"]) == n_pred


def test_reorganize_preds_keeps_order_and_first_prediction(g):
    from gdrnpp_bop2022_amd.gdrn_modeling import gdrn_custom_evaluator as CE

    _, preds, _ = PR.table_case(g)
    res = CE.reorganize_preds(preds)
    assert list(res) == g["names"][:-1] + ["no_such_object"]
    i = [k for k in range(len(g["obj"])) if g["obj"][k] == 1][0]
    both = res[g["names"][1]][f"img_{i}"]
    assert len(both) == 2 and both[0]["score"] == pytest.approx(0.5 + 0.001 * i) and both[1]["score"] == 0.1
    assert set(both[0]) == {"score", "R", "t", "time"}


def test_evaluate_writes_the_reference_files(g, tmp_path):
    """``evaluate`` end to end on the host, with the one device call served by the restatement."""
    from gdrnpp_bop2022_amd.gdrn_modeling import gdrn_custom_evaluator as CE
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg

    gts, preds, walk = PR.table_case(g)
    calls = []

    class HostEvaluator(CE.GDRN_EvaluatorCustom):
        def pair_errors(self, pairs):
            calls.append(len(pairs))
            return g["errors"][walk]

    for precision in (False, True):
        cfg = get_cfg("ycbv_convnext_a6")
        cfg.EXP_ID = g["exp_id"]
        assert "DATASETS" not in cfg and "EVAL_PRECISION" not in cfg.VAL          # the defaults of config.py stay as they are
        out = tmp_path / ("p" if precision else "r")
        kw = dict(obj_names=g["names"], obj2id={n: i + 1 for i, n in enumerate(g["names"])}, models=types.SimpleNamespace(n_obj=24),
                  diameters=g["diameters"], gts=gts, sym_infos=g["sym_infos"])
        ev = HostEvaluator(cfg, g["dataset_name"], False, str(out), **kw)
        assert ev.eval_precision is False and ev.sym_objs == []                  # configs without the keys work
        cfg.VAL.EVAL_PRECISION = precision
        cfg.DATASETS = {"SYM_OBJS": g["sym_objs"]}
        ev = HostEvaluator(cfg, g["dataset_name"], False, str(out), **kw)
        ev.reset()
        ev._predictions.extend(preds)
        assert ev.evaluate() == {}
        stem = f"{g['exp_id'].replace('_', '-')}_{g['dataset_name']}"
        tab, rate = ("_tab_precisions.txt", "_precisions.pkl") if precision else ("_tab.txt", "_recalls.pkl")
        assert sorted(os.listdir(out)) == sorted([stem + tab, stem + "_errors.pkl", stem + rate])
        assert open(out / (stem + tab)).read() == g["precision_table" if precision else "recall_table"]
        errors = pickle.load(open(out / (stem + "_errors.pkl"), "rb"))
        assert np.array_equal(np.array([errors[n]["re"][0] for n in errors]), g["errors"][[[k for k in walk if g["obj"][k] == c][0] for c in range(23)], 1])
    assert calls == [len(walk), len(walk)]                                       # one call per evaluate


def test_shims_have_the_reference_signatures_and_no_cpu_fallback(monkeypatch):
    import inspect

    import torch

    from gdrnpp_bop2022_amd.lib.pysixd import pose_error as PE

    assert list(inspect.signature(PE.add).parameters) == ["R_est", "t_est", "R_gt", "t_gt", "pts"] == list(inspect.signature(PE.adi).parameters)
    assert list(inspect.signature(PE.re).parameters) == ["R_est", "R_gt"] and list(inspect.signature(PE.te).parameters) == ["t_est", "t_gt"]
    assert list(inspect.signature(PE.arp_2d).parameters) == ["R_est", "t_est", "R_gt", "t_gt", "pts", "K"]
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    R, t, pts = np.eye(3), np.zeros(3), np.zeros((4, 3))
    for call in (lambda: PE.add(R, t, R, t, pts), lambda: PE.adi(R, t, R, t, pts), lambda: PE.re(R, R), lambda: PE.te(t, t),
                 lambda: PE.arp_2d(R, t, R, t, pts, np.eye(3))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
