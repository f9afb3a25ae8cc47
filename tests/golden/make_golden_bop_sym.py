"""Golden symmetry-aware reS / teS / projS values and scores from the reference's own functions and scripts (authoring container only:
needs /root/reference).  Nothing new is invented here: the inputs are what the committed fixtures already hold.

(a) function level: the reference's ``lib/pysixd/pose_error.py`` ``re_sym / te_sym / arp_2d_sym`` are executed from their source, through
    tests/golden/_refimport.py, on every pair of bop_error_golden.npz (67 pairs; point counts 1 .. 1025 and symmetry counts 1 .. 628 at
    the wave, workgroup and chunk edges of csrc/sym_error.hip, the same as csrc/bop_error.hip's; one exact-identity pair), with the
    reference's ``get_symmetry_transformations`` at the recorded ``max_sym_disc_step`` -> ``errors`` f64[pairs,3] = reS (deg), teS (mm),
    projS (px); beside them per pair ``sin_re`` = sin(reS) and ``max_dist2d``, the largest per-point 2-D distance over all symmetries
    (what the test derives its tolerances from).
(b) script level: ``lib/pysixd/scripts/eval_pose_results_more.py`` is run UNMODIFIED, in-process, exactly as make_golden_bop_eval.py and
    make_golden_vsd.py run it (their helpers are imported, the files are not edited), on the dataset of bop_eval_golden.npz (hb layout)
    with ``--error_types=reS,teS,projS`` and on the dataset of vsd_golden.npz (lmo layout, with depth) with
    ``--error_types=ad,reS,teS,projS``, for ``n_top`` -1 and 1.  Per type: the ``errors_*.json`` content, per threshold the matches and the
    ``scores_*.json`` content, and ``scores_bop19.json``.

Conditions asserted here, about the reference alone: every error element is at least 1e-3 * th away from every threshold of its type; on
the function-level inputs every posed point has z >= 300 mm and every per-point 2-D distance is below 2e3 px; for each of the three types
the recalls at 2, 5 and 10 are not all equal on at least one dataset; the file is smaller than 1 MiB."""
import glob
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))

import make_golden_bop_eval as MB  # noqa: E402  (installs _refimport; a temporary BOP tree of its own)
import make_golden_vsd as MV  # noqa: E402

from tests import bop_golden as BG  # noqa: E402
from tests import vsd_golden as VG  # noqa: E402

SYM_TYPES = ["reS", "teS", "projS"]
SYM_THS = [2, 5, 10]                                                # eval_pose_results_more.py:136-155
RUNS = {"hb": (MB, ["reS", "teS", "projS"]), "lmo": (MV, ["ad", "reS", "teS", "projS"])}
N_TOPS = [-1, 1]
MIN_REL_GAP = 1e-3


def function_level():
    from lib.pysixd import misc as M
    from lib.pysixd import pose_error as PE

    g = BG.load_error()
    n = len(g["obj"])
    errors, sin_re, max_dist = np.empty((n, 3)), np.empty(n), np.empty(n)
    for i, c in enumerate(g["obj"]):
        syms = M.get_symmetry_transformations(g["models_info"][int(c) + 1], g["max_sym_disc_step"])
        assert len(syms) == g["sym_off"][c + 1] - g["sym_off"][c]
        pts = g["verts_list"][c].astype(np.float64)
        Re, te, Rg, tg, K = g["R_est"][i].reshape(3, 3), g["t_est"][i].reshape(3, 1), g["R_gt"][i].reshape(3, 3), g["t_gt"][i].reshape(3, 1), g["K"][i].reshape(3, 3)
        errors[i] = [PE.re_sym(Re, Rg, syms), PE.te_sym(te, tg, Rg, syms), PE.arp_2d_sym(Re, te, Rg, tg, pts, K, syms)]
        sin_re[i] = np.sin(np.deg2rad(errors[i, 0]))
        est_2d = PE.transform_pts_Rt_2d(pts, Re, te, K)
        assert PE.transform_pts_Rt(pts, Re, te)[:, 2].min() >= 300.0, i
        worst = 0.0
        for s in syms:
            R, t = Rg.dot(s["R"]), Rg.dot(s["t"]) + tg
            assert PE.transform_pts_Rt(pts, R, t)[:, 2].min() >= 300.0, i
            worst = max(worst, float(np.linalg.norm(est_2d - PE.transform_pts_Rt_2d(pts, R, t, K), axis=1).max()))
        assert worst < 2e3, (i, worst)
        max_dist[i] = worst
    ident = int(g["identity"])
    assert errors[ident, 1] == 0.0 and errors[ident, 2] == 0.0
    print("function level:", n, "pairs; reS", errors[:, 0].min(), errors[:, 0].max(), " teS", errors[:, 1].min(), errors[:, 1].max(),
          " projS", errors[:, 2].min(), errors[:, 2].max(), " largest 2-D distance", max_dist.max())
    return errors, sin_re, max_dist


def hb_tree():
    g = BG.load_eval()
    ints = lambda d: {int(k): v for k, v in d.items()}
    scene_gt = {s: {im: [{"obj_id": x["obj_id"], "cam_R_m2c": np.array(x["cam_R_m2c"], np.float64).reshape(3, 3),
                          "cam_t_m2c": np.array(x["cam_t_m2c"], np.float64)} for x in gts] for im, gts in ints(v).items()}
                for s, v in ints(g["scene_gt"]).items()}
    scene_gt_info = {s: ints(v) for s, v in ints(g["scene_gt_info"]).items()}
    scene_camera = {s: {im: {"cam_K": np.array(c["cam_K"], np.float64).reshape(3, 3), "depth_scale": 1.0} for im, c in ints(v).items()}
                    for s, v in ints(g["scene_camera"]).items()}
    ests = [dict(scene_id=int(r["scene_id"]), im_id=r["im_id"], obj_id=r["obj_id"], score=r["score"], R=np.array(r["R"]).reshape(3, 3),
                 t=np.array(r["t"]), time=r["time"]) for r in g["records"]]
    return MB.write_tree(g["vertices"], g["models_info"], scene_gt, scene_gt_info, scene_camera, g["targets"], ests), g["dataset"]["result_name"]


def lmo_tree():
    e = VG.load()["script"]
    scene = e["dataset"]["scene_id"]
    ints = lambda d: {int(k): v for k, v in d.items()}
    scene_gt = {im: [{"obj_id": x["obj_id"], "cam_R_m2c": np.array(x["cam_R_m2c"], np.float64).reshape(3, 3),
                      "cam_t_m2c": np.array(x["cam_t_m2c"], np.float64)} for x in gts] for im, gts in ints(e["scene_gt"][str(scene)]).items()}
    scene_gt_info = ints(e["scene_gt_info"][str(scene)])
    scene_camera = {im: {"cam_K": np.array(c["cam_K"], np.float64).reshape(3, 3), "depth_scale": c["depth_scale"]}
                    for im, c in ints(e["scene_camera"][str(scene)]).items()}
    ests = [dict(scene_id=int(r["scene_id"]), im_id=r["im_id"], obj_id=r["obj_id"], score=r["score"], R=np.array(r["R"]).reshape(3, 3),
                 t=np.array(r["t"]), time=r["time"]) for r in e["records"]]
    assert MV.SCENE == scene
    return MV.write_tree(e["vertices"], e["faces"], e["models_info"], scene_gt, scene_gt_info, scene_camera, e["targets"],
                         e["depth_stored"][scene], ests), e["dataset"]["result_name"]


def run_scripts(mod, results_path, result_name, error_types):
    """eval_pose_results_more.py on the tree ``mod`` wrote, for both n_top -> what make_golden_bop_eval.py records per type."""
    import lib.pysixd.config as ref_config

    ref_config.datasets_path = os.path.join(mod.TMP, "datasets")   # the scripts read it at each run
    script = os.path.join(MB._refimport.REF, "lib", "pysixd", "scripts", "eval_pose_results_more.py")
    recorded = {}
    for n_top in N_TOPS:
        eval_path = os.path.join(mod.TMP, f"eval_sym_ntop{n_top}")
        mod.run_script_in_process(["python", script, f"--result_filenames={result_name}.csv", f"--results_path={results_path}",
                                   f"--eval_path={eval_path}", f"--targets_filename={mod.TARGETS}", "--error_types=" + ",".join(error_types),
                                   f"--n_top={n_top}"])
        rec = {"final": json.load(open(os.path.join(eval_path, result_name, "scores_bop19.json"))), "types": {}}
        for t in error_types:
            d = os.path.join(eval_path, result_name, f"error:{t}_ntop:{n_top}")
            errors = {int(os.path.basename(p)[7:13]): json.load(open(p)) for p in sorted(glob.glob(os.path.join(d, "errors_*.json")))}
            per_th = []
            for p in sorted(glob.glob(os.path.join(d, "scores_th:*.json")),
                          key=lambda q: float(os.path.basename(q)[len("scores_th:"):].split("_")[0].split("-")[0])):
                sign = os.path.basename(p)[len("scores_"):-len(".json")]
                ms = json.load(open(os.path.join(d, f"matches_{sign}.json")))
                per_th.append({"sign": sign, "scores": json.load(open(p)),
                               "matches": [[m["scene_id"], m["im_id"], m["obj_id"], m["gt_id"], m["est_id"], bool(m["valid"])] for m in ms]})
            assert errors and len(per_th) == 3, (t, d)
            rec["types"][t] = {"errors": errors, "thresholds": per_th}
        recorded[str(n_top)] = rec
    return recorded


def main():
    errors, sin_re, max_dist = function_level()

    real_call = subprocess.call
    subprocess.call = MB.run_script_in_process
    recorded = {}
    try:
        for name, tree in (("hb", hb_tree), ("lmo", lmo_tree)):
            mod, types = RUNS[name]
            results_path, result_name = tree()
            recorded[name] = run_scripts(mod, results_path, result_name, types)
    finally:
        subprocess.call = real_call

    # ---- conditions, about the reference alone ---------------------------------------------------------------------------------------
    gaps, spread = {}, {t: False for t in SYM_TYPES}
    for name, per_top in recorded.items():
        gap = np.inf
        for n_top, rec in per_top.items():
            for t in SYM_TYPES:
                r = rec["types"][t]
                for errs in r["errors"].values():
                    for e in errs:
                        for vals in e["errors"].values():
                            assert len(vals) == 1 and np.isfinite(vals[0]), (t, e)
                            gap = min(gap, min(abs(vals[0] - th) / th for th in SYM_THS))
                recalls = [x["scores"]["recall"] for x in r["thresholds"]]
                assert rec["final"][f"bop19_average_recall_{t}"] == float(np.mean(recalls)), t
                spread[t] |= len(set(recalls)) > 1
                print(name, n_top, t, ["%.3f" % x for x in recalls])
            assert "bop19_average_recall" not in rec["final"]
        gaps[name] = gap
        assert gap >= MIN_REL_GAP, (name, gap)
    assert all(spread.values()), spread
    print("smallest relative gap to a threshold:", gaps)

    path = os.path.join(HERE, "bop_sym_golden.npz")
    np.savez_compressed(path, errors=errors, sin_re=sin_re, max_dist2d=max_dist, thresholds=np.array(SYM_THS, np.float64),
                        error_types=json.dumps({name: types for name, (_, types) in RUNS.items()}), recorded=json.dumps(recorded))
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("wrote bop_sym_golden.npz:", len(errors), "pairs,", size, "bytes; final:", {k: v["-1"]["final"] for k, v in recorded.items()})


if __name__ == "__main__":
    main()
