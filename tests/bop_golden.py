"""Loaders of tests/golden/bop_error_golden.npz and bop_eval_golden.npz (recorded from the reference's own functions and scripts by
tests/golden/make_golden_bop_error.py / make_golden_bop_eval.py), shared by test_bop_eval_cpu.py and test_gpu_bop_error.py."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _int_keys(d):
    return {int(k): v for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def load_error():
    z = np.load(os.path.join(GOLDEN, "bop_error_golden.npz"))
    g = {k: z[k] for k in z.files}
    g["models_info"] = _int_keys(json.loads(str(z["models_info"])))
    g["kinds"] = json.loads(str(z["kinds"]))
    g["max_sym_disc_step"] = float(z["max_sym_disc_step"])
    g["verts_list"] = [g["verts"][g["vert_off"][c]:g["vert_off"][c + 1]] for c in range(len(g["vert_off"]) - 1)]
    return g


@functools.lru_cache(maxsize=None)
def load_eval():
    z = np.load(os.path.join(GOLDEN, "bop_eval_golden.npz"))
    g = {k: json.loads(str(z[k])) for k in ("dataset", "models_info", "targets", "scene_gt", "scene_gt_info", "scene_camera", "recorded")}
    g["models_info"] = _int_keys(g["models_info"])
    obj_ids = g["dataset"]["obj_ids"]
    g["vertices"] = {o: z["verts"][z["vert_off"][k]:z["vert_off"][k + 1]] for k, o in enumerate(obj_ids)}
    g["records"] = [dict(scene_id=str(int(i[0])), im_id=int(i[1]), obj_id=int(i[2]), score=float(s), R=R.tolist(), t=t.tolist(), time=float(tm))
                    for i, s, R, t, tm in zip(z["est_ids"], z["est_score"], z["est_R"], z["est_t"], z["est_time"])]
    return g


def bop_gt(g):
    from gdrnpp_bop2022_amd.gdrn_modeling.bop_eval import BopGT

    d = g["dataset"]
    return BopGT(g["scene_gt"], g["scene_gt_info"], g["scene_camera"], g["targets"], g["models_info"], d["symmetric_obj_ids"],
                 g["vertices"], d["im_width"], obj_ids=d["obj_ids"], scene_ids=d["scene_ids"])


def recorded_errors(g, n_top, error_type):
    """{scene_id: [{"im_id", "obj_id", "est_id", "score", "errors": {gt_id: [...]}}]} as eval_calc_scores.py loads them (integer keys)."""
    raw = g["recorded"][str(n_top)]["types"][error_type]["errors"]
    return {int(s): [dict(e, errors={int(k): [float(x) for x in v] for k, v in e["errors"].items()}) for e in errs] for s, errs in raw.items()}
