"""Loader of tests/golden/vsd_golden.npz (recorded from the reference's own ``pose_error.vsd`` and evaluation scripts by
tests/golden/make_golden_vsd.py), shared by test_vsd_cpu.py and test_gpu_vsd.py."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _int_keys(d):
    return {int(k): v for k, v in d.items()}


@functools.lru_cache(maxsize=None)
def load():
    z = np.load(os.path.join(GOLDEN, "vsd_golden.npz"))
    e = {k: json.loads(str(z[k])) for k in ("dataset", "models_info", "targets", "scene_gt", "scene_gt_info", "scene_camera", "recorded")}
    e["models_info"] = _int_keys(e["models_info"])
    d = e["dataset"]
    obj_ids, scene, im_ids = d["obj_ids"], d["scene_id"], d["im_ids"]
    verts_list = [z["verts"][z["vert_off"][k]:z["vert_off"][k + 1]] for k in range(len(obj_ids))]
    faces_list = [z["faces"][z["face_off"][k]:z["face_off"][k + 1]] for k in range(len(obj_ids))]
    e["vertices"], e["faces"] = dict(zip(obj_ids, verts_list)), dict(zip(obj_ids, faces_list))
    e["records"] = [dict(scene_id=str(int(i[0])), im_id=int(i[1]), obj_id=int(i[2]), score=float(s), R=R.tolist(), t=t.tolist(), time=float(tm))
                    for i, s, R, t, tm in zip(z["est_ids"], z["est_score"], z["est_R"], z["est_t"], z["est_time"])]
    e["depth_stored"] = {scene: {im: z["depth"][k] for k, im in enumerate(im_ids)}}          # uint16, as the PNGs hold it
    scale = {im: float(e["scene_camera"][str(scene)][str(im)]["depth_scale"]) for im in im_ids}
    depth_mm = np.stack([z["depth"][k].astype(np.float32) * np.float32(scale[im]) for k, im in enumerate(im_ids)])
    # function level: one row per (estimate, ground truth of its object in its image)
    gts = e["scene_gt"][str(scene)]
    pe, pim, pgt = z["pair_est"], z["pair_im"], z["pair_gt"]
    g = [gts[str(int(im))][int(k)] for im, k in zip(pim, pgt)]
    K = np.array([e["scene_camera"][str(scene)][str(int(im))]["cam_K"] for im in pim], np.float64)
    obj = np.array([obj_ids.index(int(z["est_ids"][k][2])) for k in pe], np.int32)
    func = dict(obj=obj, im=np.array([im_ids.index(int(im)) for im in pim], np.int32), R_est=z["est_R"][pe], t_est=z["est_t"][pe],
                R_gt=np.array([x["cam_R_m2c"] for x in g], np.float64), t_gt=np.array([x["cam_t_m2c"] for x in g], np.float64), K=K,
                diameter=np.array([e["models_info"][obj_ids[o]]["diameter"] for o in obj], np.float64), depth=depth_mm,
                counts=z["pair_counts"], errors=z["pair_errors"], overlap=z["pair_overlap"])
    return dict(script=e, func=func, taus=[float(t) for t in z["taus"]], delta=float(z["delta"]), verts_list=verts_list, faces_list=faces_list)


def bop_gt(g, with_depth=True):
    from gdrnpp_bop2022_amd.gdrn_modeling.bop_eval import BopGT

    e = g["script"]
    d = e["dataset"]
    extra = dict(faces=e["faces"], depth=e["depth_stored"], im_size=d["im_size"], dataset=d["name"]) if with_depth else {}
    return BopGT(e["scene_gt"], e["scene_gt_info"], e["scene_camera"], e["targets"], e["models_info"], d["symmetric_obj_ids"], e["vertices"],
                 d["im_width"], obj_ids=d["obj_ids"], scene_ids=d["scene_ids"], **extra)


def recorded_errors(g, n_top, error_type):
    """{scene_id: [{"im_id", "obj_id", "est_id", "score", "errors": {gt_id: [...]}}]} with integer keys.  For ``vsd`` the scripts write
    one file set per tau, each holding that tau's element alone: they are put back together, all taus per ground truth."""
    rec = g["script"]["recorded"][str(n_top)]["types"][error_type]

    def ints(raw):
        return {int(s): [dict(e, errors={int(k): [float(x) for x in v] for k, v in e["errors"].items()}) for e in errs] for s, errs in raw.items()}

    if error_type != "vsd":
        return ints(rec["errors"])
    per_tau = [ints(x["errors"]) for x in rec]
    out = per_tau[0]
    for other in per_tau[1:]:
        for s in out:
            for e, o in zip(out[s], other[s]):
                assert (e["im_id"], e["obj_id"], e["est_id"]) == (o["im_id"], o["obj_id"], o["est_id"])
                for k in e["errors"]:
                    e["errors"][k] = e["errors"][k] + o["errors"][k]
    return out


def recorded_vsd_recalls(g, n_top):
    """[tau][threshold] recalls as the scripts' scores files hold them."""
    return [[th["scores"]["recall"] for th in x["thresholds"]] for x in g["script"]["recorded"][str(n_top)]["types"]["vsd"]]
