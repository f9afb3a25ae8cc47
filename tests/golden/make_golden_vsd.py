"""Golden BOP19 VSD errors and scores from the reference's own function and scripts (authoring container only: needs /root/reference).

A synthetic BOP dataset laid out as ``lmo`` / ``test`` (scene 2, 640x480, 4 images with 16-bit PNG depth) is written to a temporary
directory, then

(a) function level: the reference's ``lib/pysixd/pose_error.vsd`` is executed from its source on every (estimate, ground truth) pair of
    the dataset.  Its ``renderer`` argument is an object whose ``render_object`` is served by ``oracle.postproc.render_depth`` (third-party
    GL, served by the oracle as everywhere else; the clip planes let everything in front of the camera through);
(b) script level: ``lib/pysixd/scripts/eval_pose_results_more.py`` is run UNMODIFIED, in-process, as make_golden_bop_eval.py runs it,
    with ``--error_types=vsd,mssd,mspd`` for ``n_top`` -1 and 1.  ``lib.pysixd.renderer.create_renderer`` (GL) and ``imageio.imread``
    (absent) are replaced for the duration by the oracle- and PIL-backed stand-ins below.

The oracle takes float32 K and R, so every rotation and the intrinsics of this dataset are float32 values (tests/test_gpu_vsd.py covers
fp64 poses against tests/vsd_ref.py).  Depth images: a fronto-parallel wall, the ground-truth objects rendered in front of it, one slab
over part of an object and one over a whole object, holes of 0; whole millimetres (one image stored at depth_scale 0.5).  Estimates: the
LADDER perturbations of make_golden_bop_eval.py, one equal to its ground truth, one whose sphere projection overlaps no ground truth, one
behind the wall, one beside its ground truth (no common pixel), one under the full slab.

Conditions asserted here (about the reference alone; the seed is advanced until they hold), so that a last-bit difference of a device
sqrt or division could not move a count: over all pairs no pixel has |d_diff - delta| < 1e-3 mm (8 float32 ulps at these distances);
no intersection pixel has |dist / diameter - tau| < 1e-6 tau; no error element is within 1e-9 of a threshold; at least three different
values of union, a pair with inter == 0 and a pair with union == 0 occur.  The NumPy restatement tests/vsd_ref.py must reproduce the
function-level errors exactly (it supplies the integer counts that are recorded beside them)."""
import glob
import json
import os
import runpy
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))

TMP = tempfile.mkdtemp(prefix="vsd_golden_")
os.environ["BOP_PATH"] = os.path.join(TMP, "datasets")             # lib/pysixd/config.py reads it at import

import _refimport  # noqa: E402

_refimport.install()

import chardet  # noqa: E402
import termcolor  # noqa: E402

chardet.detect = lambda data: {"encoding": "ascii", "confidence": 1.0, "language": ""}      # the ply files below are 7-bit
termcolor.colored = lambda text, *a, **k: text

from PIL import Image  # noqa: E402

from gdrnpp_bop2022_amd import synthetic as S  # noqa: E402
from tests import vsd_ref as V  # noqa: E402

DATASET, SPLIT, IM_SIZE = "lmo", "test", (640, 480)
OBJ_IDS, SCENE_IDS, SYMMETRIC = [1, 5, 6, 8, 9, 10, 11, 12], [2], [10, 11]                  # dataset_params.py, lmo
SCENE = 2
ERROR_TYPES = ["vsd", "mssd", "mspd"]
N_TOPS = [-1, 1]
RESULT_NAME = "gdrn-iter0_lmo-test"
TARGETS = "test_targets_bop19.json"
DELTA = 15.0                                                        # eval_pose_results_more.py:45-59, lmo
TAUS = list(np.arange(0.05, 0.51, 0.05))
Z_NEAR, Z_FAR = 1.0, 1e6
WALL = 1500.0
LADDER = [(0.005, 0.5), (0.03, 3.0), (0.1, 8.0), (0.3, 25.0), (1.0, 80.0)]      # (rad, mm)
# image -> (ground-truth objects, {target object: inst_count}, visib_fract per ground truth, depth_scale)
LAYOUT = {
    0: ([1, 6, 6, 6, 5], {1: 1, 6: 3}, [0.95, 0.9, 0.6, 0.8, 0.7], 1.0),
    1: ([10, 10, 1], {10: 2, 1: 1}, [0.8, 0.85, 0.4], 0.5),
    3: ([6, 10, 5, 8], {6: 1, 10: 1, 8: 1}, [0.5, 0.75, 0.9, 0.1], 1.0),
    7: ([8, 9, 12], {8: 1, 9: 1, 12: 1}, [0.9, 0.8, 0.7], 1.0),
}


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


K = f32([[572.4114, 0.0, 325.2611], [0.0, 573.57043, 242.04899], [0.0, 0.0, 1.0]])


def rotvec(axis, angle):
    from scipy.spatial.transform import Rotation
    return Rotation.from_rotvec(np.asarray(axis, np.float64) / np.linalg.norm(axis) * angle).as_matrix()


def write_ply(path, pts, faces):
    with open(path, "w") as f:
        f.write("ply\nformat ascii 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\n"
                "element face %d\nproperty list uchar int vertex_indices\nend_header\n" % (len(pts), len(faces)))
        for p in pts:
            f.write(" ".join(repr(float(v)) for v in p) + "\n")
        for t in faces:
            f.write("3 %d %d %d\n" % tuple(int(i) for i in t))


class OracleRenderer:
    """Stand-in for lib.pysixd.renderer's GL renderers: ``render_object`` served by oracle/raster_oracle.c."""

    def __init__(self, width, height, models=None):
        self.width, self.height, self.models = width, height, dict(models or {})

    def add_object(self, obj_id, model_path, **kwargs):
        from lib.pysixd import inout
        m = inout.load_ply(model_path)
        self.models[obj_id] = (np.asarray(m["pts"], np.float32), np.asarray(m["faces"], np.int32))

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        v, f = self.models[obj_id]
        Kr = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        return {"depth": V.render_oracle(v, f, Kr, R, np.asarray(t, np.float64).reshape(3), self.width, self.height, Z_NEAR, Z_FAR)}


def imread(path):
    """imageio.imread for the 16-bit PNGs written here."""
    with Image.open(path) as im:
        return np.asarray(im)


def build_dataset(rng):
    verts_m, faces, _ = S.make_models(len(OBJ_IDS), rng, 2)         # 162 points, 320 faces each
    vertices = {o: (verts_m[k] * np.float32(350.0)).astype(np.float32) for k, o in enumerate(OBJ_IDS)}     # ~100 mm across
    faces = {o: np.asarray(faces[k], np.int32) for k, o in enumerate(OBJ_IDS)}
    models_info = {o: {"diameter": float(np.linalg.norm(vertices[o].max(0) - vertices[o].min(0)))} for o in OBJ_IDS}
    sym6 = np.eye(4)
    sym6[:3, :3], sym6[:3, 3] = rotvec([0, 0, 1], np.pi), [0.5, -0.25, 0.0]
    models_info[6]["symmetries_discrete"] = [sym6.reshape(-1).tolist()]
    models_info[10]["symmetries_continuous"] = [{"axis": [0, 0, 1], "offset": [0.0, 0.0, 0.0]}]
    ren = OracleRenderer(*IM_SIZE, {o: (vertices[o], faces[o]) for o in OBJ_IDS})
    scene_gt, scene_gt_info, scene_camera, targets, depth = {}, {}, {}, [], {}
    for im, (objs, tars, visib, scale) in LAYOUT.items():
        gts = []
        for k, o in enumerate(objs):                                # one column of the image per ground truth, so that most are apart
            u = (k + 0.5) / len(objs) * IM_SIZE[0] + rng.uniform(-25, 25)
            v = rng.uniform(120, 360)
            z = rng.uniform(800, 1200)
            t = np.array([(u - K[0, 2]) / K[0, 0] * z, (v - K[1, 2]) / K[1, 1] * z, z])
            gts.append({"obj_id": o, "cam_R_m2c": f32(S.random_rotation(rng)), "cam_t_m2c": t})
        if im == 0:                                                 # two instances of the symmetric object 25 mm apart
            gts[2]["cam_t_m2c"] = gts[1]["cam_t_m2c"] + np.array([25.0, 0.0, 0.0])
            gts[2]["cam_R_m2c"] = f32(gts[1]["cam_R_m2c"].dot(rotvec([0, 0, 1], 0.05)))
        d = np.full(IM_SIZE[::-1], WALL, np.float32)
        for g in gts:
            r = ren.render_object(g["obj_id"], g["cam_R_m2c"], g["cam_t_m2c"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])["depth"]
            d = np.where((r > 0) & (r < d), r, d)

        def centre(g):
            t = g["cam_t_m2c"]
            return int(K[0, 0] * t[0] / t[2] + K[0, 2]), int(K[1, 1] * t[1] / t[2] + K[1, 2])

        d[rng.integers(0, IM_SIZE[1], 40), rng.integers(0, IM_SIZE[0], 40)] = 0.0
        cu, cv = centre(gts[1])
        d[cv - 4:cv + 3, cu - 30:cu + 10] = 0.0                     # a hole across an object
        if im == 0:                                                 # a slab over the right half of the first object
            cu, cv = centre(gts[0])
            d[cv - 60:cv + 60, cu:cu + 60] = 500.0
        if im == 3:                                                 # a slab over the whole of the last object (and the holes there)
            cu, cv = centre(gts[3])
            d[max(cv - 80, 0):cv + 80, cu - 80:cu + 80] = 450.0
        stored = np.round(d / scale)
        assert stored.max() < 65536
        depth[im] = stored.astype(np.uint16)
        scene_gt[im] = gts
        scene_gt_info[im] = [{"visib_fract": x} for x in visib]
        scene_camera[im] = {"cam_K": K, "depth_scale": scale}
        targets += [{"scene_id": SCENE, "im_id": im, "obj_id": o, "inst_count": c} for o, c in tars.items()]
    return vertices, faces, models_info, scene_gt, scene_gt_info, scene_camera, targets, depth


def build_estimates(rng, scene_gt, models_info):
    from lib.pysixd import misc as M

    ests = []

    def near(im, gt_id, step, score, shift=None, exact=False):
        g = scene_gt[im][gt_id]
        if exact:
            R, t = g["cam_R_m2c"], g["cam_t_m2c"]
        else:
            syms = M.get_symmetry_transformations(models_info[g["obj_id"]], 0.01)
            sym = syms[rng.integers(len(syms))]
            rp, tp = LADDER[step]
            R = g["cam_R_m2c"].dot(sym["R"]).dot(rotvec(rng.standard_normal(3), rp * rng.uniform(0.7, 1.0)))
            d = rng.standard_normal(3)
            t = g["cam_R_m2c"].dot(sym["t"]).reshape(3) + g["cam_t_m2c"] + d / np.linalg.norm(d) * tp * rng.uniform(0.7, 1.0)
        if shift is not None:
            t = t + np.asarray(shift)
        ests.append({"scene_id": SCENE, "im_id": im, "obj_id": g["obj_id"], "score": score, "R": f32(R), "t": f32(t)})

    dia = lambda im, k: models_info[scene_gt[im][k]["obj_id"]]["diameter"]
    # image 0: object 1 (half under the slab) twice; object 6 five times for inst_count 3; object 5 (no target) once
    near(0, 0, 3, 0.6); near(0, 0, 0, 0.9)
    near(0, 1, 1, 0.8, shift=[14.0, 0.0, 0.0]); near(0, 1, 1, 0.7, shift=[9.0, 0.0, 0.0]); near(0, 3, 2, 0.7)
    near(0, 3, 0, 0.95, exact=True)                                 # equal to its ground truth
    near(0, 3, 0, 0.5, shift=[0.0, 0.0, WALL - 600.0])              # behind the wall
    near(0, 4, 1, 0.9)
    # image 1 (depth_scale 0.5): three estimates for two instances; one far to the side (its sphere projection overlaps no ground truth)
    near(1, 0, 2, 0.5); near(1, 1, 1, 0.9); near(1, 1, 4, 0.7); near(1, 2, 1, 0.8)
    near(1, 2, 0, 0.3, shift=[-500.0, 300.0, 0.0])
    # image 3: tied scores; an estimate beside its ground truth (spheres' projections overlap, silhouettes do not); one under the full slab
    near(3, 0, 0, 0.6); near(3, 0, 3, 0.6); near(3, 1, 2, 0.9); near(3, 2, 0, 0.9)
    near(3, 1, 0, 0.4, shift=[0.0, 0.97 * dia(3, 1), 0.0])
    near(3, 3, 1, 0.8)
    # image 7
    near(7, 0, 4, 0.9); near(7, 1, 0, 0.3); near(7, 2, 3, 0.8); near(7, 2, 1, 0.85)
    im_order = list(LAYOUT)
    for e in ests:
        e["time"] = 0.05 + 0.01 * im_order.index(e["im_id"])
    return ests


def all_pairs(ests, scene_gt):
    """Every (estimate, ground truth of the same object in the image)."""
    return [(k, e["im_id"], gt_id) for k, e in enumerate(ests) for gt_id, g in enumerate(scene_gt[e["im_id"]]) if g["obj_id"] == e["obj_id"]]


def restated(pairs, ests, scene_gt, vertices, faces, models_info, depth_mm):
    """tests/vsd_ref.py on every pair: counts and the margins of the comparisons."""
    counts, m_delta, m_tau = [], np.inf, np.inf
    for k, im, gt_id in pairs:
        e, g = ests[k], scene_gt[im][gt_id]
        o = e["obj_id"]
        c, md, mt = V.vsd_counts_ref(vertices[o], faces[o], e["R"], e["t"], g["cam_R_m2c"], g["cam_t_m2c"], K, depth_mm[im], DELTA, TAUS,
                                     models_info[o]["diameter"], Z_NEAR, Z_FAR, render="oracle", details=True)
        counts.append(c)
        m_delta, m_tau = min(m_delta, md), min(m_tau, mt)
    return np.array(counts, np.int64), m_delta, m_tau


def conditions(counts, m_delta, m_tau):
    errs = V.errors_from_counts(counts)
    th_gap = min(abs(x - th) for x in errs.reshape(-1) for th in TAUS)
    return (m_delta >= 1e-3 and m_tau >= 1e-6 and th_gap >= 1e-9 and len(set(counts[:, 0].tolist())) >= 3
            and ((counts[:, 1] == 0) & (counts[:, 0] > 0)).any() and (counts[:, 0] == 0).any()), (m_delta, m_tau, th_gap)


def write_tree(vertices, faces, models_info, scene_gt, scene_gt_info, scene_camera, targets, depth, ests):
    base = os.path.join(TMP, "datasets", DATASET)
    models = os.path.join(base, "models_eval")
    os.makedirs(models)
    json.dump({str(o): v for o, v in models_info.items()}, open(os.path.join(models, "models_info.json"), "w"))
    for o, v in vertices.items():
        write_ply(os.path.join(models, f"obj_{o:06d}.ply"), v, faces[o])
    json.dump(targets, open(os.path.join(base, TARGETS), "w"))
    d = os.path.join(base, SPLIT, f"{SCENE:06d}")
    os.makedirs(os.path.join(d, "depth"))
    json.dump({str(im): [{"obj_id": g["obj_id"], "cam_R_m2c": g["cam_R_m2c"].reshape(-1).tolist(), "cam_t_m2c": g["cam_t_m2c"].tolist()}
                         for g in gts] for im, gts in scene_gt.items()}, open(os.path.join(d, "scene_gt.json"), "w"))
    json.dump({str(im): v for im, v in scene_gt_info.items()}, open(os.path.join(d, "scene_gt_info.json"), "w"))
    json.dump({str(im): {"cam_K": c["cam_K"].reshape(-1).tolist(), "depth_scale": c["depth_scale"]} for im, c in scene_camera.items()},
              open(os.path.join(d, "scene_camera.json"), "w"))
    for im, img in depth.items():
        Image.fromarray(img).save(os.path.join(d, "depth", f"{im:06d}.png"))
        assert np.array_equal(imread(os.path.join(d, "depth", f"{im:06d}.png")), img)
    results = os.path.join(TMP, "results")
    os.makedirs(results)
    with open(os.path.join(results, RESULT_NAME + ".csv"), "w") as f:
        f.write("scene_id,im_id,obj_id,score,R,t,time\n")
        for e in ests:
            f.write("{},{},{},{},{},{},{}\n".format(e["scene_id"], e["im_id"], e["obj_id"], e["score"],
                                                    " ".join("{}".format(float(v)) for v in e["R"].reshape(-1)),
                                                    " ".join("{}".format(float(v)) for v in e["t"]), e["time"]))
    return results


def run_script_in_process(cmd):
    """Stand-in for ``subprocess.call(["python", script, *args])``: the same script file, the same arguments, this process."""
    assert cmd[0] == "python" and os.path.isfile(cmd[1]), cmd
    saved = sys.argv
    sys.argv = list(cmd[1:])
    try:
        runpy.run_path(cmd[1], run_name="__main__")
    finally:
        sys.argv = saved
    return 0


def main():
    seed = 20220925 + 71
    while True:
        rng = np.random.default_rng(seed)
        vertices, faces, models_info, scene_gt, scene_gt_info, scene_camera, targets, depth = build_dataset(rng)
        ests = build_estimates(rng, scene_gt, models_info)
        depth_mm = {im: depth[im].astype(np.float32) * np.float32(scene_camera[im]["depth_scale"]) for im in depth}
        pairs = all_pairs(ests, scene_gt)
        counts, m_delta, m_tau = restated(pairs, ests, scene_gt, vertices, faces, models_info, depth_mm)
        ok, margins = conditions(counts, m_delta, m_tau)
        print("seed", seed, "margins (delta mm, tau rel, threshold):", margins, "unions", sorted(set(counts[:, 0].tolist()))[:4], "inter == 0:",
              int(((counts[:, 1] == 0) & (counts[:, 0] > 0)).sum()), "ok" if ok else "again", flush=True)
        if ok:
            break
        seed += 1

    # ---- (a) the reference's pose_error.vsd on every pair ------------------------------------------------------------------------
    from lib.pysixd import misc as M
    from lib.pysixd import pose_error as PE

    ren = OracleRenderer(*IM_SIZE, {o: (vertices[o], faces[o]) for o in OBJ_IDS})
    func_errors, overlaps = [], []
    for k, im, gt_id in pairs:
        e, g = ests[k], scene_gt[im][gt_id]
        o = e["obj_id"]
        func_errors.append(PE.vsd(e["R"], e["t"].reshape(3, 1), g["cam_R_m2c"], g["cam_t_m2c"].reshape(3, 1), depth_mm[im].copy(), K, DELTA, TAUS,
                                  True, models_info[o]["diameter"], ren, o, "step"))
        overlaps.append(bool(M.overlapping_sphere_projections(0.5 * models_info[o]["diameter"], e["t"].squeeze(), g["cam_t_m2c"].squeeze())))
    func_errors = np.array(func_errors, np.float64)
    assert np.array_equal(func_errors, V.errors_from_counts(counts)), "tests/vsd_ref.py does not restate pose_error.vsd"
    assert not all(overlaps) and any(overlaps)

    # ---- (b) the evaluation scripts ----------------------------------------------------------------------------------------------
    results_path = write_tree(vertices, faces, models_info, scene_gt, scene_gt_info, scene_camera, targets, depth, ests)
    script = os.path.join(_refimport.REF, "lib", "pysixd", "scripts", "eval_pose_results_more.py")
    import imageio
    import lib.pysixd.renderer as ref_renderer

    saved = subprocess.call, ref_renderer.create_renderer, getattr(imageio, "imread", None)
    subprocess.call = run_script_in_process
    ref_renderer.create_renderer = lambda width, height, renderer_type="cpp", mode="rgb+depth", **k: OracleRenderer(width, height)
    imageio.imread = imread
    recorded = {}
    try:
        for n_top in N_TOPS:
            eval_path = os.path.join(TMP, f"eval_ntop{n_top}")
            run_script_in_process(["python", script, f"--result_filenames={RESULT_NAME}.csv", f"--results_path={results_path}",
                                   f"--eval_path={eval_path}", f"--targets_filename={TARGETS}", "--error_types=" + ",".join(ERROR_TYPES),
                                   f"--n_top={n_top}"])
            rec = {"final": json.load(open(os.path.join(eval_path, RESULT_NAME, "scores_bop19.json"))), "types": {}}
            for t in ERROR_TYPES:
                dirs = sorted(glob.glob(os.path.join(eval_path, RESULT_NAME, f"error:{t}_ntop:{n_top}*")),
                              key=lambda q: float(q.split("tau:")[1]) if "tau:" in q else 0.0)      # vsd: one directory per tau
                assert len(dirs) == (len(TAUS) if t == "vsd" else 1), (t, dirs)
                per_dir = []
                for d in dirs:
                    errors = {int(os.path.basename(p)[7:13]): json.load(open(p)) for p in sorted(glob.glob(os.path.join(d, "errors_*.json")))}
                    per_th = []
                    for p in sorted(glob.glob(os.path.join(d, "scores_th:*.json")),
                                  key=lambda q: float(os.path.basename(q)[len("scores_th:"):].split("_")[0].split("-")[0])):
                        sign = os.path.basename(p)[len("scores_"):-len(".json")]
                        ms = json.load(open(os.path.join(d, f"matches_{sign}.json")))
                        per_th.append({"sign": sign, "scores": json.load(open(p)),
                                       "matches": [[m["scene_id"], m["im_id"], m["obj_id"], m["gt_id"], m["est_id"], bool(m["valid"])] for m in ms]})
                    per_dir.append({"dir": os.path.basename(d), "errors": errors, "thresholds": per_th})
                rec["types"][t] = per_dir if t == "vsd" else per_dir[0]
            recorded[str(n_top)] = rec
    finally:
        subprocess.call, ref_renderer.create_renderer = saved[:2]
        if saved[2] is not None:
            imageio.imread = saved[2]

    # ---- conditions on what the scripts wrote --------------------------------------------------------------------------------------
    for n_top, rec in recorded.items():
        assert "bop19_average_recall" in rec["final"]
        vs = rec["types"]["vsd"]
        assert len(vs) == len(TAUS) and all(len(x["thresholds"]) == len(TAUS) for x in vs)
        recalls = [th["scores"]["recall"] for x in vs for th in x["thresholds"]]
        assert rec["final"]["bop19_average_recall_vsd"] == float(np.mean(recalls))
        for k, x in enumerate(vs):                                  # the per-tau files hold column k of the function-level errors
            for errs in x["errors"].values():
                for e in errs:
                    for vals in e["errors"].values():
                        assert len(vals) == 1 and all(abs(vals[0] - th) >= 1e-9 for th in TAUS)
        assert len(set(recalls)) > 3, recalls
        print(n_top, "vsd recalls per tau:", [["%.2f" % th["scores"]["recall"] for th in x["thresholds"]] for x in vs][:3], rec["final"])

    est_of = np.array([p[0] for p in pairs], np.int32)
    im_ids = list(LAYOUT)
    path = os.path.join(HERE, "vsd_golden.npz")
    np.savez_compressed(
        path, dataset=json.dumps(dict(name=DATASET, split=SPLIT, im_width=IM_SIZE[0], im_size=IM_SIZE, obj_ids=OBJ_IDS, scene_ids=SCENE_IDS,
                                      symmetric_obj_ids=SYMMETRIC, result_name=RESULT_NAME, error_types=ERROR_TYPES, scene_id=SCENE,
                                      im_ids=im_ids, seed=seed)),
        taus=np.array(TAUS), delta=np.float64(DELTA), z_near=np.float64(Z_NEAR), z_far=np.float64(Z_FAR),
        models_info=json.dumps(models_info), targets=json.dumps(targets),
        scene_gt=json.dumps({SCENE: {im: [{"obj_id": g["obj_id"], "cam_R_m2c": g["cam_R_m2c"].reshape(-1).tolist(),
                                           "cam_t_m2c": g["cam_t_m2c"].tolist()} for g in gts] for im, gts in scene_gt.items()}}),
        scene_gt_info=json.dumps({SCENE: scene_gt_info}),
        scene_camera=json.dumps({SCENE: {im: {"cam_K": c["cam_K"].reshape(-1).tolist(), "depth_scale": c["depth_scale"]} for im, c in scene_camera.items()}}),
        verts=np.concatenate([vertices[o] for o in OBJ_IDS]), vert_off=np.cumsum([0] + [len(vertices[o]) for o in OBJ_IDS]).astype(np.int32),
        faces=np.concatenate([faces[o] for o in OBJ_IDS]), face_off=np.cumsum([0] + [len(faces[o]) for o in OBJ_IDS]).astype(np.int32),
        depth=np.stack([depth[im] for im in im_ids]),
        est_ids=np.array([[e["scene_id"], e["im_id"], e["obj_id"]] for e in ests], np.int32), est_score=np.array([e["score"] for e in ests]),
        est_R=np.stack([e["R"].reshape(9) for e in ests]), est_t=np.stack([e["t"] for e in ests]), est_time=np.array([e["time"] for e in ests]),
        pair_est=est_of, pair_im=np.array([p[1] for p in pairs], np.int32), pair_gt=np.array([p[2] for p in pairs], np.int32),
        pair_counts=counts, pair_errors=func_errors, pair_overlap=np.array(overlaps), recorded=json.dumps(recorded))
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("wrote vsd_golden.npz:", len(ests), "estimates,", len(pairs), "pairs,", size, "bytes; final:", recorded["-1"]["final"])


if __name__ == "__main__":
    main()
