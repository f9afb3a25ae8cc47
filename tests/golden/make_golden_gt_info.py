"""Golden ground-truth info and masks from the reference's own scripts (authoring container only: needs /root/reference).

A synthetic BOP dataset laid out as ``lm`` / ``test`` (the pair both scripts hard-code; scene 3, 640x480, 3 images with 16-bit PNG depth,
one of them stored at depth_scale 0.5) is written to a temporary directory, then ``lib/pysixd/scripts/calc_gt_masks.py`` and
``lib/pysixd/scripts/calc_gt_info.py`` are run UNMODIFIED, in-process, with ``runpy``.  For the duration of the runs

* ``lib.pysixd.renderer.create_renderer`` (GL) is replaced by the oracle-backed stand-in of make_golden_vsd.py (it ignores the model
  files of ``lm`` objects this dataset does not hold, and keeps the last render it served so that its silhouette can be recorded);
* ``imageio.imread`` / ``imageio.imwrite`` (absent) are replaced by PIL stand-ins;
* for calc_gt_info.py only, ``misc.calc_2d_bbox`` — which the script calls and the reference's fork of the toolkit no longer defines — is
  installed with the BOP toolkit's rule: ``[x_min, y_min, x_max - x_min, y_max - y_min]``, no ``+ 1``, no clipping.

Recorded: the ``scene_gt_info.json`` the script wrote, both mask sets as ``np.packbits``, and separately the raw extents from
``nonzero()`` of what the reference produced: of the 3W x 3H renders calc_gt_info.py was served and of the mask images.

Conditions asserted here (about the reference alone; the seed is advanced until they hold): fx, fy, cx, cy, cx + W, cy + H are float32
values (the oracle takes float32 K, so the device's fp64 sum cx + W equals it); over all poses no pixel has |d_diff - delta| < 1e-3 mm;
tests/gt_info_ref.py reproduces every recorded integer and mask exactly in both canvas modes, and its masks of the two canvases agree on
the window for every pose (so one recorded mask set serves both modes); at least one pose occurs of each kind: cut by the left edge, cut by
the bottom-right corner, wholly outside the image but inside the canvas, outside the canvas, behind the camera, wholly under an occluder,
partly occluded, over a depth hole (valid < visib), two overlapping instances."""
import json
import os
import runpy
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "..", ".."))

TMP = tempfile.mkdtemp(prefix="gt_info_golden_")
os.environ["BOP_PATH"] = os.path.join(TMP, "datasets")             # lib/pysixd/config.py reads it at import

import _refimport  # noqa: E402

_refimport.install()

import chardet  # noqa: E402
import termcolor  # noqa: E402

chardet.detect = lambda data: {"encoding": "ascii", "confidence": 1.0, "language": ""}      # the ply files below are 7-bit
termcolor.colored = lambda text, *a, **k: text

from PIL import Image  # noqa: E402

from gdrnpp_bop2022_amd import synthetic as S  # noqa: E402
from tests import gt_info_ref as G  # noqa: E402
from tests import vsd_ref as V  # noqa: E402

DATASET, SPLIT, IM_SIZE, SCENE = "lm", "test", (640, 480), 3
OBJ_IDS = [1, 2, 5, 6, 9, 12]                                       # a subset of dataset_params.py's lm objects
DELTA = 15.0                                                        # both scripts' p["delta"]
Z_NEAR, Z_FAR = 1.0, 1e6
WALL = 1500.0
W, H = IM_SIZE


def f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


K = np.array([[572.4114, 0.0, np.round(325.2611 * 8192) / 8192], [0.0, 573.57043, np.round(242.04899 * 8192) / 8192], [0.0, 0.0, 1.0]])
K[0, 0], K[1, 1] = f32(K[0, 0]), f32(K[1, 1])
for value in (K[0, 0], K[1, 1], K[0, 2], K[1, 2], K[0, 2] + W, K[1, 2] + H):
    assert f32(value) == value, value

# image -> (depth_scale, [(kind, object, centre u, centre v, z)]); a centre of None places the pose by hand in build_dataset
LAYOUT = {
    0: (1.0, [("hole", 1, 320, 240, 900), ("left", 2, 6, 200, 1000), ("corner", 5, 633, 474, 950), ("beside", 6, -220, 240, 1000),
              ("off_canvas", 9, -2400, 240, 1000)]),
    4: (0.5, [("front", 6, 200, 200, 1000), ("overlap", 6, None, None, None), ("behind_camera", 12, None, None, None),
              ("under_slab", 1, 480, 300, 1100)]),
    9: (1.0, [("half_slab", 2, 300, 250, 950), ("free", 9, 500, 150, 1000), ("free", 5, 100, 380, 1050)]),
}


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

    last = None                                                     # the last depth image served, for the raw extents

    def __init__(self, width, height, models=None):
        self.width, self.height, self.models = width, height, dict(models or {})

    def add_object(self, obj_id, model_path, **kwargs):
        from lib.pysixd import inout
        if not os.path.exists(model_path):                          # an lm object this dataset does not hold
            return
        m = inout.load_ply(model_path)
        self.models[obj_id] = (np.asarray(m["pts"], np.float32), np.asarray(m["faces"], np.int32))

    def render_object(self, obj_id, R, t, fx, fy, cx, cy):
        v, f = self.models[obj_id]
        Kr = np.array([[fx, 0.0, cx], [0.0, fy, cy], [0.0, 0.0, 1.0]])
        d = V.render_oracle(v, f, Kr, np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3), self.width, self.height,
                            Z_NEAR, Z_FAR)
        OracleRenderer.last = d
        return {"depth": d}


def imread(path):
    with Image.open(path) as im:
        return np.asarray(im)


def imwrite(path, im, **kwargs):
    Image.fromarray(np.asarray(im)).save(path)


def build_dataset(rng):
    verts_m, faces, _ = S.make_models(len(OBJ_IDS), rng, 2)         # 162 points, 320 faces each
    vertices = {o: (verts_m[k] * np.float32(350.0)).astype(np.float32) for k, o in enumerate(OBJ_IDS)}
    faces = {o: np.asarray(faces[k], np.int32) for k, o in enumerate(OBJ_IDS)}
    ren = OracleRenderer(W, H, {o: (vertices[o], faces[o]) for o in OBJ_IDS})
    scene_gt, scene_camera, depth, kinds = {}, {}, {}, {}

    def centre(g):
        t = g["cam_t_m2c"]
        return int(K[0, 0] * t[0] / t[2] + K[0, 2]), int(K[1, 1] * t[1] / t[2] + K[1, 2])

    for im, (scale, poses) in LAYOUT.items():
        gts = []
        for kind, o, u, v, z in poses:
            R = f32(S.random_rotation(rng))
            if kind == "overlap":                                   # the same object 25 mm beside and 30 mm behind the previous one
                t = gts[-1]["cam_t_m2c"] + np.array([25.0, 0.0, 30.0])
            elif kind == "behind_camera":
                t = np.array([10.0, -20.0, -800.0])
            else:
                z = z + rng.uniform(-30, 30)
                t = np.array([(u + rng.uniform(-2, 2) - K[0, 2]) / K[0, 0] * z, (v + rng.uniform(-2, 2) - K[1, 2]) / K[1, 1] * z, z])
            gts.append({"obj_id": o, "cam_R_m2c": R, "cam_t_m2c": t})
        d = np.full((H, W), WALL, np.float32)
        for g in gts:
            r = ren.render_object(g["obj_id"], g["cam_R_m2c"], g["cam_t_m2c"], K[0, 0], K[1, 1], K[0, 2], K[1, 2])["depth"]
            d = np.where((r > 0) & (r < d), r, d)
        d[rng.integers(0, H, 40), rng.integers(0, W, 40)] = 0.0
        for (kind, *_), g in zip(poses, gts):
            cu, cv = centre(g) if g["cam_t_m2c"][2] > 0 else (0, 0)
            if kind == "hole":                                      # a hole across the object
                d[cv - 4:cv + 3, cu - 30:cu + 10] = 0.0
            if kind == "half_slab":                                 # a slab over the right half of the object
                d[cv - 70:cv + 70, cu:cu + 70] = 500.0
            if kind == "under_slab":                                # a slab over the whole object (and the holes there)
                d[max(cv - 90, 0):cv + 90, cu - 90:cu + 90] = 450.0
        stored = np.round(d / scale)
        assert stored.max() < 65536
        depth[im] = stored.astype(np.uint16)
        scene_gt[im], kinds[im] = gts, [p[0] for p in poses]
        scene_camera[im] = {"cam_K": K, "depth_scale": scale}
    models_info = {o: {"diameter": float(np.linalg.norm(vertices[o].max(0) - vertices[o].min(0)))} for o in OBJ_IDS}
    return vertices, faces, models_info, scene_gt, scene_camera, depth, kinds


def write_tree(vertices, faces, models_info, scene_gt, scene_camera, depth):
    base = os.path.join(TMP, "datasets", DATASET)
    models = os.path.join(base, "models")
    os.makedirs(models)
    json.dump({str(o): v for o, v in models_info.items()}, open(os.path.join(models, "models_info.json"), "w"))
    for o, v in vertices.items():
        write_ply(os.path.join(models, f"obj_{o:06d}.ply"), v, faces[o])
    d = os.path.join(base, SPLIT, f"{SCENE:06d}")
    os.makedirs(os.path.join(d, "depth"))
    json.dump({str(im): [{"obj_id": g["obj_id"], "cam_R_m2c": g["cam_R_m2c"].reshape(-1).tolist(), "cam_t_m2c": g["cam_t_m2c"].tolist()}
                         for g in gts] for im, gts in scene_gt.items()}, open(os.path.join(d, "scene_gt.json"), "w"))
    json.dump({str(im): {"cam_K": c["cam_K"].reshape(-1).tolist(), "depth_scale": c["depth_scale"]} for im, c in scene_camera.items()},
              open(os.path.join(d, "scene_camera.json"), "w"))
    for im, img in depth.items():
        Image.fromarray(img).save(os.path.join(d, "depth", f"{im:06d}.png"))
        assert np.array_equal(imread(os.path.join(d, "depth", f"{im:06d}.png")), img)
    return d


def restated(scene_gt, scene_camera, vertices, faces, depth_mm):
    """tests/gt_info_ref.py on every pose, both canvases -> (keys, info (W, H), info (0, 0), masks, visibs, margin, canvases agree)."""
    keys, canvas, plain, masks, visibs, margin, agree = [], [], [], [], [], np.inf, True
    for im in sorted(scene_gt):
        for k, g in enumerate(scene_gt[im]):
            o = g["obj_id"]
            a = (vertices[o], faces[o], g["cam_R_m2c"], g["cam_t_m2c"], scene_camera[im]["cam_K"], depth_mm[im], DELTA)
            ic, mc, vc, m1 = G.gt_visibility_ref(*a, (W, H), Z_NEAR, Z_FAR, render="oracle", details=True)
            ip, mp, vp, m2 = G.gt_visibility_ref(*a, (0, 0), Z_NEAR, Z_FAR, render="oracle", details=True)
            agree = agree and np.array_equal(mc, mp) and np.array_equal(vc, vp)
            keys.append((im, k)); canvas.append(ic); plain.append(ip); masks.append(mp); visibs.append(vp)
            margin = min(margin, m1, m2)
    return keys, np.array(canvas), np.array(plain), np.array(masks), np.array(visibs), margin, agree


def kinds_ok(keys, kinds, canvas, masks, visibs):
    row = {(im, k): r for (im, k), r in zip(keys, canvas)}
    at = {(im, k): n for n, (im, k) in enumerate(keys)}
    first = lambda kind: next((im, k) for im in kinds for k, x in enumerate(kinds[im]) if x == kind)  # noqa: E731
    r = row[first("left")]
    ok = r[2] > 0 and r[3] < 0 and r[7] == 0
    r = row[first("corner")]
    ok = ok and r[2] > 0 and r[5] > W - 1 and r[6] > H - 1 and r[9] == W - 1 and r[10] == H - 1
    r = row[first("beside")]
    ok = ok and r[0] > 0 and r[2] == 0 and r[5] < 0
    ok = ok and row[first("off_canvas")][0] == 0 and row[first("behind_camera")][0] == 0
    r = row[first("under_slab")]
    ok = ok and r[0] > 0 and r[2] == 0 and masks[at[first("under_slab")]].sum() == r[0]
    r, n = row[first("half_slab")], at[first("half_slab")]
    ok = ok and masks[n].sum() == r[0] and 0.2 * r[0] < r[2] < 0.8 * r[0]
    r = row[first("hole")]
    ok = ok and r[1] < r[2]
    ok = ok and (masks[at[first("front")]] & masks[at[first("overlap")]]).sum() > 100
    return bool(ok)


def run_script(name):
    script = os.path.join(_refimport.REF, "lib", "pysixd", "scripts", name)
    saved = sys.argv
    sys.argv = [script]
    try:
        runpy.run_path(script, run_name="__main__")
    finally:
        sys.argv = saved


def main():
    seed = 20220925 + 113
    while True:
        rng = np.random.default_rng(seed)
        vertices, faces, models_info, scene_gt, scene_camera, depth, kinds = build_dataset(rng)
        depth_mm = {im: depth[im].astype(np.float32) * np.float32(scene_camera[im]["depth_scale"]) for im in depth}
        keys, canvas, plain, masks, visibs, margin, agree = restated(scene_gt, scene_camera, vertices, faces, depth_mm)
        ok = margin >= 1e-3 and agree and kinds_ok(keys, kinds, canvas, masks, visibs)
        print("seed", seed, "margin (mm):", margin, "canvases agree:", agree, "ok" if ok else "again", flush=True)
        if ok:
            break
        seed += 1

    scene_dir = write_tree(vertices, faces, models_info, scene_gt, scene_camera, depth)
    import imageio
    import lib.pysixd.misc as ref_misc
    import lib.pysixd.renderer as ref_renderer

    assert not hasattr(ref_misc, "calc_2d_bbox"), "the reference defines calc_2d_bbox again: record its own"
    saved = ref_renderer.create_renderer, getattr(imageio, "imread", None), getattr(imageio, "imwrite", None)
    ref_renderer.create_renderer = lambda width, height, renderer_type="cpp", mode="rgb+depth", **k: OracleRenderer(width, height)
    imageio.imread, imageio.imwrite = imread, imwrite
    larges = []
    try:
        run_script("calc_gt_masks.py")
        # calc_gt_info.py takes the render's silhouette before it asks for the next one: keep every render it is served
        served = OracleRenderer.render_object

        def keeping(self, *a):
            out = served(self, *a)
            larges.append(out["depth"] > 0)
            return out

        OracleRenderer.render_object = keeping
        ref_misc.calc_2d_bbox = lambda xs, ys, im_size=None, clip=False: [xs.min(), ys.min(), xs.max() - xs.min(), ys.max() - ys.min()]
        try:
            run_script("calc_gt_info.py")
        finally:
            del ref_misc.calc_2d_bbox
            OracleRenderer.render_object = served
    finally:
        ref_renderer.create_renderer = saved[0]
        for name, fn in (("imread", saved[1]), ("imwrite", saved[2])):
            if fn is not None:
                setattr(imageio, name, fn)

    # ---- what the scripts wrote ------------------------------------------------------------------------------------------------------
    written = json.load(open(os.path.join(scene_dir, "scene_gt_info.json")))
    rec_mask = np.array([imread(os.path.join(scene_dir, "mask", f"{im:06d}_{k:06d}.png")) for im, k in keys])
    rec_visib = np.array([imread(os.path.join(scene_dir, "mask_visib", f"{im:06d}_{k:06d}.png")) for im, k in keys])
    assert rec_mask.dtype == np.uint8 and set(np.unique(rec_mask)) <= {0, 255} and set(np.unique(rec_visib)) <= {0, 255}
    assert len(larges) == len(keys) and all(m.shape == (3 * H, 3 * W) for m in larges)
    recs = [written[str(im)][k] for im, k in keys]
    raw_canvas = np.array([[r["px_count_all"], r["px_count_valid"], r["px_count_visib"]] + G.extents(larges[n], W, H) + G.extents(rec_visib[n] > 0)
                           for n, r in enumerate(recs)], np.int64)
    raw_plain = np.array([[int((rec_mask[n] > 0).sum()), int((depth_mm[im][rec_mask[n] > 0] > 0).sum()), int((rec_visib[n] > 0).sum())]
                          + G.extents(rec_mask[n] > 0) + G.extents(rec_visib[n] > 0) for n, (im, _) in enumerate(keys)], np.int64)
    # tests/gt_info_ref.py restates the reference: every integer, every mask, and the formatted records
    assert np.array_equal(raw_canvas, canvas), (raw_canvas.tolist(), canvas.tolist())
    assert np.array_equal(raw_plain, plain)
    assert np.array_equal(rec_mask > 0, masks) and np.array_equal(rec_visib > 0, visibs)
    assert G.records_ref(canvas) == recs
    for r in recs:
        assert [type(r[k]) for k in ("px_count_all", "px_count_valid", "px_count_visib", "visib_fract")] == [int, int, int, float]
    targets = [{"scene_id": SCENE, "im_id": im, "obj_id": o, "inst_count": sum(1 for g in gts if g["obj_id"] == o)}
               for im, gts in scene_gt.items() for o in sorted({g["obj_id"] for g in gts})]

    path = os.path.join(HERE, "gt_info_golden.npz")
    np.savez_compressed(
        path, dataset=json.dumps(dict(name=DATASET, split=SPLIT, im_size=IM_SIZE, obj_ids=OBJ_IDS, scene_id=SCENE, im_ids=sorted(scene_gt), seed=seed,
                                      kinds={str(im): v for im, v in kinds.items()})),
        delta=np.float64(DELTA), z_near=np.float64(Z_NEAR), z_far=np.float64(Z_FAR), models_info=json.dumps(models_info), targets=json.dumps(targets),
        scene_gt=json.dumps({im: [{"obj_id": g["obj_id"], "cam_R_m2c": g["cam_R_m2c"].reshape(-1).tolist(), "cam_t_m2c": g["cam_t_m2c"].tolist()}
                                  for g in gts] for im, gts in scene_gt.items()}),
        scene_camera=json.dumps({im: {"cam_K": c["cam_K"].reshape(-1).tolist(), "depth_scale": c["depth_scale"]} for im, c in scene_camera.items()}),
        scene_gt_info=json.dumps(written),
        verts=np.concatenate([vertices[o] for o in OBJ_IDS]), vert_off=np.cumsum([0] + [len(vertices[o]) for o in OBJ_IDS]).astype(np.int32),
        faces=np.concatenate([faces[o] for o in OBJ_IDS]), face_off=np.cumsum([0] + [len(faces[o]) for o in OBJ_IDS]).astype(np.int32),
        depth=np.stack([depth[im] for im in sorted(depth)]), pose_im=np.array([k[0] for k in keys], np.int32), pose_gt=np.array([k[1] for k in keys], np.int32),
        raw_canvas=raw_canvas, raw_plain=raw_plain, mask=np.packbits(rec_mask > 0, axis=None), mask_visib=np.packbits(rec_visib > 0, axis=None))
    size = os.path.getsize(path)
    assert size < (1 << 20), size
    print("wrote gt_info_golden.npz:", len(keys), "poses,", size, "bytes; visib_fract:", [round(r["visib_fract"], 3) for r in recs])


if __name__ == "__main__":
    main()
