"""BOP19 scoring of a results file: what the reference does offline with its BOP-toolkit fork after ``GDRN_Evaluator`` wrote the csv
(core/gdrn_modeling/engine/test_utils.py:33-80 -> lib/pysixd/scripts/eval_pose_results_more.py:39-156, 354-381 -> eval_calc_errors.py:254-612
and eval_calc_scores.py:180-276), with the per-pair NumPy arithmetic replaced by a handful of kernel calls for the whole dataset:

    reference, per error type:   a process per type, per (estimate, ground truth) pair a NumPy pass over the model per symmetry
    here:                        pair every estimate with the ground truths of its object in its image once, then ONE
                                 ``hip_lib.bop_errors`` call (mssd, mspd) and ONE ``hip_lib.pose_errors`` call per ADD / ADI flavour
                                 (ad, add, adi, re, te, rete, proj) and ONE ``hip_lib.sym_errors`` call (reS, teS, projS: the minima over
                                 the object's symmetry transformations, csrc/sym_error.hip) for all pairs; matching and recall stay host code
    reference, vsd:              per pair two GL renders and half a dozen full-image NumPy passes
    here, vsd:                   the pairs whose bounding spheres' projections overlap, grouped by image, in ONE ``hip_lib.vsd_errors``
                                 call per chunk of depth images: a tiled render-and-compare kernel (csrc/vsd_error.hip)

VSD needs the split's depth images and the eval models' faces: a ``BopGT`` built with ``depth=`` (``from_bop_dir(with_depth=True)``).
Without them ``vsd`` raises NotImplementedError, as ``cus``, ``reteS`` and the ``ABS*`` and ``AUC*`` types always do: the absolute-threshold and
area-under-curve family of ADD(-S) is deliberately left out as a whole (serving half of it would be worse than none).  ``reS``, ``teS`` and
``projS`` are computed, so the reference's own config line ``VAL.ERROR_TYPES = "mspd,mssd,vsd,ad,reS,teS"`` is scored as it stands.  With
mspd, mssd and vsd all computed the result holds ``bop19_average_recall``, the number a BOP submission is ranked by.  Units are those of a BOP results file:
translations, model vertices and depth in millimetres."""
from __future__ import annotations

import json
import logging
import os

import numpy as np
import torch

from .. import hip_lib
from ..lib.pysixd import inout, misc, pose_matching, score

logger = logging.getLogger(__name__)

MAX_SYM_DISC_STEP = 0.01            # eval_pose_results_more.py:162
# eval_pose_results_more.py:39-156, the same expressions so that the floats are the same
CORRECT_THS = {
    "mssd": [[th] for th in np.arange(0.05, 0.51, 0.05)],
    "mspd": [[th] for th in np.arange(5, 51, 5)],
    "ad": [[th] for th in [0.02, 0.05, 0.1]],
    "add": [[th] for th in [0.02, 0.05, 0.1]],
    "adi": [[th] for th in [0.02, 0.05, 0.1]],
    "re": [[th] for th in [2, 5, 10]],
    "te": [[th] for th in [2, 5, 10]],
    "rete": [[2, 2], [5, 5], [10, 10]],
    "proj": [[th] for th in [2, 5, 10]],
}
# VSD (eval_pose_results_more.py:42-63, eval_calc_errors.py:37-53): kept beside CORRECT_THS, not in it — vsd is scored per tau
VSD_TAUS = list(np.arange(0.05, 0.51, 0.05))
VSD_CORRECT_THS = [[th] for th in np.arange(0.05, 0.51, 0.05)]
VSD_DELTAS = {"hb": 15, "hbs": 15, "icbin": 15, "icmi": 15, "itodd": 5, "lm": 15, "lmo": 15, "ruapc": 15, "tless": 15, "tudl": 15, "tyol": 15,
              "ycbv": 15, "hope": 15}
VSD_NORMALIZED_BY_DIAMETER = True
VSD_IMAGE_BYTES = 256 << 20         # depth images uploaded per ``hip_lib.vsd_errors`` call
# the symmetry-aware types (eval_pose_results_more.py:136-155; deg, cm, px): kept beside CORRECT_THS, not in it, as the VSD thresholds are
SYM_CORRECT_THS = {
    "reS": [[th] for th in [2, 5, 10]],
    "teS": [[th] for th in [2, 5, 10]],
    "projS": [[th] for th in [2, 5, 10]],
}
KNOWN_NOT_IMPLEMENTED = ("vsd", "cus", "reteS", "ABSad", "ABSadd", "ABSadi", "AUCad", "AUCadd", "AUCadi")
NORMALIZED_BY_DIAMETER = ("ad", "add", "adi", "mssd")      # eval_calc_scores.py:70-72
NORMALIZED_BY_IM_WIDTH = ("mspd",)


class BopGT:
    """What scoring needs of a BOP dataset split, loaded once:

    scene_gt {scene_id: {im_id: [{"obj_id", "cam_R_m2c" f64[3,3], "cam_t_m2c" f64[3] (mm)}, ...]}}, scene_gt_info {scene_id: {im_id:
    [{"visib_fract"}, ...]}}, scene_camera {scene_id: {im_id: {"cam_K" f64[3,3]}}}, targets [{"scene_id", "im_id", "obj_id",
    "inst_count"}, ...], models_info {obj_id: {"diameter", "symmetries_discrete", "symmetries_continuous"}}, symmetric_obj_ids (the
    objects that ``ad`` scores with ADI), vertices {obj_id: f32[n,3] eval-model points in mm}, im_width, and the id lists the recall
    averages run over: obj_ids (default: the models), scene_ids (default: the scenes of the targets).

    For VSD, keyword-only: faces {obj_id: i32[n,3]} of the eval models; depth, the test depth images, either {scene_id: {im_id: f32[H,W]
    array or path of a 16-bit PNG}} or a callable (scene_id, im_id) -> array or path, in the stored unit (each image is multiplied by its
    ``depth_scale`` of scene_camera, default 1.0, to millimetres); im_size (W, H), checked against the images when given; dataset, the
    name ``VSD_DELTAS`` is asked for the visibility tolerance, or an explicit vsd_delta."""

    def __init__(self, scene_gt, scene_gt_info, scene_camera, targets, models_info, symmetric_obj_ids, vertices, im_width,
                 obj_ids=None, scene_ids=None, *, faces=None, depth=None, im_size=None, dataset=None, vsd_delta=None):
        self.scene_gt = {int(s): {int(i): [dict(obj_id=int(g["obj_id"]), cam_R_m2c=np.asarray(g["cam_R_m2c"], np.float64).reshape(3, 3),
                                                cam_t_m2c=np.asarray(g["cam_t_m2c"], np.float64).reshape(3)) for g in gts]
                                  for i, gts in per_im.items()} for s, per_im in scene_gt.items()}
        self.scene_gt_info = {int(s): {int(i): [dict(visib_fract=g["visib_fract"]) for g in infos] for i, infos in per_im.items()}
                              for s, per_im in scene_gt_info.items()}
        self.scene_camera = {int(s): {int(i): dict(cam_K=np.asarray(c["cam_K"], np.float64).reshape(3, 3), depth_scale=float(c.get("depth_scale", 1.0)))
                                      for i, c in per_im.items()} for s, per_im in scene_camera.items()}
        self.targets = [dict(scene_id=int(t["scene_id"]), im_id=int(t["im_id"]), obj_id=int(t["obj_id"]),
                             inst_count=int(t["inst_count"])) for t in targets]
        self.models_info = {int(k): v for k, v in models_info.items()}
        self.symmetric_obj_ids = [int(o) for o in symmetric_obj_ids]
        self.vertices = {int(k): np.ascontiguousarray(v, np.float32).reshape(-1, 3) for k, v in vertices.items()}
        self.im_width = im_width
        self.obj_ids = [int(o) for o in obj_ids] if obj_ids is not None else sorted(self.models_info)
        self.scene_ids = [int(s) for s in scene_ids] if scene_ids is not None else sorted({t["scene_id"] for t in self.targets})
        self.faces = None if faces is None else {int(k): np.ascontiguousarray(f, np.int32).reshape(-1, 3) for k, f in faces.items()}
        self.depth = depth if depth is None or callable(depth) else {int(s): {int(i): d for i, d in per_im.items()} for s, per_im in depth.items()}
        self.im_size = None if im_size is None else (int(im_size[0]), int(im_size[1]))
        self.dataset, self.vsd_delta = dataset, vsd_delta

    @property
    def has_depth(self) -> bool:
        return self.depth is not None

    def vsd_tolerance(self) -> float:
        """delta of the visibility test: the explicit ``vsd_delta``, else the dataset's entry of ``VSD_DELTAS``."""
        if self.vsd_delta is not None:
            return float(self.vsd_delta)
        if self.dataset not in VSD_DELTAS:
            raise ValueError(f"BopGT: vsd needs vsd_delta= or a dataset= of {sorted(VSD_DELTAS)}, got dataset={self.dataset!r}")
        return float(VSD_DELTAS[self.dataset])

    def depth_mm(self, scene_id, im_id) -> np.ndarray:
        """The test depth image in millimetres, f32[H,W]: loaded (``inout.load_depth``) if the source names a path, then scaled as
        eval_calc_errors.py:299-304 does, in float32."""
        d = self.depth(scene_id, im_id) if callable(self.depth) else self.depth[scene_id][im_id]
        if isinstance(d, (str, os.PathLike)):
            d = inout.load_depth(d)
        d = np.array(d, np.float32)
        d *= self.scene_camera[scene_id][im_id]["depth_scale"]
        if d.ndim != 2 or (self.im_size is not None and d.shape != (self.im_size[1], self.im_size[0])):
            raise ValueError(f"BopGT: depth image of scene {scene_id}, image {im_id} has shape {d.shape}, im_size is {self.im_size}")
        return d

    @classmethod
    def from_bop_dir(cls, dataset_dir, split="test", targets_filename="test_targets_bop19.json", models_dir="models_eval",
                     symmetric_obj_ids=(), im_width=640, obj_ids=None, scene_ids=None, with_depth=False, im_size=None, dataset=None,
                     vsd_delta=None, gt_info="file", device="cuda"):
        """The standard BOP layout: ``<dataset_dir>/<models_dir>/models_info.json`` + ``obj_{id:06d}.ply``,
        ``<dataset_dir>/<targets_filename>`` and ``<dataset_dir>/<split>/{scene_id:06d}/scene_gt.json | scene_gt_info.json |
        scene_camera.json`` for the scenes the targets name.  with_depth: also the faces of the eval models and, for the images the targets
        name, the paths ``<split>/{scene_id:06d}/depth/{im_id:06d}.png`` (read when VSD asks for them); dataset defaults to the directory's
        name when ``VSD_DELTAS`` knows it.  gt_info: where ``scene_gt_info`` comes from.  "file" reads ``scene_gt_info.json``; "compute" renders
        every ground truth of the scenes with the models of ``models_dir`` against the depth images ``<split>/{scene_id:06d}/depth/
        {im_id:06d}.png`` (needed whether or not ``with_depth`` is set; im_size defaults to the first image's) on ``device`` and takes
        ``bop_gt_info.calc_gt_info``'s records, with the tolerance ``vsd_tolerance()`` would give; "auto" reads the file where it exists
        and computes where it does not."""
        if gt_info not in ("file", "compute", "auto"):
            raise ValueError(f"BopGT.from_bop_dir: gt_info must be 'file', 'compute' or 'auto', got {gt_info!r}")

        def load(*parts):
            with open(os.path.join(dataset_dir, *parts)) as f:
                return json.load(f)

        targets = load(targets_filename)
        models_info = {int(k): v for k, v in load(models_dir, "models_info.json").items()}
        plys = {o: inout.load_ply(os.path.join(dataset_dir, models_dir, f"obj_{o:06d}.ply")) for o in models_info}
        vertices = {o: m["pts"] for o, m in plys.items()}
        per_scene = {name: {} for name in ("scene_gt", "scene_gt_info", "scene_camera")}
        computed = []
        for s in sorted({int(t["scene_id"]) for t in targets}):
            have = gt_info == "file" or (gt_info == "auto" and os.path.exists(os.path.join(dataset_dir, split, f"{s:06d}", "scene_gt_info.json")))
            for name in per_scene:
                if name == "scene_gt_info" and not have:
                    computed.append(s)
                    continue
                per_scene[name][s] = load(split, f"{s:06d}", name + ".json")
        name = os.path.basename(os.path.normpath(str(dataset_dir)))
        if computed:
            from . import bop_gt_info

            probe = cls({}, {}, {}, [], models_info, (), {}, im_width, dataset=dataset if dataset is not None else name, vsd_delta=vsd_delta)
            delta = probe.vsd_tolerance()
            ids = sorted(models_info)
            meshes = hip_lib.MeshSet([np.asarray(plys[o]["pts"], np.float32) for o in ids], [np.asarray(plys[o]["faces"], np.int32) for o in ids],
                                     device=device)
            for s in computed:
                paths = {int(i): os.path.join(dataset_dir, split, f"{s:06d}", "depth", f"{int(i):06d}.png") for i in per_scene["scene_gt"][s]}
                size = im_size
                if size is None and paths:
                    size = inout.load_depth(paths[min(paths)]).shape[::-1]
                per_scene["scene_gt_info"][s] = bop_gt_info.calc_gt_info(per_scene["scene_gt"][s], {int(i): c for i, c in per_scene["scene_camera"][s].items()},
                                                                         paths, meshes, ids, size, delta)
        extra = {}
        if with_depth:
            depth = {}
            for t in targets:
                s, i = int(t["scene_id"]), int(t["im_id"])
                depth.setdefault(s, {})[i] = os.path.join(dataset_dir, split, f"{s:06d}", "depth", f"{i:06d}.png")
            extra = dict(faces={o: m["faces"] for o, m in plys.items()}, depth=depth, im_size=im_size,
                         dataset=dataset if dataset is not None else (name if name in VSD_DELTAS else None), vsd_delta=vsd_delta)
        return cls(per_scene["scene_gt"], per_scene["scene_gt_info"], per_scene["scene_camera"], targets, models_info, symmetric_obj_ids,
                   vertices, im_width, obj_ids, scene_ids, **extra)

    def meshes(self, device="cuda"):
        """The eval models as a ``hip_lib.MeshSet`` in ``sorted(models_info)`` order: with their faces when ``faces`` was given (VSD
        renders them), points only otherwise."""
        no_face = np.zeros((1, 3), np.int32)
        ids = sorted(self.models_info)
        faces = [no_face] * len(ids) if self.faces is None else [self.faces[o] for o in ids]
        return hip_lib.MeshSet([self.vertices[o] for o in ids], faces, device=device)


def average_time_per_image(records) -> float:
    """eval_pose_results_more.py:243-265: the mean of the per-image times; -1 once an estimate has none (< 0); the estimates of an
    image must agree within 1e-3."""
    times = {}
    for r in records:
        key = (int(r["scene_id"]), int(r["im_id"]))
        if r["time"] < 0:
            return -1.0
        if key in times:
            if abs(times[key] - r["time"]) > 0.001:
                raise ValueError("The running time for scene {} and image {} is not the same for all estimates.".format(*key))
        else:
            times[key] = r["time"]
    return float(np.mean(list(times.values())))


def _check_types(error_types, gt=None):
    for t in error_types:
        if t == "vsd":
            if gt is None or not gt.has_depth or gt.faces is None:
                raise NotImplementedError("bop19_scores: error type 'vsd' is not computed here without the split's depth images and the eval "
                                          "models' faces: build the BopGT with depth= and faces= (BopGT.from_bop_dir(..., with_depth=True))")
        elif t not in CORRECT_THS and t not in SYM_CORRECT_THS:
            raise NotImplementedError(f"bop19_scores: error type {t!r} is not computed here"
                                      + ("" if t in KNOWN_NOT_IMPLEMENTED else " (and unknown to the BOP toolkit)"))


def _organize_targets(targets):
    org = {}
    for t in targets:
        org.setdefault(t["scene_id"], {}).setdefault(t["im_id"], {})[t["obj_id"]] = t
    return org


def pair_estimates(records, gt: BopGT, targets, n_top: int):
    """eval_calc_errors.py:254-358.  -> (ests, pairs): ``ests`` one entry per evaluated estimate, in the script's order (targets by
    scene, image, object; estimates by falling score, stable) ``{"scene_id", "im_id", "obj_id", "est_id", "score", "gt_ids", "pairs"}``
    with ``est_id`` the estimate's position among its object's estimates of the image before the sort; ``pairs`` a list of
    (R_e f64[9], t_e f64[3], obj_id, scene_id, im_id, gt_id), one per (estimate, ground truth of the same object in the image)."""
    ests_org = {}
    for r in records:
        ests_org.setdefault(int(r["scene_id"]), {}).setdefault(int(r["im_id"]), {}).setdefault(int(r["obj_id"]), []).append(r)
    ests, pairs = [], []
    for scene_id, scene_targets in _organize_targets(targets).items():
        for im_id, im_targets in scene_targets.items():
            for obj_id, target in im_targets.items():
                n_top_curr = None if n_top == 0 else (target["inst_count"] if n_top == -1 else n_top)
                obj_ests = ests_org.get(scene_id, {}).get(im_id, {}).get(obj_id, [])
                ranked = sorted(enumerate(obj_ests), key=lambda x: x[1]["score"], reverse=True)[slice(0, n_top_curr)]
                for est_id, est in ranked:
                    entry = dict(scene_id=scene_id, im_id=im_id, obj_id=obj_id, est_id=est_id, score=est["score"], gt_ids=[], pairs=[])
                    R_e, t_e = np.asarray(est["R"], np.float64).reshape(9), np.asarray(est["t"], np.float64).reshape(3)
                    for gt_id, g in enumerate(gt.scene_gt[scene_id][im_id]):
                        if g["obj_id"] != obj_id:
                            continue
                        entry["gt_ids"].append(gt_id)
                        entry["pairs"].append(len(pairs))
                        pairs.append((R_e, t_e, obj_id, scene_id, im_id, gt_id))
                    ests.append(entry)
    return ests, pairs


def calc_errors(records, gt: BopGT, targets, models_info, meshes, error_types, n_top: int):
    """-> {error_type: {scene_id: [{"im_id", "obj_id", "est_id", "score", "errors": {gt_id: [elements]}}, ...]}}: the content of the
    script's ``errors_{scene_id:06d}.json`` files (eval_calc_errors.py:343-612), un-normalised."""
    _check_types(error_types, gt)
    ests, pairs = pair_estimates(records, gt, targets, n_top)
    ids = sorted(models_info)
    index = {o: k for k, o in enumerate(ids)}
    P = len(pairs)
    values = {}
    if P:
        dev = meshes.verts.device
        R_e = np.stack([p[0] for p in pairs])
        t_e = np.stack([p[1] for p in pairs])
        obj_ids = np.array([p[2] for p in pairs])
        g = [gt.scene_gt[p[3]][p[4]][p[5]] for p in pairs]
        R_g = np.stack([x["cam_R_m2c"].reshape(9) for x in g])
        t_g = np.stack([x["cam_t_m2c"] for x in g])
        K = np.stack([gt.scene_camera[p[3]][p[4]]["cam_K"].reshape(9) for p in pairs])
        obj = np.array([index[o] for o in obj_ids], np.int32)
        # eval_calc_errors.py:373-374, per pair as the script does it
        overlap = np.array([np.linalg.norm(t_e[i].reshape(3, 1) - t_g[i].reshape(3, 1)) < models_info[obj_ids[i]]["diameter"]
                            for i in range(P)], bool)

        def dev_args(sel):
            return [torch.from_numpy(np.ascontiguousarray(a[sel])).to(dev) for a in (obj, R_e, t_e, R_g, t_g, K)]

        def scatter(sel, out, cols):
            full = np.full((P, cols), np.inf)
            full[sel] = out.cpu().numpy()
            return full

        everything, near = np.arange(P), np.nonzero(overlap)[0]
        if any(t in error_types for t in ("mssd", "mspd", *SYM_CORRECT_THS)):
            syms = [misc.get_symmetry_transformations(models_info[o], MAX_SYM_DISC_STEP) for o in ids]
            sym_R, sym_t, sym_off = misc.flatten_symmetry_transformations(syms)
            sym_R, sym_t = torch.from_numpy(sym_R).to(dev), torch.from_numpy(sym_t).to(dev)
        if "mssd" in error_types or "mspd" in error_types:
            sel = everything if "mspd" in error_types else near
            if len(sel):
                out = hip_lib.bop_errors(meshes, *dev_args(sel), sym_R, sym_t, sym_off)
                full = scatter(sel, out, 2)
                values["mssd"], values["mspd"] = np.where(overlap, full[:, 0], np.inf), full[:, 1]
        if any(t in error_types for t in SYM_CORRECT_THS):      # eval_calc_errors.py:545-596: every pair, no sphere-overlap cut
            args = dev_args(everything)
            if "projS" not in error_types:
                args[5] = None                                  # no K: nothing runs over the model points
            full = hip_lib.sym_errors(meshes, *args, sym_R, sym_t, sym_off).cpu().numpy()
            values["reS"], values["teS"], values["projS"] = full[:, 0], full[:, 1] / 10, full[:, 2]          # teS: mm -> cm
        plain = [t for t in error_types if t in ("add", "re", "te", "rete", "proj")]
        flavours = []                                          # (the types served, pairs, ADI flags)
        if plain:
            flavours.append((plain, near if plain == ["add"] else everything, None))
        if "adi" in error_types:
            flavours.append((["adi"], near, np.ones(len(ids), np.uint8)))
        if "ad" in error_types:
            flavours.append((["ad"], near, np.array([o in gt.symmetric_obj_ids for o in ids], np.uint8)))
        for served, sel, flags in flavours:
            if not len(sel):
                continue
            symmetric = torch.from_numpy(flags).to(dev) if flags is not None else None
            full = scatter(sel, hip_lib.pose_errors(meshes, *dev_args(sel), symmetric=symmetric), 4)
            for t in served:
                if t in ("ad", "add", "adi"):
                    values[t] = np.where(overlap, full[:, 0], np.inf)
                else:
                    values["re"], values["te"], values["proj"] = full[:, 1], full[:, 2] / 10, full[:, 3]     # te: mm -> cm
        if "vsd" in error_types:
            values["vsd"] = _vsd_errors(pairs, gt, models_info, meshes, obj, obj_ids, R_e, t_e, R_g, t_g, K)
    inf = np.full((P,), np.inf)

    def elements(t, k):
        if t == "vsd":
            return [float(x) for x in values["vsd"][k]]
        if t == "rete":
            return [float(values["re"][k]), float(values["te"][k])]
        return [float(values.get(t, inf)[k])]

    out = {}
    for t in error_types:
        per_scene = {s: [] for s in _organize_targets(targets)}
        for e in ests:
            per_scene[e["scene_id"]].append(dict(im_id=e["im_id"], obj_id=e["obj_id"], est_id=e["est_id"], score=e["score"],
                                                 errors={g_id: elements(t, k) for g_id, k in zip(e["gt_ids"], e["pairs"])}))
        out[t] = per_scene
    return out


def _vsd_errors(pairs, gt, models_info, meshes, obj, obj_ids, R_e, t_e, R_g, t_g, K):
    """eval_calc_errors.py:296-304, 360-395 for all pairs -> f64[P, n_tau].  A pair whose bounding spheres' projections do not overlap gets
    1.0 for every tau without a launch; the images the others name are loaded once each and uploaded in chunks of at most
    ``VSD_IMAGE_BYTES``, each chunk scored by one ``hip_lib.vsd_errors`` call."""
    P, n_tau = len(pairs), len(VSD_TAUS)
    out = np.ones((P, n_tau))
    delta = gt.vsd_tolerance()
    near = [i for i in range(P) if misc.overlapping_sphere_projections(0.5 * models_info[obj_ids[i]]["diameter"], t_e[i], t_g[i])]
    by_image = {}
    for i in near:
        by_image.setdefault((pairs[i][3], pairs[i][4]), []).append(i)
    dev = meshes.verts.device
    diameter = np.array([models_info[o]["diameter"] if VSD_NORMALIZED_BY_DIAMETER else 1.0 for o in obj_ids], np.float64)
    keys = list(by_image)
    k0 = 0
    while k0 < len(keys):
        images = [gt.depth_mm(*keys[k0])]
        k1 = k0 + 1
        while k1 < len(keys) and (len(images) + 1) * images[0].nbytes <= VSD_IMAGE_BYTES:
            images.append(gt.depth_mm(*keys[k1]))
            k1 += 1
        if any(im.shape != images[0].shape for im in images):
            raise ValueError("bop19_scores: the depth images of a split must have one size")
        sel = np.array([i for k in range(k0, k1) for i in by_image[keys[k]]])
        im_idx = np.array([k - k0 for k in range(k0, k1) for _ in by_image[keys[k]]], np.int32)
        args = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (obj[sel], im_idx, R_e[sel], t_e[sel], R_g[sel], t_g[sel], K[sel], diameter[sel])]
        depth = torch.from_numpy(np.stack(images)).to(dev)
        out[sel] = hip_lib.vsd_errors(meshes, *args, depth, VSD_TAUS, delta).cpu().numpy()
        k0 = k1
    if np.isnan(out).any():
        raise RuntimeError("bop19_scores: vsd could not render an object (the eval models need faces)")
    return out


def valid_gts(gt: BopGT, scene_id, scene_targets):
    """eval_calc_scores.py:205-238 with ``visib_gt_min = -1``: per target image, the ``inst_count`` most visible ground truths of every
    target object are valid (a stable sort by falling ``visib_fract``), all others are not."""
    valid = {}
    for im_id, im_targets in scene_targets.items():
        im_gt, info = gt.scene_gt[scene_id][im_id], gt.scene_gt_info[scene_id][im_id]
        left = {obj_id: t["inst_count"] for obj_id, t in im_targets.items()}
        valid[im_id] = [False] * len(im_gt)
        for gt_id in sorted(range(len(im_gt)), key=lambda k: info[k]["visib_fract"], reverse=True):
            obj_id = im_gt[gt_id]["obj_id"]
            if left.get(obj_id, 0) > 0:
                valid[im_id][gt_id] = True
                left[obj_id] -= 1
    return valid


def score_errors(errors_by_scene, gt: BopGT, targets, models_info, error_type, correct_th, n_top, im_width, do_print=False):
    """eval_calc_scores.py:180-276 for one threshold: normalise (by the object's diameter, or by 640 / image width), match per scene,
    count.  -> (matches, scores)."""
    matches = []
    for scene_id, scene_targets in _organize_targets(targets).items():
        scene_gt_curr = {im_id: gt.scene_gt[scene_id][im_id] for im_id in scene_targets}
        errs = []
        for e in errors_by_scene.get(scene_id, []):
            if error_type in NORMALIZED_BY_DIAMETER:
                diameter = float(models_info[e["obj_id"]]["diameter"])
                e = dict(e, errors={k: [x / diameter for x in v] for k, v in e["errors"].items()})
            elif error_type in NORMALIZED_BY_IM_WIDTH:
                factor = 640.0 / float(im_width)
                e = dict(e, errors={k: [factor * x for x in v] for k, v in e["errors"].items()})
            errs.append(e)
        matches += pose_matching.match_poses_scene(scene_id, scene_gt_curr, valid_gts(gt, scene_id, scene_targets), errs,
                                                   [float(th) for th in correct_th], n_top)
    return matches, score.calc_localization_scores(gt.scene_ids, gt.obj_ids, matches, n_top, do_print=do_print)


def scores_from_errors(errors, records, gt: BopGT, targets, models_info, error_types, n_top, im_width) -> dict:
    """eval_pose_results_more.py:268-381 from computed errors: per type the recall at every threshold and their mean."""
    final, recalls_of, obj_recalls_of = {}, {}, {}
    for t in error_types:
        recalls, obj_recalls = [], []
        if t == "vsd":      # eval_pose_results_more.py:306-354: every tau's single-element errors against every threshold, 10 x 10 recalls
            for k in range(len(VSD_TAUS)):
                view = {s: [dict(e, errors={g_id: [v[k]] for g_id, v in e["errors"].items()}) for e in errs] for s, errs in errors[t].items()}
                scored = [score_errors(view, gt, targets, models_info, t, th, n_top, im_width)[1] for th in VSD_CORRECT_THS]
                recalls.append([s["recall"] for s in scored])
                obj_recalls.append([s["obj_recalls"] for s in scored])
            recalls_of[t], obj_recalls_of[t] = recalls, obj_recalls
            final["bop19_average_recall_vsd"] = float(np.mean([r for per_tau in recalls for r in per_tau]))
            continue
        for th in (CORRECT_THS[t] if t in CORRECT_THS else SYM_CORRECT_THS[t]):
            _, s = score_errors(errors[t], gt, targets, models_info, t, th, n_top, im_width)
            recalls.append(s["recall"])
            obj_recalls.append(s["obj_recalls"])
        recalls_of[t], obj_recalls_of[t] = recalls, obj_recalls
        final[f"bop19_average_recall_{t}"] = float(np.mean(recalls))
    if all(t in error_types for t in ("mspd", "mssd", "vsd")):          # eval_pose_results_more.py:371-378
        final["bop19_average_recall"] = float(np.mean([final[f"bop19_average_recall_{t}"] for t in ("mspd", "mssd", "vsd")]))
    final["bop19_average_time_per_image"] = average_time_per_image(records)
    final["recalls"] = recalls_of                     # per type: the recall at each threshold of CORRECT_THS / SYM_CORRECT_THS; vsd: per tau, per threshold
    final["obj_recalls"] = obj_recalls_of             # per type: {obj_id: recall} at each threshold; vsd: nested per tau likewise
    return final


def bop19_scores(records, gt: BopGT, targets=None, models_info=None, meshes=None, error_types=("mssd", "mspd"), n_top=-1,
                 im_width=None) -> dict:
    """records: BOP estimates ``{"scene_id", "im_id", "obj_id", "score", "R" (9 values), "t" (3, mm), "time"}`` (what ``GDRN_Evaluator``
    writes to the csv).  targets / models_info / im_width default to ``gt``'s; meshes: the eval models as a ``hip_lib.MeshSet`` in
    ``sorted(models_info)`` order (default: built from ``gt.vertices``).  error_types: a sequence, or the comma-separated string of
    ``VAL.ERROR_TYPES``.  n_top: estimates per target, -1 = the target's ``inst_count``, 0 = all.

    -> ``bop19_average_recall_<type>`` per type (the mean recall over the type's thresholds), ``bop19_average_time_per_image``,
    ``recalls`` and ``obj_recalls`` (per type, per threshold; for vsd per tau, per threshold); ``bop19_average_recall`` only if mspd, mssd
    and vsd were all computed.  ``vsd`` needs a ``gt`` with depth images and faces."""
    if isinstance(error_types, str):
        error_types = [t for t in error_types.split(",") if t]
    error_types = list(error_types)
    targets = gt.targets if targets is None else targets
    models_info = gt.models_info if models_info is None else {int(k): v for k, v in models_info.items()}
    im_width = gt.im_width if im_width is None else im_width
    _check_types(error_types, gt)                                        # before anything is launched
    if meshes is None:
        meshes = gt.meshes()
    errors = calc_errors(records, gt, targets, models_info, meshes, error_types, int(n_top))
    return scores_from_errors(errors, records, gt, targets, models_info, error_types, int(n_top), im_width)
