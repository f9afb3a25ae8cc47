"""Write the ``xyz_crop/{scene:06d}/{im:06d}_{inst:06d}-xyz.pkl`` training targets of a BOP dataset split, as the reference's
core/gdrn_modeling/tools/*/*_1_gen_xyz.py do (tless, tudl, icbin, itodd ``*_pbr_1_gen_xyz.py``; lm_egl_1_gen_xyz.py's recipe on a split in
the BOP scene layout), computed on the device (gdrn_modeling/bop_xyz.py, csrc/xyz_crop.hip).

    python tools/gen_xyz.py --dataset-dir DIR --split train_pbr --models-dir models [--scenes 0 1 ...] [--im-size W H]
                            [--vertex-scale 0.001] [--znear 0.01] [--zfar 6.5] [--overwrite]

DIR holds ``<models-dir>/obj_{id:06d}.ply`` (millimetres) and ``<split>/{scene_id:06d}/scene_gt.json | scene_camera.json``; the files go to
``<split>/xyz_crop/``.  The image size defaults to the one the reference's tool of that dataset (the directory's name) renders at; any
other dataset needs --im-size.  One line per scene; an instance without a rendered pixel is listed as the tools list it and gets their
full-image zero record."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# IM_W, IM_H of lm_egl_1_gen_xyz.py and the tless / tudl / icbin / itodd *_pbr_1_gen_xyz.py
IM_SIZES = {"lm": (640, 480), "tless": (720, 540), "tudl": (640, 480), "icbin": (640, 480), "itodd": (1280, 960)}
IMAGES_PER_CHUNK = 64


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--dataset-dir", required=True)
    ap.add_argument("--split", required=True)
    ap.add_argument("--models-dir", required=True, help="relative to --dataset-dir, or absolute")
    ap.add_argument("--scenes", type=int, nargs="*", default=None)
    ap.add_argument("--im-size", type=int, nargs=2, metavar=("W", "H"), default=None)
    ap.add_argument("--vertex-scale", type=float, default=0.001)
    ap.add_argument("--znear", type=float, default=0.01)
    ap.add_argument("--zfar", type=float, default=6.5)
    ap.add_argument("--overwrite", action="store_true", help="rewrite files that exist (the tools skip them)")
    args = ap.parse_args(argv)
    name = os.path.basename(os.path.normpath(args.dataset_dir))
    if args.im_size is None:
        if name not in IM_SIZES:
            ap.error(f"--im-size is needed: {name!r} is not one of {sorted(IM_SIZES)}")
        args.im_size = IM_SIZES[name]
    args.im_size = (int(args.im_size[0]), int(args.im_size[1]))
    return args


def main(argv=None):
    args = parse_args(argv)

    import numpy as np

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import bop_xyz as X
    from gdrnpp_bop2022_amd.lib.pysixd import inout

    models_dir = os.path.join(args.dataset_dir, args.models_dir)
    obj_ids = sorted(int(f[4:10]) for f in os.listdir(models_dir) if f.startswith("obj_") and f.endswith(".ply"))
    plys = [inout.load_ply(os.path.join(models_dir, f"obj_{o:06d}.ply"), vertex_scale=args.vertex_scale) for o in obj_ids]
    meshes = hip_lib.MeshSet([np.asarray(m["pts"], np.float32) for m in plys], [np.asarray(m["faces"], np.int32) for m in plys])
    split_dir = os.path.join(args.dataset_dir, args.split)
    scenes = args.scenes if args.scenes is not None else sorted(int(d) for d in os.listdir(split_dir) if d.isdigit())
    W, H = args.im_size
    for s in scenes:
        d = os.path.join(split_dir, f"{s:06d}")
        with open(os.path.join(d, "scene_gt.json")) as f:
            scene_gt = {int(k): v for k, v in json.load(f).items()}
        with open(os.path.join(d, "scene_camera.json")) as f:
            scene_camera = {int(k): v for k, v in json.load(f).items()}
        n_inst = n_written = n_invisible = 0
        im_ids = sorted(scene_gt)
        for k0 in range(0, len(im_ids), IMAGES_PER_CHUNK):
            chunk = {im: scene_gt[im] for im in im_ids[k0:k0 + IMAGES_PER_CHUNK]}
            if not args.overwrite:                           # the tools' skip of finished files, before anything is rendered
                todo = {im: [g for g in range(len(v)) if not _done(X.xyz_crop_path(args.dataset_dir, args.split, s, im, g))] for im, v in chunk.items()}
                if not any(todo.values()):
                    n_inst += sum(len(v) for v in chunk.values())
                    continue
            crops = X.calc_xyz_crops(chunk, scene_camera, meshes, obj_ids, args.im_size, args.znear, args.zfar)
            for (im, g), rec in sorted(crops.items()):
                if rec["xyz_crop"].shape[:2] == (H, W) and rec["xyxy"] == [0, 0, W - 1, H - 1] and not rec["xyz_crop"].any():
                    o = scene_gt[im][g]["obj_id"]
                    print(f"not visible, cls {o}, im {im:06d} inst {g} obj {o}")
                    n_invisible += 1
            n_inst += len(crops)
            n_written += X.write_xyz_crops(args.dataset_dir, args.split, s, crops, overwrite=args.overwrite)
        print(f"scene {s:06d}: {len(im_ids)} images, {n_inst} instances, {n_written} files written, {n_invisible} not visible", flush=True)


def _done(path):
    return os.path.exists(path) and os.path.getsize(path) > 0


if __name__ == "__main__":
    main()
