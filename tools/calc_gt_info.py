"""Write ``scene_gt_info.json`` (and with ``--masks`` the ``mask/`` and ``mask_visib/`` images) of a BOP dataset split, as the reference's
lib/pysixd/scripts/calc_gt_info.py and calc_gt_masks.py do, computed on the device (gdrn_modeling/bop_gt_info.py, csrc/gt_visib.hip).

    python tools/calc_gt_info.py DATASET_DIR [--split test] [--models-dir models] [--delta 15] [--scenes 1 2 ...] [--masks] [--no-info]

DATASET_DIR holds ``<models-dir>/models_info.json`` + ``obj_{id:06d}.ply`` and ``<split>/{scene_id:06d}/scene_gt.json | scene_camera.json |
depth/{im_id:06d}.png``.  delta defaults to the dataset's visibility tolerance (``bop_eval.VSD_DELTAS`` by the directory's name)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("dataset_dir")
    ap.add_argument("--split", default="test")
    ap.add_argument("--models-dir", default="models")
    ap.add_argument("--delta", type=float, default=None)
    ap.add_argument("--scenes", type=int, nargs="*", default=None)
    ap.add_argument("--masks", action="store_true", help="also write mask/ and mask_visib/")
    ap.add_argument("--no-info", action="store_true", help="do not write scene_gt_info.json")
    args = ap.parse_args()

    import numpy as np

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import bop_gt_info as G
    from gdrnpp_bop2022_amd.gdrn_modeling.bop_eval import VSD_DELTAS
    from gdrnpp_bop2022_amd.lib.pysixd import inout

    name = os.path.basename(os.path.normpath(args.dataset_dir))
    if args.delta is None and name not in VSD_DELTAS:
        raise SystemExit(f"--delta is needed: {name!r} is not one of {sorted(VSD_DELTAS)}")
    delta = float(VSD_DELTAS[name]) if args.delta is None else args.delta
    with open(os.path.join(args.dataset_dir, args.models_dir, "models_info.json")) as f:
        obj_ids = sorted(int(k) for k in json.load(f))
    plys = [inout.load_ply(os.path.join(args.dataset_dir, args.models_dir, f"obj_{o:06d}.ply")) for o in obj_ids]
    meshes = hip_lib.MeshSet([np.asarray(m["pts"], np.float32) for m in plys], [np.asarray(m["faces"], np.int32) for m in plys])
    split_dir = os.path.join(args.dataset_dir, args.split)
    scenes = args.scenes if args.scenes is not None else sorted(int(d) for d in os.listdir(split_dir) if d.isdigit())
    for s in scenes:
        d = os.path.join(split_dir, f"{s:06d}")
        with open(os.path.join(d, "scene_gt.json")) as f:
            scene_gt = {int(k): v for k, v in json.load(f).items()}
        with open(os.path.join(d, "scene_camera.json")) as f:
            scene_camera = {int(k): v for k, v in json.load(f).items()}
        if not scene_gt:
            continue
        depth = {im: os.path.join(d, "depth", f"{im:06d}.png") for im in scene_gt}
        im_size = inout.load_depth(depth[min(depth)]).shape[::-1]
        walk = (scene_gt, scene_camera, depth, meshes, obj_ids, im_size, delta)
        if not args.no_info:
            print("wrote", G.write_scene_gt_info(args.dataset_dir, args.split, s, G.calc_gt_info(*walk)), flush=True)
        if args.masks:
            print("scene", s, "masks of", G.write_gt_masks(args.dataset_dir, args.split, s, G.calc_gt_masks(*walk)), "ground truths", flush=True)


if __name__ == "__main__":
    main()
