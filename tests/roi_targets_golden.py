"""Loader of tests/golden/readdata_train_golden.npz (what the reference's ``read_data_train``, executed from its source, returned on the
200x136 split of xyz_crop_golden.npz; generator: tests/golden/make_golden_readdata_train.py) for the CPU and GPU tests: the variants'
configs, the instances as ``gdrn_modeling.train_targets`` takes them, and the random state the reference's DZI drew from."""
import functools
import json
import os

import numpy as np

from conftest import GOLDEN
from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
from tests import xyz_crop_golden as XG

MAPS = ("roi_mask_trunc", "roi_mask_visib", "roi_mask_obj", "roi_mask_full", "roi_region", "roi_xyz", "roi_xyz_bin")
HOST = ("bbox_center", "scale", "roi_wh", "resize_ratio", "trans_ratio")


@functools.lru_cache(maxsize=None)
def load():
    z = np.load(os.path.join(GOLDEN, "readdata_train_golden.npz"))
    meta = json.loads(str(z["meta"]))
    return dict(z=z, meta=meta, im_size=tuple(meta["im_size"]), variants={k: tuple(v) for k, v in meta["variants"].items()},
                keys=[tuple(int(x) for x in k) for k in z["keys"]], syn_key=tuple(meta["syn_key"]), extents=z["extents"],
                fps={4: z["fps4"], 64: z["fps64"]}, records=XG.load()["records"])


def cfg_of(tag):
    loss_type, mask_gt, n_bin, num_regions, bbox_type, dzi_type = load()["variants"][tag]
    return get_cfg("tless_convnext_a6", [f"MODEL.POSE_NET.LOSS_CFG.XYZ_LOSS_TYPE={loss_type}", f"MODEL.POSE_NET.LOSS_CFG.XYZ_LOSS_MASK_GT={mask_gt}",
                                         f"MODEL.POSE_NET.GEO_HEAD.XYZ_BIN={n_bin}", f"MODEL.POSE_NET.GEO_HEAD.NUM_REGIONS={num_regions}",
                                         f"MODEL.BBOX_TYPE={bbox_type}", f"INPUT.DZI_TYPE={dzi_type}", "INPUT.DZI_SCALE_RATIO=0.25",
                                         "INPUT.DZI_SHIFT_RATIO=0.25"])


def given(key, name):
    return load()["z"][f"in_{key[0]}_{key[1]}_{name}"]


def recorded(tag, key, name):
    return load()["z"][f"{tag}_{key[0]}_{key[1]}_{name}"]


def present(tag, key):
    return [str(m) for m in recorded(tag, key, "present")]


def rng_of(tag, key):
    """np.random as the reference's DZI found it: seeded, then one rand() drawn for a "real" image (against INPUT.CHANGE_BG_PROB)."""
    rng = np.random.RandomState(int(recorded(tag, key, "seed")))
    for _ in range(int(recorded(tag, key, "pre_draws"))):
        rng.rand()
    return rng


def host_masks():
    """-> (masks u8[3 * n_keys, H, W], {key: (visib_idx, trunc_idx, full_idx)}): segmentation, mask_full and mask_trunc of every instance;
    only the "syn" instance has a truncation mask in the reference's run."""
    g = load()
    planes, idx = [], {}
    for k in g["keys"]:
        idx[k] = (len(planes), len(planes) + 2 if k == g["syn_key"] else -1, len(planes) + 1)
        planes += [given(k, "segmentation"), given(k, "mask_full"), given(k, "mask_trunc").astype(np.uint8)]
    return np.stack(planes).astype(np.uint8), idx


def instances():
    """One dict per fixture instance, in the order of ``load()["keys"]``, as ``train_targets.roi_train_targets`` takes them."""
    _, idx = host_masks()
    out = []
    for i, k in enumerate(load()["keys"]):
        v, t, f = idx[k]
        out.append(dict(roi_cls=int(given(k, "roi_cls")), trans=given(k, "trans"), centroid_2d=given(k, "centroid_2d"), bbox_obj=given(k, "bbox_obj"),
                        xyz_idx=i, visib_idx=v, trunc_idx=t, full_idx=f))
    return out


def bbox_of(tag, key):
    """:476-489 -> the box the DZI starts from."""
    g = load()
    W, H = g["im_size"]
    bbox_type = g["variants"][tag][4].lower()
    if bbox_type == "visib":
        return list(g["records"][key]["xyxy"])
    ax1, ay1, ax2, ay2 = given(key, "bbox_obj")
    return [max(ax1, 0), max(ay1, 0), min(ax2, W), min(ay2, H)]


def assert_same(ours, tag, key, what=""):
    """{name: array} of one instance against the reference's record: the same keys among MAPS, dtype, shape and every element."""
    names = present(tag, key)
    assert sorted(k for k in ours if k in MAPS) == sorted(names), (what, tag, key, sorted(ours), names)
    for name in names + [h for h in HOST if h in ours]:
        ref, got = recorded(tag, key, name), np.asarray(ours[name])
        assert got.dtype == ref.dtype and got.shape == ref.shape, (what, tag, key, name, got.dtype, ref.dtype, got.shape, ref.shape)
        assert np.array_equal(got, ref), (what, tag, key, name, int((got != ref).sum()))
