"""The training loader's background replacement: what ``replace_bg``, ``trunc_mask``, ``get_bg_image``, ``get_bg_image_v2``
(reference core/base_data_loader.py:413-579) and ``resize_short_edge`` (core/utils/data_utils.py:208-235) do per sample on the host, here
for a batch of full images with one call of ``hip_lib.replace_bg`` (csrc/replace_bg.hip).  The host keeps what is cheap and sequential —
the random draws in the reference's order and the size arithmetic of the crop and of cv2.resize — and the device does every per-pixel
pass: the mask's extents, the cut, the resize of the background and the composite.

    bg_geometry        crop of a background and the cv2.resize the reference asks for it: sizes, form and interpolation scales
    draw_replace_bg    the per-image random draws of read_data_train (:360-369), replace_bg and trunc_mask, in their order
    replace_bg_batch   draws + geometry + table + launch -> (images, mask_trunc, trunc_idx); the last two feed
                       ``hip_lib.roi_train_targets(masks=mask_trunc, trunc_idx=trunc_idx)`` as they stand
    BgPool, bg_paths   the decoded backgrounds in one device buffer; the reference's listing of background files (``_bg_img_paths``)

The result is the full composited u8 image: the reference's colour augmentation sits between ``replace_bg`` and the ROI crop, so the two
are not fused.  Out of scope, each raising NotImplementedError where it would be reached: colour augmentation itself (``COLOR_AUG_*``,
imgaug), depth backgrounds (``BG_TYPE`` "SUN_RGBD", ``INPUT.WITH_BG_DEPTH``, ``with_bg_depth=True``) and ``AUG_DEPTH``."""
from __future__ import annotations

import os
import random as _py_random

import numpy as np
import torch

from .. import hip_lib
from ..hip_lib.cv_resize import MODE_AREA, MODE_COPY, MODE_LINEAR, cv_round, resize_request  # noqa: F401  (cv2.resize's request: hip_lib's, read here too)

BG_DEFAULTS = dict(CHANGE_BG_PROB=0.5, TRUNCATE_FG=False, BG_KEEP_ASPECT_RATIO=True, BG_TYPE="VOC_table", WITH_BG_DEPTH=False,
                   BG_IMGS_ROOT="datasets/VOCdevkit/VOC2012/", NUM_BG_IMGS=10000)                  # configs/_base_/common_base.py:49-57


def _input(cfg, key):
    node = cfg["INPUT"] if "INPUT" in cfg else {}
    return node[key] if key in node else BG_DEFAULTS[key]


def bg_geometry(bg_h, bg_w, im_H, im_W, keep_aspect=True, rng=None) -> dict:
    """The crop of a bg_h x bg_w background and its resize for an im_H x im_W image -> dict(x0, y0, cw, ch, dw, dh, mode, scale_x, scale_y)
    (``hip_lib.REPLACE_BG_COLUMNS``' names).

    keep_aspect (``INPUT.BG_KEEP_ASPECT_RATIO``, the default): ``get_bg_image``.  Its four aspect branches cut the longer side of the
    background to ``int(np.ceil(...))`` of the image's aspect; two of them compare the new length with the old one first, the other two
    slice without asking and NumPy clips the slice, so all four keep min(new, old).  ``resize_short_edge`` then scales by
    target / shorter side unless ``np.round`` of the longer side exceeds the image's longer side, and calls cv2.resize with fx = fy.  The
    result is pasted top-left onto zeros, so it may leave a zero column or row (a 37 x 50 crop for 48 x 64 comes out 63 wide).
    Otherwise: ``get_bg_image_v2``, four ``randint`` draws from ``rng`` (``np.random`` or a RandomState) in its order — x1, y1, x2, y2 —
    and a resize of [y1:y2, x1:x2] to exactly (im_W, im_H)."""
    bg_h, bg_w, im_H, im_W = int(bg_h), int(bg_w), int(im_H), int(im_W)
    if keep_aspect:
        real_hw_ratio = float(im_H) / float(im_W)
        x0 = y0 = 0
        if bg_h >= bg_w:
            cw, ch = bg_w, min(int(np.ceil(bg_w * real_hw_ratio)), bg_h)
        else:
            cw, ch = min(int(np.ceil(bg_h / real_hw_ratio)), bg_w), bg_h
        target_size, max_size = min(im_H, im_W), max(im_H, im_W)
        im_scale = float(target_size) / float(min(ch, cw))
        if np.round(im_scale * max(ch, cw)) > max_size:
            im_scale = float(max_size) / float(max(ch, cw))
        req = resize_request(cw, ch, fx=im_scale, fy=im_scale)
        if req["dw"] > im_W or req["dh"] > im_H:
            raise ValueError(f"bg_geometry: a {bg_w} x {bg_h} background comes out {req['dw']} x {req['dh']} for a {im_W} x {im_H} image: "
                             f"the reference's paste fails here")
    else:
        rng = np.random if rng is None else rng
        x1 = int(rng.randint(0, int(bg_w / 3)))
        y1 = int(rng.randint(0, int(bg_h / 3)))
        x2 = int(rng.randint(int(2 * bg_w / 3), bg_w))
        y2 = int(rng.randint(int(2 * bg_h / 3), bg_h))
        x0, y0, cw, ch = x1, y1, x2 - x1, y2 - y1
        req = resize_request(cw, ch, dsize=(im_W, im_H))
    return dict(x0=x0, y0=y0, cw=cw, ch=ch, **req)


def draw_replace_bg(cfg, img_types, n_bg, py_random=None, np_random=None, *, bg_sizes=None, im_size=None) -> list:
    """The random draws of background replacement, image after image in the reference's order -> [dict(do, ind, geometry, cut, u)]:

      1. ``np_random.rand()`` against ``INPUT.CHANGE_BG_PROB``, only when the image's ``img_type`` is not "syn" (read_data_train :362-368);
         an image that stays as it is draws nothing more and gets dict(do=0);
      2. ``py_random.randint(0, n_bg - 1)``: the background (replace_bg :417);
      3. without ``INPUT.BG_KEEP_ASPECT_RATIO`` the four ``np_random.randint`` of ``get_bg_image_v2``'s crop — these need the chosen
         background's size: bg_sizes [(h, w)] and im_size (W, H); with them given ``geometry`` is ``bg_geometry``'s dict in either form,
         else None;
      4. with ``INPUT.TRUNCATE_FG`` ``py_random.random()`` picks trunc_mask's branch: < 0.2 block upper, < 0.4 bottom, < 0.6 left, < 0.8
         right, else no cut (cut = index into ``hip_lib.REPLACE_BG_CUTS``);
      5. a cutting branch draws one more ``py_random.random()``: the ``u`` of its ``random.uniform(a, b)`` = a + (b - a) u.

    py_random: the ``random`` module or a ``random.Random``; np_random: ``np.random`` or a RandomState.  Both are consumed exactly as
    the reference consumes its global ones for these steps, so generators seeded like the reference's give its backgrounds and cuts.  The
    reference's other per-sample draws (DZI, colour augmentation) come after these for each sample: a caller that wants its whole
    sequence from one pair of generators calls this sample by sample."""
    py_random = _py_random if py_random is None else py_random
    np_random = np.random if np_random is None else np_random
    if _input(cfg, "WITH_BG_DEPTH"):
        raise NotImplementedError("draw_replace_bg: INPUT.WITH_BG_DEPTH (depth backgrounds) is not carried")
    keep_aspect = bool(_input(cfg, "BG_KEEP_ASPECT_RATIO"))
    if not keep_aspect and (bg_sizes is None or im_size is None):
        raise ValueError("draw_replace_bg: INPUT.BG_KEEP_ASPECT_RATIO=False draws a crop of the chosen background: bg_sizes and im_size are needed")
    if n_bg < 1 or (bg_sizes is not None and len(bg_sizes) != n_bg):
        raise ValueError(f"draw_replace_bg: n_bg = {n_bg} backgrounds" + ("" if bg_sizes is None else f", {len(bg_sizes)} sizes"))
    prob, truncate = _input(cfg, "CHANGE_BG_PROB"), bool(_input(cfg, "TRUNCATE_FG"))
    draws = []
    for img_type in img_types:
        if img_type != "syn" and not np_random.rand() < prob:
            draws.append(dict(do=0))
            continue
        ind = py_random.randint(0, n_bg - 1)
        geometry = None
        if bg_sizes is not None and im_size is not None:
            geometry = bg_geometry(bg_sizes[ind][0], bg_sizes[ind][1], im_size[1], im_size[0], keep_aspect, np_random)
        cut, u = 0, 0.0
        if truncate:
            rnd = py_random.random()
            cut = 1 if rnd < 0.2 else 2 if rnd < 0.4 else 3 if rnd < 0.6 else 4 if rnd < 0.8 else 0
            if cut:
                u = py_random.random()
        draws.append(dict(do=1, ind=ind, geometry=geometry, cut=cut, u=u))
    return draws


def bg_paths(cfg, np_random=None) -> list:
    """``_bg_img_paths`` (core/base_data_loader.py:340-411) without its cache file: the background files of ``INPUT.BG_TYPE`` "coco", "VOC",
    "VOC_table" or "SUN2012" under ``INPUT.BG_IMGS_ROOT``, listed as the reference lists them, of which ``np_random.choice`` draws
    min(count, ``INPUT.NUM_BG_IMGS``) — with replacement, as the reference does."""
    np_random = np.random if np_random is None else np_random
    bg_type, root = _input(cfg, "BG_TYPE"), _input(cfg, "BG_IMGS_ROOT")
    if bg_type == "SUN_RGBD" or _input(cfg, "WITH_BG_DEPTH"):
        raise NotImplementedError("bg_paths: depth backgrounds (BG_TYPE='SUN_RGBD', INPUT.WITH_BG_DEPTH) are not carried")
    if not os.path.exists(root):
        raise FileNotFoundError(f"bg_paths: INPUT.BG_IMGS_ROOT {root} does not exist")
    if bg_type == "coco":
        paths = [os.path.join(root, fn.name) for fn in os.scandir(root) if ".png" in fn.name or "jpg" in fn.name]
    elif bg_type == "VOC_table":
        with open(os.path.join(root, "ImageSets/Main", "diningtable_trainval.txt")) as f:
            lines = [line.strip("\r\n").split() for line in f.readlines()]
        paths = [os.path.join(root, "JPEGImages/{}.jpg".format(parts[0])) for parts in lines if parts[1] == "1"]
    elif bg_type in ("VOC", "SUN2012"):
        paths = [os.path.join(root, "JPEGImages", fn.name) for fn in os.scandir(os.path.join(root, "JPEGImages")) if ".jpg" in fn.name]
    else:
        raise ValueError(f"bg_paths: BG_TYPE: {bg_type} is not supported")
    if not paths:
        raise ValueError(f"bg_paths: no background images of type {bg_type} under {root}")
    num = min(len(paths), int(_input(cfg, "NUM_BG_IMGS")))
    sel = np_random.choice([i for i in range(len(paths))], num)
    return [paths[i] for i in sel]


class BgPool:
    """Decoded backgrounds on the device: one flat u8 buffer (``data``) with per image its byte offset and (h, w) (``offsets``,
    ``sizes``), the layout ``hip_lib.replace_bg`` reads.  Images are u8[h,w,3] in the loader's channel order."""

    def __init__(self, images, device="cuda"):
        images = [np.asarray(im) for im in images]
        for k, im in enumerate(images):
            if im.dtype != np.uint8 or im.ndim != 3 or im.shape[2] != 3 or im.shape[0] < 1 or im.shape[1] < 1:
                raise ValueError(f"BgPool: background {k} must be u8[h,w,3], got {im.shape} of {im.dtype}")
        if not images:
            raise ValueError("BgPool: no backgrounds")
        self.sizes = [(int(im.shape[0]), int(im.shape[1])) for im in images]
        nbytes = [3 * h * w for h, w in self.sizes]
        self.offsets = [int(v) for v in np.concatenate([[0], np.cumsum(nbytes)[:-1]])]
        self.data = torch.from_numpy(np.concatenate([np.ascontiguousarray(im).reshape(-1) for im in images])).to(device)

    @classmethod
    def from_config(cls, cfg, reader, device="cuda", np_random=None):
        """The backgrounds ``bg_paths`` lists for ``cfg``, each decoded by ``reader(path) -> u8[h,w,3]`` (the caller's image reader, in the
        loader's channel order; this project decodes no image files)."""
        return cls([reader(p) for p in bg_paths(cfg, np_random)], device)

    def __len__(self):
        return len(self.sizes)


def replace_bg_batch(cfg, images, masks, img_types, bg_pool, *, py_random=None, np_random=None, with_bg_depth=False, out_mask=None):
    """Background replacement for a batch: the draws (``draw_replace_bg``), the geometry (``bg_geometry``), the table and one call of
    ``hip_lib.replace_bg``.  images u8[B,H,W,3] on the device, composited in place; masks u8[B,H,W], the instance masks
    (``cocosegm2mask`` of the annotation); img_types: per image "syn" (always replaced) or anything else (replaced with
    ``INPUT.CHANGE_BG_PROB``); bg_pool: a ``BgPool``.
    -> (images, mask_trunc u8[B,H,W], trunc_idx host i64[B]: b for a replaced image, -1 for one left untouched, whose row of mask_trunc
    is not written — the reference's ``mask_trunc is None``).  ``hip_lib.roi_train_targets(masks=mask_trunc, trunc_idx=trunc_idx[...])``
    takes the pair as it stands."""
    if with_bg_depth:
        raise NotImplementedError("replace_bg_batch: with_bg_depth=True (depth backgrounds) is not carried")
    B, H, W = int(images.shape[0]), int(images.shape[1]), int(images.shape[2])
    if len(img_types) != B:
        raise ValueError(f"replace_bg_batch: {len(img_types)} img_types for {B} images")
    draws = draw_replace_bg(cfg, img_types, len(bg_pool), py_random, np_random, bg_sizes=bg_pool.sizes, im_size=(W, H))
    rows = []
    for d in draws:
        if not d["do"]:
            rows.append(dict(do=0))
            continue
        rows.append(dict(do=1, bg_off=bg_pool.offsets[d["ind"]], bg_stride=bg_pool.sizes[d["ind"]][1], cut=d["cut"], u=d["u"], **d["geometry"]))
    mask_trunc, _ = hip_lib.replace_bg(images, masks, bg_pool.data, hip_lib.replace_bg_table(rows), out_mask=out_mask)
    trunc_idx = np.array([b if d["do"] else -1 for b, d in enumerate(draws)], np.int64)
    return images, mask_trunc, trunc_idx
