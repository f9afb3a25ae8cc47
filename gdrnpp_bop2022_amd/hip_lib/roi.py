"""ROI preparation: crop + resize of the detections' boxes, ROIAlign / RoIPool, the device-side ROI table filled from
detections, the per-ROI training targets, and the background replacement of the training images they are cut from."""
from __future__ import annotations

import ctypes

import torch

from .abi import dev_ptr, f32_ptr, gdrnpp_roi_table, launch, load, opt_f32_ptr
from .cv_resize import RESIZE_MODES


def crop_resize_roi(images, depths, im_idx, centers, scales, out_res: int = 256, out_res_small: int = 64,
                    pixel_mean=(0.0, 0.0, 0.0), pixel_std=(255.0, 255.0, 255.0), want_img=True, want_coord2d=True):
    """GPU ROI preparation (read_data_test, data_loader.py:754-797).  images u8[n_im,H,W,3] BGR, depths f32[n_im,H,W]
    or None, im_idx i32[b] or None, centers f64[b,2], scales f64[b] ->
    (roi_img f32[b,3,out,out] | None, roi_depth f32[b,1,out,out] | None, roi_coord_2d f32[b,2,os,os] | None)."""
    n_im, H, W, _ = images.shape
    b = centers.shape[0]
    dev = images.device
    roi_img = torch.empty((b, 3, out_res, out_res), dtype=torch.float32, device=dev) if want_img else None
    roi_depth = torch.empty((b, 1, out_res, out_res), dtype=torch.float32, device=dev) if depths is not None else None
    roi_c2d = (torch.empty((b, 2, out_res_small, out_res_small), dtype=torch.float32, device=dev)
               if want_coord2d else None)
    mean = (ctypes.c_double * 3)(*[float(v) for v in pixel_mean])
    std = (ctypes.c_double * 3)(*[float(v) for v in pixel_std])
    launch("gdrnpp_crop_resize_roi", dev_ptr(images, torch.uint8, "images"), opt_f32_ptr(depths, "depths"),
           n_im, H, W, dev_ptr(im_idx, torch.int32, "im_idx") if im_idx is not None else None,
           dev_ptr(centers, torch.float64, "centers"), dev_ptr(scales, torch.float64, "scales"),
           roi_img.data_ptr() if want_img else None, roi_depth.data_ptr() if roi_depth is not None else None,
           roi_c2d.data_ptr() if want_coord2d else None, b, out_res, out_res_small,
           ctypes.cast(mean, ctypes.c_void_p), ctypes.cast(std, ctypes.c_void_p))
    return roi_img, roi_depth, roi_c2d


def roi_align(x, rois, output_size, spatial_scale: float = 1.0, sampling_ratio: int = 0, aligned: bool = True):
    """detectron2.layers.ROIAlign(output_size, spatial_scale, sampling_ratio, aligned)(x, rois): x f32[B,C,H,W] (NCHW
    contiguous), rois f32[N,5] -> f32[N,C,oh,ow]."""
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else output_size
    bsz, c, h, w = x.shape
    n = rois.shape[0]
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    launch("gdrnpp_roi_align", f32_ptr(x, "x"), f32_ptr(rois, "rois"), out.data_ptr(), n, c, h, w, oh, ow, float(spatial_scale),
           int(sampling_ratio), 1 if aligned else 0)
    return out


def roi_pool(x, rois, output_size, spatial_scale: float = 1.0):
    """torchvision.ops.RoIPool(output_size, spatial_scale)(x, rois): x f32[B,C,H,W] (NCHW contiguous), rois f32[N,5] ->
    f32[N,C,oh,ow] (max over integer pixel bins)."""
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else output_size
    bsz, c, h, w = x.shape
    n = rois.shape[0]
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    launch("gdrnpp_roi_pool", f32_ptr(x, "x"), f32_ptr(rois, "rois"), out.data_ptr(), n, c, h, w, oh, ow, float(spatial_scale))
    return out


# column -> (torch dtype, trailing shape): the keys and dtypes of roi_stream.roi_host_arrays, in its order
ROI_TABLE_COLUMNS = {
    "center64": (torch.float64, (2,)), "scale64": (torch.float64, ()), "im_idx": (torch.int32, ()), "roi_cls": (torch.int64, ()),
    "roi_cam": (torch.float32, (3, 3)), "roi_center": (torch.float32, (2,)), "roi_wh": (torch.float32, (2,)),
    "scale": (torch.float32, ()), "resize_ratio": (torch.float32, ()), "roi_extent": (torch.float32, (3,)),
    "score": (torch.float32, ()), "roi_id": (torch.int32, ()),
}


def roi_table(cap: int, device) -> dict:
    """An empty ROI table of ``cap`` rows: one device allocation, every column a 16-byte aligned typed view of it."""
    sizes, total = {}, 0
    for k, (dt, tail) in ROI_TABLE_COLUMNS.items():
        n = cap * torch.empty((), dtype=dt).element_size()
        for t in tail:
            n *= t
        total = (total + 15) & ~15
        sizes[k] = (total, n)
        total += n
    raw = torch.zeros((total,), dtype=torch.uint8, device=device)
    return {k: raw[off:off + n].view(ROI_TABLE_COLUMNS[k][0]).reshape((cap,) + ROI_TABLE_COLUMNS[k][1]) for k, (off, n) in sizes.items()}


def rois_from_dets(dets, count, ratio: float, H: int, W: int, cam, extents, dzi_pad_scale: float = 1.5, out_res: int = 64,
                   score_thr: float = 0.0, top_k_per_obj: int = 0, cap: int = 256, table: dict | None = None, counts=None):
    """``gdrnpp_rois_from_dets``: ``yolox_postprocess`` output -> (table, counts).  ``table`` = {column: tensor of ``cap`` rows}
    (``roi_table``; the keys and dtypes of ``roi_stream.roi_host_arrays``), ``counts`` i32[1 + B] = (n_rois, per-image counts);
    rows from n_rois on are not written.  cam f32[3,3] or f32[B,3,3], extents f32[C,3], all on the device."""
    b, max_det, seven = dets.shape
    if seven != 7 or count.numel() != b:
        raise RuntimeError(f"rois_from_dets: dets f32[B,max_det,7] and count i32[B], got {tuple(dets.shape)} and {tuple(count.shape)}")
    if cam.numel() not in (9, 9 * b) or extents.dim() != 2 or extents.shape[1] != 3:
        raise RuntimeError(f"rois_from_dets: cam f32[3,3] or f32[B,3,3], extents f32[C,3], got {tuple(cam.shape)} and {tuple(extents.shape)}")
    table = table if table is not None else roi_table(cap, dets.device)
    if any(table[k].shape[0] != cap for k in ROI_TABLE_COLUMNS):
        raise RuntimeError(f"rois_from_dets: every table column must hold cap = {cap} rows")
    counts = counts if counts is not None else torch.zeros((1 + b,), dtype=torch.int32, device=dets.device)
    nbytes = load().gdrnpp_rois_from_dets_workspace_bytes(b, max_det)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dets.device)
    ctab = gdrnpp_roi_table(**{k: dev_ptr(table[k], ROI_TABLE_COLUMNS[k][0], k) for k in ROI_TABLE_COLUMNS})
    cnt = dev_ptr(counts, torch.int32, "counts")
    launch("gdrnpp_rois_from_dets", f32_ptr(dets, "dets"), dev_ptr(count, torch.int32, "count"), b, max_det, extents.shape[0], float(ratio),
           int(H), int(W), float(dzi_pad_scale), int(out_res), f32_ptr(cam, "cam"), 1 if cam.dim() == 3 else 0,
           f32_ptr(extents, "extents"), float(score_thr), int(top_k_per_obj), int(cap), ctypes.byref(ctab), cnt, cnt + 4,
           ws.data_ptr(), nbytes)
    return table, counts


# key -> (torch dtype, channels or None): the reference's names of read_data_train's targets, batched along dim 0
ROI_TARGET_KEYS = {
    "roi_mask_obj": (torch.float32, None), "roi_mask_visib": (torch.float32, None), "roi_mask_trunc": (torch.float32, None),
    "roi_mask_full": (torch.float32, None), "roi_region": (torch.int32, None), "roi_xyz": (torch.float32, 3),
    "roi_xyz_bin": (torch.uint8, 3),
}
ROI_BIN_MASKS = ("trunc", "visib", "obj", "full")        # LOSS_CFG.XYZ_LOSS_MASK_GT -> bin_mask of gdrnpp_roi_train_targets
ROI_MAX_FPS = 256


def _host_i64(x, n, name, what):
    import numpy as np

    a = np.asarray(x.cpu() if isinstance(x, torch.Tensor) else x)
    if a.shape != (n,) or (n and a.dtype.kind not in "iu"):
        raise RuntimeError(f"{what}: {name} must hold {n} integers, got shape {a.shape} of {a.dtype}")
    return a.astype(np.int64)


def roi_train_targets(packed, table, centers, scales, im_size, *, src=None, masks=None, visib_idx=None, trunc_idx=None, full_idx=None,
                      obj=None, extents=None, fps=None, out_res: int = 64, n_bin: int = 0, bin_mask="visib", want=None, out=None) -> dict:
    """``gdrnpp_roi_train_targets``: the per-ROI targets of read_data_train (data_loader.py:448-612, TRAIN.VIS off) for n ROIs in one
    launch -> {key: device tensor} under the reference's keys (``ROI_TARGET_KEYS``): roi_mask_obj / _visib / _trunc / _full f32[n,o,o],
    roi_region i32[n,o,o], roi_xyz f32[n,3,o,o], roi_xyz_bin u8[n,3,o,o].

    packed f16[px,3] on the device and table i64[m,11] on the host: ``hip_lib.gt_xyz_crops``'s pair (render with ``out=`` to keep the
    pixels on the device; ``XYZ_CROP_COLUMNS``).  src: per ROI the table row it crops (host integers; None: ROI k crops row k).
    centers f64[n,2], scales f64[n], im_size (W, H).  masks u8[n_masks,H,W] on the device with the host columns visib_idx (-1: visib =
    obj), trunc_idx (-1: trunc = visib), full_idx (-1: roi_mask_full is 0); a column left None is all -1.  obj: host integers into extents
    f32[n_obj,3] and fps f64[n_obj,F,3] (device).  n_bin > 0 asks for bins under ``bin_mask`` (a name of ``ROI_BIN_MASKS`` or its index)
    and clips roi_xyz as the reference does.  want: the keys to compute; None = the masks (roi_mask_full when full_idx is given), roi_region
    when fps is given, roi_xyz when extents is given, roi_xyz_bin when n_bin > 0.  out: {key: tensor} to write into instead of allocating.
    Everything the kernel indexes with is checked here on the host, before it is uploaded in one copy."""
    import numpy as np

    what = "roi_train_targets"
    W, H = int(im_size[0]), int(im_size[1])
    dev = packed.device
    ppx = dev_ptr(packed, torch.float16, "packed")
    if packed.numel() % 3:
        raise RuntimeError(f"{what}: packed must hold 3 values per pixel, got {tuple(packed.shape)}")
    n_px = packed.numel() // 3
    table = np.asarray(table.cpu() if isinstance(table, torch.Tensor) else table)
    if table.ndim != 2 or table.shape[1] != 11 or table.dtype.kind not in "iu":
        raise RuntimeError(f"{what}: table must be the i64[m,11] of gt_xyz_crops, got {table.shape} of {table.dtype}")
    table = table.astype(np.int64)
    n = int(scales.shape[0])
    src = np.arange(n, dtype=np.int64) if src is None else _host_i64(src, n, "src", what)
    if n and (src.min() < 0 or src.max() >= len(table)):
        raise RuntimeError(f"{what}: src must index the {len(table)} rows of table")
    rows = table[src]
    if (rows[:, 0] != 0).any():
        raise RuntimeError(f"{what}: table row {int(src[np.nonzero(rows[:, 0])[0][0]])} is not a served pose (status != 0)")
    bx1, bx2, by1, by2, off = (rows[:, c] for c in (6, 7, 8, 9, 10))
    some = (bx2 >= bx1) & (by2 >= by1)
    box_px = np.where(some, (bx2 - bx1 + 1) * (by2 - by1 + 1), 0)
    if (some & ((bx1 < 0) | (by1 < 0) | (bx2 >= W) | (by2 >= H))).any():
        raise RuntimeError(f"{what}: a pose's box leaves the {W} x {H} image")
    if (some & ((off < 0) | (off + box_px > n_px))).any():
        raise RuntimeError(f"{what}: a pose's box ends beyond the {n_px} pixels of packed")
    n_masks = 0
    if masks is not None:
        dev_ptr(masks, torch.uint8, "masks")
        if masks.dim() != 3 or tuple(masks.shape[1:]) != (H, W):
            raise RuntimeError(f"{what}: masks must be u8[n_masks,{H},{W}], got {tuple(masks.shape)}")
        n_masks = int(masks.shape[0])
    cols = []
    for name, x in (("visib_idx", visib_idx), ("trunc_idx", trunc_idx), ("full_idx", full_idx)):
        c = np.full((n,), -1, np.int64) if x is None else _host_i64(x, n, name, what)
        if n and (c.min() < -1 or c.max() >= n_masks):
            raise RuntimeError(f"{what}: {name} must be -1 or index the {n_masks} masks")
        cols.append(c)
    if isinstance(bin_mask, str):
        if bin_mask not in ROI_BIN_MASKS:
            raise RuntimeError(f"{what}: bin_mask must be one of {ROI_BIN_MASKS}, got {bin_mask!r}")
        bin_mask = ROI_BIN_MASKS.index(bin_mask)
    n_obj, F = 0, 0
    if extents is not None:
        f32_ptr(extents, "extents")
        if extents.dim() != 2 or extents.shape[1] != 3:
            raise RuntimeError(f"{what}: extents must be f32[n_obj,3], got {tuple(extents.shape)}")
        n_obj = int(extents.shape[0])
    if fps is not None:
        dev_ptr(fps, torch.float64, "fps")
        if fps.dim() != 3 or fps.shape[2] != 3 or (extents is not None and fps.shape[0] != n_obj):
            raise RuntimeError(f"{what}: fps must be f64[n_obj,F,3] with the n_obj of extents, got {tuple(fps.shape)}")
        n_obj, F = int(fps.shape[0]), int(fps.shape[1])
        if F > ROI_MAX_FPS:
            raise RuntimeError(f"{what}: F = {F} points per object exceeds {ROI_MAX_FPS}")
    if want is None:
        want = ["roi_mask_obj", "roi_mask_visib", "roi_mask_trunc"] + (["roi_mask_full"] if full_idx is not None else [])
        want += (["roi_region"] if F > 0 else []) + (["roi_xyz"] if extents is not None else []) + (["roi_xyz_bin"] if n_bin > 0 else [])
    want = list(want)
    for k in want:
        if k not in ROI_TARGET_KEYS:
            raise RuntimeError(f"{what}: unknown output {k!r}; the keys are {tuple(ROI_TARGET_KEYS)}")
    if "roi_region" in want and F == 0:
        raise RuntimeError(f"{what}: roi_region needs fps with F > 0")
    if ("roi_xyz" in want or "roi_xyz_bin" in want) and extents is None:
        raise RuntimeError(f"{what}: roi_xyz / roi_xyz_bin need extents")
    if "roi_xyz_bin" in want and not 0 < int(n_bin) <= 255:
        raise RuntimeError(f"{what}: roi_xyz_bin needs 0 < n_bin <= 255, got {n_bin}")
    obj_col = np.zeros((n,), np.int64)
    if any(k in want for k in ("roi_region", "roi_xyz", "roi_xyz_bin")):
        if obj is None:
            raise RuntimeError(f"{what}: obj is needed for roi_region / roi_xyz / roi_xyz_bin")
        obj_col = _host_i64(obj, n, "obj", what)
        if n and (obj_col.min() < 0 or obj_col.max() >= n_obj):
            raise RuntimeError(f"{what}: obj must index the {n_obj} objects of extents / fps")
    o = int(out_res)
    res = {}
    for k in want:
        dt, ch = ROI_TARGET_KEYS[k]
        shape = (n, o, o) if ch is None else (n, ch, o, o)
        if out is not None and k in out:
            dev_ptr(out[k], dt, f"out[{k!r}]")
            if tuple(out[k].shape) != shape:
                raise RuntimeError(f"{what}: out[{k!r}] must have shape {shape}, got {tuple(out[k].shape)}")
            res[k] = out[k]
        else:
            res[k] = torch.empty(shape, dtype=dt, device=dev)
    for x, name, cnt in ((centers, "centers", 2 * n), (scales, "scales", n)):
        dev_ptr(x, torch.float64, name)
        if x.numel() != cnt:
            raise RuntimeError(f"{what}: {name} must hold {cnt} values, got {tuple(x.shape)}")
    if n == 0:
        return res
    # one upload: the offsets i64[n], then as i32 the boxes [n,4] and the columns visib, trunc, full, obj [n] each
    i32 = np.concatenate([np.stack([bx1, by1, bx2, by2], 1).reshape(-1), *cols, obj_col]).astype(np.int32)
    host = np.concatenate([np.where(some, off, 0), i32.view(np.int64)])
    idx = torch.from_numpy(host).to(dev)
    p_i32 = idx.data_ptr() + 8 * n
    ptr = lambda k: res[k].data_ptr() if k in res else None                                    # noqa: E731
    launch("gdrnpp_roi_train_targets", ppx if n_px else None, n_px, idx.data_ptr(), p_i32, masks.data_ptr() if masks is not None else None, n_masks,
           p_i32 + 16 * n, p_i32 + 20 * n, p_i32 + 24 * n, H, W, centers.data_ptr(), scales.data_ptr(), p_i32 + 28 * n,
           extents.data_ptr() if extents is not None else None, n_obj, fps.data_ptr() if fps is not None else None, F, o, int(n_bin),
           int(bin_mask), ptr("roi_mask_obj"), ptr("roi_mask_visib"), ptr("roi_mask_trunc"), ptr("roi_mask_full"), ptr("roi_region"),
           ptr("roi_xyz"), ptr("roi_xyz_bin"), n)
    return res


# the columns of replace_bg's host table (include/gdrnpp_hip.h); scale_x, scale_y and u hold the bits of an fp64
REPLACE_BG_COLUMNS = ("do", "bg_off", "bg_stride", "x0", "y0", "cw", "ch", "dw", "dh", "mode", "scale_x", "scale_y", "cut", "u")
REPLACE_BG_F64 = ("scale_x", "scale_y", "u")
REPLACE_BG_MODES = RESIZE_MODES                                               # cv2.resize's forms: mode = index
REPLACE_BG_CUTS = ("none", "upper", "bottom", "left", "right")                # trunc_mask's branches: cut = index


def replace_bg_table(rows):
    """[{column: value}] -> the i64[B,14] host table of ``replace_bg``; a column left out is 0, the fp64 columns are stored as their bits."""
    import numpy as np

    table = np.zeros((len(rows), len(REPLACE_BG_COLUMNS)), np.int64)
    for b, row in enumerate(rows):
        unknown = set(row) - set(REPLACE_BG_COLUMNS)
        if unknown:
            raise RuntimeError(f"replace_bg_table: unknown columns {sorted(unknown)}; the columns are {REPLACE_BG_COLUMNS}")
        for k, name in enumerate(REPLACE_BG_COLUMNS):
            if name in row:
                table[b, k] = np.float64(row[name]).view(np.int64) if name in REPLACE_BG_F64 else int(row[name])
    return table


def replace_bg(images, masks, bg, table, *, out_mask=None):
    """``gdrnpp_replace_bg``: ``replace_bg`` + ``trunc_mask`` (core/base_data_loader.py:413-478) for B images in one call.

    images u8[B,H,W,3] on the device, composited IN PLACE: wherever the truncated mask is 0 the pixel takes the background's, bytes of
    kept pixels are never written.  masks u8[B,H,W] (non-zero = foreground).  bg: a flat u8 device tensor of decoded backgrounds, 3 bytes
    per pixel, rows dense.  table: host i64[B,14] with the columns ``REPLACE_BG_COLUMNS`` (``replace_bg_table``): per image whether to
    touch it at all, where its background's crop lies in ``bg``, the size and form of the cv2.resize, and the cut with its random draw.
    The library checks every value the kernel indexes with before it uploads the table in one copy; a bad row raises RuntimeError.
    out_mask: the u8[B,H,W] to write mask_trunc into (rows of images with do = 0 are left as they are); None allocates zeros.
    -> (mask_trunc u8[B,H,W] of 0 / 1, flags i32[B]: 1 where a cut met an empty mask and was skipped).  Nothing is read back."""
    import numpy as np

    what = "replace_bg"
    dev_ptr(images, torch.uint8, "images")
    if images.dim() != 4 or images.shape[3] != 3:
        raise RuntimeError(f"{what}: images must be u8[B,H,W,3], got {tuple(images.shape)}")
    B, H, W, _ = (int(v) for v in images.shape)
    dev_ptr(masks, torch.uint8, "masks")
    if tuple(masks.shape) != (B, H, W):
        raise RuntimeError(f"{what}: masks must be u8[{B},{H},{W}], got {tuple(masks.shape)}")
    dev_ptr(bg, torch.uint8, "bg")
    table = np.ascontiguousarray(table.cpu().numpy() if isinstance(table, torch.Tensor) else table)
    if table.shape != (B, len(REPLACE_BG_COLUMNS)) or table.dtype != np.int64:
        raise RuntimeError(f"{what}: table must be a host i64[{B},{len(REPLACE_BG_COLUMNS)}], got {table.shape} of {table.dtype}")
    dev = images.device
    if out_mask is None:
        out_mask = torch.zeros((B, H, W), dtype=torch.uint8, device=dev)
    dev_ptr(out_mask, torch.uint8, "out_mask")
    if tuple(out_mask.shape) != (B, H, W):
        raise RuntimeError(f"{what}: out_mask must be u8[{B},{H},{W}], got {tuple(out_mask.shape)}")
    flags = torch.zeros((B,), dtype=torch.int32, device=dev)
    if B == 0:
        return out_mask, flags
    nbytes = load().gdrnpp_replace_bg_workspace_bytes(B)
    ws = torch.empty(((nbytes + 7) // 8,), dtype=torch.int64, device=dev)
    launch("gdrnpp_replace_bg", images.data_ptr(), masks.data_ptr(), out_mask.data_ptr(), B, H, W, bg.data_ptr() if bg.numel() else None,
           bg.numel(), table.ctypes.data, flags.data_ptr(), ws.data_ptr(), nbytes)
    return out_mask, flags
