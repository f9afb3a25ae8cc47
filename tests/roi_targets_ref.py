"""NumPy restatement of the per-instance target path of ``GDRN_DatasetFromList.read_data_train`` (reference
core/gdrn_modeling/datasets/data_loader.py:448-612 with TRAIN.VIS and INPUT.SMOOTH_XYZ off), the yardstick of
``hip_lib.roi_train_targets`` and ``gdrn_modeling.train_targets``.  It materialises what the reference materialises: the crop pasted
into a zeroed full image, the full-image float masks, one nearest-neighbour ``warpAffine`` per map (``oracle.postproc.warp_affine``, the
restatement of OpenCV), then ``xyz_to_region`` (core/utils/data_utils.py:267-280) with scipy's ``cdist`` written out as the explicit fp64
expression sqrt((dx dx + dy dy) + dz dz), the normalisation, the clipping and the bins.  No scipy: it may be absent where the GPU tests run."""
import numpy as np

from oracle import postproc as P

BIN_MASKS = ("trunc", "visib", "obj", "full")


def paste(rec, W, H):
    """:449-454 -> the full-image float32 map of a record {"xyz_crop": f16[h,w,3], "xyxy": [x1, y1, x2, y2]}."""
    x1, y1, x2, y2 = (int(v) for v in rec["xyxy"])
    xyz = np.zeros((H, W, 3), dtype=np.float32)
    xyz[y1:y2 + 1, x1:x2 + 1, :] = rec["xyz_crop"]
    return xyz


def region_of(roi_xyz, fps_points):
    """xyz_to_region: roi_xyz f32[h,w,3], fps_points [F,3] -> int64[h,w], 1..F on the object, 0 on the background."""
    bh, bw = roi_xyz.shape[:2]
    mask = ((roi_xyz[:, :, 0] != 0) | (roi_xyz[:, :, 1] != 0) | (roi_xyz[:, :, 2] != 0)).astype("uint8")
    a = roi_xyz.reshape(bh * bw, 3).astype(np.float64)
    b = np.asarray(fps_points, np.float64)
    dx, dy, dz = (a[:, None, c] - b[None, :, c] for c in range(3))
    dists = np.sqrt((dx * dx + dy * dy) + dz * dz)
    return mask * (np.argmin(dists, axis=1).reshape(bh, bw) + 1)


def roi_targets_ref(xyz, center, scale, out_res, *, visib=None, trunc=None, full=None, extent=None, fps=None, n_bin=0, bin_mask="visib"):
    """One instance.  xyz f32[H,W,3] (``paste``); visib / trunc / full: full-image masks (any dtype, non-zero = 1) or None = the index -1
    of the kernel (visib = obj; trunc = visib; roi_mask_full all zero).  -> dict under the reference's keys: roi_mask_obj / _visib /
    _trunc / _full f32[o,o], roi_region i32[o,o] (with fps), roi_xyz f32[3,o,o] (with extent; clipped when n_bin > 0), roi_xyz_bin
    u8[3,o,o] (n_bin > 0)."""
    H, W = xyz.shape[:2]
    mask_obj = ((xyz[:, :, 0] != 0) | (xyz[:, :, 1] != 0) | (xyz[:, :, 2] != 0)).astype(bool).astype(np.float32)
    one = lambda m: (np.asarray(m) != 0).astype(np.float32)             # noqa: E731
    mask_visib = mask_obj if visib is None else one(visib) * mask_obj
    mask_trunc = mask_visib if trunc is None else mask_visib * one(trunc)
    M = P.get_affine_transform(center, scale, out_res)
    warp = lambda m: P.warp_affine(np.ascontiguousarray(m, np.float32), M, out_res, nearest=True)      # noqa: E731
    out = dict(roi_mask_trunc=warp(mask_trunc), roi_mask_visib=warp(mask_visib), roi_mask_obj=warp(mask_obj),
               roi_mask_full=warp(one(full)) if full is not None else np.zeros((out_res, out_res), np.float32))
    roi_xyz = warp(xyz)
    if fps is not None and len(fps):
        out["roi_region"] = region_of(roi_xyz, fps).astype(np.int32)
    if extent is None:
        return out
    ext = np.asarray(extent, np.float32)
    roi_xyz = np.ascontiguousarray(roi_xyz.transpose(2, 0, 1))
    for c in range(3):
        roi_xyz[c] = roi_xyz[c] / ext[c] + np.float32(0.5)
    if n_bin > 0:
        bins = np.zeros_like(roi_xyz)
        sel = out["roi_mask_" + (bin_mask if isinstance(bin_mask, str) else BIN_MASKS[bin_mask])]
        for c in range(3):
            v = roi_xyz[c]
            v[v < 0] = 0
            v[v > np.float32(0.999999)] = np.float32(0.999999)
            bins[c] = np.asarray(v * np.float32(n_bin), dtype=np.uint8)
            bins[c][sel == 0] = n_bin
        out["roi_xyz_bin"] = bins.astype("uint8")
    out["roi_xyz"] = roi_xyz
    return out


def aug_bbox_dzi_ref(bbox_xyxy, im_H, im_W, dzi_type, pad_scale, scale_ratio, shift_ratio, rng):
    """aug_bbox_DZI's uniform and plain branches (core/base_data_loader.py:188-231) drawing from ``rng`` (np.random.RandomState)."""
    x1, y1, x2, y2 = bbox_xyxy
    cx, cy = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
    bh, bw = y2 - y1, x2 - x1
    if dzi_type == "uniform":
        s = 1 + scale_ratio * (2 * rng.random_sample() - 1)
        sh = shift_ratio * (2 * rng.random_sample(2) - 1)
        center = np.array([cx + bw * sh[0], cy + bh * sh[1]])
        scale = max(y2 - y1, x2 - x1) * s * pad_scale
    else:
        center = np.array([cx, cy])
        scale = max(y2 - y1, x2 - x1)
    return center, min(scale, max(im_H, im_W)) * 1.0


def batch_ref(packed, table, centers, scales, im_size, *, src=None, masks=None, visib_idx=None, trunc_idx=None, full_idx=None, obj=None,
              extents=None, fps=None, out_res=64, n_bin=0, bin_mask="visib", want=None, out=None):
    """``hip_lib.roi_train_targets`` on host arrays, ROI after ROI through ``roi_targets_ref``: the same arguments (NumPy instead of device
    tensors), the same keys and default ``want`` -> {key: stacked array}."""
    W, H = int(im_size[0]), int(im_size[1])
    packed = np.asarray(packed).reshape(-1, 3)
    n = len(scales)
    src = np.arange(n) if src is None else np.asarray(src)
    col = lambda c: np.full((n,), -1) if c is None else np.asarray(c)            # noqa: E731
    vi, ti, fi = col(visib_idx), col(trunc_idx), col(full_idx)
    F = 0 if fps is None else np.shape(fps)[1]
    if want is None:
        want = ["roi_mask_obj", "roi_mask_visib", "roi_mask_trunc"] + (["roi_mask_full"] if full_idx is not None else [])
        want += (["roi_region"] if F > 0 else []) + (["roi_xyz"] if extents is not None else []) + (["roi_xyz_bin"] if n_bin > 0 else [])
    shapes = {"roi_xyz": ((3, out_res, out_res), np.float32), "roi_xyz_bin": ((3, out_res, out_res), np.uint8), "roi_region": ((out_res, out_res), np.int32)}
    res = {k: np.zeros((n,) + shapes.get(k, ((out_res, out_res), np.float32))[0], shapes.get(k, (None, np.float32))[1]) for k in want}
    for k in range(n):
        row = [int(v) for v in np.asarray(table)[src[k]]]
        x1, x2, y1, y2, off = row[6:11]
        xyz = np.zeros((H, W, 3), np.float32)
        if x2 >= x1 and y2 >= y1:
            bw, bh = x2 - x1 + 1, y2 - y1 + 1
            xyz[y1:y2 + 1, x1:x2 + 1] = packed[off:off + bw * bh].reshape(bh, bw, 3)
        m = lambda i: None if i < 0 else np.asarray(masks[i])                    # noqa: E731
        one = roi_targets_ref(xyz, np.asarray(centers)[k], float(np.asarray(scales)[k]), out_res, visib=m(vi[k]), trunc=m(ti[k]), full=m(fi[k]),
                              extent=None if extents is None or obj is None else np.asarray(extents)[obj[k]],
                              fps=None if fps is None or obj is None else np.asarray(fps)[obj[k]], n_bin=n_bin, bin_mask=bin_mask)
        for key in want:
            res[key][k] = one[key]
    return res
