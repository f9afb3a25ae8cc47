"""Test-side restatement of the toolkit's ground-truth info and masks (lib/pysixd/scripts/calc_gt_info.py:98-173, calc_gt_masks.py:83-111
with visibility.py:9-54 "bop19" and misc.py:628-647) in NumPy, down to the eleven integers per pose and the two masks that
``gdrnpp_gt_visibility`` returns.  Built on tests/vsd_ref.py: ``render_depth_f64`` (fp64 poses and intrinsics) or ``render_oracle`` (the C
oracle, float32 K and R) for the render, ``dist_im`` for the distance images."""
import numpy as np

from tests import vsd_ref as V

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
EMPTY = [INT_MAX, INT_MAX, INT_MIN, INT_MIN]


def extents(mask, ox=0, oy=0):
    """Inclusive x_min, y_min, x_max, y_max of a boolean image, minus the offset; ``EMPTY`` for an empty one."""
    ys, xs = mask.nonzero()
    if xs.size == 0:
        return list(EMPTY)
    return [int(xs.min()) - ox, int(ys.min()) - oy, int(xs.max()) - ox, int(ys.max()) - oy]


def canvas_K(K, ox, oy):
    """What the scripts hand the renderer: fx, fy, cx + ox, cy + oy."""
    Kr = V.render_K(K)
    Kr[0, 2], Kr[1, 2] = Kr[0, 2] + float(ox), Kr[1, 2] + float(oy)
    return Kr


def gt_visibility_ref(verts, faces, R, t, K, depth, delta, canvas_offset=(0, 0), z_near=1.0, z_far=1e6, render="f64", details=False):
    """One pose -> (info i64[11], mask bool[H,W], visib bool[H,W]).  depth f32[H,W] in mm.  ``details``: also min |d_diff - delta| over
    the silhouette pixels with a depth measurement (inf when there is none)."""
    depth = np.asarray(depth, np.float32)
    H, W = depth.shape
    ox, oy = int(canvas_offset[0]), int(canvas_offset[1])
    ren = V.render_depth_f64 if render == "f64" else V.render_oracle
    large = ren(verts, faces, canvas_K(K, ox, oy), np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3), W + 2 * ox,
                H + 2 * oy, z_near, z_far)
    depth_gt = large[oy:oy + H, ox:ox + W]
    dist_gt, dist_t = V.dist_im(depth_gt, K), V.dist_im(depth, K)
    d_diff = dist_gt.astype(np.float32) - dist_t.astype(np.float32)
    visib = np.logical_and(np.logical_or(d_diff <= np.float32(delta), dist_t == 0), dist_gt > 0)
    mask_large, mask = large > 0, dist_gt > 0
    info = np.array([mask_large.sum(), (dist_t[mask] > 0).sum(), visib.sum()] + extents(mask_large, ox, oy) + extents(visib), np.int64)
    if not details:
        return info, mask, visib
    sel = mask & (dist_t != 0)
    margin = float(np.abs(d_diff[sel].astype(np.float64) - float(np.float32(delta))).min()) if sel.any() else np.inf
    return info, mask, visib, margin


def records_ref(info):
    """calc_gt_info.py:142-172 on rows of eleven integers, with the BOP toolkit's calc_2d_bbox: [x_min, y_min, x_max - x_min, y_max - y_min]."""
    out = []
    for r in np.asarray(info, np.int64).tolist():
        px_all, px_valid, px_visib = r[:3]
        bbox = bbox_visib = [-1, -1, -1, -1]
        if px_visib > 0:
            bbox = [r[3], r[4], r[5] - r[3], r[6] - r[4]]
            bbox_visib = [r[7], r[8], r[9] - r[7], r[10] - r[8]]
        out.append({"px_count_all": px_all, "px_count_valid": px_valid, "px_count_visib": px_visib,
                    "visib_fract": px_visib / float(px_all) if px_all > 0 else 0.0, "bbox_obj": list(bbox), "bbox_visib": list(bbox_visib)})
    return out
