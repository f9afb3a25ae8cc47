"""Test-side NumPy restatement of the reference's xyz_crop generation (core/gdrn_modeling/tools/tless/tless_pbr_1_gen_xyz.py:95-187 with
lib/pysixd/misc.py:381-409, calc_xyz_bp_torch) in the fixed evaluation order csrc/xyz_crop.hip documents: the fp64 render of
tests/vsd_ref.py (``render_depth_f64``, rounded to float32), then per covered pixel in float32, every operand an ``np.float32`` scalar or
array so that nothing is silently promoted,

    gx = f32(x) - f32(cx), gy = f32(y) - f32(cy);  c = ((gx d) / fx, (gy d) / fy, d);  e = c - f32(t)
    xyz_i = (R_0i e_0 + R_1i e_1) + R_2i e_2,  R_ji = f32(R[j][i])

the extents from ``nonzero``, the crop and ``astype(float16)``.  Beside the values, per element, S_i = sum_j |R_ji| |e_j|: the scale of the
rounding error of that three-term dot product, which bounds how far another evaluation order (the reference's einsum) can be."""
import numpy as np

from tests import vsd_ref as V

INT_MAX, INT_MIN = 2 ** 31 - 1, -2 ** 31
EMPTY = [INT_MAX, INT_MAX, INT_MIN, INT_MIN]


def render(verts, faces, K, R, t, W, H, z_near=0.01, z_far=6.5):
    """-> depth f32[H,W], 0 = background: the plain image under fx, fy, cx, cy."""
    return V.render_depth_f64(verts, faces, V.render_K(K), np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3), W, H, z_near,
                              z_far)


def pose_box(verts, K, R, t, W, H, z_near=0.01, z_far=6.5):
    """The conservative pixel box of tile_raster.hpp's stage_vertices_and_box, its fp64 expressions in its order -> [i_lo, i_hi, j_lo, j_hi]
    (inclusive; empty when lo > hi; the whole image once a vertex is nearer than z_near)."""
    K, R, t = V.render_K(K).reshape(9), np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)
    v = np.asarray(verts, np.float32).astype(np.float64)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    X = ((R[0] * x + R[1] * y) + R[2] * z) + t[0]
    Y = ((R[3] * x + R[4] * y) + R[5] * z) + t[1]
    Z = ((R[6] * x + R[7] * y) + R[8] * z) + t[2]
    h0, h1, h2 = (K[0] * X + K[1] * Y) + K[2] * Z, (K[3] * X + K[4] * Y) + K[5] * Z, (K[6] * X + K[7] * Y) + K[8] * Z
    front = h2 >= z_near
    if h2.max() < z_near or h2.min() > z_far or not front.any():
        return [1, 0, 1, 0]
    if h2.min() < z_near:
        return [0, W - 1, 0, H - 1]
    pu, pv = h0 / h2, h1 / h2
    clamp = lambda a, lo, hi: int(min(max(a, float(lo)), float(hi)))   # noqa: E731
    return [clamp(np.ceil(pu.min() - 0.5 - 1e-6), 0, W), clamp(np.floor(pu.max() - 0.5 + 1e-6), -1, W - 1),
            clamp(np.ceil(pv.min() - 0.5 - 1e-6), 0, H), clamp(np.floor(pv.max() - 0.5 + 1e-6), -1, H - 1)]


def backproject(depth, K, R, t):
    """depth f32[H,W] -> (xyz f32[H,W,3], S f32[H,W,3]); background pixels are +0 in both."""
    depth = np.asarray(depth)
    assert depth.dtype == np.float32
    H, W = depth.shape
    K32, R32 = np.asarray(K, np.float64).reshape(3, 3).astype(np.float32), np.asarray(R, np.float64).reshape(3, 3).astype(np.float32)
    t32 = np.asarray(t, np.float64).reshape(3).astype(np.float32)
    gx = np.arange(W).astype(np.float32)[None, :] - K32[0, 2]
    gy = np.arange(H).astype(np.float32)[:, None] - K32[1, 2]
    with np.errstate(all="ignore"):
        e = [(gx * depth) / K32[0, 0] - t32[0], (gy * depth) / K32[1, 1] - t32[1], depth - t32[2]]
        xyz = np.stack([(R32[0, i] * e[0] + R32[1, i] * e[1]) + R32[2, i] * e[2] for i in range(3)], 2)
        S = np.stack([(np.abs(R32[0, i]) * np.abs(e[0]) + np.abs(R32[1, i]) * np.abs(e[1])) + np.abs(R32[2, i]) * np.abs(e[2]) for i in range(3)], 2)
    assert xyz.dtype == np.float32 and S.dtype == np.float32
    covered = depth != 0
    return np.where(covered[..., None], xyz, np.float32(0.0)), np.where(covered[..., None], S, np.float32(0.0))


def xyz_crop_ref(verts, faces, R, t, K, W, H, z_near=0.01, z_far=6.5):
    """One pose -> dict: count, xyxy (``EMPTY`` without a covered pixel), xyz_crop f16[h,w,3] and S f32[h,w,3] over the extents (None when
    empty), and the full-image f16 map ``full`` with its float32 ``S_full`` (what a box of any shape is cut from)."""
    depth = render(verts, faces, K, R, t, W, H, z_near, z_far)
    xyz, S = backproject(depth, K, R, t)
    with np.errstate(over="ignore"):
        full = xyz.astype(np.float16)
    ys, xs = np.nonzero(depth > 0)
    out = dict(count=int(ys.size), xyxy=list(EMPTY), xyz_crop=None, S=None, full=full, S_full=S, depth=depth)
    if ys.size:
        x1, y1, x2, y2 = int(xs.min()), int(ys.min()), int(xs.max()), int(ys.max())
        out.update(xyxy=[x1, y1, x2, y2], xyz_crop=full[y1:y2 + 1, x1:x2 + 1], S=S[y1:y2 + 1, x1:x2 + 1])
    return out


def record(ref, W, H):
    """The tool's record of a pose (:128-171): the crop and its extents, or for an invisible instance the full-image zeros."""
    if ref["count"] == 0:
        return {"xyz_crop": np.zeros((H, W, 3), np.float16), "xyxy": [0, 0, W - 1, H - 1]}
    return {"xyz_crop": ref["xyz_crop"], "xyxy": list(ref["xyxy"])}


def ulp16(a):
    """The spacing of float16 at |a| (the subnormal spacing 2^-24 below 2^-14)."""
    a = np.abs(np.asarray(a, np.float64))
    with np.errstate(divide="ignore"):
        ex = np.floor(np.log2(np.where(a > 0, a, 1.0)))
    return np.exp2(np.maximum(ex, -14.0) - 10.0)


def within_bound(ours, ref, S):
    """|ours - ref| <= 7 2^-24 S + ulp16(max(|ours|, |ref|)) per element -> (bool array, the worst ratio of difference to bound)."""
    a, b = np.asarray(ours, np.float64), np.asarray(ref, np.float64)
    bound = 7.0 * 2.0 ** -24 * np.asarray(S, np.float64) + ulp16(np.maximum(np.abs(a), np.abs(b)))
    diff = np.abs(a - b)
    return diff <= bound, float((diff / bound).max()) if diff.size else 0.0
