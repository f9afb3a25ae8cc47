"""Test-side restatement of BOP19 VSD (lib/pysixd/pose_error.py:22-128 with visibility.py:9-74 "bop19" and misc.py:604-647) in NumPy,
down to the integer pixel counts that ``gdrnpp_vsd_counts`` returns, and of the raster rule of oracle/raster_oracle.c in fp64 NumPy.

``render_depth_f64`` exists because the C oracle takes float32 K and R, while real ground-truth poses and intrinsics are not
float32-representable: it evaluates the oracle's expressions in the oracle's order (NumPy rounds every operation, no FMA), vectorised
per triangle over its candidate box, and equals ``oracle.postproc.render_depth`` bit for bit where K and R are float32 values
(tests/test_vsd_cpu.py)."""
import numpy as np


def _cross3(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _clampi(v, lo, hi):
    return int(min(max(v, float(lo)), float(hi)))


def render_depth_f64(verts, faces, K, R, t, res_w, res_h, z_near=0.1, z_far=100.0):
    """verts f32[V,3], faces i32[F,3], K, R fp64 3x3, t fp64[3] -> depth f32[res_h,res_w], 0 = background."""
    K, R, t = np.asarray(K, np.float64).reshape(9), np.asarray(R, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)
    v = np.asarray(verts, np.float32).astype(np.float64)
    faces = np.asarray(faces).reshape(-1, 3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    X = ((R[0] * x + R[1] * y) + R[2] * z) + t[0]
    Y = ((R[3] * x + R[4] * y) + R[5] * z) + t[1]
    Z = ((R[6] * x + R[7] * y) + R[8] * z) + t[2]
    h = np.stack([(K[0] * X + K[1] * Y) + K[2] * Z, (K[3] * X + K[4] * Y) + K[5] * Z, (K[6] * X + K[7] * Y) + K[8] * Z], 1)
    depth = np.full((res_h, res_w), np.inf, np.float32)
    with np.errstate(all="ignore"):
        for f in faces:
            h0, h1, h2 = h[f[0]], h[f[1]], h[f[2]]
            e0, e1, e2 = _cross3(h1, h2), _cross3(h2, h0), _cross3(h0, h1)
            D = (h0[0] * e0[0] + h0[1] * e0[1]) + h0[2] * e0[2]
            if not D != 0.0:
                continue
            zmin, zmax = min(h0[2], h1[2], h2[2]), max(h0[2], h1[2], h2[2])
            us, vs = [], []
            if zmin >= z_near:
                us, vs = [h0[0] / h0[2], h1[0] / h1[2], h2[0] / h2[2]], [h0[1] / h0[2], h1[1] / h1[2], h2[1] / h2[2]]
            else:
                hv = (h0, h1, h2)
                for e in range(3):
                    a, b = hv[e], hv[(e + 1) % 3]
                    ain, bin_ = a[2] >= z_near, b[2] >= z_near
                    if ain:
                        us.append(a[0] / a[2]); vs.append(a[1] / a[2])
                    if ain != bin_:
                        tt = (z_near - a[2]) / (b[2] - a[2])
                        us.append((a[0] + tt * (b[0] - a[0])) / z_near); vs.append((a[1] + tt * (b[1] - a[1])) / z_near)
            if zmax < z_near or zmin > z_far or not us:
                continue
            umin, umax, vmin, vmax = min(us), max(us), min(vs), max(vs)
            if not umin <= umax:
                continue
            i_lo, i_hi = _clampi(np.floor(umin - 0.5), 0, res_w), _clampi(np.ceil(umax - 0.5), -1, res_w - 1)
            j_lo, j_hi = _clampi(np.floor(vmin - 0.5), 0, res_h), _clampi(np.ceil(vmax - 0.5), -1, res_h - 1)
            if i_lo > i_hi or j_lo > j_hi:
                continue
            u = np.arange(i_lo, i_hi + 1, dtype=np.float64)[None, :] + 0.5
            w = np.arange(j_lo, j_hi + 1, dtype=np.float64)[:, None] + 0.5
            w0 = (e0[0] * u + e0[1] * w) + e0[2]
            w1 = (e1[0] * u + e1[1] * w) + e1[2]
            w2 = (e2[0] * u + e2[1] * w) + e2[2]
            inside = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
            s = (w0 + w1) + w2
            Zp = D / s
            ok = inside & (s != 0.0) & (Zp >= z_near) & (Zp <= z_far)
            zf = np.where(ok, Zp, np.inf).astype(np.float32)
            win = depth[j_lo:j_hi + 1, i_lo:i_hi + 1]
            np.minimum(win, zf, out=win)
    depth[np.isinf(depth)] = 0.0
    return depth


def render_K(K):
    """What the toolkit's renderer sees of K: fx, fy, cx, cy (pose_error.py:60-64)."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    return np.array([[K[0, 0], 0.0, K[0, 2]], [0.0, K[1, 1], K[1, 2]], [0.0, 0.0, 1.0]])


def render_oracle(verts, faces, K, R, t, res_w, res_h, z_near, z_far):
    """The C oracle; K and R must be float32 values."""
    from oracle import postproc as O

    K, R = np.asarray(K, np.float64), np.asarray(R, np.float64)
    assert np.array_equal(K.astype(np.float32), K) and np.array_equal(R.astype(np.float32), R), "the C oracle takes float32 K and R"
    return O.render_depth(verts, faces, K, R, t, res_w, res_h, z_near, z_far)


def dist_im(depth, K):
    """misc.depth_im_to_dist_im_fast, the same NumPy expressions."""
    K = np.asarray(K, np.float64).reshape(3, 3)
    xs, ys = np.meshgrid(np.arange(depth.shape[1]), np.arange(depth.shape[0]))
    pre_Xs = (xs - K[0, 2]) / np.float64(K[0, 0])
    pre_Ys = (ys - K[1, 2]) / np.float64(K[1, 1])
    return np.sqrt(np.multiply(pre_Xs, depth) ** 2 + np.multiply(pre_Ys, depth) ** 2 + depth.astype(np.float64) ** 2)


def counts_from_depths(depth_e, depth_g, depth_t, K, delta, taus, diameter, details=False):
    """-> i64[2 + n_tau] = union, inter, cost_k, from the three depth images (f32[H,W]).  ``details``: also the margins of the
    comparisons, (min |d_diff - delta| over both masks, min |dist / diameter - tau| / tau over the intersection)."""
    depth_t = np.asarray(depth_t, np.float32)
    dist_t, dist_g, dist_e = dist_im(depth_t, K), dist_im(depth_g, K), dist_im(depth_e, K)
    delta32 = np.float32(delta)
    diff_g = dist_g.astype(np.float32) - dist_t.astype(np.float32)
    diff_e = dist_e.astype(np.float32) - dist_t.astype(np.float32)
    visib_g = np.logical_and(np.logical_or(diff_g <= delta32, dist_t == 0), dist_g > 0)
    visib_e = np.logical_and(np.logical_or(diff_e <= delta32, dist_t == 0), dist_e > 0)
    visib_e = np.logical_or(visib_e, np.logical_and(visib_g, dist_e > 0))
    inter, union = np.logical_and(visib_g, visib_e), np.logical_or(visib_g, visib_e)
    dists = np.abs(dist_g[inter] - dist_e[inter]) / np.float64(diameter)
    out = np.array([union.sum(), inter.sum()] + [(dists >= tau).sum() for tau in taus], np.int64)
    if not details:
        return out
    m_delta = np.inf
    for diff, dist in ((diff_g, dist_g), (diff_e, dist_e)):
        sel = (dist > 0) & (dist_t != 0)
        if sel.any():
            m_delta = min(m_delta, float(np.abs(diff[sel].astype(np.float64) - float(delta32)).min()))
    m_tau = min([float((np.abs(dists - tau) / tau).min()) for tau in taus], default=np.inf) if dists.size else np.inf
    return out, m_delta, m_tau


def vsd_counts_ref(verts, faces, R_est, t_est, R_gt, t_gt, K, depth_t, delta, taus, diameter, z_near=1.0, z_far=1e6, render="f64",
                   details=False):
    """One pair.  render: "f64" (``render_depth_f64``) or "oracle" (oracle/raster_oracle.c; float32 K and R only)."""
    H, W = depth_t.shape
    ren = render_depth_f64 if render == "f64" else render_oracle
    Kr = render_K(K)
    d_e = ren(verts, faces, Kr, np.asarray(R_est, np.float64).reshape(3, 3), np.asarray(t_est, np.float64).reshape(3), W, H, z_near, z_far)
    d_g = ren(verts, faces, Kr, np.asarray(R_gt, np.float64).reshape(3, 3), np.asarray(t_gt, np.float64).reshape(3), W, H, z_near, z_far)
    return counts_from_depths(d_e, d_g, depth_t, K, delta, taus, diameter, details)


def errors_from_counts(c):
    """pose_error.py:110-126: i[..., 2 + n_tau] -> f64[..., n_tau]; 1.0 where union is 0, NaN where the row is -1."""
    c = np.asarray(c, np.int64)
    union, inter = c[..., 0:1], c[..., 1:2]
    with np.errstate(all="ignore"):
        e = (c[..., 2:] + (union - inter)) / union.astype(np.float64)
    e = np.where(union == 0, 1.0, e)
    return np.where(union < 0, np.nan, e)
