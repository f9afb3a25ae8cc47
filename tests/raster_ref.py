"""Plain NumPy fp64 reference of the depth rasteriser (csrc/raster.hpp) WITHOUT a candidate box: every pixel centre is tested
against every triangle.  oracle/raster_oracle.c restates raster.hpp's box with the same expressions, so a mistake in the box
logic (the 1e-6 / 1e-3 px widenings, the near-plane clipping, the far-plane drop) would be shared by kernel and oracle; this
module is the judge that has no box, no clipping and no early-out to share.

Arithmetic, in the evaluation order of raster.hpp (NumPy's element-wise double operations do not fuse):

    project_vertex   X = ((R0 x + R1 y) + R2 z) + t0 ...;  h = ((K0 X + K1 Y) + K2 Z) ...
    cross3           e0 = h1 x h2, e1 = h2 x h0, e2 = h0 x h1;  D = (h0x e0x + h0y e0y) + h0z e0z
    sample_triangle  w_k = (e_k0 u + e_k1 v) + e_k2 at (u, v) = (i + 0.5, j + 0.5);  Z = D / ((w0 + w1) + w2)
    coverage         all w >= 0 or all w <= 0, sum != 0, D != 0, z_near <= Z <= z_far
    depth            the minimum of float32(Z) per pixel, background 0
    xyz              float32((l0 v0 + l1 v1) + l2 v2), l_k = w_k / sum, of the lowest face id among equal float-Z values
                     (the device's 64-bit key is (Z bits << 32) | face id; Z >= z_near > 0, so equal values are equal bits)
"""
import numpy as np

_CHUNK = 256        # faces per pass: _CHUNK x res^2 doubles per temporary


def project(verts, K, R, t):
    """-> h f64[V,3], the homogeneous pixel-space vertices (K, R float32 values widened, t float64)."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    K = np.asarray(K, np.float32).astype(np.float64).reshape(9)
    R = np.asarray(R, np.float32).astype(np.float64).reshape(9)
    t = np.asarray(t, np.float64).reshape(3)
    x, y, z = v[:, 0], v[:, 1], v[:, 2]
    X = ((R[0] * x + R[1] * y) + R[2] * z) + t[0]
    Y = ((R[3] * x + R[4] * y) + R[5] * z) + t[1]
    Z = ((R[6] * x + R[7] * y) + R[8] * z) + t[2]
    return np.stack([(K[0] * X + K[1] * Y) + K[2] * Z, (K[3] * X + K[4] * Y) + K[5] * Z, (K[6] * X + K[7] * Y) + K[8] * Z], 1)


def _cross(a, b):
    return np.stack([a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]], 1)


def edge_planes(h, faces):
    """-> e0, e1, e2 f64[F,3], D f64[F]."""
    h0, h1, h2 = h[faces[:, 0]], h[faces[:, 1]], h[faces[:, 2]]
    e0, e1, e2 = _cross(h1, h2), _cross(h2, h0), _cross(h0, h1)
    D = (h0[:, 0] * e0[:, 0] + h0[:, 1] * e0[:, 1]) + h0[:, 2] * e0[:, 2]
    return e0, e1, e2, D


def _weights(e, u, v):
    return (e[:, 0:1] * u + e[:, 1:2] * v) + e[:, 2:3]


def _covered(verts, faces, K, R, t, res, zn, zf):
    """Per chunk of faces: (first face id, covered bool[Fc,P], Z f64[Fc,P]) plus what xyz needs."""
    h = project(verts, K, R, t)
    e0, e1, e2, D = edge_planes(h, faces)
    jj, ii = np.divmod(np.arange(res * res), res)
    u, v = (ii.astype(np.float64) + 0.5)[None], (jj.astype(np.float64) + 0.5)[None]

    def chunks():
        with np.errstate(all="ignore"):
            for f0 in range(0, len(faces), _CHUNK):
                s = slice(f0, f0 + _CHUNK)
                w0, w1, w2 = _weights(e0[s], u, v), _weights(e1[s], u, v), _weights(e2[s], u, v)
                cov = ((w0 >= 0) & (w1 >= 0) & (w2 >= 0)) | ((w0 <= 0) & (w1 <= 0) & (w2 <= 0))
                tot = (w0 + w1) + w2
                Z = D[s, None] / tot
                yield f0, cov & (tot != 0) & (D[s, None] != 0) & (Z >= zn) & (Z <= zf), Z

    return chunks(), (e0, e1, e2), u[0], v[0]


def render(verts, faces, K, R, t, res, z_near=0.1, z_far=100.0, want_xyz=False, want_face=False):
    """-> depth f32[res,res] (, xyz f32[res,res,3]) (, face i32[res,res], -1 = background).  z_near / z_far are used as the
    doubles given: pass float32 values where the kernel is the other side (it widens its float arguments)."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    chunks, (e0, e1, e2), u, v = _covered(verts, faces, K, R, t, res, float(z_near), float(z_far))
    best = np.full(res * res, np.inf, np.float32)
    face = np.full(res * res, -1, np.int64)
    for f0, cov, Z in chunks:
        zf32 = np.where(cov, Z, np.inf).astype(np.float32)
        k = zf32.argmin(0)                                  # first minimum = lowest face id of the chunk
        zmin = zf32[k, np.arange(res * res)]
        better = zmin < best                                # strict: an earlier chunk's equal depth keeps its lower id
        best[better] = zmin[better]
        face[better] = f0 + k[better]
    hit = np.isfinite(best)
    depth = np.where(hit, best, np.float32(0)).astype(np.float32).reshape(res, res)
    out = [depth]
    if want_xyz:
        xyz = np.zeros((res * res, 3), np.float32)
        p = np.flatnonzero(hit)
        f = face[p]
        w = [(e[f, 0] * u[p] + e[f, 1] * v[p]) + e[f, 2] for e in (e0, e1, e2)]
        tot = (w[0] + w[1]) + w[2]
        lam = [wk / tot for wk in w]
        vv = [verts[faces[f, c]].astype(np.float64) for c in range(3)]
        xyz[p] = ((lam[0][:, None] * vv[0] + lam[1][:, None] * vv[1]) + lam[2][:, None] * vv[2]).astype(np.float32)
        out.append(xyz.reshape(res, res, 3))
    if want_face:
        out.append(face.astype(np.int32).reshape(res, res))
    return out[0] if len(out) == 1 else tuple(out)


def covering_faces(verts, faces, K, R, t, res, z_near=0.1, z_far=100.0):
    """-> i32[res,res]: how many faces attain the pixel's float32 minimum depth (ties the lowest face id has to win)."""
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    depth = render(verts, faces, K, R, t, res, z_near, z_far).reshape(-1)
    chunks = _covered(np.asarray(verts, np.float32), faces, K, R, t, res, float(z_near), float(z_far))[0]
    n = np.zeros(res * res, np.int32)
    for _, cov, Z in chunks:
        with np.errstate(all="ignore"):
            n += (cov & (Z.astype(np.float32) == depth[None])).sum(0).astype(np.int32)
    return n.reshape(res, res)
