"""Case builders for depth_refine_kernel / render_depth_kernel (csrc/depth_refine.hip) at their queue, stage and size edges,
shared by tests/test_gpu_refine_edges.py (kernel against oracle/postproc.py) and tests/test_refine_edge_cases_cpu.py (plain
reference tests/raster_ref.py against the oracle, and the preconditions that make each case reach what it is named for).  Plain
helper module: no fixtures; builders are cached and their arrays are read-only.

The limits are read out of depth_refine.hip, so a retune moves the cases with it:

    kLargeArea              box pixel centres above which a triangle goes to the LDS queue and is rasterised by a whole wave
    kMaxLargeS              slots of that queue; triangles beyond it are rasterised by their own lane (overflow)
    kMaxStagedVerts         largest mesh whose transformed vertices live in LDS; above it the workspace kernel runs
    GDRNPP_REFINE_THREADS   threads of a refine workgroup: a thread owns pixels tid, tid + threads, ...
    kT                      threads of a render_depth workgroup: faces are taken kT at a time

Every refine case is a ``SimpleNamespace`` of: verts, faces (lists, one per object), obj i32[b], coor_x / coor_y / coor_z / mask
f32[b,1,res,res], roi_depth f32[b,1,4res,4res], cam f32[b,3,3], center f32[b,2], scale f32[b], K_crop f32[b,3,3] (= zoom_K of
those), R f32[b,3,3], t_in f32[b,3], res, iters, threshold, mask_type, z_near, z_far (float32 values) and ``kernel_only``: ROIs
whose mask the reference cannot normalise (see nan_mask_roi).
"""
import os
import re
from functools import lru_cache
from types import SimpleNamespace

import numpy as np

from gdrnpp_bop2022_amd import synthetic as S
from oracle import postproc as P

_SRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gdrnpp_bop2022_amd", "csrc", "depth_refine.hip")


def _constant(name, text):
    m = re.search(r"(?:constexpr\s+int\s+%s\s*=|#define\s+%s)\s+(\d+)" % (name, name), text)
    assert m, f"{name} not found in depth_refine.hip"
    return int(m.group(1))


with open(_SRC) as _f:
    _TEXT = _f.read()
LARGE_AREA = _constant("kLargeArea", _TEXT)
MAX_LARGE = _constant("kMaxLargeS", _TEXT)
MAX_STAGED = _constant("kMaxStagedVerts", _TEXT)
REFINE_THREADS = _constant("GDRNPP_REFINE_THREADS", _TEXT)
RENDER_THREADS = _constant("kT", _TEXT)
STAGE_BYTES = _constant("kStageBytes", _TEXT)
MAX_PIX = _constant("kMaxPix", _TEXT)

STABLE_MARGIN = 1e-4            # no pixel's q within this fraction of qmax of the threshold: the selected set cannot flip
f32 = np.float32


def _frozen(case):
    for v in vars(case).values():
        for a in (v if isinstance(v, list) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return case


# ------------------------------------------------------------------------------------------------------------- meshes
def ellipsoid(subdiv, semi=(0.05, 0.04, 0.045)):
    v, f = S.icosphere(subdiv)
    return (v * np.asarray(semi)).astype(f32), f.astype(np.int32)


GRID = 8                        # cells per side of a layer: 2 * GRID^2 = 128 triangles, (GRID + 1)^2 = 81 vertices


def layered_grid(n_faces, seed=0, half=0.048):
    """Layers of GRID x GRID cells (two triangles each) 4 mm apart, later layers nearer, with +-20 mm of per-vertex z jitter, so that
    different layers win different pixels and the last triangles of the list matter most; the first ``n_faces`` triangles.  At f = 300 px, t_z = 0.5 a cell spans 6.3 to 7.7 px and the grid stays inside
    the crop: every triangle's box holds at least 6 x 6 centres, more than kLargeArea."""
    rng = np.random.default_rng([31, seed])
    per = 2 * GRID * GRID
    layers = -(-n_faces // per)
    g = np.linspace(-half, half, GRID + 1)
    verts, faces = [], []
    for layer in range(layers):
        x, y = np.meshgrid(g, g)
        z = -0.004 * layer + rng.uniform(-0.02, 0.02, x.shape)
        base = layer * (GRID + 1) ** 2
        verts.append(np.stack([x, y, z], -1).reshape(-1, 3))
        for j in range(GRID):
            for i in range(GRID):
                a = base + j * (GRID + 1) + i
                b, c, d = a + 1, a + GRID + 2, a + GRID + 1
                faces += [(a, b, c), (a, c, d)]
    return np.concatenate(verts).astype(f32), np.asarray(faces[:n_faces], np.int32)


STAGE_BASE_SUBDIV = 4           # 2562 vertices / 5120 faces


def stage_mesh(n_verts):
    """The subdiv-4 ellipsoid plus a flat zigzag ribbon of small triangles in its equatorial plane, 10 to 25 % outside the surface
    (the silhouette's rim when seen along the object's z axis), that brings the vertex count to exactly ``n_verts``.  The ribbon's vertices are the
    LAST ones: the highest staged index, next to the padding of an odd count, belongs to visible triangles."""
    v, f = ellipsoid(STAGE_BASE_SUBDIV)
    extra = n_verts - len(v)
    assert extra >= 3
    th = 2 * np.pi * np.arange(extra) / extra
    rad = 1.10 + 0.15 * (np.arange(extra) % 2)
    rib = np.stack([0.05 * rad * np.cos(th), 0.04 * rad * np.sin(th), np.zeros(extra)], 1)
    k = len(v) + np.arange(extra - 2)
    return (np.concatenate([v, rib.astype(f32)]), np.concatenate([f, np.stack([k, k + 1, k + 2], 1).astype(np.int32)]))


def lattice_mesh():
    """Vertices on a 1/128 grid in the plane z = 0 (and 1/64 in z = 1), for K = [[64, 0, 32], [0, 64, 32], [0, 0, 1]], R = I,
    t = (0, 0, 1): a vertex (x, y, 0) projects to (64 x + 32, 64 y + 32) exactly, one at depth 2 to (32 x + 32, 32 y + 32).
    ``px(i, j)`` puts a vertex on the centre of pixel (column i, row j).

      faces  0..71    6 x 6 quads of 4 px, two triangles each, corners ON pixel centres: every edge runs through a row, a column
                      or a diagonal of centres (edge functions exactly 0 there), shared edges are covered by both neighbours
             72..79   copies of faces 0..7 on vertices of their own: equal depth over whole triangles, the lower id must win
             80, 81   zero-area: three collinear centres; two identical corners
             82       corners on pixel CORNERS (integer coordinates): edges pass between centres
             83       reaches 4.5 px left of and above the crop: the clamp at 0
             84       a large triangle at depth 2 behind everything, corners on centres (queue / ballot path)
             85       umin, vmin exactly on the centre of the last column / row's neighbour: box edge on a centre at the border
    """
    def px(i, j, z=0.0):
        s = 64.0 if z == 0.0 else 32.0
        return ((i + 0.5 - 32.0) / s, (j + 0.5 - 32.0) / s, z)

    verts, faces = [], []
    for b in range(7):
        for a in range(7):
            verts.append(px(8 + 4 * a, 8 + 4 * b))
    for b in range(6):
        for a in range(6):
            v0 = 7 * b + a
            faces += [(v0, v0 + 1, v0 + 8), (v0, v0 + 8, v0 + 7)]
    for k in range(8):
        base = len(verts)
        verts += [verts[i] for i in faces[k]]
        faces.append((base, base + 1, base + 2))
    base = len(verts)
    verts += [px(40, 8), px(44, 8), px(52, 8)]
    faces.append((base, base + 1, base + 2))
    faces.append((base, base, base + 2))
    base = len(verts)
    verts += [px(39.5, 39.5), px(47.5, 39.5), px(39.5, 49.5)]
    faces.append((base, base + 1, base + 2))
    base = len(verts)
    verts += [px(-5, -5), px(6, 2), px(2, 6)]
    faces.append((base, base + 1, base + 2))
    base = len(verts)
    verts += [px(36, 2, 1.0), px(62, 30, 1.0), px(34, 60, 1.0)]
    faces.append((base, base + 1, base + 2))
    base = len(verts)
    verts += [px(60, 60), px(63, 60), px(60, 63)]
    faces.append((base, base + 1, base + 2))
    v = np.asarray(verts, np.float64)
    assert np.array_equal(v * 128, np.round(v * 128))
    return v.astype(f32), np.asarray(faces, np.int32)


LATTICE_K = np.array([[64, 0, 32], [0, 64, 32], [0, 0, 1]], f32)
LATTICE_T = np.array([[0, 0, 1], [1 / 64, -3 / 128, 1]], f32)        # the second pose: one pixel right, 1.5 px up


# --------------------------------------------------------------------------------------------- the kernel's own branch tests
def staged_projections(verts, K, R, t):
    """{u, v, z} as the refine kernel stages them: fp64 h, then float32 h0 / h2, h1 / h2, h2."""
    import raster_ref as RR

    h = RR.project(verts, K, R, np.asarray(t, f32).astype(np.float64))
    with np.errstate(all="ignore"):
        hz = h[:, 2].astype(f32)
        return h, np.stack([h[:, 0].astype(f32) / hz, h[:, 1].astype(f32) / hz, hz], 1)


def _exact_box(h0, h1, h2, res, zn, zf):
    """raster.hpp triangle_bbox in Python doubles -> (i_lo, i_hi, j_lo, j_hi) or None."""
    hs = (h0, h1, h2)
    zmin, zmax = min(h[2] for h in hs), max(h[2] for h in hs)
    us, vs = [], []
    with np.errstate(all="ignore"):
        if zmin >= zn:
            us, vs = [h[0] / h[2] for h in hs], [h[1] / h[2] for h in hs]
        else:
            for e in range(3):
                a, b = hs[e], hs[(e + 1) % 3]
                ain, bin_ = a[2] >= zn, b[2] >= zn
                if ain:
                    us.append(a[0] / a[2]); vs.append(a[1] / a[2])
                if ain != bin_:
                    tt = (zn - a[2]) / (b[2] - a[2])
                    us.append((a[0] + tt * (b[0] - a[0])) / zn); vs.append((a[1] + tt * (b[1] - a[1])) / zn)
    if not us or zmax < zn or zmin > zf:
        return None
    umin, umax, vmin, vmax = min(us), max(us), min(vs), max(vs)
    if not (umin <= umax):
        return None

    def clampi(x, lo, hi):
        return int(min(max(x, lo), hi))

    box = (clampi(np.ceil(umin - 0.5 - 1e-6), 0, res), clampi(np.floor(umax - 0.5 + 1e-6), -1, res - 1),
           clampi(np.ceil(vmin - 0.5 - 1e-6), 0, res), clampi(np.floor(vmax - 0.5 + 1e-6), -1, res - 1))
    return box if box[0] <= box[1] and box[2] <= box[3] else None


def branch_counts(verts, faces, K, R, t, res, z_near=0.1, z_far=100.0):
    """Which branches of the refine rasteriser a render reaches (triangle_bbox_f32, the cand == 2 exact path, the kLargeArea
    test), restated in NumPy float32 / float64 -> dict(n_exact = triangles on the cand == 2 path, n_cand = triangles with
    candidate pixels, n_large = of those with more than kLargeArea, n_cells = candidates summed, max_box)."""
    import raster_ref as RR

    faces = np.asarray(faces, np.int64)
    h, uvz = staged_projections(verts, K, R, t)
    D = RR.edge_planes(h, faces)[3]
    a, b, c = uvz[faces[:, 0]], uvz[faces[:, 1]], uvz[faces[:, 2]]
    zn, zf = f32(z_near), f32(z_far)
    with np.errstate(all="ignore"):
        zmin = np.fmin(a[:, 2], np.fmin(b[:, 2], c[:, 2]))
        exact = ~(zmin >= zn * f32(1.00001))
        far = ~exact & (zmin > zf * f32(1.00001))
        umin, umax = np.fmin(a[:, 0], np.fmin(b[:, 0], c[:, 0])), np.fmax(a[:, 0], np.fmax(b[:, 0], c[:, 0]))
        vmin, vmax = np.fmin(a[:, 1], np.fmin(b[:, 1], c[:, 1])), np.fmax(a[:, 1], np.fmax(b[:, 1], c[:, 1]))
        exact |= ~far & (~(umin <= umax) | ~(vmin <= vmax))
        lo_u, hi_u = np.maximum(np.ceil(umin - f32(0.501)), f32(0)), np.minimum(np.floor(umax - f32(0.499)), f32(res - 1))
        lo_v, hi_v = np.maximum(np.ceil(vmin - f32(0.501)), f32(0)), np.minimum(np.floor(vmax - f32(0.499)), f32(res - 1))
        fast = ~exact & ~far & (lo_u <= hi_u) & (lo_v <= hi_v)
    area = np.zeros(len(faces), np.int64)
    area[fast] = ((hi_u - lo_u + 1) * (hi_v - lo_v + 1))[fast].astype(np.int64)
    for k in np.flatnonzero(exact):
        box = _exact_box(*(h[faces[k, j]] for j in range(3)), res, float(zn), float(zf))
        if box:
            area[k] = (box[1] - box[0] + 1) * (box[3] - box[2] + 1)
    area[~(D != 0)] = 0
    return dict(n_exact=int(exact.sum()), n_cand=int((area > 0).sum()), n_large=int((area > LARGE_AREA).sum()),
                n_cells=int(area.sum()), max_box=int(area.max(initial=0)))


# -------------------------------------------------------------------------------------------------------- case assembly
CAM = np.array([[600, 0, 320], [0, 600, 240], [0, 0, 1]], f32)      # with centre (320, 240), scale 128: K_crop = f 300 res / 64
CENTER, SCALE = (320.0, 240.0), 128.0


def rot(axis, angle):
    return P.axangle2mat(axis, angle).astype(f32)


def _render_fn(verts, faces, z_near, z_far):
    def fn(obj, K, R, t, res):
        d, x = zip(*[P.render_depth(verts[obj[i]], faces[obj[i]], K[i], R[i], t[i].astype(np.float64), res_w=res,
                                    z_near=float(z_near), z_far=float(z_far), want_xyz=True) for i in range(len(obj))])
        return np.stack(d), np.stack(x)
    return fn


def oracle_refine(case, i, iters=None, stats=None, return_debug=False):
    """P.depth_refine_roi on ROI i of a case (mask normalised as mask_type says)."""
    if case.mask_type == 0:
        m = P.get_out_mask(case.mask[i:i + 1])[0, 0]
    else:
        assert case.mask_type == 2
        m = case.mask[i, 0]
    o = int(case.obj[i])
    xyz = np.concatenate([case.coor_x[i], case.coor_y[i], case.coor_z[i]], 0).transpose(1, 2, 0)
    return P.depth_refine_roi(xyz, m, case.roi_depth[i, 0], case.K_crop[i], case.R[i], case.t_in[i], case.verts[o], case.faces[o],
                              iters=case.iters if iters is None else iters, threshold=case.threshold, crop_res=case.res,
                              z_near=float(case.z_near), z_far=float(case.z_far), stats=stats, return_debug=return_debug)


def iteration_poses(case, i):
    """The translation each iteration renders with: t_in, then the float32 value of the translation after iteration 0, ..."""
    return [np.asarray(case.t_in[i] if k == 0 else oracle_refine(case, i, iters=k), f32) for k in range(case.iters)]


def _stabilise(case):
    """Move the mask value of every pixel whose q lies within 2 * STABLE_MARGIN of the threshold (in any iteration) by 3 % of
    the mask's range, until none is left: the device sums norm_sum in another order than NumPy (a few fp32 ulps), so such a pixel
    could be selected on one side and not on the other.  A condition on the INPUTS, asserted by the CPU tests."""
    for _ in range(12):
        moved = False
        for i in range(len(case.obj)):
            if i in case.kernel_only:
                continue
            st = []
            oracle_refine(case, i, stats=st)
            near = [s["closest"] for s in st if s["stepped"] and s["margin"] < 2 * STABLE_MARGIN]
            if near:
                m = case.mask[i, 0].reshape(-1)
                m[near] -= f32(0.03) * (m.max() - m.min())
                moved = True
        if not moved:
            return case
    raise AssertionError("selection did not become stable")


def make_case(seed, verts, faces, obj, R, t_gt, res=64, iters=2, threshold=0.8, mask_type=0, z_near=0.1, z_far=100.0,
              cam=CAM, t_exact=False, stabilise=True, holes=True):
    """Map inputs as synthetic.make_map_inputs builds them (rendered xyz maps + noise, a box-filtered visibility mask with
    a random gain and offset, the render as sensor depth + 2 mm noise + 5 % holes, t_in = t_gt + N(0, 3 cm) along z unless
    ``t_exact``; ``holes`` False fills the holes again) for ROIs that all use centre (320, 240), scale 128 of camera ``cam``."""
    b = len(obj)
    rng = np.random.default_rng([17, seed])
    ext = np.stack([(v.max(0) - v.min(0)).astype(f32) for v in verts])
    ext = np.maximum(ext, f32(1e-3))                                   # flat meshes: keep xyz / extent finite
    obj = np.asarray(obj, np.int32)
    det = dict(roi_cls=obj.astype(np.int64), roi_center=np.tile(np.asarray(CENTER, f32), (b, 1)), scale=np.full(b, SCALE, f32),
               roi_cam=np.tile(np.asarray(cam, f32), (b, 1, 1)), roi_extent=ext[obj], R_gt=np.asarray(R, f32).reshape(b, 3, 3),
               t_gt=np.asarray(t_gt, f32).reshape(b, 3))
    zn, zf = f32(z_near), f32(z_far)
    maps = S.make_map_inputs(det, verts, faces, _render_fn(verts, faces, zn, zf), rng, out_res=res)
    if not holes:
        big = np.repeat(np.repeat(_render_fn(verts, faces, zn, zf)(obj, maps["K_crop"], det["R_gt"], det["t_gt"], res)[0], 4, 1), 4, 2)
        rd = maps["roi_depth"][:, 0]
        rd[rd == 0] = big[rd == 0]
    case = SimpleNamespace(
        verts=list(verts), faces=list(faces), obj=obj, coor_x=maps["coor_x"], coor_y=maps["coor_y"], coor_z=maps["coor_z"],
        mask=maps["mask"], roi_depth=maps["roi_depth"], cam=det["roi_cam"], center=det["roi_center"], scale=det["scale"],
        K_crop=P.zoom_K(det["roi_cam"], det["roi_center"], det["scale"], res), R=det["R_gt"],
        t_in=det["t_gt"].copy() if t_exact else maps["t_init"], t_gt=det["t_gt"], res=res, iters=iters, threshold=threshold,
        mask_type=mask_type, z_near=zn, z_far=zf, kernel_only=())
    return _stabilise(case) if stabilise else case


def copy_maps(case, src, dst):
    for name in ("coor_x", "coor_y", "coor_z", "mask", "roi_depth"):
        getattr(case, name)[dst] = getattr(case, name)[src]


# ------------------------------------------------------------------------------------------- large-triangle queue, mixed
NAN_MASK_ROI = 3


@lru_cache(maxsize=None)
def queue_mixed_case():
    """Ellipsoids of 80 / 320 / 1280 faces, twice the usual size so that they fill the crop, at t_z = 0.5 and 0.35: small and large triangles in one pass, more
    than one queue round per wave.  ROI NAN_MASK_ROI carries a CONSTANT mask under mask_type 0: its normalisation is 0 / 0, every
    q is NaN, nothing is selected and the kernel keeps t_in (the reference would take the median of nothing)."""
    verts, faces = zip(*[ellipsoid(s, (0.1, 0.08, 0.09)) for s in (1, 2, 3)])
    obj = [0, 1, 2, 1, 0, 1, 2]
    rng = np.random.default_rng(41)
    R = [S.random_rotation(rng) for _ in obj]
    t = [(0.004, -0.003, 0.5), (-0.002, 0.005, 0.5), (0.0, 0.002, 0.5), (0.001, 0.001, 0.5),
         (0.003, 0.002, 0.35), (-0.004, 0.0, 0.35), (0.002, -0.003, 0.35)]
    case = make_case(1, verts, faces, obj, R, t, stabilise=False)
    case.mask[NAN_MASK_ROI] = f32(0.7)
    case.kernel_only = (NAN_MASK_ROI,)
    return _frozen(_stabilise(case))


# ---------------------------------------------------------------------------------------------------- queue at its limit
QUEUE_COUNTS = (MAX_LARGE - 1, MAX_LARGE, MAX_LARGE + 1, -(-MAX_LARGE * 8 // 5 // 128) * 128)


@lru_cache(maxsize=None)
def queue_limit_case(staged):
    """Objects 0..3: layered grids of QUEUE_COUNTS triangles, ALL of them large in ROIs 0..3 (R = I, t_z = 0.5); ROIs 4..7 see the
    same objects rotated and closer.  ``staged`` False appends an object of kMaxStagedVerts + 1 vertices that no ROI uses: the
    same geometry through the workspace kernel."""
    verts, faces = map(list, zip(*[layered_grid(n, k) for k, n in enumerate(QUEUE_COUNTS)]))
    if not staged:
        v, f = stage_mesh(MAX_STAGED + 1)
        verts.append(v); faces.append(f)
    R2 = rot((0, 0, 1), 0.3) @ rot((1, 0, 0), 0.1)
    obj = [0, 1, 2, 3, 0, 1, 2, 3]
    R = [np.eye(3)] * 4 + [R2] * 4
    t = [(0.0, 0.0, 0.5)] * 4 + [(0.002, -0.001, 0.44)] * 4
    case = make_case(2, verts, faces, obj, R, t, stabilise=False, holes=False)
    case.t_in[:4] = (0.0, 0.0, 0.49)                  # 1 cm too close
    return _frozen(_stabilise(case))


# -------------------------------------------------------------------------------- near plane, camera plane, far plane, empty
PLANE_ROIS = dict(near_cut=0, far_cut=1, beyond_far=2, off_crop=3, straddles_camera=4, vertex_on_camera_plane=5)


@lru_cache(maxsize=None)
def plane_case():
    """One launch with z_near = 0.5, z_far = 1.0.  Object 0: the 320-face ellipsoid; object 1: the same, 0.6 long in z, plus one
    vertex at z = -0.25 exactly with a triangle of its own.
      ROI 0  cut by z_near, every vertex at z > 0        ROI 1  cut by z_far (the rim of its front surface)
      ROI 2  wholly beyond z_far (maps of ROI 1)         ROI 3  beside the crop (maps of ROI 1): empty renders, t_out = t_in
      ROI 4  object 1 across the camera plane (z from -0.3 to 0.9)
      ROI 5  object 1 with R = I, t = (0, 0, 0.25): the extra vertex has camera-space z == 0 exactly"""
    v0, f0 = ellipsoid(2)
    v1, f1 = ellipsoid(2, (0.05, 0.04, 0.6))
    n = len(v1)
    v1 = np.concatenate([v1, np.array([[0.0625, 0.03125, -0.25]], f32)])
    f1 = np.concatenate([f1, np.array([[n, 0, 1]], np.int32)])
    I = np.eye(3)
    R = [rot((1, 1, 0), 0.4), rot((0, 1, 1), 0.7), I, I, rot((1, 0, 0), 0.2), I]
    t = [(0.002, 0.001, 0.5), (-0.001, 0.003, 1.03), (0.0, 0.0, 1.5), (0.5, 0.0, 0.75), (0.003, -0.002, 0.3), (0.0, 0.0, 0.25)]
    case = make_case(3, [v0, v1], [f0, f1], [0, 0, 0, 0, 1, 1], R, t, z_near=0.5, z_far=1.0, stabilise=False)
    copy_maps(case, 1, 2)
    copy_maps(case, 1, 3)
    case.t_in[:2] = case.t_gt[:2]                     # the cuts go through the objects' middles
    case.t_in[5] = case.t_gt[5]                       # powers of two: the vertex stays on the camera plane in iteration 0
    return _frozen(_stabilise(case))


# ------------------------------------------------------------------------------------------------------------ stage limit
STAGE_VERTS = (MAX_STAGED - 1, MAX_STAGED, MAX_STAGED + 1)


@lru_cache(maxsize=None)
def stage_case(n_verts):
    """Mesh set {162-vertex ellipsoid, stage_mesh(n_verts)}: ROIs 0 and 2 use the small object (max_verts, which lays out the
    stage, belongs to the other), ROIs 1 and 3 the large one."""
    small, big = ellipsoid(2), stage_mesh(n_verts)
    rng = np.random.default_rng(43)
    R = [S.random_rotation(rng), rot((1, 0, 0), 0.3), S.random_rotation(rng), rot((0, 1, 0), 0.4) @ rot((0, 0, 1), 1.0)]
    t = [(0.003, 0.0, 0.5), (0.0, -0.002, 0.5), (-0.002, 0.004, 0.42), (0.001, 0.002, 0.6)]
    return _frozen(make_case(4, [small[0], big[0]], [small[1], big[1]], [0, 1, 0, 1], R, t))


def workspace_bytes(n_verts, b):
    return 0 if n_verts <= MAX_STAGED else b * ((n_verts + 1) & ~1) * STAGE_BYTES


# ------------------------------------------------------------------------------------------------------------ resolutions
REFINE_RES = (8, 16, 24, 32, 48, 64)        # 64, 256, 576, 1024, 2304, 4096 pixels against REFINE_THREADS per pass
RENDER_RES = (1, 8, 63, 78, 79, 128)        # 78 / 79: the 48 KiB default LDS limit of the u64 z-buffer; 128: the limit


@lru_cache(maxsize=None)
def res_case(res):
    """642-vertex, 42-vertex and (partly outside the crop) 162-vertex ellipsoids at crop resolution ``res``; roi_depth is
    4 res x 4 res and K_crop scales with res."""
    verts, faces = zip(*[ellipsoid(s) for s in (3, 1, 2)])
    rng = np.random.default_rng(47)
    R = [S.random_rotation(rng) for _ in range(3)]
    t = [(0.002, -0.001, 0.5), (-0.003, 0.002, 0.45), (0.04, 0.03, 0.5)]
    return _frozen(make_case(5 + res, verts, faces, [0, 1, 2], R, t, res=res))


@lru_cache(maxsize=None)
def render_res_case(res):
    """-> verts, faces, K f32[3,3,3], R, t for render_depth at ``res``: the 1280-face ellipsoid (2.5 x kT faces) in front of the
    camera, close enough for large triangles, and across the camera plane."""
    v, f = ellipsoid(3)
    assert len(f) > RENDER_THREADS and len(f) % RENDER_THREADS
    rng = np.random.default_rng(53)
    fl = 300.0 * res / 64.0
    K = np.tile(np.array([[fl, 0, res / 2], [0, fl, res / 2], [0, 0, 1]], f32), (3, 1, 1))
    R = np.stack([S.random_rotation(rng) for _ in range(3)]).astype(f32)
    t = np.array([[0.002, -0.001, 0.5], [0.01, 0.0, 0.12], [0.0, 0.005, 0.03]], f32)
    return _frozen(SimpleNamespace(verts=v, faces=f, K=K, R=R, t=t))


# ----------------------------------------------------------------------------------------------------------------- median
MEDIAN_K = (1, 2, 3, 4, REFINE_THREADS - 1, REFINE_THREADS, REFINE_THREADS + 1, 0)      # 0: every rendered pixel
MEDIAN_UNIT = 2.0 ** -25                      # one ulp of a render in [0.25, 0.5): every designed difference is a multiple
_A = 1 << 16                                  # 2^-9 m = 1.95 mm in units of MEDIAN_UNIT: there a unit is 128 ulps of the difference


def median_pattern(k):
    """The k depth differences of an ROI, in units of MEDIAN_UNIT (sorted).  r0 = (k - 1) // 2 and r1 = k // 2 are the ranks.
      k = 1  one value            k = 2  -A and 2 A: the ranks lie in different top-byte bins (sign), a mean is taken
      k = 3  -A, +0, A            k = 4  the middle two differ in their lowest byte only (A, A + 1)
      k odd, large    a group of 7 identical values around the rank (ties through all four byte passes), next to a group that
                      differs in the lowest byte; for k = REFINE_THREADS + 1 the group is +0
      k even, large   5 identical negative values ending at r0, 5 identical positive ones starting at r1"""
    if k == 1:
        return np.array([_A])
    if k == 2:
        return np.array([-_A, 2 * _A])
    if k == 3:
        return np.array([-_A, 0, _A])
    if k == 4:
        return np.array([-_A, _A, _A + 1, 3 * _A])
    r0, r1 = (k - 1) // 2, k // 2
    v = np.empty(k, np.int64)
    j = np.arange(k)
    v[:] = np.where(j < r0, -(2 * _A + j % 37), 2 * _A + 3 * (j % 41))
    if k % 2:
        mid = 0 if k == REFINE_THREADS + 1 else _A
        v[r0 - 3:r0 + 4] = mid
        v[r0 + 4:r0 + 8] = mid + 1
    else:
        v[r0 - 4:r0 + 1] = -_A - 3
        v[r1:r1 + 5] = _A + 7
    return np.sort(v)


@lru_cache(maxsize=None)
def median_case():
    """mask_type 2, ||xyz|| = 0.6 everywhere, mask 1 on k hot pixels and 0.5 elsewhere: the hot pixels tie at qmax, the rest sit
    at half of it, nsel = k.  Sensor depth = iteration 0's render + median_pattern(k) on the hot pixels; renders lie in
    [0.3, 0.4], so render + difference and their float32 subtraction are exact.  (-0 cannot occur: a selected pixel has render > 0
    and sensor > 0, and the difference of two positive floats is never -0.)  -> case, hot (list of flat pixel indices per ROI)"""
    v, f = ellipsoid(3)
    b = len(MEDIAN_K)
    rng = np.random.default_rng(59)
    cam = np.array([[400, 0, 320], [0, 400, 240], [0, 0, 1]], f32)          # K_crop f = 200
    R = [S.random_rotation(rng) for _ in range(b)]
    t = [(0.001 * (i % 3 - 1), 0.001 * (i % 2), 0.375) for i in range(b)]
    case = make_case(6, [v], [f], [0] * b, R, t, mask_type=2, cam=cam, t_exact=True, stabilise=False)
    jj, ii = np.divmod(np.arange(64 * 64), 64)
    inner = np.hypot(ii - 31.5, jj - 31.5) < 17
    hot = []
    for i, k in enumerate(MEDIAN_K):
        ren = P.render_depth(v, f, case.K_crop[i], case.R[i], case.t_in[i].astype(np.float64), 64).reshape(-1)
        assert ren[inner].min() >= 0.3 and ren.max() <= 0.4
        cand = np.flatnonzero(ren > 0) if k == 0 else rng.permutation(np.flatnonzero(inner))[:k]
        pat = median_pattern(len(cand))
        ds = np.where(ren > 0, ren + f32(_A * MEDIAN_UNIT), f32(0.375)).astype(f32)
        ds[cand] = ren[cand] + (rng.permutation(pat) * MEDIAN_UNIT).astype(f32)
        case.roi_depth[i, 0] = np.repeat(np.repeat(ds.reshape(64, 64), 4, 0), 4, 1)
        m = np.full(64 * 64, 0.5, f32)
        m[cand] = 1.0
        case.mask[i, 0] = m.reshape(64, 64)
        case.coor_x[i], case.coor_y[i], case.coor_z[i] = f32(0.6), f32(0), f32(0)
        hot.append(np.sort(cand))
    return _frozen(case), hot


# ---------------------------------------------------------------------------------------------------------------- lattice
@lru_cache(maxsize=None)
def lattice_case():
    """The lattice mesh under K = LATTICE_K, R = I and the two translations of LATTICE_T, as a refine case (t_in = the exact
    lattice pose, so iteration 0 renders the lattice itself)."""
    v, f = lattice_mesh()
    cam = np.array([[128, 0, 320], [0, 128, 240], [0, 0, 1]], f32)
    case = make_case(7, [v], [f], [0, 0], [np.eye(3)] * 2, LATTICE_T, cam=cam, t_exact=True)
    assert np.array_equal(case.K_crop[0], LATTICE_K)
    return _frozen(case)
