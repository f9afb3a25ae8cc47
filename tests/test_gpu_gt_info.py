"""-m gpu: ``gdrnpp_gt_visibility`` (csrc/gt_visib.hip) through the C ABI, the binding and ``gdrn_modeling.bop_gt_info``.  The kernel
returns integer counts, integer extents and mask bytes, so everything here is compared for EQUALITY, on every pose and every pixel:
against tests/gt_info_ref.py (the toolkit's NumPy recipe fed by an fp64 restatement of oracle/raster_oracle.c, with poses and intrinsics
that are not float32-representable) at the kernel's tile, window, border and size edges, and against what the reference's own
calc_gt_info.py and calc_gt_masks.py recorded in tests/golden/gt_info_golden.npz.

Why equality is the right bound: coverage and depth are the oracle's fp64 expressions in the oracle's order on the canvas's own pixel
indices (no contraction), the distance images use IEEE division and square root on both sides, and the outputs are integer sums, minima
and maxima.  Nothing is rounded differently, so no comparison can fall on another side."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd import synthetic as S
from gdrnpp_bop2022_amd.gdrn_modeling import bop_gt_info as BG
from tests import gt_info_golden as GG
from tests import gt_info_ref as G
from tests import vsd_ref as V

pytestmark = pytest.mark.gpu
DEV = "cuda"
DELTA = 15.0
FX, FY = 572.4114, 573.57043                                   # not float32 values
EMPTY = G.EMPTY


def T(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def cam(W, H, fx=FX, fy=FY, skew=0.37):
    """A camera matrix with a skew entry: the toolkit hands its renderer fx, fy, cx, cy only, so the entry must be ignored."""
    return np.array([[fx, skew, W / 2 + 0.317], [0.0, fy, H / 2 - 0.211], [0.0, 0.0, 1.0]])


@functools.lru_cache(maxsize=None)
def models():
    """Objects of 4, 42, 162, 642 and 2562 vertices (mm): a 400 x 300 quad in z = 0 and four ellipsoids."""
    quad = (np.array([[-200, -150, 0], [200, -150, 0], [200, 150, 0], [-200, 150, 0]], np.float32), np.array([[0, 1, 2], [0, 2, 3]], np.int32))
    out = [quad]
    for sub, scale in ((1, (40, 30, 25)), (2, (50, 35, 25)), (3, (45, 45, 30)), (4, (30, 30, 30))):
        v, f = S.icosphere(sub)
        out.append(((v * np.array(scale, np.float64)).astype(np.float32), f.astype(np.int32)))
    return out


@functools.lru_cache(maxsize=None)
def meshset():
    return hip_lib.MeshSet([v for v, _ in models()], [f for _, f in models()], DEV)


def scene_depth(rng, gts, K, W, H, wall=900.0, slab=None, holes=True):
    """A wall at constant Z with the ground-truth objects in front of it, rounded to whole millimetres; an occluding slab and holes."""
    ms = models()
    d = np.full((H, W), wall, np.float32)
    for o, R, t in gts:
        r = V.render_depth_f64(ms[o][0], ms[o][1], V.render_K(K), R, t, W, H, 1.0, 1e6)
        d = np.where((r > 0) & (r < d), np.round(r), d).astype(np.float32)
    if slab is not None:
        x0, x1, y0, y1, z = slab
        d[y0:y1, x0:x1] = z
    if holes:
        d[rng.integers(0, H, 12), rng.integers(0, W, 12)] = 0.0
        d[H // 3:H // 3 + 3, W // 2:W // 2 + 5] = 0.0
    return d


def _args(poses):
    """poses: [(obj, im, R, t, K)] -> the five device tensors."""
    return (T(np.array([p[0] for p in poses], np.int32)), T(np.array([p[1] for p in poses], np.int32)), T(np.stack([p[2].reshape(9) for p in poses])),
            T(np.stack([p[3] for p in poses])), T(np.stack([p[4].reshape(9) for p in poses])))


def gpu(poses, images, offset, delta=DELTA, ms=None, **kw):
    """-> (info i32[n,11], mask u8[n,H,W], mask_visib u8[n,H,W]) as arrays, through hip_lib.gt_visibility."""
    info, mask, visib = hip_lib.gt_visibility(ms or meshset(), *_args(poses), T(np.asarray(images, np.float32)), delta, canvas_offset=offset,
                                              want_masks=True, **kw)
    assert info.dtype == torch.int32 and mask.dtype == visib.dtype == torch.uint8
    return info.cpu().numpy(), mask.cpu().numpy(), visib.cpu().numpy()


def ref(poses, images, offset, delta=DELTA):
    ms = models()
    rows = [G.gt_visibility_ref(ms[o][0], ms[o][1], R, t, K, images[im], delta, offset) for o, im, R, t, K in poses]
    return np.array([r[0] for r in rows], np.int64), np.array([r[1] for r in rows]), np.array([r[2] for r in rows])


def check(poses, images, offset, what, delta=DELTA, **kw):
    got, want = gpu(poses, images, offset, delta, **kw), ref(poses, images, offset, delta)
    print(what, "offset", offset, "all / valid / visib:", want[0][:, :3].tolist())
    assert np.array_equal(got[0], want[0]), (what, offset, got[0].tolist(), want[0].tolist())
    for k, name in ((1, "mask"), (2, "mask_visib")):
        assert set(np.unique(got[k])) <= {0, 255}
        assert np.array_equal(got[k] == 255, want[k]), (what, offset, name)
    return got


# ---- 1. small images: below a tile, across tile corners, exactly a tile; the window at and off a tile boundary -----------------------
@pytest.mark.parametrize("canvas", ["3x", "plain"])
@pytest.mark.parametrize("W,H,centre", [(24, 20, (0.0, 0.0)), (100, 70, (-11.0, 14.0)), (64, 64, (0.0, 0.0)), (129, 65, (54.0, 30.0))])
def test_small_images_against_the_fp64_restatement(hip, W, H, centre, canvas):
    """24x20: smaller than a tile both ways (canvas 72x60); 100x70: the window starts mid-tile at (100, 70) of a 300x210 canvas; 64x64:
    window = the canvas's middle tile; 129x65: a one-pixel last column and row of tiles, the object there.  Six poses of the 162-vertex,
    320-face model: two inside, one perturbed, one over the left border, one over the bottom, one under the slab."""
    rng = np.random.default_rng(W * 1000 + H)
    K = cam(W, H)
    z = 600.0 if W > 24 else 2500.0
    place = lambda du, dv, dz=0.0: np.array([(centre[0] + du) * z / FX + rng.uniform(-3, 3), (centre[1] + dv) * z / FY + rng.uniform(-3, 3), z + dz])  # noqa: E731
    gts = [(2, S.random_rotation(rng), place(0, 0)), (2, S.random_rotation(rng), place(8, -5, 60.0))]
    img = scene_depth(rng, gts, K, W, H, wall=z + 300.0, slab=(W // 2, W // 2 + 6, 0, H, z - 200.0))
    poses = [(o, 0, R, t, K) for o, R, t in gts]
    poses.append((2, 0, S.random_rotation(rng), gts[0][2] + np.array([4.0, -3.0, 9.0]), K))
    poses.append((2, 0, S.random_rotation(rng), place(-centre[0] - W / 2, 0), K))
    poses.append((2, 0, S.random_rotation(rng), place(0, -centre[1] + H / 2), K))
    poses.append((2, 0, S.random_rotation(rng), place(6 - centre[0], 0, -100.0), K))
    assert len(poses) == 6 and models()[2][0].shape == (162, 3) and models()[2][1].shape == (320, 3)
    offset = (W, H) if canvas == "3x" else (0, 0)
    got = check(poses, img[None], offset, f"{W}x{H}")
    assert (got[0][:, 0] > 0).all() and (got[0][:, 2] > 0).sum() >= 4
    noskew = K.copy()
    noskew[0, 1] = 0.0
    same = gpu([p[:4] + (noskew,) for p in poses], img[None], offset)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, same))      # the skew entry is not read


# ---- 2. one pose of each kind of truncation ---------------------------------------------------------------------------------------
def test_poses_cut_by_each_border_beside_the_window_off_the_canvas_and_behind(hip):
    W, H = 100, 90
    rng = np.random.default_rng(5)
    K = cam(W, H)
    z = 500.0
    R = S.random_rotation(rng)
    spots = {"left": (-W / 2, 0), "right": (W / 2, 0), "top": (0, -H / 2), "bottom": (0, H / 2), "corner": (W / 2, H / 2)}
    cut = [(2, 0, R, np.array([du * z / FX, dv * z / FY, z + 0.123]), K) for du, dv in spots.values()]
    img = scene_depth(rng, [(2, R, cut[0][3])], K, W, H, wall=800.0)
    beside = (2, 0, R, np.array([-100.0 * 1000.0 / FX, 3.0, 1000.0]), K)       # 57 px across at x = -50: left of the window, on the 3x canvas
    off_canvas = (2, 0, R, np.array([900.0, 0.0, z]), K)
    behind = (2, 0, R, np.array([0.0, 0.0, -z]), K)
    near = (2, 0, R, np.array([3.0, -2.0, 10.0]), K)                            # the camera inside the object: vertices nearer than z_near
    poses = cut + [beside, off_canvas, behind, near]
    for offset in ((W, H), (0, 0)):
        info, mask, visib = check(poses, img[None], offset, "kinds")
        recs = BG.gt_info_records(info)
        for k in range(5):
            assert info[k, 2] > 0 and recs[k]["bbox_visib"][0] >= 0 and recs[k]["bbox_obj"] != [-1] * 4
        if offset == (W, H):                                        # the silhouette reaches beyond the image on the cut side
            assert info[0, 3] < 0 and info[1, 5] > W - 1 and info[2, 4] < 0 and info[3, 6] > H - 1 and info[4, 5] > W - 1 and info[4, 6] > H - 1
            assert info[5, 0] > 0 and info[5, 5] < 0 and info[5, 2] == 0 and info[5, 1] == 0
            assert recs[5]["bbox_obj"] == recs[5]["bbox_visib"] == [-1] * 4 and recs[5]["visib_fract"] == 0.0
        else:                                                       # on the plain image the extents stop at the border
            assert info[0, 3] == 0 and info[1, 5] == W - 1 and info[2, 4] == 0 and info[3, 6] == H - 1
            assert (info[5, :3] == 0).all()
        for k in (6, 7):
            assert (info[k, :3] == 0).all() and info[k, 3:].tolist() == EMPTY + EMPTY and not mask[k].any() and not visib[k].any()
            assert recs[k] == dict(px_count_all=0, px_count_valid=0, px_count_visib=0, visib_fract=0.0, bbox_obj=[-1] * 4, bbox_visib=[-1] * 4)
        assert info[8, 0] > 0.5 * (W + 2 * offset[0]) * (H + 2 * offset[1])     # seen from inside, the object fills most of the canvas


# ---- 3. the raster's two extremes ---------------------------------------------------------------------------------------------------
def test_quad_over_the_whole_canvas_and_subpixel_triangles(hip):
    W, H = 50, 30                                              # canvas 150 x 90: 3 x 2 tiles
    K = cam(W, H)
    tq = np.array([0.4, -0.3, 100.0])                          # 400 x 300 mm at 100 mm: 2288 x 1720 px, covers everything
    img = np.full((H, W), 120.0, np.float32)
    img[10:20, 5:40] = 0.0
    img[20:28, 30:50] = 50.0
    info, mask, visib = check([(0, 0, np.eye(3), tq, K)], img[None], (W, H), "quad over the canvas")
    assert info[0, 0] == (3 * W) * (3 * H) and info[0, 3:7].tolist() == [-W, -H, 2 * W - 1, 2 * H - 1] and mask.all()
    assert info[0, 1] == W * H - 350 and info[0, 2] == W * H - 160 and info[0, 7:].tolist() == [0, 0, W - 1, H - 1]
    info, _, _ = check([(0, 0, np.eye(3), tq, K)], img[None], (0, 0), "quad over the image")
    assert info[0, 0] == W * H and info[0, 3:7].tolist() == [0, 0, W - 1, H - 1]
    # subdivision 4 (5120 faces, 60 mm) at 60 m: 0.57 px across, centred on a pixel corner: no centre is covered
    zs = 60000.0
    ts = np.array([(25.0 - K[0, 2]) / FX * zs, (14.0 - K[1, 2]) / FY * zs, zs])
    Rs = S.random_rotation(np.random.default_rng(9))
    for offset in ((W, H), (0, 0)):
        info, mask, visib = check([(4, 0, Rs, ts, K)], img[None], offset, "sub-pixel triangles")
        assert info[0].tolist() == [0, 0, 0] + EMPTY + EMPTY and not mask.any() and not visib.any()


# ---- 4. what the depth image means ----------------------------------------------------------------------------------------------------
def test_zero_depth_occluders_around_the_tolerance_and_a_hole(hip):
    W, H = 96, 80
    rng = np.random.default_rng(11)
    K = cam(W, H)
    ms = models()
    R, t = S.random_rotation(rng), np.array([10.3, -7.7, 900.9])
    Zg = V.render_depth_f64(ms[3][0], ms[3][1], V.render_K(K), R, t, W, H, 1.0, 1e6).astype(np.float64)
    xs, ys = np.meshgrid(np.arange(W), np.arange(H))
    ray = np.sqrt(((xs - K[0, 2]) / K[0, 0]) ** 2 + ((ys - K[1, 2]) / K[1, 1]) ** 2 + 1.0)       # dist = Z * ray
    inside = Zg > 0
    holed = np.full((H, W), 1200.0, np.float32)
    holed[38:43, :] = 0.0
    imgs = np.stack([np.zeros((H, W)), np.full((H, W), 600.0), np.where(inside, Zg - (DELTA - 1.0) / ray, 1200.0),
                     np.where(inside, Zg - (DELTA + 1.0) / ray, 1200.0), holed]).astype(np.float32)
    poses = [(3, im, R, t, K) for im in range(5)]
    for offset in ((W, H), (0, 0)):
        info, mask, visib = check(poses, imgs, offset, "depth semantics")
        n = int(inside.sum())
        assert n > 500 and (info[:, 0] == n).all() and all(np.array_equal(m == 255, inside) for m in mask)
        assert info[0, 1] == 0 and info[0, 2] == n and np.array_equal(visib[0], mask[0])         # all missing: visible, none valid
        assert info[1, 1] == n and info[1, 2] == 0 and not visib[1].any()                        # an occluder 300 mm in front
        assert info[2, 2] == n and np.array_equal(visib[2], mask[2])                             # 14 mm in front: within the tolerance
        assert info[3, 2] == 0 and not visib[3].any()                                            # 16 mm in front: occluded
        band = int(inside[38:43].sum())
        assert band > 0 and info[4, 1] == n - band and info[4, 2] == n                           # over the hole: valid < visib
    assert BG.gt_info_records(info)[1]["bbox_obj"] == [-1] * 4                                   # guarded by the VISIBLE count


# ---- 5. many poses, chunks, order ------------------------------------------------------------------------------------------------------
def test_seventy_poses_three_images_four_objects_chunked(hip):
    W, H = 96, 80
    rng = np.random.default_rng(13)
    K = [cam(W, H), cam(W, H, 480.25, 481.75), cam(W, H, 610.1, 608.3)]
    distinct, imgs = [], []
    for im in range(3):
        g = []
        for o in (1, 2, 3, 0)[: 3 + (im == 2)]:
            z = 700.0 if o else 2600.0
            g.append((o, S.random_rotation(rng), np.array([rng.uniform(-40, 40), rng.uniform(-30, 30), z + rng.uniform(-30, 30)])))
        imgs.append(scene_depth(rng, g, K[im], W, H, wall=3000.0, slab=(10 + 20 * im, 30 + 20 * im, 20, 60, 400.0)))
        distinct += [(o, im, R, t, K[im]) for o, R, t in g]
    imgs = np.stack(imgs)
    far = distinct[0]
    distinct += [(3, 1, far[2], np.array([5.0 + 40 * k, 5.0, 900.0 + 50 * k]), K[1]) for k in range(14 - len(distinct))]
    assert len(distinct) == 14 and len({p[0] for p in distinct}) == 4
    want = ref(distinct, imgs, (W, H))
    order = rng.permutation(np.repeat(np.arange(14), 5))
    poses = [distinct[k] for k in order]
    per_pose = hip_lib.load().gdrnpp_gt_visibility_workspace_bytes(meshset().c, 1)
    assert per_pose == 2562 * 40 + 16
    whole = gpu(poses, imgs, (W, H))
    assert np.array_equal(whole[0], want[0][order]) and np.array_equal(whole[1] == 255, want[1][order]) and np.array_equal(whole[2] == 255, want[2][order])
    for budget in (1, 3 * per_pose + 5, 69 * per_pose):         # 1, 3 and 69 poses per launch
        chunked = gpu(poses, imgs, (W, H), workspace_budget=budget)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(chunked, whole)), budget
    again = gpu(poses, imgs, (W, H))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(again, whole))
    back = gpu(poses[::-1], imgs, (W, H))
    assert all(np.array_equal(a[::-1], b) for a, b in zip(back, whole))
    info, none1, none2 = hip_lib.gt_visibility(meshset(), *_args(poses), T(imgs), DELTA, canvas_offset=(W, H))
    assert none1 is None and none2 is None and np.array_equal(info.cpu().numpy(), whole[0])      # without masks: the same rows


# ---- 6. what only the device can see -----------------------------------------------------------------------------------------------------
def test_out_of_range_obj_and_im_idx_give_minus_one_rows_and_zero_masks(hip):
    W, H = 64, 48
    rng = np.random.default_rng(17)
    K = cam(W, H)
    R, t = S.random_rotation(rng), np.array([1.0, 2.0, 500.0])
    img = scene_depth(rng, [(2, R, t)], K, W, H, wall=800.0)[None]
    good = (2, 0, R, t, K)
    want = ref([good], img, (W, H))
    n_obj = len(models())
    poses = [good, (n_obj, 0) + good[2:], good, (-1, 0) + good[2:], (2, 1) + good[2:], good, (2, -1) + good[2:], (2 ** 30, 2 ** 30) + good[2:], good]
    info, mask, visib = gpu(poses, img, (W, H))
    for k, p in enumerate(poses):
        if p is good:
            assert np.array_equal(info[k], want[0][0]) and np.array_equal(mask[k] == 255, want[1][0]) and np.array_equal(visib[k] == 255, want[2][0]), k
        else:
            assert (info[k] == -1).all() and not mask[k].any() and not visib[k].any(), k
    with pytest.raises(RuntimeError, match="could not be rendered"):
        BG.gt_info_records(info)
    ms = models()
    bare = hip_lib.MeshSet([ms[2][0], ms[1][0]], [np.zeros((0, 3), np.int32), ms[1][1]], DEV)   # an object without faces
    info, _, _ = gpu([(0, 0) + good[2:], (1, 0) + good[2:]], img, (0, 0), ms=bare)
    assert (info[0] == -1).all() and info[1, 0] > 0


# ---- 7. the C contract ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_return_a_status_and_touch_nothing(hip):
    lib = hip_lib.load()
    W, H, n = 64, 48, 3
    rng = np.random.default_rng(19)
    K = cam(W, H)
    R, t = S.random_rotation(rng), np.array([1.0, 2.0, 500.0])
    img = scene_depth(rng, [(2, R, t)], K, W, H, wall=800.0)[None]
    poses = [(2, 0, R, t + k, K) for k in range(n)]
    a = list(_args(poses)) + [T(img)]
    m = meshset()
    info = torch.full((n, 11), -7, dtype=torch.int32, device=DEV)
    mask = torch.full((n, H, W), 9, dtype=torch.uint8, device=DEV)
    visib = torch.full((n, H, W), 9, dtype=torch.uint8, device=DEV)
    need = lib.gdrnpp_gt_visibility_workspace_bytes(m.c, n)
    assert need == n * (2562 * 40 + 16) and lib.gdrnpp_gt_visibility_workspace_bytes(m.c, 0) == 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    p = [x.data_ptr() for x in a]

    def call(ptrs=p, nb=n, ws_ptr=ws.data_ptr(), ws_bytes=need, mc=m.c, n_im=1, h=H, w=W, ox=W, oy=H, zn=1.0, zf=1e6, o=info.data_ptr(),
             mk=mask.data_ptr(), mv=visib.data_ptr()):
        return lib.gdrnpp_gt_visibility(mc, *ptrs, n_im, h, w, ox, oy, DELTA, zn, zf, o, mk, mv, nb, ws_ptr, ws_bytes, None)

    def said(text):
        return text in lib.gdrnpp_last_error()

    for k in range(len(p)):                                    # every pointer in turn
        assert call(ptrs=p[:k] + [None] + p[k + 1:]) == -1 and said(b"null pointer"), k
    assert call(o=None) == -1 and said(b"null pointer")
    assert call(nb=-2) == -1 and said(b"n=-2")
    assert call(h=0) == -1 and said(b"H=0") and call(w=-1) == -1 and said(b"W=-1") and call(n_im=0) == -1
    assert call(ox=-1) == -1 and said(b"offset") and call(oy=-3) == -1 and said(b"offset")
    assert call(zn=0.0) == -1 and said(b"z_near") and call(zn=10.0, zf=5.0) == -1
    assert call(ws_bytes=need - 1) == -1 and said(b"workspace") and call(ws_ptr=None) == -1
    assert call(mc=None) == -1 and said(b"invalid mesh set")
    unset = hip_lib.gdrnpp_meshes(m.verts.data_ptr(), m.faces.data_ptr(), m.vert_off.data_ptr(), m.face_off.data_ptr(), m.n_obj, 0, 5120)
    assert call(mc=ctypes.byref(unset)) == -1 and said(b"max_verts") and lib.gdrnpp_gt_visibility_workspace_bytes(ctypes.byref(unset), n) == 0
    faceless = hip_lib.gdrnpp_meshes(m.verts.data_ptr(), None, m.vert_off.data_ptr(), None, m.n_obj, 2562, 0)
    assert call(mc=ctypes.byref(faceless)) == -1 and said(b"faces")
    assert call(nb=2 ** 30, ws_bytes=2 ** 62) == -2 and said(b"split the poses")
    assert call(ox=2 ** 20, oy=2 ** 20) == -2 and said(b"32-bit counters")
    assert call(nb=0) == 0                                     # no pose: a success that launches nothing
    torch.cuda.synchronize()
    assert (info == -7).all() and (mask == 9).all() and (visib == 9).all() and (ws == 0).all()   # nothing ran, nothing was cleared
    with pytest.raises(RuntimeError, match="dtype"):
        hip_lib.gt_visibility(m, a[0], a[1], a[2].float(), *a[3:], DELTA)
    with pytest.raises(RuntimeError, match="t must hold"):
        hip_lib.gt_visibility(m, *a[:3], a[3][:-1].contiguous(), *a[4:], DELTA)
    with pytest.raises(RuntimeError, match="offset"):
        hip_lib.gt_visibility(m, *a, DELTA, canvas_offset=(-1, 0))
    assert call() == 0                                         # and the same arguments, complete, run
    torch.cuda.synchronize()
    want = ref(poses, img, (W, H))
    assert np.array_equal(info.cpu().numpy(), want[0]) and np.array_equal(mask.cpu().numpy() == 255, want[1])
    assert np.array_equal(visib.cpu().numpy() == 255, want[2]) and set(np.unique(mask.cpu().numpy())) == {0, 255}
    assert call(mk=None, mv=None) == 0                         # masks are optional
    torch.cuda.synchronize()
    assert np.array_equal(info.cpu().numpy(), want[0])
    e_info, e_mask, e_visib = hip_lib.gt_visibility(m, *[x[:0] for x in a[:5]], a[5], DELTA, want_masks=True)
    assert e_info.shape == (0, 11) and e_mask.shape == e_visib.shape == (0, H, W)
    e_info, e_mask, e_visib = hip_lib.gt_visibility(m, *[x[:0] for x in a[:5]], a[5], DELTA)
    assert e_info.shape == (0, 11) and e_mask is None and e_visib is None


def test_pysixd_shim_runs_the_entry_point(hip):
    from gdrnpp_bop2022_amd.lib.pysixd import pose_error as PE
    from gdrnpp_bop2022_amd.lib.pysixd import visibility as VI

    W, H = 96, 80
    rng = np.random.default_rng(23)
    K = cam(W, H)
    ms = models()
    R, t = S.random_rotation(rng), np.array([10.0, -5.0, 520.0])
    img = scene_depth(rng, [(2, R, t)], K, W, H, wall=800.0, slab=(50, 70, 0, H, 300.0))
    pose = VI.GtPose(PE.VsdRenderer(meshset(), {7: 2}), 7, R, t.reshape(3, 1), K)
    got = VI.estimate_visib_mask_gt(img, pose, DELTA)
    _, _, want = G.gt_visibility_ref(ms[2][0], ms[2][1], R, t, K, img, DELTA)
    assert got.dtype == bool and want.any() and np.array_equal(got, want)
    with pytest.raises(NotImplementedError, match="bop18"):
        VI.estimate_visib_mask_gt(img, pose, DELTA, "bop18")
    with pytest.raises(NotImplementedError):
        VI.estimate_visib_mask_est(img, img, got, DELTA)


# ---- 8. the recorded reference: calc_gt_info.py and calc_gt_masks.py ---------------------------------------------------------------------------
def _fixture(g, offset, want_masks=True):
    p = g["poses"]
    ms = hip_lib.MeshSet(g["verts_list"], g["faces_list"], DEV)
    info, mask, visib = hip_lib.gt_visibility(ms, T(p["obj"]), T(p["im"]), T(p["R"]), T(p["t"]), T(p["K"]), T(g["depth_mm"]), g["delta"],
                                              canvas_offset=offset, want_masks=want_masks)
    return info.cpu().numpy(), None if mask is None else mask.cpu().numpy(), None if visib is None else visib.cpu().numpy()


def test_fixture_info_extents_and_masks_in_both_canvas_modes(hip):
    g = GG.load()
    W, H = g["dataset"]["im_size"]
    info, mask, visib = _fixture(g, (W, H))
    assert np.array_equal(info, g["raw_canvas"])                # the three counts the script wrote and the raw extents of its renders
    assert BG.gt_info_records(info) == g["records"]             # scene_gt_info.json, dict for dict
    assert np.array_equal(mask == 255, g["mask"]) and np.array_equal(visib == 255, g["mask_visib"])
    assert set(np.unique(mask)) == {0, 255}
    info, mask, visib = _fixture(g, (0, 0))
    assert np.array_equal(info, g["raw_plain"])                 # counts and extents of the mask images calc_gt_masks.py wrote
    assert np.array_equal(mask == 255, g["mask"]) and np.array_equal(visib == 255, g["mask_visib"])
    assert np.array_equal(_fixture(g, (W, H), want_masks=False)[0], g["raw_canvas"])


# ---- 9. the public layer on the fixture's tree --------------------------------------------------------------------------------------------------
def test_from_bop_dir_computes_scene_gt_info_and_the_writers_round_trip(hip, tmp_path):
    from PIL import Image

    from gdrnpp_bop2022_amd.gdrn_modeling import bop_eval as BE

    g = GG.load()
    d = g["dataset"]
    scene, split = d["scene_id"], d["split"]
    with_file = GG.write_tree(g, tmp_path / "a", with_info=True)
    without = GG.write_tree(g, tmp_path / "b", with_info=False)
    from_file = BE.BopGT.from_bop_dir(with_file)
    want = {scene: {im: [dict(visib_fract=r["visib_fract"]) for r in recs] for im, recs in g["scene_gt_info"].items()}}
    assert from_file.scene_gt_info == want
    for base, mode in ((without, "compute"), (without, "auto"), (with_file, "compute")):
        gt = BE.BopGT.from_bop_dir(base, gt_info=mode)
        assert gt.scene_gt_info == want, mode                       # the recorded visib_fract list, float for float
        assert gt.depth is None and gt.faces is None                # with_depth was not asked for
        targets = BE._organize_targets(gt.targets)[scene]
        assert BE.valid_gts(gt, scene, targets) == BE.valid_gts(from_file, scene, targets)
    own = str(tmp_path / "c" / "my_dataset")                        # a dataset VSD_DELTAS does not know: the tolerance must be given
    os.rename(GG.write_tree(g, tmp_path / "c", with_info=False), own)
    with pytest.raises(ValueError, match="vsd_delta"):
        BE.BopGT.from_bop_dir(own, gt_info="compute")
    assert BE.BopGT.from_bop_dir(own, gt_info="compute", vsd_delta=g["delta"]).scene_gt_info == want
    # the two walks and their writers
    ms = hip_lib.MeshSet(g["verts_list"], g["faces_list"], DEV)
    walk = (g["scene_gt"], g["scene_camera"], g["depth_stored"], ms, d["obj_ids"], d["im_size"], g["delta"])
    computed = BG.calc_gt_info(*walk)
    assert computed == g["scene_gt_info"]
    raw = BG.calc_gt_info(*walk, raw=True)
    assert np.array_equal(np.array([raw[im][k] for im, k in g["poses"]["keys"]]), g["raw_canvas"])
    path = BG.write_scene_gt_info(without, split, scene, computed)
    assert path == os.path.join(without, split, f"{scene:06d}", "scene_gt_info.json")
    assert {int(k): v for k, v in json.load(open(path)).items()} == g["scene_gt_info"]
    assert BE.BopGT.from_bop_dir(without).scene_gt_info == want      # "file" now finds what was written
    by_path = {im: os.path.join(without, split, f"{scene:06d}", "depth", f"{im:06d}.png") for im in g["scene_gt"]}
    assert BG.write_gt_masks(without, split, scene, BG.calc_gt_masks(*walk[:2], by_path, *walk[3:])) == len(g["poses"]["keys"])
    for n, (im, k) in enumerate(g["poses"]["keys"]):
        for sub, rec in (("mask", g["mask"]), ("mask_visib", g["mask_visib"])):
            with Image.open(os.path.join(without, split, f"{scene:06d}", sub, f"{im:06d}_{k:06d}.png")) as f:
                arr = np.asarray(f)
            assert arr.dtype == np.uint8 and np.array_equal(arr, rec[n].astype(np.uint8) * 255), (sub, im, k)


def test_evaluator_scores_a_split_without_scene_gt_info(hip, tmp_path):
    """``GDRN_Evaluator(bop_gt=BopGT.from_bop_dir(..., gt_info="compute"))`` on a split that has no scene_gt_info.json gives the scores
    it gives with the recorded file: which ground truths are valid is decided by the computed visib_fract."""
    from gdrnpp_bop2022_amd.gdrn_modeling import bop_eval as BE
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from gdrnpp_bop2022_amd.gdrn_modeling.gdrn_evaluator import GDRN_Evaluator

    g = GG.load()
    d = g["dataset"]
    rng = np.random.default_rng(29)
    records = []
    for im, gts in g["scene_gt"].items():
        for k, x in enumerate(gts):
            t = np.asarray(x["cam_t_m2c"]) + rng.standard_normal(3) * (2.0 if k % 2 else 40.0)
            records.append(dict(scene_id=str(d["scene_id"]), im_id=im, obj_id=x["obj_id"], score=0.5 + 0.01 * k, R=np.asarray(x["cam_R_m2c"]).reshape(3, 3).tolist(),
                                t=t.tolist(), time=0.05))
    names = [f"obj_{o:06d}" for o in d["obj_ids"]]
    scores = {}
    for what, with_info, mode in (("file", True, "file"), ("compute", False, "compute")):
        gt = BE.BopGT.from_bop_dir(GG.write_tree(g, tmp_path / what, with_info=with_info), gt_info=mode)
        cfg = get_cfg("ycbv_convnext_a6")
        cfg.EXP_ID = "gdrn"
        cfg.VAL.USE_BOP = True
        cfg.VAL.SAVE_BOP_CSV_ONLY = False
        cfg.VAL.ERROR_TYPES = "mssd,mspd"
        cfg.VAL.N_TOP = -1
        out = tmp_path / (what + "_out")
        out.mkdir()
        ev = GDRN_Evaluator(cfg, d["name"] + "_test", False, str(out), obj_names=names, obj2id=dict(zip(names, d["obj_ids"])), bop_gt=gt)
        ev.reset()
        ev._predictions = [dict(r) for r in records]
        scores[what] = {k: v for k, v in ev.evaluate().items() if k.startswith("bop19_")}
    print(scores)
    assert scores["compute"] == scores["file"] and 0.0 < scores["file"]["bop19_average_recall_mssd"] < 1.0
