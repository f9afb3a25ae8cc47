"""Parity of the HIP path against the CPU oracle on the same seeded inputs (-m gpu).
Bit-exact for indices / flags / counts / depth maps; fp tolerances are stated per test."""
import os

import numpy as np
import pytest
import torch

from gdrnpp_bop2022_amd import synthetic as S
from oracle import postproc as P
from test_postproc_oracle import make_case

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.to(DEV)


# ------------------------------------------------------------------ FPS
def test_fps_golden_bit_exact(hip, golden_dir):
    g = np.load(os.path.join(golden_dir, "fps_golden.npz"))
    k = 0
    while f"pts{k}" in g:
        pts, ic, rd = g[f"pts{k}"], g[f"init_center{k}"], g[f"random{k}"]
        out = hip.fps(T(pts)[None], len(ic), init_center=True).cpu().numpy()[0]
        assert np.array_equal(out, ic), k
        out = hip.fps(T(pts)[None], len(rd), init_center=False,
                      start_idx=torch.tensor([int(rd[0])], dtype=torch.int32, device=DEV)).cpu().numpy()[0]
        assert np.array_equal(out, rd), k
        k += 1


@pytest.mark.parametrize("pn,sn", [(2562, 8), (12288, 64), (12289, 32), (100000, 16), (5, 9)])
def test_fps_batched_vs_oracle(hip, pn, sn):
    rng = np.random.default_rng(pn)
    pts = (rng.standard_normal((3, pn, 3)) * 0.1).astype(np.float32)
    out = hip.fps(T(pts), sn, init_center=True).cpu().numpy()
    start = rng.integers(0, pn, 3).astype(np.int32)
    out2 = hip.fps(T(pts), sn, init_center=False, start_idx=T(start)).cpu().numpy()
    for b in range(3):
        assert np.array_equal(out[b], P.fps(pts[b], sn, True))
        assert np.array_equal(out2[b], P.fps(pts[b], sn, False, int(start[b])))


def test_fps_host_abi_symbols(hip):
    """The cffi-shaped drop-in symbols (host pointers, fps/src/ext.h:1-14) called like fps_utils.py:13-19."""
    import ctypes
    lib = hip.load()
    rng = np.random.default_rng(0)
    pts = rng.standard_normal((3000, 3)).astype(np.float32)
    idxs = np.zeros(16, np.int32)
    lib.farthest_point_sampling_init_center(pts.ctypes.data_as(ctypes.c_void_p), idxs.ctypes.data_as(ctypes.c_void_p),
                                            3000, 16)
    assert np.array_equal(idxs, P.fps(pts, 16, True))
    lib.farthest_point_sampling(pts.ctypes.data_as(ctypes.c_void_p), idxs.ctypes.data_as(ctypes.c_void_p), 3000, 16)
    assert np.array_equal(idxs, P.fps(pts, 16, False, int(idxs[0])))


# ------------------------------------------------------------------ NN distance
def test_nnd_golden_bit_exact(hip, golden_dir):
    g = np.load(os.path.join(golden_dir, "nnd_golden.npz"))
    for k in range(3):
        x1, x2 = T(g[f"x1_{k}"]), T(g[f"x2_{k}"])
        b, n, _ = x1.shape
        m = x2.shape[1]
        d1 = torch.zeros(b, n, device=DEV); d2 = torch.zeros(b, m, device=DEV)
        i1 = torch.zeros(b, n, dtype=torch.int32, device=DEV); i2 = torch.zeros(b, m, dtype=torch.int32, device=DEV)
        hip.nnd_forward(x1, x2, d1, d2, i1, i2)
        assert np.array_equal(i1.cpu().numpy(), g[f"i1_{k}"]) and np.array_equal(i2.cpu().numpy(), g[f"i2_{k}"])
        assert np.array_equal(d1.cpu().numpy(), g[f"d1_{k}"]) and np.array_equal(d2.cpu().numpy(), g[f"d2_{k}"])
        g1 = torch.empty_like(x1); g2 = torch.empty_like(x2)
        hip.nnd_backward(x1, x2, g1, g2, T(g[f"gd1_{k}"]), T(g[f"gd2_{k}"]), i1, i2)
        # atomics reorder the fp32 scatter-add: tolerance instead of bit equality
        np.testing.assert_allclose(g1.cpu().numpy(), g[f"g1_{k}"], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(g2.cpu().numpy(), g[f"g2_{k}"], rtol=1e-5, atol=1e-6)


def test_nnd_reference_smoke_size(hip):
    """core/csrc/torch_nndistance/test.py sizes: [10,1000,3] vs [10,1500,3]."""
    rng = np.random.default_rng(7)
    x1 = rng.uniform(0, 1, (10, 1000, 3)).astype(np.float32)
    x2 = rng.uniform(0, 1, (10, 1500, 3)).astype(np.float32)
    d1 = torch.zeros(10, 1000, device=DEV); d2 = torch.zeros(10, 1500, device=DEV)
    i1 = torch.zeros(10, 1000, dtype=torch.int32, device=DEV); i2 = torch.zeros(10, 1500, dtype=torch.int32, device=DEV)
    hip.nnd_forward(T(x1), T(x2), d1, d2, i1, i2)
    od1, od2, oi1, oi2 = P.nnd_forward(x1, x2)
    assert np.array_equal(i1.cpu().numpy(), oi1) and np.array_equal(i2.cpu().numpy(), oi2)
    assert np.array_equal(d1.cpu().numpy(), od1) and np.array_equal(d2.cpu().numpy(), od2)


# ------------------------------------------------------------------ RANSAC voting
def _voting_case(rng, tn=1500, vn=9, hn=128):
    coords = np.stack([rng.integers(0, 64, tn), rng.integers(0, 64, tn)], 1).astype(np.float32)
    kp = rng.uniform(-20, 84, (vn, 2)).astype(np.float32)
    d = kp[None] - coords[:, None]
    d = d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-6) + rng.normal(0, 0.05, d.shape)
    direct = d.astype(np.float32)
    direct[:5] = 0  # zero-norm directions
    idxs = rng.integers(0, tn, (hn, vn, 2)).astype(np.int32)
    idxs[0, :, 1] = idxs[0, :, 0]  # degenerate (parallel) pairs
    return direct, coords, idxs


@pytest.mark.parametrize("vp", [False, True])
def test_ransac_voting_kernels_bit_exact(hip, vp):
    lib = hip.load()
    rng = np.random.default_rng(11)
    direct, coords, idxs = _voting_case(rng)
    tn, vn, _ = direct.shape
    hn = idxs.shape[0]
    hyp_o = P.generate_hypothesis(direct, coords, idxs, vp)
    d_direct, d_coords, d_idxs = T(direct), T(coords), T(idxs)
    hyp = torch.full((hn, vn, 3 if vp else 2), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream
    gen = lib.gdrnpp_generate_hypothesis_vanishing_point if vp else lib.gdrnpp_generate_hypothesis
    assert gen(d_direct.data_ptr(), d_coords.data_ptr(), d_idxs.data_ptr(), hyp.data_ptr(), tn, vn, hn, st) == 0
    assert np.array_equal(hyp.cpu().numpy().view(np.uint32), hyp_o.view(np.uint32))
    for thr in (0.99, 0.999):
        inl_o = P.voting_for_hypothesis(direct, coords, hyp_o, thr, vp)
        inl = torch.zeros((hn, vn, tn), dtype=torch.uint8, device=DEV)
        vote = lib.gdrnpp_voting_for_hypothesis_vanishing_point if vp else lib.gdrnpp_voting_for_hypothesis
        assert vote(d_direct.data_ptr(), d_coords.data_ptr(), hyp.data_ptr(), inl.data_ptr(), tn, vn, hn, thr, st) == 0
        assert np.array_equal(inl.cpu().numpy(), inl_o)
        cnt = torch.zeros((hn, vn), dtype=torch.int32, device=DEV)
        assert lib.gdrnpp_vote_count(d_direct.data_ptr(), d_coords.data_ptr(), hyp.data_ptr(), cnt.data_ptr(), tn, vn,
                                     hn, thr, 1 if vp else 0, st) == 0
        assert np.array_equal(cnt.cpu().numpy(), inl_o.sum(2).astype(np.int32))
        assert inl_o.sum() > 0


# ------------------------------------------------------------------ uncertainty PnP
def test_upnp_batched_vs_oracle(hip, golden_dir):
    """fp64; tolerance 1e-9 on (angle-axis, t) against the oracle running the same LM schedule,
    and identical iteration counts / termination codes."""
    g = np.load(os.path.join(golden_dir, "upnp_golden.npz"))
    for k in range(3):
        p2, p3, w, init = g[f"lm_p2_{k}"], g[f"lm_p3_{k}"], g[f"lm_w_{k}"], g[f"lm_init_{k}"]
        b = 5
        rng = np.random.default_rng(k)
        inits = init[None] + rng.uniform(-0.02, 0.02, (b, 6))
        P2, P3, W = np.tile(p2, (b, 1, 1)), np.tile(p3, (b, 1, 1)), np.tile(w, (b, 1, 1))
        Kb = np.tile(g["K"], (b, 1))
        out, info = hip.uncertainty_pnp_batched(T(P2), T(P3), T(W), T(Kb), T(inits), return_info=True)
        o_out, o_info = P.uncertainty_pnp_batched(P2, P3, W, Kb, inits)
        np.testing.assert_allclose(out.cpu().numpy(), o_out, atol=1e-9)
        assert np.array_equal(info.cpu().numpy(), o_info)
        np.testing.assert_allclose(out.cpu().numpy()[0], g[f"lm_opt_{k}"], atol=1e-4)  # R/t within 1e-4 of the optimum


def test_upnp_host_abi_symbol(hip):
    import ctypes
    lib = hip.load()
    rng = np.random.default_rng(5)
    K = np.array([400.0, 0, 128, 0, 400, 128, 0, 0, 1])
    rt = np.array([0.3, -0.2, 0.5, 0.1, -0.05, 1.2])
    p3 = rng.uniform(0, 1, (8, 3)) - 0.5
    init = rt + rng.uniform(0, 0.1, 6)
    th = np.linalg.norm(rt[:3]); k = rt[:3] / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    R = np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx
    X = p3 @ R.T + rt[3:]
    p2 = np.ascontiguousarray(np.stack([400 * X[:, 0] / X[:, 2] + 128, 400 * X[:, 1] / X[:, 2] + 128], 1))
    w = np.tile([1.0, 0.0, 1.0], (8, 1))
    res = np.zeros(6)
    vp = ctypes.c_void_p
    lib.uncertainty_pnp(p2.ctypes.data_as(vp), p3.ctypes.data_as(vp), w.ctypes.data_as(vp), K.ctypes.data_as(vp),
                        init.ctypes.data_as(vp), res.ctypes.data_as(vp), 8)
    np.testing.assert_allclose(res, rt, atol=1e-6)
    np.testing.assert_allclose(res, P.uncertainty_pnp(p2, p3, w, K, init), atol=1e-10)


# ------------------------------------------------------------------ maps: decode + correspondences, pose, zoom K
@pytest.mark.parametrize("seed", [0, 1])
def test_decode_correspondences_bit_exact(hip, seed):
    verts, faces, det, maps = make_case(b=12, seed=seed)
    maps["mask"][3] = 1.0  # constant map -> NaN mask -> zero correspondences (sentinel pose path)
    cnt, sel, ip, mp, om = hip.decode_correspondences(
        T(maps["coor_x"]), T(maps["coor_y"]), T(maps["coor_z"]), T(maps["mask"]), T(maps["roi_coord_2d"]),
        T(det["roi_extent"]), T(np.stack([det["im_W"], det["im_H"]], 1)))
    cnt, sel, ip, mp, om = (x.cpu().numpy() for x in (cnt, sel, ip, mp, om))
    omask = P.get_out_mask(maps["mask"])
    assert np.array_equal(om.view(np.uint32), omask.view(np.uint32))
    for i in range(12):
        xyz = np.concatenate([maps["coor_x"][i], maps["coor_y"][i], maps["coor_z"][i]], 0).transpose(1, 2, 0)
        oip, omp, osel = P.get_img_model_points_with_coords2d(omask[i, 0], xyz, maps["roi_coord_2d"][i].transpose(1, 2, 0),
                                                              480, 640, det["roi_extent"][i])
        n = len(oip)
        assert cnt[i] == n
        assert np.array_equal(sel[i, :n], np.flatnonzero(osel.reshape(-1)))
        assert np.array_equal(ip[i, :n].view(np.uint32), oip.view(np.uint32))
        assert np.array_equal(mp[i, :n].view(np.uint32), omp.view(np.uint32))
    assert cnt[3] == 0 and cnt.sum() > 100


@pytest.mark.parametrize("res", [8, 32, 48, 64, 80])
def test_decode_correspondences_other_map_sizes(hip, res):
    """OUTPUT_RES other than 64: up to 64 x 64 the register-resident kernel (ragged last wave at 48 x 48, a single
    partial wave at 8 x 8), above it the looping kernel; random maps, one constant mask, one mask with a NaN."""
    rng = np.random.default_rng(res)
    b = 5
    cx, cy, cz = (rng.random((b, 1, res, res), dtype=np.float32) for _ in range(3))
    cx[rng.random(cx.shape) < 0.2] = 0.5                     # |x| <= 1e-4 * extent -> rejected
    mask = rng.standard_normal((b, 1, res, res)).astype(np.float32)
    mask[1] = 0.25
    mask[2, 0, res // 2, 1] = np.nan
    c2 = rng.random((b, 2, res, res), dtype=np.float32)
    ext = rng.uniform(0.05, 0.3, (b, 3)).astype(np.float32)
    imwh = np.tile(np.array([[640.0, 480.0]], np.float32), (b, 1))
    cnt, sel, ip, mp, om = hip.decode_correspondences(T(cx), T(cy), T(cz), T(mask), T(c2), T(ext), T(imwh))
    cnt, sel, ip, mp, om = (x.cpu().numpy() for x in (cnt, sel, ip, mp, om))
    with np.errstate(invalid="ignore", divide="ignore"):
        omask = P.get_out_mask(mask)
    assert np.array_equal(om.view(np.uint32)[[0, 3, 4]], omask.view(np.uint32)[[0, 3, 4]])
    assert np.isnan(om[1]).all() and np.isnan(om[2]).all()    # 0/0 and NaN min/max: nothing selected
    for i in range(b):
        xyz = np.concatenate([cx[i], cy[i], cz[i]], 0).transpose(1, 2, 0)
        with np.errstate(invalid="ignore"):
            oip, omp, osel = P.get_img_model_points_with_coords2d(omask[i, 0], xyz, c2[i].transpose(1, 2, 0), 480, 640, ext[i])
        n = len(oip)
        assert cnt[i] == n
        assert np.array_equal(sel[i, :n], np.flatnonzero(osel.reshape(-1)))
        assert np.array_equal(ip[i, :n].view(np.uint32), oip.view(np.uint32))
        assert np.array_equal(mp[i, :n].view(np.uint32), omp.view(np.uint32))
    assert cnt[1] == 0 and cnt[2] == 0 and cnt[0] > 0


def test_pose_from_pred_and_zoom_K(hip):
    rng = np.random.default_rng(3)
    b = 64
    det = S.make_detections(b, 5, np.full((5, 3), 0.1, np.float32), rng)
    rot6d = rng.standard_normal((b, 6)).astype(np.float32)
    t_ = np.concatenate([rng.uniform(-0.2, 0.2, (b, 2)), rng.uniform(0.5, 2.0, (b, 1))], 1).astype(np.float32)
    rot, trans = hip.pose_from_pred_centroid_z(T(rot6d), T(t_), T(det["roi_cam"]), T(det["roi_center"]),
                                               T(det["roi_wh"]), T(det["resize_ratio"]))
    Ra = P.rot6d_to_mat_batch(rot6d)
    Re, tr = P.pose_from_predictions_test(Ra, t_[:, :2], t_[:, 2:3], det["roi_cam"], det["roi_center"],
                                          det["resize_ratio"], det["roi_wh"])
    np.testing.assert_allclose(trans.cpu().numpy(), tr, rtol=1e-6, atol=1e-7)   # fp32 op order
    np.testing.assert_allclose(rot.cpu().numpy(), Re, atol=2e-6)                # R within 1e-4 required
    Kc = hip.zoom_K(T(det["roi_cam"]), T(det["roi_center"]), T(det["scale"]), 64).cpu().numpy()
    assert np.array_equal(Kc, P.zoom_K(det["roi_cam"], det["roi_center"], det["scale"], 64))


# ------------------------------------------------------------------ depth render + refine
def test_render_depth_bit_exact(hip):
    verts, faces, det, maps = make_case(b=10, seed=2, subdiv=4, num_classes=3)
    meshes = hip.MeshSet(verts, faces)
    d, x = hip.render_depth(meshes, T(det["roi_cls"].astype(np.int32)), T(maps["K_crop"]), T(det["R_gt"]),
                            T(det["t_gt"]), 64, want_xyz=True)
    d, x = d.cpu().numpy(), x.cpu().numpy()
    for i in range(10):
        o = int(det["roi_cls"][i])
        od, ox = P.render_depth(verts[o], faces[o], maps["K_crop"][i], det["R_gt"][i],
                                det["t_gt"][i].astype(np.float64), 64, want_xyz=True)
        assert np.array_equal(d[i].view(np.uint32), od.view(np.uint32)), i
        assert (od > 0).sum() > 50
        np.testing.assert_allclose(x[i], ox, atol=1e-6)


def test_render_depth_low_poly_and_behind_camera(hip):
    """Large triangles (cooperative path) and triangles crossing the camera plane."""
    v = np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0], [0, 0, 3.0]], np.float32)
    f = np.array([[0, 1, 2], [0, 2, 3], [0, 1, 4], [1, 2, 4]], np.int32)
    meshes = hip.MeshSet([v], [f])
    K = np.array([[[60.0, 0, 32], [0, 60, 32], [0, 0, 1]]], np.float32)
    ang = 1.2
    R = np.array([[[1, 0, 0], [0, np.cos(ang), -np.sin(ang)], [0, np.sin(ang), np.cos(ang)]]], np.float32)
    t = np.array([[0.0, 0.2, 0.9]], np.float32)
    d = hip.render_depth(meshes, torch.zeros(1, dtype=torch.int32, device=DEV), T(K), T(R), T(t), 64).cpu().numpy()[0]
    od = P.render_depth(v, f, K[0], R[0], t[0].astype(np.float64), 64)
    assert np.array_equal(d.view(np.uint32), od.view(np.uint32))
    assert (od > 0).sum() > 500


@pytest.mark.parametrize("use_coor_z", [False, True])
def test_depth_refine_vs_oracle(hip, use_coor_z):
    """Renders bit-exact; refined translation within 1e-6 m of the NumPy restatement (required: 1e-4)."""
    b = 16
    verts, faces, det, maps = make_case(b=b, seed=4, subdiv=4, num_classes=5)
    maps["roi_depth"][5] = 0.0   # no valid sensor depth -> norm_sum == 0 -> translation unchanged
    meshes = hip.MeshSet(verts, faces)
    t_out, dbg = hip.depth_refine(meshes, T(det["roi_cls"].astype(np.int32)), T(maps["coor_x"]), T(maps["coor_y"]),
                                  T(maps["coor_z"]), T(maps["mask"]), T(maps["roi_depth"]), T(maps["K_crop"]),
                                  T(det["R_gt"]), T(maps["t_init"]), use_coor_z=use_coor_z, debug=True)
    t_out, dbg = t_out.cpu().numpy(), dbg.cpu().numpy()
    omask = P.get_out_mask(maps["mask"])
    moved = 0
    for i in range(b):
        o = int(det["roi_cls"][i])
        xyz = np.concatenate([maps["coor_x"][i], maps["coor_y"][i], maps["coor_z"][i]], 0).transpose(1, 2, 0)
        ot, rend = P.depth_refine_roi(xyz, omask[i, 0], maps["roi_depth"][i, 0], maps["K_crop"][i], det["R_gt"][i],
                                      maps["t_init"][i], verts[o], faces[o], use_coor_z=use_coor_z, return_debug=True)
        assert np.array_equal(dbg[i, 0].view(np.uint32), rend[0].view(np.uint32)), i
        np.testing.assert_allclose(t_out[i], ot, atol=1e-6, rtol=0)
        moved += int(np.abs(ot - maps["t_init"][i]).max() > 1e-4)
    assert np.array_equal(t_out[5], maps["t_init"][5].astype(np.float64))
    assert moved >= b - 3
    if not use_coor_z:
        err0 = np.abs(maps["t_init"][:, 2] - det["t_gt"][:, 2])
        err1 = np.abs(t_out[:, 2] - det["t_gt"][:, 2])
        assert np.median(np.delete(err1, 5)) < 0.3 * np.median(np.delete(err0, 5))


def test_depth_refine_full_size_properties(hip):
    """BASELINE config 3 size (128 ROIs, 2562/5120 meshes): size-independent properties —
    idempotence of a zero-iteration call, determinism across launches, and agreement of the fused
    kernel with (stand-alone render + oracle compare) on a sample of ROIs."""
    b = 128
    rng = np.random.default_rng(9)
    verts, faces, ext = S.make_models(21, rng, 4)
    det = S.make_detections(b, 21, ext, rng)
    meshes = hip.MeshSet(verts, faces)

    def render_fn(obj, K, R, t, res):
        d, x = hip.render_depth(meshes, T(obj), T(K), T(R), T(t), res, want_xyz=True)
        return d.cpu().numpy(), x.cpu().numpy()

    maps = S.make_map_inputs(det, verts, faces, render_fn, rng)
    args = (meshes, T(det["roi_cls"].astype(np.int32)), T(maps["coor_x"]), T(maps["coor_y"]), T(maps["coor_z"]),
            T(maps["mask"]), T(maps["roi_depth"]), T(maps["K_crop"]), T(det["R_gt"]), T(maps["t_init"]))
    t0 = hip.depth_refine(*args, iters=0).cpu().numpy()
    assert np.array_equal(t0, maps["t_init"].astype(np.float64))
    t1 = hip.depth_refine(*args).cpu().numpy()
    t2 = hip.depth_refine(*args).cpu().numpy()
    assert np.array_equal(t1, t2)
    omask = P.get_out_mask(maps["mask"])
    for i in range(0, b, 16):
        o = int(det["roi_cls"][i])
        xyz = np.concatenate([maps["coor_x"][i], maps["coor_y"][i], maps["coor_z"][i]], 0).transpose(1, 2, 0)
        ot = P.depth_refine_roi(xyz, omask[i, 0], maps["roi_depth"][i, 0], maps["K_crop"][i], det["R_gt"][i],
                                maps["t_init"][i], verts[o], faces[o])
        np.testing.assert_allclose(t1[i], ot, atol=1e-6, rtol=0)
    err0 = np.abs(maps["t_init"][:, 2] - det["t_gt"][:, 2])
    err1 = np.abs(t1[:, 2] - det["t_gt"][:, 2])
    assert np.median(err1) < 0.3 * np.median(err0)


def test_decode_and_refine_sigmoid_mask_type(hip):
    """MASK_LOSS_TYPE = BCE: get_out_mask is a sigmoid (engine_utils.py:326-328).  exp() differs in the last ulps
    between libm and the device, so the mask is compared to 1e-6 and the selection on pixels away from the 0.5 tie."""
    verts, faces, det, maps = make_case(b=6, seed=12, subdiv=3)
    logits = ((maps["mask"] - maps["mask"].mean()) * 4).astype(np.float32)
    cnt, sel, ip, mp, om = hip.decode_correspondences(
        T(maps["coor_x"]), T(maps["coor_y"]), T(maps["coor_z"]), T(logits), T(maps["roi_coord_2d"]),
        T(det["roi_extent"]), T(np.stack([det["im_W"], det["im_H"]], 1)), mask_type=1)
    omask = P.get_out_mask(logits, "BCE")
    np.testing.assert_allclose(om.cpu().numpy(), omask, atol=1e-6)
    for i in range(6):
        xyz = np.concatenate([maps["coor_x"][i], maps["coor_y"][i], maps["coor_z"][i]], 0).transpose(1, 2, 0)
        _, _, osel = P.get_img_model_points_with_coords2d(omask[i, 0], xyz, maps["roi_coord_2d"][i].transpose(1, 2, 0),
                                                          480, 640, det["roi_extent"][i])
        mine = np.zeros(4096, bool)
        mine[sel[i, :int(cnt[i])].cpu().numpy()] = True
        safe = np.abs(logits[i, 0].reshape(-1)) > 1e-4
        assert np.array_equal(mine[safe], osel.reshape(-1)[safe])
    meshes = hip.MeshSet(verts, faces)
    t = hip.depth_refine(meshes, T(det["roi_cls"].astype(np.int32)), T(maps["coor_x"]), T(maps["coor_y"]),
                         T(maps["coor_z"]), T(logits), T(maps["roi_depth"]), T(maps["K_crop"]), T(det["R_gt"]),
                         T(maps["t_init"]), mask_type=1).cpu().numpy()
    for i in range(6):
        o = int(det["roi_cls"][i])
        xyz = np.concatenate([maps["coor_x"][i], maps["coor_y"][i], maps["coor_z"][i]], 0).transpose(1, 2, 0)
        ot = P.depth_refine_roi(xyz, omask[i, 0], maps["roi_depth"][i, 0], maps["K_crop"][i], det["R_gt"][i],
                                maps["t_init"][i], verts[o], faces[o])
        np.testing.assert_allclose(t[i], ot, atol=1e-5)


def test_fallback_refine_kernel_for_large_meshes(hip):
    """Meshes above the LDS staging limit (kMaxStagedVerts = 2688 vertices) take the non-staged kernel: same results.  The limit
    itself is tests/test_gpu_refine_edges.py's."""
    b = 4
    verts, faces, det, maps = make_case(b=b, seed=13, subdiv=5, num_classes=2)   # 10242 V / 20480 F
    assert len(verts[0]) > 4096
    meshes = hip.MeshSet(verts, faces)
    t_out, dbg = hip.depth_refine(meshes, T(det["roi_cls"].astype(np.int32)), T(maps["coor_x"]), T(maps["coor_y"]),
                                  T(maps["coor_z"]), T(maps["mask"]), T(maps["roi_depth"]), T(maps["K_crop"]),
                                  T(det["R_gt"]), T(maps["t_init"]), debug=True)
    omask = P.get_out_mask(maps["mask"])
    for i in range(b):
        o = int(det["roi_cls"][i])
        xyz = np.concatenate([maps["coor_x"][i], maps["coor_y"][i], maps["coor_z"][i]], 0).transpose(1, 2, 0)
        ot, rend = P.depth_refine_roi(xyz, omask[i, 0], maps["roi_depth"][i, 0], maps["K_crop"][i], det["R_gt"][i],
                                      maps["t_init"][i], verts[o], faces[o], return_debug=True)
        assert np.array_equal(dbg[i, 0].cpu().numpy().view(np.uint32), rend[0].view(np.uint32))
        np.testing.assert_allclose(t_out[i].cpu().numpy(), ot, atol=1e-6, rtol=0)


def test_net_iter_pnp_from_correspondences(hip):
    """TEST.USE_PNP / PNP_TYPE=net_iter_pnp (gdrn_evaluator.py:241-371): decode -> compaction -> net-initialised LM,
    all ROIs in one launch, against the per-ROI NumPy/C oracle.  R, t within 1e-5 (bar 1e-4); with clean synthetic
    maps the refined pose must be much closer to the ground truth than the perturbed network pose."""
    b = 12
    verts, faces, det, maps = make_case(b=b, seed=21, subdiv=3)
    maps["mask"][2] = 1.0                                   # constant mask -> 0 correspondences -> network pose kept
    rng = np.random.default_rng(0)
    R_net = np.stack([det["R_gt"][i] @ P.rodrigues_exp(rng.normal(0, 0.03, 3)).astype(np.float32) for i in range(b)])
    t_net = (det["t_gt"] + rng.normal(0, 0.01, (b, 3))).astype(np.float32)
    cnt, sel, ip, mp, om = hip.decode_correspondences(
        T(maps["coor_x"]), T(maps["coor_y"]), T(maps["coor_z"]), T(maps["mask"]), T(maps["roi_coord_2d"]),
        T(det["roi_extent"]), T(np.stack([det["im_W"], det["im_H"]], 1)))
    R, t, info = hip.pnp_iter_from_correspondences(ip, mp, cnt, T(det["roi_cam"].reshape(b, 9)), T(R_net.reshape(b, 9)),
                                                   T(t_net), return_info=True)
    R, t, cnt = R.cpu().numpy(), t.cpu().numpy(), cnt.cpu().numpy()
    omask = P.get_out_mask(maps["mask"])
    err_net, err_pnp = [], []
    for i in range(b):
        xyz = np.concatenate([maps["coor_x"][i], maps["coor_y"][i], maps["coor_z"][i]], 0).transpose(1, 2, 0)
        oip, omp, _ = P.get_img_model_points_with_coords2d(omask[i, 0], xyz, maps["roi_coord_2d"][i].transpose(1, 2, 0),
                                                           480, 640, det["roi_extent"][i])
        oR, ot = P.net_iter_pnp(oip, omp, det["roi_cam"][i], R_net[i], t_net[i])
        np.testing.assert_allclose(R[i], oR, atol=1e-5)
        np.testing.assert_allclose(t[i], ot, atol=1e-5)
        if i != 2:
            err_net.append(np.linalg.norm(t_net[i] - det["t_gt"][i]))
            err_pnp.append(np.linalg.norm(t[i] - det["t_gt"][i]))
    assert cnt[2] == 0 and np.array_equal(R[2], R_net[2]) and np.array_equal(t[2], t_net[2])
    assert np.median(err_pnp) < 0.5 * np.median(err_net)


def test_flow_forward_bit_exact(hip, golden_dir):
    """gdrnpp_flow_forward vs the oracle (and through it the reference's flow_cpu.cpp golden): flow and valid bit-exact,
    single images and a mixed batch; plus the flow_torch shim (pose inputs)."""
    import os
    from oracle import postproc as P
    g = np.load(os.path.join(golden_dir, "flow_golden.npz"))
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    for k in range(3):
        f, v = hip.flow_forward(T(g[f"ds{k}"]), T(g[f"dt{k}"]), T(g[f"KT{k}"]), T(g[f"Kinv{k}"]))
        assert np.array_equal(f.cpu().numpy(), g[f"flow{k}"]) and np.array_equal(v.cpu().numpy(), g[f"valid{k}"])
    rng = np.random.default_rng(3)
    b, h, w = 5, 96, 128
    yy, xx = np.mgrid[0:h, 0:w]
    ds = np.stack([(0.7 + 0.05 * i + 0.1 * np.sin(xx / (9.0 + i)) * np.cos(yy / 7.0))[None] for i in range(b)]).astype(np.float32)
    ds[rng.random(ds.shape) < 0.1] = 0
    dt = (ds + rng.normal(0, 1.5e-3, ds.shape)).astype(np.float32)
    K = np.array([[500.0, 0, 64], [0, 500.0, 48], [0, 0, 1]], np.float32)
    KT = np.stack([K @ np.concatenate([np.eye(3, dtype=np.float32), rng.normal(0, 2e-3, (3, 1)).astype(np.float32)], 1) for _ in range(b)])
    Kinv = np.stack([np.linalg.inv(K).astype(np.float32)] * b)
    fo, vo = P.flow_forward(ds, dt, KT, Kinv)
    f, v = hip.flow_forward(T(ds), T(dt), T(KT), T(Kinv))
    assert np.array_equal(f.cpu().numpy(), fo) and np.array_equal(v.cpu().numpy(), vo) and 0.1 < vo.mean() < 0.95
    from gdrnpp_bop2022_amd.core.csrc.flow.flow_torch import flow as flow_fn
    pose = torch.eye(3, 4, device=DEV).repeat(b, 1, 1)
    f2, v2 = flow_fn(T(ds), T(ds), pose, pose, T(np.stack([K] * b)))
    # identity motion onto itself: valid wherever there is depth, except border pixels whose re-projection rounds outside
    assert v2.shape == (b, 1, h, w) and not ((v2 > 0) & ~(T(ds) > 1e-3)).any() and v2.mean().item() > 0.85
    assert f2.abs().max().item() < 1e-3


@pytest.mark.parametrize("conf,agnostic", [(0.3, False), (0.3, True), (0.001, False), (0.9999, False)])
def test_yolox_postprocess_bit_exact(hip, conf, agnostic):
    """Decode + confidence filter + (batched) NMS vs the oracle: identical kept rows in identical order, including a
    dense low-threshold case (thousands of candidates), duplicate scores (tie order = anchor index) and an image with
    nothing above the threshold."""
    from oracle import postproc as P
    from gdrnpp_bop2022_amd.det.yolox.utils.boxes import postprocess
    rng = np.random.default_rng(7)
    b, a, c = 3, 8400, 21
    det = np.zeros((b, a, 5 + c), np.float32)
    centres = rng.uniform(40, 600, (b, 60, 2))
    which = rng.integers(0, 60, (b, a))
    det[..., 0:2] = np.take_along_axis(centres, which[..., None].repeat(2, -1), 1) + rng.normal(0, 6, (b, a, 2))
    det[..., 2:4] = rng.uniform(30, 160, (b, a, 2))
    det[..., 4] = rng.uniform(0, 1, (b, a)) ** 2
    det[..., 5:] = rng.uniform(0, 1, (b, a, c)) ** 4
    det[0, 100:140] = det[0, 100]          # exact duplicates: equal scores, fully overlapping
    det[2, :, 4] *= 1e-4 if conf > 0.1 else 1.0   # image 2: nothing survives a high threshold
    want = P.yolox_postprocess(det, c, conf, 0.45, agnostic)
    got = postprocess(torch.from_numpy(det).to(DEV), c, conf, 0.45, agnostic)
    n_tot = 0
    for w, g in zip(want, got):
        assert (w is None) == (g is None)
        if w is not None:
            assert np.array_equal(g.cpu().numpy(), w)
            n_tot += len(w)
    if conf < 0.9:
        assert n_tot > 50


def test_yolox_postprocess_equals_the_reference_function(hip):
    """The device ``postprocess`` against yolox_golden.npz: the reference's own ``postprocess`` (det/yolox/utils/boxes.py:34-74)
    executed from its source text, with only torchvision's NMS primitive served by a stand-in (tests/golden/make_golden_yolox.py):
    class-aware and class-agnostic, one class, an image where nothing survives, two-decimal scores (exact ties)."""
    import os

    from gdrnpp_bop2022_amd.det.yolox.utils.boxes import postprocess
    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "yolox_golden.npz"))
    for name in "abcd":
        c, conf, thr, agn = z[name + "_args"]
        got = postprocess(torch.from_numpy(z[name + "_det"].copy()).to(DEV), int(c), float(conf), float(thr), bool(agn))
        counts = [0 if g is None else g.shape[0] for g in got]
        assert counts == z[name + "_count"].tolist(), name
        cat = np.concatenate([np.zeros((0, 7), np.float32)] + [g.cpu().numpy() for g in got if g is not None])
        assert np.array_equal(cat, z[name + "_out"]), name


def test_paste_masks_rle_bit_exact(hip):
    """gdrnpp_paste_masks_rle vs the oracle: identical COCO run lengths per instance (boxes inside, partly outside and
    tiny; an empty and a full mask; a buffer that is too small and gets re-run), and the evaluator-side helper."""
    from oracle import postproc as P
    from gdrnpp_bop2022_amd.gdrn_modeling import engine
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from gdrnpp_bop2022_amd.lib.utils import mask_utils as M
    rng = np.random.default_rng(9)
    yy, xx = np.mgrid[0:64, 0:64]
    H, W = 480, 640
    boxes = np.array([[100.3, 50.7, 260.9, 200.2], [-40.0, 300.0, 120.0, 520.0], [500.0, 100.0, 700.0, 300.0], [320.2, 240.1, 326.9, 249.7],
                      [10.0, 10.0, 200.0, 200.0], [10.0, 10.0, 200.0, 200.0]], np.float32)
    masks = np.stack([(np.clip(1.4 - np.hypot(yy - 31.5 + k, xx - 31.5) / (12.0 + 2 * k), 0, 1) * 0.9 + 0.1 * rng.random((64, 64))) for k in range(6)]).astype(np.float32)
    masks[4] = 0.0
    masks[5] = 1.0
    got = hip.paste_masks_rle(torch.from_numpy(masks).to(DEV), torch.from_numpy(boxes).to(DEV), H, W, 0.5, max_runs=64)
    for i in range(6):
        want = P.paste_mask_rle(masks[i], boxes[i], H, W, 0.5)
        assert got[i] == want, i
    assert got[4] == [H * W] and len(got[5]) > 100
    # ... and against the reference's own encoder (binary_mask_to_rle(compressed=False) run from source: pyref_golden.npz rle_*)
    fx = np.load(os.path.join(os.path.dirname(__file__), "golden", "pyref_golden.npz"))
    gm, lens = fx["rle_masks"], fx["rle_counts_len"]
    want_ref = np.split(fx["rle_counts"], np.cumsum(lens)[:-1])
    gh, gw = gm.shape[1:]
    got_ref = hip.paste_masks_rle(torch.from_numpy(fx["rle_soft"]).to(DEV), torch.from_numpy(fx["rle_boxes"].astype(np.float32)).to(DEV), gh, gw, 0.5)
    assert all(got_ref[k] == want_ref[k].tolist() for k in range(4))
    ident = torch.tensor([[0.0, 0.0, float(gw), float(gh)]] * len(gm), device=DEV)
    got_ref = hip.paste_masks_rle(torch.from_numpy(gm.astype(np.float32)).to(DEV), ident, gh, gw, 0.5, max_runs=256)   # 9 628 runs: re-run with a larger buffer
    assert all(got_ref[k] == want_ref[k].tolist() for k in range(len(gm)))
    cfg = get_cfg("ycbv_convnext_a6", [])
    raw = torch.from_numpy(masks[:4, None] * 3.0 - 1.0).to(DEV)          # un-normalised L1 maps
    centre = torch.from_numpy((boxes[:4, :2] + boxes[:4, 2:]) / 2).to(DEV)
    scale = torch.from_numpy(boxes[:4, 2] - boxes[:4, 0]).to(DEV)
    batch = dict(roi_center=centre, scale=scale, im_H=torch.full((4,), H), im_W=torch.full((4,), W))
    rles = engine.mask_rles(cfg, batch, {"mask": raw})
    assert len(rles) == 4 and all(r["size"] == [H, W] and isinstance(r["counts"], str) for r in rles)
    assert 0 < M.rle_to_binary_mask(rles[0]).sum() < H * W


def test_fused_tail_equals_the_three_launches(hip):
    """gdrnpp_refine_to_records (K_crop + refinement + record packing in ONE launch) against zoom_K -> depth_refine ->
    pack_pose_records: bitwise equal records; an object id outside the mesh set keeps the network translation and is
    marked invalid instead of reading out of bounds."""
    rng = np.random.default_rng(77)
    verts, faces, ext = S.make_models(4, rng, 3)
    b = 9
    det = S.make_detections(b, 4, ext, rng)

    def render_fn(obj, K, R, t, res):
        d, x = zip(*[P.render_depth(verts[obj[i]], faces[obj[i]], K[i], R[i], t[i].astype(np.float64), res_w=res, want_xyz=True)
                     for i in range(len(obj))])
        return np.stack(d), np.stack(x)

    maps = S.make_map_inputs(det, verts, faces, render_fn, rng)
    meshes = hip.MeshSet(verts, faces)
    obj = T(det["roi_cls"].astype(np.int32))
    ids = torch.arange(100, 100 + b, dtype=torch.int32, device=DEV)
    common = (T(maps["coor_x"]), T(maps["coor_y"]), T(maps["coor_z"]), T(maps["mask"]), T(maps["roi_depth"]))
    K_crop = hip.zoom_K(T(det["roi_cam"]).reshape(b, 9), T(det["roi_center"]), T(det["scale"]), 64)
    assert np.array_equal(K_crop.cpu().numpy().reshape(b, 3, 3), maps["K_crop"])
    t_ref = hip.depth_refine(meshes, obj, *common, K_crop, T(det["R_gt"]).reshape(b, 9), T(maps["t_init"]))
    rec3 = hip.pack_pose_records(T(det["R_gt"]).reshape(b, 9), t_ref, T(maps["t_init"]), T(det["score"]), obj, ids)
    rec1 = hip.refine_to_records(meshes, obj, *common, T(det["roi_cam"]).reshape(b, 9), T(det["roi_center"]), T(det["scale"]),
                                 T(det["R_gt"]).reshape(b, 9), T(maps["t_init"]), T(det["score"]), ids)
    assert torch.equal(rec1, rec3)
    bad = obj.clone()
    bad[2] = 17
    bad[5] = -1
    rec_bad = hip.refine_to_records(meshes, bad, *common, T(det["roi_cam"]).reshape(b, 9), T(det["roi_center"]), T(det["scale"]),
                                    T(det["R_gt"]).reshape(b, 9), T(maps["t_init"]), T(det["score"]), ids).cpu().numpy()
    r1 = rec1.cpu().numpy()
    for i in range(b):
        if i in (2, 5):
            assert rec_bad[i, 15] == 0 and np.array_equal(rec_bad[i, 9:12], maps["t_init"][i]) and rec_bad[i, 13] == bad[i].item()
        else:
            assert np.array_equal(rec_bad[i], r1[i])
    with pytest.raises(RuntimeError, match="4 x"):
        hip.depth_refine(meshes, obj, *common[:4], T(maps["roi_depth"][:, :, ::2, ::2].copy()), K_crop, T(det["R_gt"]).reshape(b, 9),
                         T(maps["t_init"]))


def test_pose_from_pred_variants(hip):
    """ROT_TYPE quaternion and TRANS_TYPE centroid_z_abs / trans (GDRN_double_mask.py:162-200) through the one kernel, against
    the reference's own formulas in torch: quat2mat_torch (pose_utils.py:349-400), pose_from_pred_centroid_z_abs.py:44-76,
    pose_from_pred.py:25-27, with the allo -> ego step checked through the rot6d path (pinned by pyref_golden.npz)."""
    torch.manual_seed(0)
    b = 33
    q = torch.randn(b, 4, device=DEV)
    t_ = torch.randn(b, 3, device=DEV) * 0.3
    t_[:, 2] = t_[:, 2].abs() + 0.5
    cams = T(np.repeat(S.YCBV_K.reshape(1, 9), b, 0))
    qn = q / q.norm(dim=1, keepdim=True)
    w, x, y, z = qn.unbind(1)
    Rq = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                      2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                      2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], 1).view(b, 3, 3)
    R_ego, tr = hip.pose_from_pred(q, t_, cams, rot_mode="quat", t_mode="trans", is_allo=False)
    assert torch.equal(tr, t_) and (R_ego - Rq).abs().max().item() < 2e-6
    R_m, _ = hip.pose_from_pred(Rq.reshape(b, 9).contiguous(), t_, cams, rot_mode="mat", t_mode="trans", is_allo=False)
    assert torch.equal(R_m, Rq)
    # allocentric -> egocentric: the quaternion path and the matrix path agree with the rot6d path on the same rotation
    d6 = torch.cat([Rq[:, :, 0], Rq[:, :, 1]], 1).contiguous()
    Ra6, _ = hip.pose_from_pred(d6, t_, cams, rot_mode="rot6d", t_mode="trans", is_allo=True)
    Raq, _ = hip.pose_from_pred(q, t_, cams, rot_mode="quat", t_mode="trans", is_allo=True)
    assert (Ra6 - Raq).abs().max().item() < 5e-6
    # centroid_z_abs: absolute centre (px) and depth
    c = torch.rand(b, 3, device=DEV) * torch.tensor([640.0, 480.0, 1.0], device=DEV) + torch.tensor([0.0, 0.0, 0.4], device=DEV)
    _, ta = hip.pose_from_pred(d6, c, cams, rot_mode="rot6d", t_mode="centroid_z_abs", is_allo=True)
    K = cams.view(b, 3, 3)
    want = torch.stack([c[:, 2] * (c[:, 0] - K[:, 0, 2]) / K[:, 0, 0], c[:, 2] * (c[:, 1] - K[:, 1, 2]) / K[:, 1, 1], c[:, 2]], 1)
    assert torch.equal(ta, want)


def test_every_trans_type_matches_the_reference_functions(hip, golden_dir):
    """gdrnpp_pose_from_pred for TRANS_TYPE centroid_z (Z_TYPE REL / ABS), centroid_z_abs and trans, allocentric and egocentric, against
    the reference's own pose_from_pred_centroid_z / pose_from_pred_centroid_z_abs / pose_from_pred run from their files with
    is_train=False (tests/golden/make_golden_pose.py -> pose_golden.npz), incl. translations on / next to the optical axis (the
    allo -> ego rotation's degenerate branch): t 1e-6 of scale, R 2e-6."""
    g = np.load(f"{golden_dir}/pose_golden.npz")
    b = g["R"].shape[0]
    R9 = T(g["R"]).reshape(b, 9).contiguous()
    cams, centers, whs, rr = T(g["cams"]).reshape(b, 9).contiguous(), T(g["centers"]), T(g["whs"]), T(g["resize_ratios"])
    tin = {"centroid_z_rel": g["t_rel"], "centroid_z_abs_z": g["t_absz"], "centroid_z_abs": g["t_cabs"], "trans": g["t_trans"]}
    for mode, t_ in tin.items():
        for allo in (True, False):
            tag = "allo" if allo else "ego"
            R, t = hip.pose_from_pred(R9, T(t_), cams, centers, whs, rr, rot_mode="mat", t_mode=mode, is_allo=allo)
            eR = np.abs(R.cpu().numpy() - g[f"{mode}_{tag}_R"]).max()
            et = np.abs(t.cpu().numpy() - g[f"{mode}_{tag}_t"]).max()
            assert eR < 2e-6 and et <= 1e-6 * np.abs(g[f"{mode}_{tag}_t"]).max(), (mode, tag, eR, et)
            if not allo:
                assert torch.equal(R, T(g["R"]))


def test_rot_types_match_reference_get_rot_mat(hip, golden_dir):
    """Every ROT_TYPE family of get_rot_mat (model_utils.py:347-359) — quaternion, log-quaternion (quaternion_lf.qexp),
    Lie vector (lie_algebra.lie_vec_to_rot, incl. its first-order small-angle branch) and rot6d — against the reference's own
    functions run from source (tests/golden/make_golden_rot.py -> rot_golden.npz); 2e-6 (fp32 sin / cos of the device)."""
    g = np.load(f"{golden_dir}/rot_golden.npz")
    b = g["quat_in"].shape[0]
    cams = T(np.repeat(S.YCBV_K.reshape(1, 9), b, 0))
    t_ = torch.zeros(b, 3, device=DEV)
    t_[:, 2] = 1.0
    for mode in ("quat", "log_quat", "lie_vec", "rot6d"):
        R, _ = hip.pose_from_pred(T(g[mode + "_in"]), t_, cams, rot_mode=mode, t_mode="trans", is_allo=False)
        err = np.abs(R.cpu().numpy() - g[mode + "_R"]).max()
        assert err < 2e-6, (mode, err)
    # and through GDRN_Net.forward: the config surface accepts the types (rot_dim 3) and returns orthonormal rotations
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from gdrnpp_bop2022_amd.gdrn_modeling.GDRN_double_mask import build_model_optimizer
    for rt in ("allo_log_quat", "ego_lie_vec"):
        cfg = get_cfg("lmo_resnet34_ape", [f"MODEL.POSE_NET.PNP_NET.ROT_TYPE={rt}"])
        torch.manual_seed(0)
        model, _ = build_model_optimizer(cfg)
        assert model.pnp_net.fc_r.out_features == 3
        x = torch.rand(3, 3, 256, 256, device=DEV)
        with torch.no_grad():
            out = model(x, roi_classes=torch.zeros(3, dtype=torch.long, device=DEV), roi_cams=cams[:3].view(3, 3, 3),
                        roi_whs=torch.full((3, 2), 100.0, device=DEV), roi_centers=torch.full((3, 2), 240.0, device=DEV),
                        resize_ratios=torch.full((3,), 0.4, device=DEV), roi_coord_2d=torch.rand(3, 2, 64, 64, device=DEV),
                        roi_extents=torch.full((3, 3), 0.1, device=DEV))
        Rm = out["rot"].double()
        assert (Rm @ Rm.transpose(1, 2) - torch.eye(3, device=DEV, dtype=torch.float64)).abs().max().item() < 1e-5
