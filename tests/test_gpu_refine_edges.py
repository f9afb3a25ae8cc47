"""-m gpu: depth_refine_kernel and render_depth_kernel (csrc/depth_refine.hip) at their queue, stage and size edges, on the cases
of tests/refine_edge_cases.py (whose preconditions, and the agreement of the oracle render with the box-free tests/raster_ref.py,
tests/test_refine_edge_cases_cpu.py asserts).  Every iteration's render is compared with the oracle's BIT FOR BIT; the refined
translation is held to the bar of test_depth_refine_vs_oracle, atol 1e-6 m, rtol 0, against P.depth_refine_roi (the selection of
every case is stable by construction, so a larger difference is the kernel's arithmetic); repeated launches, the LDS-staged and the
workspace kernel on the same geometry, and the fused record tail against its three launches are compared with array_equal."""
from functools import lru_cache

import numpy as np
import pytest
import torch

import raster_ref as RR
import refine_edge_cases as C
from oracle import postproc as P

pytestmark = pytest.mark.gpu
DEV = "cuda"


def T(a):
    return torch.from_numpy(np.array(a, order="C", copy=True)).to(DEV)      # the builders' arrays are read-only


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def maps_of(case):
    return tuple(T(getattr(case, n)) for n in ("coor_x", "coor_y", "coor_z", "mask", "roi_depth"))


def params_of(case):
    return dict(res=case.res, iters=case.iters, threshold=case.threshold, mask_type=case.mask_type, z_near=float(case.z_near),
                z_far=float(case.z_far))


def refine(hip, case, meshes, iters=None):
    """-> t_out f64[b,3], renders f32[b,iters,res,res] of one launch."""
    b = len(case.obj)
    kw = params_of(case)
    if iters is not None:
        kw["iters"] = iters
    t_out, dbg = hip.depth_refine(meshes, T(case.obj), *maps_of(case), T(case.K_crop).reshape(b, 9), T(case.R).reshape(b, 9),
                                  T(case.t_in), debug=True, **kw)
    return t_out.cpu().numpy(), dbg.cpu().numpy()


@lru_cache(maxsize=None)
def oracle(name, *key):
    """Per ROI of a case, from P.depth_refine_roi: [(t f64[3] after k iterations, k = 1..iters), renders]: computed once, shared
    by the tests of that case."""
    case = getattr(C, name)(*key)
    case = case[0] if isinstance(case, tuple) else case
    out = []
    for i in range(len(case.obj)):
        if i in case.kernel_only:
            out.append(None)
            continue
        t_last, renders = C.oracle_refine(case, i, return_debug=True)
        out.append(([C.oracle_refine(case, i, iters=k) for k in range(1, case.iters)] + [t_last], renders))
    return out


def assert_equals_oracle(hip, case, meshes, ref, t_out, dbg, what):
    """Iteration 0's render, and every later one whose pose the kernel and the oracle round to the same float32 values, EQUAL
    to the oracle's (return_debug).  The pose entering iteration k >= 1 is a float64 that the two sides compute in different
    summation orders (held to 1e-6 m here like the final one); both hand its float32 VALUE to the render, and where those
    roundings differ the oracle render is taken at the kernel's float32 pose, read from a launch of k iterations: still the
    oracle's render, still bit for bit."""
    t_after = {k: refine(hip, case, meshes, iters=k)[0] for k in range(1, case.iters)}
    t_after[case.iters] = t_out
    worst, rerendered, bad = 0.0, 0, []
    for i in range(len(case.obj)):
        if ref[i] is None:
            continue
        ts, renders = ref[i]
        o = int(case.obj[i])
        for k in range(case.iters):
            want = renders[k]
            if k and not np.array_equal(bits(t_after[k][i].astype(np.float32)), bits(ts[k - 1].astype(np.float32))):
                rerendered += 1
                want = P.render_depth(case.verts[o], case.faces[o], case.K_crop[i], case.R[i],
                                      t_after[k][i].astype(np.float32).astype(np.float64), case.res,
                                      z_near=float(case.z_near), z_far=float(case.z_far))
            n = int((bits(dbg[i, k]) != bits(want)).sum())
            if n:
                bad.append((i, k, n))
            worst = max(worst, float(np.abs(t_after[k + 1][i] - ts[k]).max()))
    print(f"{what}: largest |t - oracle| after any iteration = {worst:.3e} m over {len(case.obj)} ROIs; "
          f"{rerendered} render(s) taken at the kernel's float32 pose; (ROI, iteration, differing pixels) = {bad}")
    assert not bad, (what, bad)
    for i in range(len(case.obj)):
        if ref[i] is not None:
            for k in range(case.iters):
                np.testing.assert_allclose(t_after[k + 1][i], ref[i][0][k], atol=1e-6, rtol=0, err_msg=f"{what} ROI {i} after {k + 1}")


def with_unused_large_object(case):
    """The case's meshes plus an object of kMaxStagedVerts + 1 vertices that no ROI uses: the workspace kernel."""
    v, f = C.stage_mesh(C.MAX_STAGED + 1)
    return list(case.verts) + [v], list(case.faces) + [f]


def assert_repeatable_and_records(hip, case, meshes, t_out, dbg):
    for _ in range(2):                                      # which triangles overflow the queue depends on atomic order:
        t2, d2 = refine(hip, case, meshes)                  # the result must not
        assert np.array_equal(t2, t_out) and np.array_equal(bits(d2), bits(dbg))
    b = len(case.obj)
    ids = torch.arange(50, 50 + b, dtype=torch.int32, device=DEV)
    score = torch.linspace(0.25, 1.0, b, device=DEV)
    obj, R, t_in = T(case.obj), T(case.R).reshape(b, 9), T(case.t_in)
    cam, center, scale = T(case.cam).reshape(b, 9), T(case.center), T(case.scale)
    K = hip.zoom_K(cam, center, scale, case.res)
    assert np.array_equal(K.cpu().numpy().reshape(b, 3, 3), case.K_crop)
    t_ref = hip.depth_refine(meshes, obj, *maps_of(case), K, R, t_in, **params_of(case))
    assert np.array_equal(t_ref.cpu().numpy(), t_out)
    rec3 = hip.pack_pose_records(R, t_ref, t_in, score, obj, ids)
    rec1 = hip.refine_to_records(meshes, obj, *maps_of(case), cam, center, scale, R, t_in, score, ids, **params_of(case))
    assert torch.equal(rec1, rec3)
    assert np.array_equal(rec1[:, 9:12].cpu().numpy(), t_out.astype(np.float32))


# ---------------------------------------------------------------------------------------------------- large-triangle queue
def test_queue_mixed_and_the_constant_mask_roi(hip):
    """Small and large triangles in one pass, several queue rounds per wave.  ROI NAN_MASK_ROI has a constant mask under
    mask_type 0: the kernel selects nothing and returns t_in bit for bit (the reference's restatement would take the median of
    nothing); its neighbours are compared with the oracle like every other ROI."""
    case = C.queue_mixed_case()
    meshes = hip.MeshSet(case.verts, case.faces)
    t_out, dbg = refine(hip, case, meshes)
    assert_equals_oracle(hip, case, meshes, oracle("queue_mixed_case"), t_out, dbg, "queue_mixed")
    i = C.NAN_MASK_ROI
    assert np.array_equal(t_out[i], case.t_in[i].astype(np.float64))
    o = int(case.obj[i])
    ren = P.render_depth(case.verts[o], case.faces[o], case.K_crop[i], case.R[i], case.t_in[i].astype(np.float64), case.res,
                         z_near=float(case.z_near), z_far=float(case.z_far))
    assert np.array_equal(bits(dbg[i, 0]), bits(ren)) and np.array_equal(bits(dbg[i, 1]), bits(ren))


def test_queue_at_its_limit_staged_and_unstaged(hip):
    """kMaxLargeS - 1, kMaxLargeS, kMaxLargeS + 1 and 1.6 kMaxLargeS large triangles per ROI, through the LDS-staged kernel and
    (with an unused large object in the mesh set) the workspace kernel: oracle-equal, equal to each other, repeatable, and the
    same through refine_to_records."""
    case = C.queue_limit_case(True)
    ref = oracle("queue_limit_case", True)
    staged = hip.MeshSet(case.verts, case.faces)
    t_s, d_s = refine(hip, case, staged)
    assert_equals_oracle(hip, case, staged, ref, t_s, d_s, "queue_limit staged")
    assert_repeatable_and_records(hip, case, staged, t_s, d_s)
    other = C.queue_limit_case(False)
    unstaged = hip.MeshSet(other.verts, other.faces)
    assert hip.load().gdrnpp_depth_refine_workspace_bytes(staged.c, 8) == 0
    assert hip.load().gdrnpp_depth_refine_workspace_bytes(unstaged.c, 8) == C.workspace_bytes(C.MAX_STAGED + 1, 8) > 0
    t_u, d_u = refine(hip, other, unstaged)
    assert_equals_oracle(hip, other, unstaged, ref, t_u, d_u, "queue_limit unstaged")
    assert np.array_equal(t_u, t_s) and np.array_equal(bits(d_u), bits(d_s))
    assert_repeatable_and_records(hip, other, unstaged, t_u, d_u)


# ----------------------------------------------------------------------------------------------------------------- planes
def test_near_camera_and_far_planes_inside_the_refine_kernel(hip):
    """The cand == 2 exact path (cut by z_near with all z > 0, across the camera plane, a vertex ON the camera plane), the far
    plane, and the two empty renders, which return t_in bit for bit."""
    case = C.plane_case()
    meshes = hip.MeshSet(case.verts, case.faces)
    t_out, dbg = refine(hip, case, meshes)
    assert_equals_oracle(hip, case, meshes, oracle("plane_case"), t_out, dbg, "plane")
    for name in ("beyond_far", "off_crop"):
        i = C.PLANE_ROIS[name]
        assert not dbg[i].any() and np.array_equal(t_out[i], case.t_in[i].astype(np.float64))
    assert (dbg[C.PLANE_ROIS["vertex_on_camera_plane"], 0] > 0).sum() > 200


# ------------------------------------------------------------------------------------------------------------ stage limit
@pytest.mark.parametrize("n_verts", C.STAGE_VERTS)
def test_stage_limit(hip, n_verts):
    """kMaxStagedVerts - 1 (odd: padded stage), kMaxStagedVerts (the largest dynamic LDS the kernel can ask for) and
    kMaxStagedVerts + 1 (first workspace launch, odd) vertices, ROIs of the small object laid out by the large one's max_verts."""
    case = C.stage_case(n_verts)
    ref = oracle("stage_case", n_verts)
    meshes = hip.MeshSet(case.verts, case.faces)
    assert hip.load().gdrnpp_depth_refine_workspace_bytes(meshes.c, 4) == C.workspace_bytes(n_verts, 4)
    t_out, dbg = refine(hip, case, meshes)
    assert_equals_oracle(hip, case, meshes, ref, t_out, dbg, f"stage {n_verts}")
    assert_repeatable_and_records(hip, case, meshes, t_out, dbg)
    if n_verts <= C.MAX_STAGED:                             # the same geometry through the workspace kernel
        t_u, d_u = refine(hip, case, hip.MeshSet(*with_unused_large_object(case)))
        assert np.array_equal(t_u, t_out) and np.array_equal(bits(d_u), bits(dbg))


def raw_refine(hip, case, meshes, t_out, workspace, workspace_bytes, res=None, in_res=None):
    from gdrnpp_bop2022_amd.hip_lib import abi

    b = len(case.obj)
    keep = [T(case.obj), *maps_of(case), T(case.K_crop).reshape(b, 9), T(case.R).reshape(b, 9), T(case.t_in)]
    abi.launch("gdrnpp_depth_refine", meshes.c, *[k.data_ptr() for k in keep], t_out.data_ptr(), None, b,
               case.res if res is None else res, 4 * case.res if in_res is None else in_res, case.iters, float(case.threshold),
               case.mask_type, 0, float(case.z_near), float(case.z_far), workspace.data_ptr() if workspace is not None else None,
               workspace_bytes)
    torch.cuda.synchronize()


def test_argument_errors_are_statuses_and_launch_nothing(hip):
    """res = 129 for the render, res^2 > 4096 and in_res != 4 res for the refinement, a missing and a one-byte-short workspace: a
    status with text, and the NaN-filled outputs untouched."""
    case = C.stage_case(C.MAX_STAGED + 1)
    meshes = hip.MeshSet(case.verts, case.faces)
    b = len(case.obj)
    need = C.workspace_bytes(C.MAX_STAGED + 1, b)
    t_out = torch.full((b, 3), float("nan"), dtype=torch.float64, device=DEV)
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError, match=f"workspace of {need} bytes"):
        raw_refine(hip, case, meshes, t_out, None, 0)
    with pytest.raises(RuntimeError, match=f"workspace of {need} bytes"):
        raw_refine(hip, case, meshes, t_out, ws, need - 1)
    with pytest.raises(RuntimeError, match="res=65 > 64"):
        raw_refine(hip, case, meshes, t_out, ws, need, res=65, in_res=260)
    with pytest.raises(RuntimeError, match="4 x"):
        raw_refine(hip, case, meshes, t_out, ws, need, in_res=4 * case.res - 1)
    assert torch.isnan(t_out).all()
    raw_refine(hip, case, meshes, t_out, ws, need)                                   # and with the workspace it asks for, it runs
    assert np.array_equal(t_out.cpu().numpy(), refine(hip, case, meshes)[0])
    from gdrnpp_bop2022_amd.hip_lib import abi

    depth = torch.full((1, 129, 129), float("nan"), device=DEV)
    keep = [T(case.obj[:1]), T(case.K_crop[:1]).reshape(1, 9), T(case.R[:1]).reshape(1, 9), T(case.t_in[:1])]
    with pytest.raises(RuntimeError, match="res=129 > 128"):
        abi.launch("gdrnpp_render_depth", meshes.c, *[k.data_ptr() for k in keep], depth.data_ptr(), None, 1, 129, 0.1, 100.0)
    torch.cuda.synchronize()
    assert torch.isnan(depth).all()


# ------------------------------------------------------------------------------------------------------------ resolutions
@pytest.mark.parametrize("res", C.REFINE_RES)
def test_refine_at_every_crop_resolution(hip, res):
    """64 ... 4096 pixels against the 512 x 8 pixel passes of a workgroup: one wave, half a block, ragged and empty passes."""
    case = C.res_case(res)
    meshes = hip.MeshSet(case.verts, case.faces)
    t_out, dbg = refine(hip, case, meshes)
    assert_equals_oracle(hip, case, meshes, oracle("res_case", res), t_out, dbg, f"res {res}")


@pytest.mark.parametrize("res", C.RENDER_RES)
def test_render_depth_at_every_resolution(hip, res):
    """1 ... 128: below and above kT pixels, the last size inside the default dynamic LDS (78), the first that raises it (79), the
    limit; a mesh of 2.5 x kT faces in front of, near and across the camera."""
    c = C.render_res_case(res)
    meshes = hip.MeshSet([c.verts], [c.faces])
    d, x = hip.render_depth(meshes, torch.zeros(3, dtype=torch.int32, device=DEV), T(c.K).reshape(3, 9), T(c.R).reshape(3, 9), T(c.t),
                            res, want_xyz=True)
    d, x = d.cpu().numpy(), x.cpu().numpy()
    for i in range(3):
        od, ox = P.render_depth(c.verts, c.faces, c.K[i], c.R[i], c.t[i].astype(np.float64), res, z_near=float(np.float32(0.1)),
                                want_xyz=True)             # the kernel widens its float z_near
        assert np.array_equal(bits(d[i]), bits(od)), (res, i)
        np.testing.assert_allclose(x[i], ox, atol=1e-6, rtol=0)


# ----------------------------------------------------------------------------------------------------------------- median
def test_median_ranks_ties_and_signs(hip):
    """nsel = 1, 2, 3, 4, 511, 512, 513 and every rendered pixel, with designed depth differences (tests/refine_edge_cases.py
    median_pattern): iteration 0's step is ray * the designed median."""
    case, hot = C.median_case()
    meshes = hip.MeshSet(case.verts, case.faces)
    t_out, dbg = refine(hip, case, meshes)
    assert_equals_oracle(hip, case, meshes, oracle("median_case"), t_out, dbg, "median")
    t1 = refine(hip, case, meshes, iters=1)[0]
    for i in range(len(hot)):
        n = len(hot[i])
        p = (C.median_pattern(n) * C.MEDIAN_UNIT).astype(np.float32)
        med = p[n // 2] if n % 2 else (p[(n - 1) // 2] + p[n // 2]) / np.float32(2)
        assert t1[i, 2] - np.float64(case.t_in[i, 2]) == np.float64(med), (i, n)     # t_z + 1 * median: exact in fp64


# ---------------------------------------------------------------------------------------------------------------- lattice
def test_pixel_centre_lattice_in_both_kernels(hip):
    """Vertices on pixel centres, edges through rows, columns and diagonals of centres, shared edges, coincident copies, zero-area
    triangles: depth bit-equal to the oracle (itself bit-equal to the box-free reference, CPU test) in render_depth and in both
    iterations of the refinement; on the tie pixels the xyz of the LOWEST face id, bit for bit."""
    case = C.lattice_case()
    meshes = hip.MeshSet(case.verts, case.faces)
    t_out, dbg = refine(hip, case, meshes)
    assert_equals_oracle(hip, case, meshes, oracle("lattice_case"), t_out, dbg, "lattice")
    v, f = case.verts[0], case.faces[0]
    d, x = hip.render_depth(meshes, T(case.obj), T(case.K_crop).reshape(2, 9), T(case.R).reshape(2, 9), T(case.t_in), 64, want_xyz=True)
    d, x = d.cpu().numpy(), x.cpu().numpy()
    for i in range(2):
        t = case.t_in[i].astype(np.float64)
        rd, rx, face = RR.render(v, f, case.K_crop[i], case.R[i], t, 64, want_xyz=True, want_face=True)
        assert np.array_equal(bits(d[i]), bits(rd)) and np.array_equal(bits(dbg[i, 0]), bits(rd))
        np.testing.assert_allclose(x[i], rx, atol=1e-6, rtol=0)
        tie = RR.covering_faces(v, f, case.K_crop[i], case.R[i], t, 64) >= 2
        assert tie.sum() > (300 if i == 0 else 30)
        assert np.array_equal(bits(x[i][tie]), bits(rx[tie]))         # same face, same expressions, no FMA: the same bits
