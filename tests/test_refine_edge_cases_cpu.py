"""The builders of tests/refine_edge_cases.py without a GPU.  Two things are asserted here:

* tests/raster_ref.py (NumPy fp64, every pixel centre against every triangle, no candidate box) and the oracle render
  (oracle/raster_oracle.c, which restates raster.hpp's box) are BIT-EQUAL for every mesh, pose, iteration and resolution of
  every case, in depth and, where asked, in xyz: the box logic the kernel shares with its oracle is judged by something that
  has none;
* every case reaches what it is named for, by the NumPy restatement of the kernel's own branch tests (branch_counts) and
  the per-iteration statistics of P.depth_refine_roi: large-triangle counts around kMaxLargeS, triangles on the exact
  (cand == 2) path, vertex counts around kMaxStagedVerts, nsel, empty renders; and no pixel of any iteration that takes a step
  lies within STABLE_MARGIN * qmax of the selection threshold, so the selected set cannot depend on the order of a sum.
"""
import ctypes
from functools import lru_cache

import numpy as np
import pytest

import raster_ref as RR
import refine_edge_cases as C
from oracle import postproc as P


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


CASES = {
    "queue_mixed": C.queue_mixed_case,
    "queue_limit": lambda: C.queue_limit_case(True),
    "plane": C.plane_case,
    "median": lambda: C.median_case()[0],
    "lattice": C.lattice_case,
    **{f"stage_{n}": (lambda n=n: C.stage_case(n)) for n in C.STAGE_VERTS},
    **{f"res_{r}": (lambda r=r: C.res_case(r)) for r in C.REFINE_RES},
}


@lru_cache(maxsize=None)
def survey(name):
    """Per ROI and iteration of a case: the statistics of P.depth_refine_roi, the branch counts of the render, and whether the
    plain reference and the oracle render agree bit for bit.  Computed once, shared by the tests below."""
    case = CASES[name]()
    rows = []
    for i in range(len(case.obj)):
        o = int(case.obj[i])
        stats = []
        if i not in case.kernel_only:
            _, renders = C.oracle_refine(case, i, stats=stats, return_debug=True)
        else:
            renders = [P.render_depth(case.verts[o], case.faces[o], case.K_crop[i], case.R[i], case.t_in[i].astype(np.float64),
                                      case.res, z_near=float(case.z_near), z_far=float(case.z_far))] * case.iters
            stats = [None] * case.iters
        its = []
        for k, t in enumerate(C.iteration_poses(case, i) if i not in case.kernel_only else [case.t_in[i]] * case.iters):
            ref = RR.render(case.verts[o], case.faces[o], case.K_crop[i], case.R[i], t.astype(np.float64), case.res,
                            case.z_near, case.z_far)
            its.append(dict(stats=stats[k], equal=np.array_equal(bits(ref), bits(renders[k])), rendered=int((ref > 0).sum()),
                            **C.branch_counts(case.verts[o], case.faces[o], case.K_crop[i], case.R[i], t, case.res,
                                              case.z_near, case.z_far)))
        rows.append(its)
    return case, rows


def test_the_constants_are_read_from_the_kernel_source():
    assert C.LARGE_AREA > 0 and C.MAX_LARGE >= 128 and C.MAX_STAGED >= 10 * 4 ** C.STAGE_BASE_SUBDIV + 2 + 4
    assert C.MAX_PIX == 4096 and C.MAX_PIX % C.REFINE_THREADS == 0 and C.RENDER_THREADS % 64 == 0
    assert C.STAGE_VERTS[0] % 2 == 1 and C.STAGE_VERTS[2] % 2 == 1            # odd counts on both sides: padded layouts
    assert C.QUEUE_COUNTS[3] >= 1.6 * C.MAX_LARGE


def test_stats_argument_leaves_the_return_value_alone():
    case = C.res_case(16)
    st = []
    a = C.oracle_refine(case, 0)
    b = C.oracle_refine(case, 0, stats=st)
    assert isinstance(a, np.ndarray) and np.array_equal(a, b) and len(st) == case.iters and st[0]["stepped"]
    assert st[0]["nsel"] == len(st[0]["diffs"]) and st[0]["median"] == np.median(st[0]["diffs"])


@pytest.mark.parametrize("name", list(CASES))
def test_plain_reference_equals_the_oracle_render_and_selection_is_stable(name):
    case, rows = survey(name)
    assert np.array_equal(case.K_crop, P.zoom_K(case.cam, case.center, case.scale, case.res))
    assert case.roi_depth.shape[-1] == 4 * case.res and len(case.obj) <= 8
    for i, its in enumerate(rows):
        for k, it in enumerate(its):
            assert it["equal"], (name, i, k)
            st = it["stats"]
            if st is not None and st["stepped"]:
                assert st["margin"] >= C.STABLE_MARGIN, (name, i, k, st["margin"])
                assert st["nsel"] >= 1


def test_queue_mixed_case_queues_small_and_large_triangles_in_one_pass():
    case, rows = survey("queue_mixed")
    n_large = [[it["n_large"] for it in its] for its in rows]
    print("queue_mixed n_large per ROI / iteration", n_large, "largest box", max(it["max_box"] for its in rows for it in its))
    for i, its in enumerate(rows):
        for it in its:
            assert it["n_large"] >= 16 and it["n_exact"] == 0 and it["rendered"] > 1000
            if case.obj[i] == 2:                                      # the 1280-face object: small and large in one pass
                assert it["n_cand"] - it["n_large"] >= 20
    waves = C.REFINE_THREADS // 64
    assert max(max(r) for r in n_large) > 8 * waves                 # many queue rounds per wave
    assert max(it["max_box"] for its in rows for it in its) > 1000
    # the constant mask: the reference's normalisation is NaN everywhere, nothing it could select
    assert np.isnan(P.get_out_mask(case.mask[C.NAN_MASK_ROI:C.NAN_MASK_ROI + 1])).all()
    assert rows[C.NAN_MASK_ROI][0]["rendered"] > 1000 and (case.roi_depth[C.NAN_MASK_ROI] > 0).mean() > 0.3


def test_queue_limit_case_sits_on_both_sides_of_the_queue():
    case, rows = survey("queue_limit")
    print("queue_limit n_large", [[it["n_large"] for it in its] for its in rows])
    for i, want in enumerate(C.QUEUE_COUNTS):
        assert len(case.faces[i]) == want
        assert rows[i][0]["n_large"] == want or i == 3          # ROIs 0..2, iteration 0: every triangle is large
        for it in rows[i]:                                      # iteration 1 moves the pose: a handful may drop out; ROI 3: 1.5 queues
            assert abs(it["n_large"] - want) <= 16 if i < 3 else it["n_large"] >= 1.5 * C.MAX_LARGE
            assert it["n_exact"] == 0
        assert rows[i][0]["rendered"] > 3000
        assert rows[i + 4][0]["n_large"] > 0.5 * want
    assert [rows[i][0]["n_large"] - C.MAX_LARGE for i in range(3)] == [-1, 0, 1]
    # different layers win different pixels: the winning face's layer takes many values
    face = RR.render(case.verts[3], case.faces[3], case.K_crop[3], case.R[3], case.t_in[3].astype(np.float64), case.res,
                     case.z_near, case.z_far, want_face=True)[1]
    assert len(np.unique(face // (2 * C.GRID ** 2))) >= 6
    # faces beyond the queue's capacity win pixels too: the overflow path decides part of the image
    assert (face >= C.MAX_LARGE).sum() > 100
    unstaged = C.queue_limit_case(False)
    assert max(len(v) for v in unstaged.verts) == C.MAX_STAGED + 1 and max(len(v) for v in case.verts) <= C.MAX_STAGED
    for name in ("obj", "mask", "roi_depth", "coor_x", "t_in", "R", "K_crop"):
        assert np.array_equal(getattr(unstaged, name), getattr(case, name)), name
    assert all(np.array_equal(a, b) for a, b in zip(unstaged.verts, case.verts))


def test_plane_case_reaches_the_exact_path_and_the_empty_renders():
    case, rows = survey("plane")
    R = C.PLANE_ROIS
    print("plane n_exact", [[it["n_exact"] for it in its] for its in rows], "rendered", [[it["rendered"] for it in its] for its in rows])
    near, far = rows[R["near_cut"]], rows[R["far_cut"]]
    o = int(case.obj[R["near_cut"]])
    z = RR.project(case.verts[o], case.K_crop[0], case.R[0], case.t_in[0].astype(np.float64))[:, 2]
    assert z.min() > 0 and (z < case.z_near).any() and (z > case.z_near).any()         # cut by z_near, all in front of the camera
    assert near[0]["n_exact"] > 50 and 0 < near[0]["rendered"]
    full = RR.render(case.verts[o], case.faces[o], case.K_crop[0], case.R[0], case.t_in[0].astype(np.float64), 64, 0.01, 100.0)
    cut = RR.render(case.verts[o], case.faces[o], case.K_crop[0], case.R[0], case.t_in[0].astype(np.float64), 64, case.z_near, 100.0)
    assert (bits(full) != bits(cut)).sum() > 100                                       # z_near changes the picture
    i = R["far_cut"]
    nofar = RR.render(case.verts[0], case.faces[0], case.K_crop[i], case.R[i], case.t_in[i].astype(np.float64), 64, case.z_near, 100.0)
    cutf = RR.render(case.verts[0], case.faces[0], case.K_crop[i], case.R[i], case.t_in[i].astype(np.float64), 64, case.z_near, case.z_far)
    assert far[0]["rendered"] > 0 and far[0]["n_exact"] == 0 and ((nofar > 0) & (cutf == 0)).sum() > 20
    for name in ("beyond_far", "off_crop"):
        for it in rows[R[name]]:
            assert it["rendered"] == 0 and it["stats"]["norm_sum"] == 0 and not it["stats"]["stepped"]
        assert (case.mask[R[name]] != 0).any() and (case.roi_depth[R[name]] > 0).any()  # empty because of the render alone
        assert np.array_equal(C.oracle_refine(case, R[name]), case.t_in[R[name]].astype(np.float64))
    i = R["straddles_camera"]
    z = RR.project(case.verts[1], case.K_crop[i], case.R[i], case.t_in[i].astype(np.float64))[:, 2]
    assert (z < 0).sum() > 10 and (z > case.z_near).sum() > 10 and rows[i][0]["n_exact"] > 50 and rows[i][0]["rendered"] > 200
    i = R["vertex_on_camera_plane"]
    z = RR.project(case.verts[1], case.K_crop[i], case.R[i], case.t_in[i].astype(np.float64))[:, 2]
    assert z[-1] == 0.0 and (case.faces[1][-1] == len(z) - 1).any() and rows[i][0]["rendered"] > 200


@pytest.mark.parametrize("n_verts", C.STAGE_VERTS)
def test_stage_cases_have_the_vertex_counts_and_a_visible_ribbon(n_verts):
    case, rows = survey(f"stage_{n_verts}")
    assert [len(v) for v in case.verts] == [162, n_verts]
    assert list(case.obj) == [0, 1, 0, 1]
    base_faces = 20 * 4 ** C.STAGE_BASE_SUBDIV
    for i in (1, 3):
        face = RR.render(case.verts[1], case.faces[1], case.K_crop[i], case.R[i], case.t_in[i].astype(np.float64), 64,
                         want_face=True)[1]
        ribbon = np.unique(face[face >= base_faces])
        assert len(ribbon) > 10                                              # the added triangles win pixels
        assert (case.faces[1][ribbon] == n_verts - 1).any()                  # among them one that uses the LAST vertex
    for its in rows:
        assert its[0]["stats"]["stepped"] and its[0]["rendered"] > 500
    assert C.workspace_bytes(n_verts, 4) == (0 if n_verts <= C.MAX_STAGED else 4 * (n_verts + 1) // 2 * 2 * 40)


def test_workspace_query_of_the_library_at_the_stage_limit():
    """gdrnpp_depth_refine_workspace_bytes is host code: 0 up to kMaxStagedVerts, b * ((V + 1) & ~1) * 40 above."""
    from gdrnpp_bop2022_amd.hip_lib import abi

    lib = abi.load()
    for v in (1, 161, 162, *C.STAGE_VERTS, C.MAX_STAGED + 2, 10242):
        for b in (1, 4, 7):
            m = abi.gdrnpp_meshes(None, None, None, None, 2, v, 8)
            assert lib.gdrnpp_depth_refine_workspace_bytes(ctypes.byref(m), b) == C.workspace_bytes(v, b), (v, b)


@pytest.mark.parametrize("res", C.REFINE_RES)
def test_res_cases_render_and_step_at_every_resolution(res):
    case, rows = survey(f"res_{res}")
    assert case.mask.shape == (3, 1, res, res) and case.roi_depth.shape == (3, 1, 4 * res, 4 * res)
    assert case.K_crop[0, 0, 0] == np.float32(300.0 * res / 64) and case.K_crop[0, 0, 2] == np.float32(res / 2)
    for its in rows:
        assert its[0]["stats"]["stepped"] and its[0]["rendered"] >= res * res // 8
    edge = RR.render(case.verts[2], case.faces[2], case.K_crop[2], case.R[2], case.t_in[2].astype(np.float64), res)
    assert (edge[:, -1] > 0).any() and (edge[-1, :] > 0).any()               # ROI 2 is cut by the crop's right and bottom edges


@pytest.mark.parametrize("res", C.RENDER_RES)
def test_render_cases_plain_reference_equals_the_oracle_in_depth_and_xyz(res):
    c = C.render_res_case(res)
    rendered = 0
    for i in range(3):
        d, x = RR.render(c.verts, c.faces, c.K[i], c.R[i], c.t[i].astype(np.float64), res, np.float32(0.1), 100.0, want_xyz=True)
        od, ox = P.render_depth(c.verts, c.faces, c.K[i], c.R[i], c.t[i].astype(np.float64), res, z_near=float(np.float32(0.1)),
                                want_xyz=True)
        assert np.array_equal(bits(d), bits(od)) and np.array_equal(bits(x), bits(ox)), (res, i)
        rendered += int((d > 0).sum())
    assert rendered >= min(res * res, 40)
    if res >= 63:
        assert C.branch_counts(c.verts, c.faces, c.K[1], c.R[1], c.t[1], res)["n_large"] > 50
        assert C.branch_counts(c.verts, c.faces, c.K[2], c.R[2], c.t[2], res)["n_exact"] > 50


def key(x):
    b = int(np.float32(x).view(np.uint32))
    return (~b) & 0xffffffff if b & 0x80000000 else b | 0x80000000


def test_median_case_places_the_ranks_where_it_says():
    (case, hot), rows = C.median_case(), survey("median")[1]
    seen = dict(neg=0, pos=0, zero=0)
    for i, k in enumerate(C.MEDIAN_K):
        st = rows[i][0]["stats"]
        n = len(hot[i])
        assert n == (k or rows[i][0]["rendered"]) and st["stepped"] and st["nsel"] == n
        want = (C.median_pattern(n) * C.MEDIAN_UNIT).astype(np.float32)
        got = np.sort(st["diffs"])
        assert np.array_equal(bits(got), bits(want)), (i, k)                     # the differences are the designed ones, exactly
        r0, r1 = (n - 1) // 2, n // 2
        assert st["median"] == (got[r0] if n % 2 else (got[r0] + got[r1]) / np.float32(2))
        if n % 2 == 0:
            assert got[r0] != got[r1]                                            # a mean is taken
        seen["neg"] += int((got < 0).sum()); seen["pos"] += int((got > 0).sum()); seen["zero"] += int((got == 0).sum())
        if n >= 5:
            assert (got == got[r0]).sum() >= 5 and (got == got[r1]).sum() >= 5   # ties that survive all four byte passes
        print(f"median ROI {i}: nsel {st['nsel']} (iteration 1: {rows[i][1]['stats'].get('nsel')}), median {st['median']:.9g}")
    assert min(seen.values()) > 0 and not np.signbit(case.roi_depth).any()
    p4 = (C.median_pattern(4) * C.MEDIAN_UNIT).astype(np.float32)
    assert key(p4[1]) ^ key(p4[2]) and (key(p4[1]) ^ key(p4[2])) < 256           # the ranks differ in their lowest byte only
    for n in (2, C.REFINE_THREADS):
        p = (C.median_pattern(n) * C.MEDIAN_UNIT).astype(np.float32)
        assert key(p[(n - 1) // 2]) >> 24 != key(p[n // 2]) >> 24                # the ranks lie in different top-byte bins
    p = (C.median_pattern(C.REFINE_THREADS - 1) * C.MEDIAN_UNIT).astype(np.float32)
    r = (len(p) - 1) // 2
    assert 0 < (key(p[r + 4]) ^ key(p[r])) < 256                                 # the tie group's neighbours: lowest byte
    assert (C.median_pattern(C.REFINE_THREADS + 1)[C.REFINE_THREADS // 2] == 0)  # median +0 among ties


def test_lattice_case_puts_centres_on_vertices_and_edges():
    case, rows = survey("lattice")
    v, f = case.verts[0], case.faces[0]
    ties = 0
    for i in range(2):
        t = case.t_in[i].astype(np.float64)
        h = RR.project(v, case.K_crop[i], case.R[i], t)
        uv = h[:, :2] / h[:, 2:3]
        if i == 0:
            assert np.array_equal(uv * 2, np.round(uv * 2))                       # exact half-integers
            on_centre = (uv % 1 == 0.5).all(1)
            assert on_centre.sum() >= 49 + 24
        e0, e1, e2, D = RR.edge_planes(h, f.astype(np.int64))
        assert (D[80:82] == 0).all() and (D[:80] != 0).all() and (D[82:] != 0).all()   # the two zero-area triangles, exactly
        jj, ii = np.divmod(np.arange(64 * 64), 64)
        w = [(e[:, 0:1] * (ii + 0.5) + e[:, 1:2] * (jj + 0.5)) + e[:, 2:3] for e in (e0, e1, e2)]
        inside = ((w[0] >= 0) & (w[1] >= 0) & (w[2] >= 0)) | ((w[0] <= 0) & (w[1] <= 0) & (w[2] <= 0))
        on_edge = inside & ((w[0] == 0) | (w[1] == 0) | (w[2] == 0)) & (D[:, None] != 0)
        assert on_edge.sum() > (400 if i == 0 else 40), on_edge.sum()              # centres exactly on edges
        n = RR.covering_faces(v, f, case.K_crop[i], case.R[i], t, 64)
        ties += int((n >= 2).sum())
        d, x, face = RR.render(v, f, case.K_crop[i], case.R[i], t, 64, want_xyz=True, want_face=True)
        od, ox = P.render_depth(v, f, case.K_crop[i], case.R[i], t, 64, want_xyz=True)
        assert np.array_equal(bits(d), bits(od)) and np.array_equal(bits(x), bits(ox))
        assert not np.isin(face, np.arange(72, 80)).any()                          # a copy never beats its lower-numbered original
        assert (face == 84).sum() > 100 and (face == 83).sum() > 0 and (face == 85).sum() > 0
        assert rows[i][0]["n_large"] >= 1 and rows[i][0]["n_cand"] - rows[i][0]["n_large"] >= 70
    assert ties > 300
