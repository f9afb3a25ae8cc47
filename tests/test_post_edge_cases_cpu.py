"""The builders of tests/post_edge_cases.py without a GPU: every precondition that makes a case of tests/test_gpu_post_edges.py
prove something is asserted here against the oracle — ties exist and span wave quarters / tiles, inliers lie beyond the pixel
tile, the ladder stays a ladder in the oracle's own float arithmetic, run counts exceed two conversion passes, valid flow pixels
lie beyond one pass of the capped grid."""
import numpy as np
import pytest

import post_edge_cases as C
from oracle import postproc as P


# ---------------------------------------------------------------------------------------------------------- NN distance
def test_nnd_shapes_hold_every_pair_and_its_swap():
    pairs = [(1, 1), (63, 255), (64, 256), (65, 257), (64, 1023), (65, 1024), (1, 1025), (130, 2049)]
    assert set(C.NND_SHAPES) == set(pairs) | {(m, n) for n, m in pairs} and len(C.NND_SHAPES) == 15
    x1, x2 = C.nnd_shape_case(65, 1024)
    assert x1.shape == (2, 65, 3) and x2.shape == (2, 1024, 3)
    assert np.array_equal(x1[1], np.round(x1[1])) and np.abs(x1[1]).max() <= 8


def test_nnd_tie_case_has_ties_across_quarters_and_tiles():
    q, t, point = C.nnd_tie_case()
    q, t = q[0], t[0]
    assert t.shape == (2049, 3) and np.array_equal(np.flatnonzero((t == point).all(1)), C.NND_TIE_INDICES)
    assert sorted({i // 256 for i in C.NND_TIE_INDICES}) == [0, 1, 2, 3, 4, 8]      # waves 0..3 of tile 0, tile 1, tile 2
    assert np.array_equal(q * 2, np.round(q * 2)) and np.abs(q).max() <= 8          # squared distances exact in fp32
    tied = C.nnd_tied_queries(q, t)
    assert tied >= 32, tied
    d1, d2, i1, i2 = P.nnd_forward(q[None], t[None])
    assert (i1[0, :4] == 5).all() and (d1[0, :4] == 0).all()                        # the lowest of the six copies
    d = ((q[:, None].astype(np.float64) - t[None]) ** 2).sum(-1)
    assert np.array_equal(i1[0], d.argmin(1)) and np.array_equal(d1[0], d.min(1).astype(np.float32))


def test_nnd_grad_lattice_case_is_exact_in_fp32_and_collides():
    x1, x2, gd1, gd2 = C.nnd_grad_case("lattice")
    _, _, i1, i2 = P.nnd_forward(x1, x2)
    g1, g2, c1, c2, s1, s2 = C.nnd_grad_reference(x1, x2, gd1, gd2, i1, i2)
    assert np.array_equal(gd1, np.round(gd1)) and np.array_equal(gd2, np.round(gd2))
    assert max(s1.max(), s2.max()) < 2 ** 24                # every term an integer, every partial sum below 2^24: order-free
    assert np.array_equal(g1, np.round(g1)) and np.array_equal(g2, np.round(g2))
    assert c2.shape == (2, 3, 3) and c2.sum() / 3 == 2 * (1000 + 3) and c2.min() > 100     # hundreds of atomics per element
    # the oracle's own backward (fp32, serial) agrees exactly on this case
    o1, o2 = P.nnd_backward(x1, x2, gd1, gd2, i1, i2)
    assert np.array_equal(o1, g1.astype(np.float32)) and np.array_equal(o2, g2.astype(np.float32))


def test_nnd_grad_reference_matches_the_oracle_backward_on_floats():
    x1, x2, gd1, gd2 = C.nnd_grad_case("float")
    assert x1.shape == (2, 65, 3) and x2.shape == (2, 1025, 3)
    _, _, i1, i2 = P.nnd_forward(x1, x2)
    g1, g2, c1, c2, s1, s2 = C.nnd_grad_reference(x1, x2, gd1, gd2, i1, i2)
    o1, o2 = P.nnd_backward(x1, x2, gd1, gd2, i1, i2)
    for got, ref, c, s in ((o1, g1, c1, s1), (o2, g2, c2, s2)):
        assert (np.abs(got - ref) <= 2 * c * 2.0 ** -24 * s + 2.0 ** -149).all()
    assert c1.max() > 10 and c2.min() >= 1


# -------------------------------------------------------------------------------------------------------- RANSAC voting
def test_voting_shapes_are_the_listed_ones():
    assert C.VOTE_SHAPES == [(1, 1, 1), (63, 1, 3), (256, 2, 5), (257, 9, 2), (4095, 3, 4), (4096, 3, 5), (4097, 1, 7),
                             (8193, 2, 6)]
    assert C.VOTE_THRESHOLDS == (0.99, 0.999)


@pytest.mark.parametrize("tn,vn,hn", C.VOTE_SHAPES)
@pytest.mark.parametrize("vp", [False, True])
def test_voting_case_has_inliers_also_beyond_the_pixel_tile(tn, vn, hn, vp):
    case = C.voting_case(tn, vn, hn)
    direct, coords, idxs, kp = case
    assert direct.shape == (tn, vn, 2) and coords.shape == (tn, 2) and idxs.shape == (hn, vn, 2)
    assert (np.abs(direct[:min(5, tn // 4)]) == 0).all() and (idxs[0, :, 0] == idxs[0, :, 1]).all()
    hyp = C.voting_hypotheses(case, vp)
    for thr in C.VOTE_THRESHOLDS:
        inl = P.voting_for_hypothesis(direct, coords, hyp, thr, vp)
        assert inl.sum() > 0
        assert inl[-1, :, -1].all()                                  # the planted keypoints take the noise-free last pixel
        if tn > C.VOTE_PIX_TILE:
            assert inl[:, :, C.VOTE_PIX_TILE:].sum() > 0
            assert inl[:-1, :, C.VOTE_PIX_TILE:].sum() > 0            # ... and so do generated hypotheses


# ------------------------------------------------------------------------------------------------- YOLOX post-processing
@pytest.mark.parametrize("a", C.YOLOX_ANCHORS)
@pytest.mark.parametrize("c", C.YOLOX_CLASSES)
def test_yolox_anchor_case_has_duplicates_and_an_empty_image(a, c):
    det = C.yolox_anchor_case(a, c)
    assert det.shape == (3, a, 5 + c)
    lo, hi = a // 3, min(a, a // 3 + 40)
    assert (det[0, lo:hi] == det[0, lo]).all()
    score = det[..., 4] * det[..., 5:].max(-1)
    assert score[0, lo] >= C.YOLOX_DENSE_CONF and (score[2] < C.YOLOX_DENSE_CONF).all()
    if a >= 64:
        assert (score[:2] >= C.YOLOX_DENSE_CONF).mean() > 0.5          # dense: most anchors are sorted and go through NMS
    if a < 4096:                                                       # (the large ones run once, in the GPU test)
        want = P.yolox_postprocess(det, c, C.YOLOX_DENSE_CONF, C.NMS_THRE, False)
        assert want[0] is not None and want[2] is None
        if hi - lo > 1:
            assert len(want[0]) <= a - (hi - lo) + 1                   # of the duplicates at most one survives


def test_yolox_anchor_list_reaches_the_limit():
    assert C.YOLOX_ANCHORS == [1, 63, 64, 65, 100, 4096, 16384] and C.YOLOX_CLASSES == [1, 21]
    assert C.YOLOX_LIMIT == max(C.YOLOX_ANCHORS)


@pytest.mark.parametrize("n", C.NMS_TILE_COUNTS)
def test_sparse_case_keeps_exactly_n(n):
    det = C.yolox_sparse_case(n)
    assert det.shape == (1, 256, 6)
    assert ((det[0, :, 4] * det[0, :, 5]) >= C.NMS_SPARSE_CONF).sum() == n
    for agnostic in (False, True):
        want = P.yolox_postprocess(det, 1, C.NMS_SPARSE_CONF, C.NMS_THRE, agnostic)[0]
        assert len(want) == n and len(set(want[:, 4].tolist())) == n
    assert C.NMS_TILE_COUNTS == [64, 65, 128, 129]


def test_ladder_stays_a_ladder_in_the_oracle_arithmetic():
    det = C.yolox_ladder_case()
    assert C.LADDER_LEN == 130
    for img, first in ((0, 0), (1, 1)):
        rows = det[img, first:first + C.LADDER_LEN]
        assert (np.diff(rows[:, 4]) < 0).all() and rows[-1, 4] * rows[-1, 5] >= C.NMS_SPARSE_CONF
        for k in range(C.LADDER_LEN - 1):
            assert C.iou_f32(rows[k], rows[k + 1]) > np.float32(C.NMS_THRE)
        for k in range(C.LADDER_LEN - 2):
            assert C.iou_f32(rows[k], rows[k + 2]) < np.float32(C.NMS_THRE)
    want = P.yolox_postprocess(det, 1, C.NMS_SPARSE_CONF, C.NMS_THRE, False)
    assert np.array_equal(want[0], _decoded(det[0, 0:C.LADDER_LEN:2]))                        # ranks 0, 2, ..., 128
    assert np.array_equal(want[1], _decoded(det[1, [0] + list(range(1, C.LADDER_LEN + 1, 2))]))   # ranks 0, 1, 3, ..., 129


def _decoded(rows):
    r = np.asarray(rows, np.float32)
    two = np.float32(2)
    return np.stack([r[:, 0] - r[:, 2] / two, r[:, 1] - r[:, 3] / two, r[:, 0] + r[:, 2] / two, r[:, 1] + r[:, 3] / two,
                     r[:, 4], r[:, 5], np.zeros(len(r), np.float32)], 1)


def test_max_det_case_keeps_more_than_every_max_det():
    det = C.yolox_max_det_case()
    want = P.yolox_postprocess(det, 1, C.NMS_SPARSE_CONF, C.NMS_THRE, False)
    assert [len(w) for w in want] == [129, 64]
    assert C.MAX_DET_CASES == [1, 64, 128] and max(C.MAX_DET_CASES) < 129


# ------------------------------------------------------------------------------------------ mask paste + run-length coding
def test_paste_lists_are_the_listed_ones():
    assert C.PASTE_IMAGES == [(1, 1), (1, 1500), (7, 1024), (7, 1025), (5, 2049), (720, 1280)]
    assert C.PASTE_MASKS == [(64, 64), (28, 40), (56, 17)]


@pytest.mark.parametrize("h,w", [s for s in C.PASTE_IMAGES if s != (720, 1280)])
def test_paste_boxes_cover_the_four_placements(h, w):
    boxes = C.paste_boxes(h, w)
    inside, edge, part, whole = boxes
    assert 0 < inside[0] < inside[2] <= w + 1 and -1 < inside[1] < inside[3] < h + 1
    if w > C.PASTE_CHUNK:
        assert edge[0] < C.PASTE_CHUNK - 1 and edge[2] > C.PASTE_CHUNK + 1
    assert part[0] < 0 and part[1] < 0 and 0 < part[2] < w and 0 < part[3] <= h + 1
    assert whole[0] < 0 and whole[1] < 0 and whole[2] > w and whole[3] > h
    if w > 1:
        runs = [len(P.paste_mask_rle(C.paste_masks(hm, wm)[i], boxes[i], h, w)) for hm, wm in C.PASTE_MASKS for i in range(4)]
        assert sum(r >= 3 for r in runs) >= 8, runs                    # most instances put foreground into the image
        if w > C.PASTE_CHUNK:                                          # foreground on both sides of the chunk edge
            for hm, wm in C.PASTE_MASKS:
                _, binary = P.paste_mask_rle(C.paste_masks(hm, wm)[1], boxes[1], h, w, want_binary=True)
                assert binary[:, :C.PASTE_CHUNK].any() and binary[:, C.PASTE_CHUNK:].any()


def test_checkerboard_has_more_runs_than_two_conversion_passes():
    mask, box = C.paste_checker_case()
    h, w = C.CHECKER_IMAGE
    counts = P.paste_mask_rle(mask[0], box[0], h, w)
    assert len(counts) > 2049, len(counts)
    assert sum(counts) == h * w and counts[0] >= 992 * h


def test_cutoff_cases_have_enough_runs_to_cut():
    cases = C.paste_cutoff_cases()
    assert [c[0] for c in cases] == ["chunk-edge", "checker"]
    runs = [len(P.paste_mask_rle(m[0], b[0], h, w)) for _, m, b, h, w in cases]
    assert 4 <= runs[0] <= 1024 < runs[1], runs


# ----------------------------------------------------------------------------------------------------------------- flow
def test_flow_shapes_and_valid_pixels_beyond_one_grid_pass():
    assert C.FLOW_SHAPES == [(1, 1, 1), (3, 1, 257), (2, 17, 33), (2, 1200, 1920)]
    assert C.FLOW_ONE_PASS == 4194304
    b, h, w = C.FLOW_SHAPES[-1]
    assert b * h * w == 4608000 > C.FLOW_ONE_PASS
    flow, valid = P.flow_forward(*C.flow_case(b, h, w))
    tail = valid.reshape(-1)[C.FLOW_ONE_PASS:]
    # the depth slope (up to 0.011 per pixel) against the 3 mm test leaves roughly a tenth of the pixels valid, as in the small
    # mixed batch; tens of thousands of them beyond the first pass are what the stride branch has to get right
    assert (tail == 1).mean() > 0.05 and (tail == 1).sum() > 20000, (tail == 1).mean()
    assert 0.05 < valid.mean() < 0.95 and np.abs(flow[1, :, -100:]).max() > 0        # rows 1100.. of image 1: all beyond


@pytest.mark.parametrize("b,h,w", C.FLOW_SHAPES[:-1])
def test_small_flow_cases_are_not_empty(b, h, w):
    ds, dt, KT, Kinv = C.flow_case(b, h, w)
    assert ds.shape == (b, 1, h, w) and KT.shape == (b, 3, 4) and Kinv.shape == (b, 3, 3)
    _, valid = P.flow_forward(ds, dt, KT, Kinv)
    if h * w > 1:
        assert valid.sum() > 0


# ------------------------------------------------------------------------------------------------------------------ FPS
def test_fps_sizes_are_the_listed_ones():
    assert C.FPS_SIZES == [1, 64, 1023, 1024, 1025]
    assert all(C.fps_sample_counts(pn)[:2] == [1, 8] and C.fps_sample_counts(pn)[2] > pn for pn in C.FPS_SIZES)
    assert C.FPS_DUPLICATE_SIZES == [12288, 12290] and C.FPS_DUPLICATE_OFFSET == 6144


@pytest.mark.parametrize("pn", C.FPS_DUPLICATE_SIZES)
@pytest.mark.parametrize("init_center", [True, False])
def test_fps_duplicate_case_meets_ties(pn, init_center):
    pts, start = C.fps_duplicate_case(pn)
    p = pts[0]
    assert np.array_equal(p[:6144], p[6144:12288]) and np.array_equal(p, np.round(p))
    idxs = P.fps(p, C.FPS_DUPLICATE_SAMPLES, init_center, int(start[0]))
    ties = C.fps_tie_steps(p, idxs, init_center)
    assert ties >= 1, ties
    # a tie between a point and its copy 6144 further on resolves to the lower index
    assert (idxs[1:] < 6144).any()


def test_fps_identical_cloud_returns_index_zero():
    pts, start = C.fps_identical_case()
    pn, sn = C.FPS_IDENTICAL
    assert pts.shape == (1, pn, 3) and (pts == pts[0, 0]).all()
    assert np.array_equal(P.fps(pts[0], sn, True), np.zeros(sn, np.int32))
    assert np.array_equal(P.fps(pts[0], sn, False, int(start[0])), np.array([start[0]] + [0] * (sn - 1), np.int32))


def test_fps_lattice_clouds_repeat_index_zero_once_exhausted():
    pts, start = C.fps_lattice_case(64)
    idxs = P.fps(pts[0], 67, True)
    assert len(set(idxs[:len(np.unique(pts[0], axis=0))].tolist())) == len(np.unique(pts[0], axis=0))
    assert (idxs[64:] == 0).all()
