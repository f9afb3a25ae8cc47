"""Case builders for the detector / evaluator post-processing kernels at their tile, wave and chunk edges, shared by
tests/test_gpu_post_edges.py (HIP kernel against oracle/postproc.py, bit for bit) and tests/test_post_edge_cases_cpu.py (the
preconditions that make each case prove something).  Plain helper module: no fixtures; builders are cached and their arrays
are read-only.

Internal boundaries the cases are placed on:

    nnd_forward_kernel     64 queries per workgroup, 1024-target LDS tile, 256-target quarter per wave, 4-wave merge
    vote_count_kernel      4096-pixel LDS tile, 4 hypotheses per workgroup; voting / generators: 256-thread blocks
    yolox_decode_sort      bitonic sort padded to a power of two in [64, 16384]; 16384 anchors is the limit
    nms_mask / nms_scan    64 x 64 tiles, triangular first tile, max_det truncation
    paste_rle_kernel       1024 columns per chunk, 1024 runs per pass of the length conversion, max_runs cut-off
    flow_kernel            grid capped at 256 * 64 blocks of 256 threads, grid-stride beyond
    fps_*                  LDS tier up to 12288 points (12 per thread), global tier above; lowest index wins ties
"""
from functools import lru_cache

import numpy as np

from oracle import postproc as P


def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


def lattice(rng, shape):
    """Integer coordinates in [-8, 8] as float32: every squared distance is an integer below 2^24, hence exact in fp32."""
    return rng.integers(-8, 9, shape).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- NN distance
_NND_PAIRS = [(1, 1), (63, 255), (64, 256), (65, 257), (64, 1023), (65, 1024), (1, 1025), (130, 2049)]
NND_SHAPES = _NND_PAIRS + [(m, n) for n, m in _NND_PAIRS if n != m]          # each pair and its swap ((1, 1) is its own)
NND_TIE_INDICES = (5, 300, 600, 900, 1030, 2048)      # one copy per wave quarter of tile 0, one in tile 1, one in tile 2
NND_QUARTER = 256


@lru_cache(maxsize=None)
def nnd_shape_case(n, m):
    """b = 2: image 0 random floats, image 1 lattice points (ties in most rows once m exceeds a few hundred)."""
    rng = np.random.default_rng([101, n, m])
    x1 = np.stack([rng.standard_normal((n, 3)).astype(np.float32), lattice(rng, (n, 3))])
    x2 = np.stack([rng.standard_normal((m, 3)).astype(np.float32), lattice(rng, (m, 3))])
    return _frozen(x1, x2)


@lru_cache(maxsize=None)
def nnd_tie_case():
    """-> (queries f32[1,130,3], targets f32[1,2049,3], point).  ``point`` sits at NND_TIE_INDICES of the targets and nowhere
    else; the queries are 4 copies of it, 62 midpoints of two distinct targets (half-integer coordinates, still exact) and 64
    lattice points."""
    rng = np.random.default_rng(102)
    m = 2049
    t = lattice(rng, (m, 3))
    point = np.array([3.0, -2.0, 5.0], np.float32)
    clash = (t == point).all(1)
    t[clash, 0] = -point[0]                                 # move the accidental copies away
    t[list(NND_TIE_INDICES)] = point
    a, b = rng.integers(0, m, 62), rng.integers(0, m, 62)
    q = np.concatenate([np.tile(point, (4, 1)), (t[a] + t[b]) * np.float32(0.5), lattice(rng, (64, 3))]).astype(np.float32)
    assert q.shape == (130, 3)
    return _frozen(q[None].copy(), t[None].copy(), point)


def nnd_tied_queries(q, t):
    """Number of queries whose minimum squared distance (exact in float64) is attained by targets of at least two different
    256-quarters (different waves of one tile, or different tiles)."""
    d = ((q[:, None, :].astype(np.float64) - t[None].astype(np.float64)) ** 2).sum(-1)
    at_min = d == d.min(1, keepdims=True)
    return sum(len(set(np.flatnonzero(row) // NND_QUARTER)) >= 2 for row in at_min)


@lru_cache(maxsize=None)
def nnd_grad_case(kind):
    """kind "lattice": b = 2, n = 1000 lattice queries on m = 3 targets (about 333 colliding atomics per target), integer
    graddist; kind "float": random floats at (65, 1025).  -> (x1, x2, gd1, gd2)."""
    if kind == "lattice":
        rng = np.random.default_rng(103)
        x1, x2 = lattice(rng, (2, 1000, 3)), lattice(rng, (2, 3, 3))
        gd1, gd2 = rng.integers(-4, 5, (2, 1000)).astype(np.float32), rng.integers(-4, 5, (2, 3)).astype(np.float32)
    else:
        rng = np.random.default_rng(104)
        x1, x2 = rng.standard_normal((2, 65, 3)).astype(np.float32), rng.standard_normal((2, 1025, 3)).astype(np.float32)
        gd1, gd2 = rng.standard_normal((2, 65)).astype(np.float32), rng.standard_normal((2, 1025)).astype(np.float32)
    return _frozen(x1, x2, gd1, gd2)


def nnd_grad_reference(x1, x2, gd1, gd2, idx1, idx2):
    """float64 scatter-add of 2 g (p1 - p2) with the forward's indices -> (g1, g2, c1, c2, s1, s2): the gradients, and per output
    element the number of terms c and the sum of their magnitudes s (what the fp32 error bound is made of)."""
    x1, x2, gd1, gd2 = (np.asarray(a, np.float64) for a in (x1, x2, gd1, gd2))
    out = [np.zeros_like(x1), np.zeros_like(x2)]
    cnt = [np.zeros_like(x1), np.zeros_like(x2)]
    mag = [np.zeros_like(x1), np.zeros_like(x2)]
    for own, other, pa, pb, gd, idx in ((0, 1, x1, x2, gd1, idx1), (1, 0, x2, x1, gd2, idx2)):
        for b in range(pa.shape[0]):
            term = 2.0 * gd[b][:, None] * (pa[b] - pb[b][idx[b]])
            out[own][b] += term
            cnt[own][b] += 1
            mag[own][b] += np.abs(term)
            np.add.at(out[other][b], idx[b], -term)
            np.add.at(cnt[other][b], idx[b], 1.0)
            np.add.at(mag[other][b], idx[b], np.abs(term))
    return out[0], out[1], cnt[0], cnt[1], mag[0], mag[1]


# -------------------------------------------------------------------------------------------------------- RANSAC voting
VOTE_SHAPES = [(1, 1, 1), (63, 1, 3), (256, 2, 5), (257, 9, 2), (4095, 3, 4), (4096, 3, 5), (4097, 1, 7), (8193, 2, 6)]   # tn, vn, hn
VOTE_THRESHOLDS = (0.99, 0.999)
VOTE_PIX_TILE = 4096


@lru_cache(maxsize=None)
def voting_case(tn, vn, hn):
    """The construction of test_gpu_parity's ``_voting_case`` (pixels on a 64 x 64 grid, unit directions to vn keypoints plus
    noise, zero-norm directions in front, hypothesis 0 from degenerate pairs) made to work down to tn = 1: min(5, tn // 4)
    zero-norm rows instead of 5, and the last pixel's directions are noise-free.  -> (direct, coords, idxs, kp); ``kp``
    f32[vn,2] are the true keypoints, which ``voting_hypotheses`` plants as the last hypothesis so that every shape, variant
    and threshold has inliers (with one pixel the only generated hypothesis is degenerate), the last pixel among them."""
    rng = np.random.default_rng([11, tn, vn, hn])
    coords = np.stack([rng.integers(0, 64, tn), rng.integers(0, 64, tn)], 1).astype(np.float32)
    kp = rng.uniform(-20, 84, (vn, 2)).astype(np.float32)
    d = kp[None] - coords[:, None]
    d = d / np.maximum(np.linalg.norm(d, axis=-1, keepdims=True), 1e-6)
    noise = rng.normal(0, 0.05, d.shape)
    noise[-1] = 0
    direct = (d + noise).astype(np.float32)
    direct[:min(5, tn // 4)] = 0
    idxs = rng.integers(0, tn, (hn, vn, 2)).astype(np.int32)
    idxs[0, :, 1] = idxs[0, :, 0]
    return _frozen(direct, coords, idxs, kp)


def voting_hypotheses(case, vp):
    """The oracle's generated hypotheses f32[hn,vn,2 or 3] with the true keypoints planted in the last row."""
    direct, coords, idxs, kp = case
    hyp = P.generate_hypothesis(direct, coords, idxs, vp).copy()
    hyp[-1, :, :2] = kp
    if vp:
        hyp[-1, :, 2] = 1.0
    return hyp


# ------------------------------------------------------------------------------------------------- YOLOX post-processing
YOLOX_ANCHORS = [1, 63, 64, 65, 100, 4096, 16384]
YOLOX_CLASSES = [1, 21]
YOLOX_LIMIT = 16384
YOLOX_DENSE_CONF = 0.001
NMS_THRE = 0.45


@lru_cache(maxsize=None)
def yolox_anchor_case(a, c):
    """test_gpu_parity's dense case at ``a`` anchors, B = 3: boxes scattered round 60 centres, image 0 with a block of exact
    duplicate rows (up to 40), image 2 with nothing above YOLOX_DENSE_CONF."""
    rng = np.random.default_rng([7, a, c])
    b = 3
    det = np.zeros((b, a, 5 + c), np.float32)
    centres = rng.uniform(40, 600, (b, 60, 2))
    which = rng.integers(0, 60, (b, a))
    det[..., 0:2] = np.take_along_axis(centres, which[..., None].repeat(2, -1), 1) + rng.normal(0, 6, (b, a, 2))
    det[..., 2:4] = rng.uniform(30, 160, (b, a, 2))
    det[..., 4] = rng.uniform(0, 1, (b, a)) ** 2
    det[..., 5:] = rng.uniform(0, 1, (b, a, c)) ** 4
    lo = a // 3
    det[0, lo, 4:] = np.maximum(det[0, lo, 4:], 0.5)          # the duplicated row is a candidate
    det[0, lo:min(a, lo + 40)] = det[0, lo]
    det[2, :, 4] *= 1e-6
    return _frozen(det)


NMS_TILE_COUNTS = [64, 65, 128, 129]
NMS_SPARSE_CONF = 0.25


@lru_cache(maxsize=None)
def yolox_sparse_case(n, seed=0):
    """A = 256 anchors, one class, 6 x 6 boxes on an 8-pixel 16 x 16 grid (nothing overlaps); exactly ``n`` anchors, a random subset,
    carry distinct scores above NMS_SPARSE_CONF, the others 0.01.  -> det f32[1,256,6]; all n must be kept."""
    rng = np.random.default_rng([8, n, seed])
    a = 256
    det = np.zeros((1, a, 6), np.float32)
    k = np.arange(a)
    det[0, :, 0], det[0, :, 1] = 8 * (k % 16) + 4, 8 * (k // 16) + 4
    det[0, :, 2:4] = 6
    det[0, :, 4] = 0.01
    det[0, :, 5] = 1.0
    det[0, rng.permutation(a)[:n], 4] = (0.3 + 0.65 * rng.permutation(n) / n).astype(np.float32)
    return _frozen(det)


LADDER_LEN = 130


@lru_cache(maxsize=None)
def yolox_ladder_case():
    """One class, B = 2, A = 131.  A ladder of LADDER_LEN 10 x 10 boxes, each shifted 3 pixels from the last (IoU 7/13 with
    the neighbour, 4/16 with the one after), scores 1 - rank / 256 descending.  Image 0: the ladder is candidates 0..129, so
    the odd ones die (63, 65, 127, 129 beside the tile edges) and 64 / 128 must survive a dead neighbour's row.  Image 1: an
    isolated box takes rank 0 and the ladder ranks 1..130, so the even ones die (64, 128) and 63 / 65 / 127 / 129 are kept."""
    a = LADDER_LEN + 1
    det = np.zeros((2, a, 6), np.float32)
    det[..., 2:4] = 10
    det[..., 5] = 1.0
    k = np.arange(LADDER_LEN)
    det[0, :LADDER_LEN, 0], det[0, :LADDER_LEN, 1] = 3 * k + 5, 20
    det[0, :LADDER_LEN, 4] = 1 - k / 256
    det[0, LADDER_LEN, 0:2] = (5, 100)                        # below the threshold
    det[0, LADDER_LEN, 4] = 0.01
    det[1, 0, 0:2] = (5, 100)                                 # isolated, best score
    det[1, 0, 4] = 1.0
    det[1, 1:, 0], det[1, 1:, 1] = 3 * k + 5, 20
    det[1, 1:, 4] = 1 - (k + 1) / 256
    return _frozen(det)


def iou_f32(r1, r2):
    """IoU of two decoded rows (cx, cy, w, h, ...) in the oracle's float arithmetic (oracle/nms_oracle.c: corners, areas,
    inter / (a1 + a2 - inter), every operation rounded to fp32)."""
    f = np.float32
    two = f(2)

    def corners(r):
        r = np.asarray(r, f)
        return r[0] - r[2] / two, r[1] - r[3] / two, r[0] + r[2] / two, r[1] + r[3] / two

    a, b = corners(r1), corners(r2)
    area_a, area_b = (a[2] - a[0]) * (a[3] - a[1]), (b[2] - b[0]) * (b[3] - b[1])
    w = max(min(a[2], b[2]) - max(a[0], b[0]), f(0))
    h = max(min(a[3], b[3]) - max(a[1], b[1]), f(0))
    inter = f(w * h)
    return f(inter / f(f(area_a + area_b) - inter))


MAX_DET_CASES = [1, 64, 128]


@lru_cache(maxsize=None)
def yolox_max_det_case():
    """B = 2 sparse images: 129 kept in image 0, 64 in image 1."""
    return _frozen(np.concatenate([yolox_sparse_case(129), yolox_sparse_case(64, seed=1)]))


# ------------------------------------------------------------------------------------------ mask paste + run-length coding
PASTE_IMAGES = [(1, 1), (1, 1500), (7, 1024), (7, 1025), (5, 2049), (720, 1280)]       # H, W
PASTE_MASKS = [(64, 64), (28, 40), (56, 17)]                                            # hm, wm
PASTE_CHUNK = 1024


def paste_boxes(h, w):
    """x0, y0, x1, y1 f32[4,4]: inside the image; centred near the column-chunk edge at x = 1024 (near the right border, and
    across it, where the image ends there or before); partly outside (top left); covering the whole image."""
    edge = min(PASTE_CHUNK, w)
    return np.array([[0.2 * w + 0.3, 0.1 * h - 0.35, 0.7 * w + 0.9, 0.8 * h + 0.45],
                     [edge - 37.6, 0.15 * h - 0.4, edge + 29.7, 0.9 * h + 0.35],
                     [-0.3 * w - 2.5, -0.2 * h - 1.5, 0.4 * w + 0.5, 0.6 * h + 0.7],
                     [-1.5, -2.5, w + 2.5, h + 1.5]], np.float32)


@lru_cache(maxsize=None)
def paste_masks(hm, wm):
    """Four soft blobs f32[4,hm,wm] (one per box of ``paste_boxes``) with 10 % noise: ragged outlines, several runs per column."""
    rng = np.random.default_rng([9, hm, wm])
    yy, xx = np.mgrid[0:hm, 0:wm]
    m = [np.clip(1.4 - np.hypot((yy - (hm - 1) / 2 + k) / hm, (xx - (wm - 1) / 2) / wm) * (4.5 - 0.5 * k), 0, 1) * 0.9
         + 0.1 * rng.random((hm, wm)) for k in range(4)]
    return _frozen(np.stack(m).astype(np.float32))


CHECKER_IMAGE = (64, 2048)


@lru_cache(maxsize=None)
def paste_checker_case():
    """A 64 x 64 checkerboard (0.9 / 0.1) pasted at identity scale over columns 992..1055 of a 64 x 2048 image: every pixel of
    those 64 columns starts a run, across the chunk edge.  -> (mask f32[1,64,64], box f32[1,4])."""
    yy, xx = np.mgrid[0:64, 0:64]
    mask = np.where((yy + xx) % 2 == 0, 0.9, 0.1).astype(np.float32)[None]
    box = np.array([[992.0, 0.0, 1056.0, 64.0]], np.float32)
    return _frozen(mask, box)


@lru_cache(maxsize=None)
def paste_cutoff_cases():
    """-> [(name, mask f32[1,hm,wm], box f32[1,4], H, W)]: an instance with a few dozen runs and the checkerboard (> 1024 runs, so the
    cut-off falls inside a later pass of the length conversion)."""
    h, w = 7, 1025
    small = (paste_masks(64, 64)[1:2], paste_boxes(h, w)[1:2], h, w)
    return [("chunk-edge",) + small, ("checker",) + paste_checker_case() + CHECKER_IMAGE]


# ----------------------------------------------------------------------------------------------------------------- flow
FLOW_SHAPES = [(1, 1, 1), (3, 1, 257), (2, 17, 33), (2, 1200, 1920)]      # B, H, W
FLOW_ONE_PASS = 256 * 64 * 256                                           # pixels one pass of the capped grid covers


@lru_cache(maxsize=None)
def flow_case(b, h, w):
    """test_gpu_parity's mixed batch at (b, h, w): smooth depth, 10 % holes, target = source + 1.5 mm noise, a translation of a few
    millimetres per image (none for image 0), principal point at the image centre.  -> (ds, dt, KT, Kinv)."""
    rng = np.random.default_rng([3, b, h, w])
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    ds = np.stack([(np.float32(0.7 + 0.05 * i) + np.float32(0.1) * np.sin(xx / np.float32(9.0 + i)) * np.cos(yy / np.float32(7.0)))[None]
                   for i in range(b)]).astype(np.float32)
    ds[rng.random(ds.shape, dtype=np.float32) < 0.1] = 0
    dt = ds + rng.standard_normal(ds.shape, dtype=np.float32) * np.float32(1.5e-3)
    K = np.array([[500.0, 0, (w - 1) / 2], [0, 500.0, (h - 1) / 2], [0, 0, 1]], np.float32)
    t = rng.normal(0, 2e-3, (b, 3, 1)).astype(np.float32)
    t[0] = 0
    KT = np.stack([K @ np.concatenate([np.eye(3, dtype=np.float32), t[i]], 1) for i in range(b)]).astype(np.float32)
    Kinv = np.stack([np.linalg.inv(K.astype(np.float64)).astype(np.float32)] * b)
    return _frozen(ds, dt, KT, Kinv)


# ------------------------------------------------------------------------------------------------------------------ FPS
FPS_SIZES = [1, 64, 1023, 1024, 1025]
FPS_LDS_POINTS = 12288


def fps_sample_counts(pn):
    return [1, 8, pn + 3]


@lru_cache(maxsize=None)
def fps_lattice_case(pn):
    """b = 2 lattice clouds and a start index per cloud for the explicit-start mode."""
    rng = np.random.default_rng([13, pn])
    return _frozen(lattice(rng, (2, pn, 3)), rng.integers(0, pn, 2).astype(np.int32))


FPS_DUPLICATE_SIZES = [FPS_LDS_POINTS, FPS_LDS_POINTS + 2]      # the last LDS-tier size, and the global tier
FPS_DUPLICATE_OFFSET = FPS_LDS_POINTS // 2
FPS_DUPLICATE_SAMPLES = 24


@lru_cache(maxsize=None)
def fps_duplicate_case(pn):
    """One lattice cloud of pn points in which point i is repeated at i + 6144 for i < 6144 (another thread, another wave):
    every farthest point exists at least twice.  -> (pts f32[1,pn,3], start i32[1])."""
    rng = np.random.default_rng([14, pn])
    half = FPS_DUPLICATE_OFFSET
    pts = lattice(rng, (pn, 3))
    pts[half:2 * half] = pts[:half]
    return _frozen(pts[None].copy(), np.array([half + 17], np.int32))


FPS_IDENTICAL = (2000, 6)       # pn, sn


@lru_cache(maxsize=None)
def fps_identical_case():
    pts = np.tile(np.array([[1.5, -2.0, 0.25]], np.float32), (FPS_IDENTICAL[0], 1))[None]
    return _frozen(pts.copy(), np.array([1234], np.int32))


def fps_tie_steps(pts, idxs, init_center):
    """Selection steps of the sequence ``idxs`` over ``pts`` [pn,3] at which the maximum of the running minimum distance is positive
    and attained by at least two points.  float64 on lattice points: exact.  The bbox-centre seeding of ``init_center`` has
    half-integer coordinates on the lattice, still exact."""
    p = np.asarray(pts, np.float64)
    md = np.full(len(p), np.inf)
    if init_center:
        c = (p.max(0) + p.min(0)) * 0.5
        md = ((p - c) ** 2).sum(1)
    live = np.ones(len(p), bool)
    ties = 0
    for s, cur in enumerate(idxs):
        if s > 0 or init_center:
            cand = np.where(live, md, -1.0)
            top = cand.max()
            assert top <= 0 or cand[cur] == top, "the sequence is not a farthest-point sequence"
            ties += int(top > 0 and (cand == top).sum() >= 2)
        live[cur] = False
        md = np.minimum(md, ((p - p[cur]) ** 2).sum(1))
    return ties
