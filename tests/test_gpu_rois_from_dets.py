"""-m gpu: gdrnpp_rois_from_dets against the host hand-off it replaces, bit for bit in the float64 and the float32 columns.

Synthetic ``gdrnpp_yolox_postprocess`` output: B = 3 images of 540 x 720 letterboxed to 640 x 640 (ratio = 640 / 720),
max_det = 16, counts (0, 5, 16), 4 classes; within image 2 two equal scores in one class (tie stability), one score below
score_thr, one box narrower than 1 px (the >= 1 clamp) and one whose scale hits the max(H, W) clamp.

  top_k_per_obj = 0       roi_host_arrays(cfg, detections_from_yolox(...))            (NMS order kept)
  top_k_per_obj = 1, 2    roi_host_arrays(cfg, detections_from_bop_json(...))          (class order, then descending score)"""
import numpy as np
import pytest
import torch

from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd.gdrn_modeling import roi_stream
from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg

pytestmark = pytest.mark.gpu
DEV = "cuda"
B, MAX_DET, C, H, W = 3, 16, 4, 540, 720
RATIO = 640 / 720
COUNTS = (0, 5, 16)
SCORE_THR = 0.3


@pytest.fixture(scope="module")
def case():
    rng = np.random.RandomState(20221104)
    dets = np.zeros((B, MAX_DET, 7), np.float32)
    for b, n in enumerate(COUNTS):
        x1 = rng.uniform(0, 400, n)
        y1 = rng.uniform(0, 300, n)
        dets[b, :n, 0], dets[b, :n, 1] = x1, y1
        dets[b, :n, 2], dets[b, :n, 3] = x1 + rng.uniform(20, 200, n), y1 + rng.uniform(20, 150, n)
        dets[b, :n, 4], dets[b, :n, 5] = rng.uniform(0.6, 1.0, n), rng.uniform(0.6, 1.0, n)
        dets[b, :n, 6] = rng.randint(0, C, n)
    dets[1, 5:] = 7.0                                     # rows beyond count: stale values that must not be read
    d = dets[2]
    d[:, 6] = np.array([2, 0, 1, 2, 3, 2, 0, 1, 2, 3, 0, 1, 2, 3, 0, 1], np.float32)
    d[8, 4:6] = d[3, 4:6]                                 # a tie within class 2, rows 3 and 8 ...
    d[0, 4:6] = (0.99, 0.99)                              # ... below the class's best score, above the others
    d[3, 4:6] = d[8, 4:6] = (0.95, 0.95)
    for j in (5, 12):
        d[j, 4:6] = (0.7, 0.7)
    d[6, 4:6] = (0.5, 0.5)                                # 0.25 < SCORE_THR
    d[9, 2] = d[9, 0] + 0.5                               # narrower than 1 px after / ratio
    d[10, :4] = (10.0, 20.0, 630.0, 470.0)                # scale = 697.5 * 1.5 > max(H, W)
    count = np.array(COUNTS, np.int32)
    cam = np.array([[572.4, 0, 325.3], [0, 573.6, 242.0], [0, 0, 1]], np.float32)
    extents = rng.uniform(0.05, 0.3, (C, 3)).astype(np.float32)
    cfg = get_cfg("ycbv_convnext_a6")
    return cfg, dets, count, cam, extents


def run(case, top_k=0, score_thr=0.0, cap=64, cam=None):
    cfg, dets, count, cam0, extents = case
    cam = cam0 if cam is None else cam
    table = {k: torch.full_like(v, 99) for k, v in hip_lib.roi_table(cap, DEV).items()}
    table, counts = hip_lib.rois_from_dets(torch.from_numpy(dets).to(DEV), torch.from_numpy(count).to(DEV), RATIO, H, W,
                                           torch.from_numpy(cam).to(DEV), torch.from_numpy(extents).to(DEV), cfg.INPUT.DZI_PAD_SCALE,
                                           cfg.MODEL.POSE_NET.OUTPUT_RES, score_thr, top_k, cap, table=table)
    torch.cuda.synchronize()
    counts = counts.cpu().tolist()
    return {k: v.cpu().numpy() for k, v in table.items()}, counts[0], counts[1:]


def host_dets(case):
    cfg, dets, count, cam, extents = case
    return roi_stream.detections_from_yolox(torch.from_numpy(dets), torch.from_numpy(count), cam, extents, RATIO)


def check(table, n, host):
    assert n == len(host["scale"])
    for k, a in host.items():
        got = table[k][:n]
        assert got.dtype == a.dtype and got.shape == a.shape, k
        assert np.array_equal(got.view(np.uint8), np.ascontiguousarray(a).view(np.uint8)), (k, got, a)
    assert np.array_equal(table["roi_id"][:n], np.arange(n, dtype=np.int32))
    for k, v in table.items():
        assert (v[n:] == 99).all(), f"{k}: rows beyond n_rois were written"


def test_nms_order_table_equals_the_host_hand_off(hip, case):
    cfg = case[0]
    det = host_dets(case)
    host = roi_stream.roi_host_arrays(cfg, det, H, W)
    table, n, per_image = run(case)
    assert n == sum(COUNTS) and per_image == list(COUNTS)
    check(table, n, host)
    assert table["roi_wh"][:n, 0].min() == 1.0 and table["scale64"][:n].max() == 720.0, "the case must reach both clamps"


def test_score_threshold_drops_in_place(hip, case):
    cfg = case[0]
    det = host_dets(case)
    keep = ~(det["score"].astype(np.float64) < SCORE_THR)
    assert keep.sum() == len(keep) - 1
    sub = dict(det, **{k: det[k][keep] for k in ("bbox", "im_idx", "roi_cls", "score")})
    table, n, per_image = run(case, score_thr=SCORE_THR)
    assert per_image == [0, 5, 15]
    check(table, n, roi_stream.roi_host_arrays(cfg, sub, H, W))


@pytest.mark.parametrize("top_k", [1, 2])
def test_top_k_per_object_equals_the_bop_selection(hip, case, top_k):
    cfg = case[0]
    det = host_dets(case)
    bb = det["bbox"].astype(np.float64)
    book = {}
    for j in range(len(det["score"])):
        book.setdefault(int(det["im_idx"][j]), []).append(
            dict(obj_id=int(det["roi_cls"][j]) + 1, bbox_est=[bb[j, 0], bb[j, 1], bb[j, 2] - bb[j, 0], bb[j, 3] - bb[j, 1]],
                 score=float(det["score"][j])))
    sel = roi_stream.detections_from_bop_json(book, list(range(B)), [1, 2, 3, 4], det["cam"], det["extents"], top_k_per_obj=top_k,
                                              score_thr=SCORE_THR)
    sel.pop("time")
    # the tie: rows 3 and 8 of image 2 (class 2) score the same, below row 0 — top 1 keeps row 0, top 2 adds row 3, never row 8
    cls2 = (sel["im_idx"] == 2) & (sel["roi_cls"] == 2)
    first = det["bbox"][5:][[0, 3]][:top_k]
    assert np.array_equal(sel["bbox"][cls2], first)
    table, n, per_image = run(case, top_k=top_k, score_thr=SCORE_THR)
    assert per_image == [int((sel["im_idx"] == b).sum()) for b in range(B)] and per_image[0] == 0
    check(table, n, roi_stream.roi_host_arrays(cfg, sel, H, W))


def test_cap_truncates_the_tail(hip, case):
    cfg = case[0]
    host = roi_stream.roi_host_arrays(cfg, host_dets(case), H, W)
    table, n, per_image = run(case, cap=4)
    assert n == 4 and per_image == [0, 4, 0]
    check(table, n, {k: v[:4] for k, v in host.items()})
    table, n, per_image = run(case, cap=7)
    assert n == 7 and per_image == [0, 5, 2]
    check(table, n, {k: v[:7] for k, v in host.items()})


def test_per_image_cameras(hip, case):
    cfg = case[0]
    cams = np.stack([case[3] * (1 + 0.1 * b) for b in range(B)]).astype(np.float32)
    det = host_dets(case)
    host = roi_stream.roi_host_arrays(cfg, dict(det, cam=cams[det["im_idx"]]), H, W)
    table, n, _ = run(case, cam=cams)
    check(table, n, host)


def test_argument_errors_launch_nothing(hip, case):
    _, dets, count, cam, extents = case
    with pytest.raises(RuntimeError, match="max_det"):
        hip_lib.rois_from_dets(torch.zeros((1, 2000, 7), device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV), 1.0, H, W,
                               torch.from_numpy(cam).to(DEV), torch.from_numpy(extents).to(DEV))
