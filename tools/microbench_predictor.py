"""Image -> pose records on one MI355X: ``YoloGdrnPredictor`` against the same chain staged with what existed before it.

YOLOX-x at 640 x 640 over 640 x 480 BGR images (r = 1: LM-O / YCB-V), ConvNeXt GDRN with depth refinement, ``--batch`` images per
call.  The detector's weights are random, so the confidence threshold is calibrated once, outside the timing, to the score that
leaves about ``--rois`` candidates per image; the ROI count of the timed calls is reported.

  (a) predictor   gdrnpp_yolox_letterbox (Focus form) -> hip_forward -> yolox_postprocess -> gdrnpp_rois_from_dets -> one pinned
                  read-back of the counts -> batch_from_uploaded -> inference_step
  (b) staged      letterbox with torch operators (canvas of 114, slice assignment of the converted image: r = 1 needs no resize)
                  -> YOLOX.forward -> yolox_postprocess -> detections_from_yolox (count.tolist(), dets.cpu()) ->
                  batch_data_test_gpu (NumPy ROI arithmetic, packed upload) -> inference_step

images/s: wall clock over ``--iters`` calls, median of ``--repeats``; ms per stage: HIP events around each stage of one call,
median over the same calls (stages with a host read-back include the wait for it).

    python tools/microbench_predictor.py [--out profiles/predictor_microbench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gdrnpp_bop2022_amd import hip_lib, synthetic as S  # noqa: E402
from gdrnpp_bop2022_amd.det.yolox.models import build_yolox, hip_forward  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling import YoloGdrnPredictor, engine  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling.GDRN_double_mask import build_model_optimizer  # noqa: E402

DEV = "cuda"


class Stages:
    """HIP events between the stages of one call; ``ms()`` after a synchronize."""

    def __init__(self):
        self.marks = []
        self.mark(None)

    def mark(self, name):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self.marks.append((name, e))

    def ms(self):
        torch.cuda.synchronize()
        return {n: a.elapsed_time(b) for (_, a), (n, b) in zip(self.marks, self.marks[1:])}


def predictor_call(p, images, depths, st=None):
    mark = st.mark if st else (lambda n: None)
    b, H, W, _ = images.shape
    foc = hip_forward.focus_buffer(p.yolox, b, p.test_size[0], p.test_size[1], images.device)
    _, ratio = hip_lib.yolox_letterbox(images, p.test_size, out=foc, focus=True)
    mark("letterbox")
    det = hip_forward.forward(p.yolox, None, focus=foc)["det_preds"]
    mark("yolox_forward")
    dets, count = hip_lib.yolox_postprocess(det, p.num_classes, p.conf_thr, p.nms_thr, p.class_agnostic, p.max_det)
    mark("postprocess")
    table, counts = hip_lib.rois_from_dets(dets, count, ratio, H, W, p.cam, p.extents, p.cfg.INPUT.DZI_PAD_SCALE,
                                           p.cfg.MODEL.POSE_NET.OUTPUT_RES, p.score_thr, p.top_k_per_obj, p.roi_cap)
    host = torch.empty((1 + b,), dtype=torch.int32, pin_memory=True)
    host.copy_(counts, non_blocking=True)
    ev = torch.cuda.Event()
    ev.record()
    ev.synchronize()
    n = int(host[0])
    mark("rois_hand_off")
    batch = engine.batch_from_uploaded(p.cfg, images, depths, {k: v[:n] for k, v in table.items()})
    mark("crop")
    rec = engine.inference_step(p.model, p.post, batch)
    mark("gdrn_step")
    return rec, n


def staged_call(p, images, depths, st=None):
    mark = st.mark if st else (lambda n: None)
    b, H, W, _ = images.shape
    ht, wt = p.test_size
    r, rh, rw = p.sizes(H, W, p.test_size)
    assert (rh, rw) == (H, W), "the staged letterbox of this tool covers r = 1 only"
    x = torch.full((b, 3, ht, wt), 114.0, device=images.device)
    x[:, :, :H, :W] = images.permute(0, 3, 1, 2).float()
    mark("letterbox")
    det = p.yolox(x)["det_preds"]
    mark("yolox_forward")
    dets, count = hip_lib.yolox_postprocess(det, p.num_classes, p.conf_thr, p.nms_thr, p.class_agnostic, p.max_det)
    mark("postprocess")
    d = engine.detections_from_yolox(dets, count, p.cam.cpu().numpy(), p.extents.cpu().numpy(), r)
    mark("rois_hand_off")
    batch = engine.batch_data_test_gpu(p.cfg, images, depths, d)
    mark("crop")
    rec = engine.inference_step(p.model, p.post, batch)
    mark("gdrn_step")
    return rec, len(d["roi_cls"])


def measure(call, p, images, depths, iters, repeats):
    with torch.no_grad():
        for _ in range(3):
            rec, n = call(p, images, depths)
        torch.cuda.synchronize()
        rates, stages = [], []
        for _ in range(repeats):
            t0 = time.perf_counter()
            for _ in range(iters):
                rec, n = call(p, images, depths)
            torch.cuda.synchronize()
            rates.append(iters * images.shape[0] / (time.perf_counter() - t0))
        for _ in range(max(5, iters)):
            st = Stages()
            call(p, images, depths, st)
            stages.append(st.ms())
    med = {k: statistics.median(s[k] for s in stages) for k in stages[0]}
    return dict(images_per_s=statistics.median(rates), ms_per_stage=med, ms_per_call_sum_of_stages=sum(med.values()), rois_per_call=n), rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictor_microbench.json"))
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--rois", type=int, default=8, help="candidates per image the confidence threshold is calibrated to")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--yolox", default="x", choices=["x", "s"])
    args = ap.parse_args()
    hip_lib.load()
    torch.manual_seed(0)
    cfg = get_cfg("ycbv_convnext_a6", opts=["TEST.USE_DEPTH_REFINE=True", "INPUT.WITH_DEPTH=True"])
    model, _ = build_model_optimizer(cfg)
    model.load_state_dict(S.seeded_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 5), strict=True)
    with torch.no_grad():
        model.pnp_net.fc_t.bias.copy_(torch.tensor([0.0, 0.0, 1.5 * float(S.YCBV_K[0, 0]) * 0.19 / 64.0]))
    rng = np.random.default_rng(9)
    nc = cfg.MODEL.POSE_NET.NUM_CLASSES
    verts, faces, ext = S.make_models(nc, rng, 2)
    post = engine.GdrnHipPost(cfg, hip_lib.MeshSet(verts, faces, DEV))
    depth, width = {"x": (1.33, 1.25), "s": (0.33, 0.50)}[args.yolox]
    yolox = build_yolox(depth, width, nc).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(1)
    images = torch.randint(0, 256, (args.batch, 480, 640, 3), dtype=torch.uint8, device=DEV, generator=g)
    depths = torch.rand((args.batch, 480, 640), device=DEV, generator=g) + 0.5
    with torch.no_grad():                    # calibration: the score that leaves ~args.rois candidates per image
        x, _ = hip_lib.yolox_letterbox(images, (640, 640))
        det = yolox(x)["det_preds"]
        score = (det[..., 4] * det[..., 5:].max(-1).values).flatten()
        conf_thr = float(torch.sort(score, descending=True).values[args.rois * args.batch])
    p = YoloGdrnPredictor(yolox, model, post, cfg, test_size=(640, 640), num_classes=nc, conf_thr=conf_thr, nms_thr=0.45,
                          cam=S.YCBV_K.astype(np.float32), extents=ext.astype(np.float32), max_det=64, roi_cap=256)
    a, rec_a = measure(predictor_call, p, images, depths, args.iters, args.repeats)
    b, rec_b = measure(staged_call, p, images, depths, args.iters, args.repeats)
    with torch.no_grad():
        rec_p, per_image = p(images, depths)
    out = dict(device=torch.cuda.get_device_name(0), detector=f"YOLOX-{args.yolox}, {nc} classes, random weights", test_size=[640, 640],
               image=[480, 640], batch=args.batch, gdrn="ycbv_convnext_a6 + depth refine", conf_thr=conf_thr, rois_per_image=per_image,
               method=dict(iters=args.iters, repeats=args.repeats), predictor=a, staged=b,
               predictor_over_staged=a["images_per_s"] / b["images_per_s"],
               records_bit_equal=bool(rec_a.shape == rec_b.shape and torch.equal(rec_a.view(torch.int32), rec_b.view(torch.int32))
                                      and torch.equal(rec_p.view(torch.int32), rec_a.view(torch.int32))))
    for name, r in (("predictor", a), ("staged", b)):
        print(f"{name}: {r['images_per_s']:.1f} images/s, {r['rois_per_call']} ROIs per call; ms per stage " +
              ", ".join(f"{k} {v:.3f}" for k, v in r["ms_per_stage"].items()), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out, "records bit-equal:", out["records_bit_equal"])


if __name__ == "__main__":
    main()
