"""Golden vectors of the YOLOX detector from the reference's own modules (authoring container only: needs the reference
checkout that tests/golden/_refimport.py imports from).

What runs here is the reference's ``YOLOX(YOLOPAFPN, YOLOXHead)`` (det/yolox/models), imported from its files, in fp32 and in
fp64 on the CPU with the seeded parameters and images of tests/golden/yolox_seeded.py.  ``det.yolox.utils`` (box utilities of
the training losses, cv2 / torchvision at import) is stood in for by an inert module: nothing of it runs in an eval forward.
Recorded per case of ``yolox_seeded.CASES`` in yolox_net_golden_<case>.npz (one file per case: each stays below 1 MiB):

  <case>/rows                         anchor rows stored (all, or a seeded subset for the 640 x 640 case)
  <case>/det64, det32                 the reference's det_preds[:, rows] in fp64 and in fp32 (fp32 is left out of the batch-2 case,
                                      whose file would pass 1 MiB: the tests compare against fp64, fp32 enters through e_ref and kept32)
  <case>/e_ref_<group>                max |fp32 - fp64| over ALL anchors per group xy, wh (pixels), obj, cls: the unit of the bars
  <case>/range_<group>                achieved (min, max) of the fp64 values; raw logit / pre-exp ranges as range_raw_<group>
  <case>/keys, shapes                 the reference's state_dict manifest
  <case>/param_digest, input_digest   digests of the seeded values
  <case>/conf_thre, nms_thre, e_ref_score, score_margin, iou_margin, kept32     the hand-off check (full-row cases): thresholds
                                      for which the reference's fp32 and fp64 outputs keep the same boxes, with their margins
  conv_shapes                         the 26 distinct (Cin, Cout, k, stride) of YOLOX-x with 21 classes
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)

import _refimport  # noqa: E402

_refimport.install()
for name in ("det.yolox.utils", "det.yolox.utils.model_utils"):
    sys.modules[name] = _refimport._StubModule(name)
    sys.modules[name].__path__ = []

import yolox_seeded as YS  # noqa: E402
from det.yolox.models import YOLOPAFPN, YOLOX, YOLOXHead  # noqa: E402
from oracle import postproc as P  # noqa: E402


def run(case, dtype):
    c = YS.CASES[case]
    ch = [256, 512, 1024]
    net = YOLOX(YOLOPAFPN(c["depth"], c["width"], in_channels=ch), YOLOXHead(c["num_classes"], c["width"], in_channels=ch))
    sd = YS.state_dict_for(net)
    net.load_state_dict(sd, strict=True)
    net = net.to(dtype).eval()
    x = YS.image(case)
    with torch.no_grad():
        det = net(x.to(dtype))["det_preds"].contiguous()
        net.head.decode_in_inference = False
        raw = net(x.to(dtype)).contiguous()
    manifest = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    return det.numpy().copy(), raw.numpy().copy(), manifest, YS.digest(sd), YS.digest({"x": x})


def iou_matrix(b):
    x1, y1, x2, y2 = b[:, 0], b[:, 1], b[:, 2], b[:, 3]
    area = (x2 - x1) * (y2 - y1)
    iw = np.clip(np.minimum(x2[:, None], x2[None]) - np.maximum(x1[:, None], x1[None]), 0, None)
    ih = np.clip(np.minimum(y2[:, None], y2[None]) - np.maximum(y1[:, None], y1[None]), 0, None)
    inter = iw * ih
    return inter / (area[:, None] + area[None] - inter)


def handoff(d32, d64, nc):
    """(conf_thre, nms_thre) for which fp32 and fp64 keep the same boxes, no score within 8 e_ref of conf_thre and no IoU of two
    same-class candidates within 1e-4 of nms_thre."""
    s32 = d32[..., 4].astype(np.float64) * d32[..., 5:].max(-1)
    s64 = d64[..., 4] * d64[..., 5:].max(-1)
    e_score = float(np.abs(s32 - s64).max())
    for conf in np.quantile(s64, [0.97, 0.975, 0.98, 0.985, 0.99, 0.95, 0.9]):
        conf = float(np.float32(conf))
        score_margin = float(min(np.abs(s32 - conf).min(), np.abs(s64 - conf).min()))
        if score_margin <= 8 * e_score:
            continue
        for nms in (0.45, 0.5, 0.4, 0.55, 0.35):
            margin = np.inf
            for d in (d32.astype(np.float64), d64):
                for i in range(d.shape[0]):
                    s = d[i, :, 4] * d[i, :, 5:].max(-1)
                    keep = s >= conf
                    cand = d[i, keep]
                    cls = cand[:, 5:].argmax(-1)
                    box = np.stack([cand[:, 0] - cand[:, 2] / 2, cand[:, 1] - cand[:, 3] / 2, cand[:, 0] + cand[:, 2] / 2,
                                    cand[:, 1] + cand[:, 3] / 2], 1)
                    iou = iou_matrix(box)
                    same = (cls[:, None] == cls[None]) & ~np.eye(len(cls), dtype=bool)
                    if same.any():
                        margin = min(margin, float(np.abs(iou[same] - nms).min()))
            if margin <= 1e-4:
                continue
            k32 = P.yolox_postprocess(d32, nc, conf, nms)
            k64 = P.yolox_postprocess(d64.astype(np.float32), nc, conf, nms)
            same_kept = all((a is None and b is None) or (a is not None and b is not None and a.shape == b.shape
                                                          and np.array_equal(a[:, 6], b[:, 6])) for a, b in zip(k32, k64))
            n_kept = sum(0 if a is None else len(a) for a in k32)
            if same_kept and n_kept >= 8:
                return conf, nms, e_score, score_margin, float(margin), k32
    raise AssertionError("no (conf_thre, nms_thre) with the required margins")


def main():
    for case, c in YS.CASES.items():
        out = dict(param_seed=np.int64(YS.PARAM_SEED), input_seed=np.int64(YS.INPUT_SEED), distributions=np.array(YS.DISTRIBUTIONS))
        out["conv_shapes"] = np.array(YS.yolox_x_conv_shapes(), np.int32)
        assert len(out["conv_shapes"]) == 26
        d32, r32, manifest, pdig, xdig = run(case, torch.float32)
        d64, r64, _, _, _ = run(case, torch.float64)
        rows = YS.stored_rows(case, d64.shape[1])
        out[f"{case}/rows"] = rows.astype(np.int32)
        out[f"{case}/det64"] = d64[:, rows]
        if d64[:, rows].size * 12 < 900_000:
            out[f"{case}/det32"] = d32[:, rows]
        out[f"{case}/keys"] = np.array([k for k, _ in manifest])
        out[f"{case}/shapes"] = np.array([",".join(map(str, s)) for _, s in manifest])
        out[f"{case}/param_digest"], out[f"{case}/input_digest"] = np.array(pdig), np.array(xdig)
        for g, sl in YS.GROUPS.items():
            e = float(np.abs(d32[..., sl].astype(np.float64) - d64[..., sl]).max())
            out[f"{case}/e_ref_{g}"] = np.float64(e)
            out[f"{case}/range_{g}"] = np.array([d64[..., sl].min(), d64[..., sl].max()])
            out[f"{case}/range_raw_{g}"] = np.array([r64[..., sl].min(), r64[..., sl].max()])
            print(f"{case:9s} {g:3s} e_ref = {e:.3e}  values {d64[..., sl].min():.4g} .. {d64[..., sl].max():.4g}")
        # the seeded values must make the comparison mean something
        logit = lambda p: np.log(p / (1 - p))  # noqa: E731
        for g in ("obj", "cls"):
            lo, hi = out[f"{case}/range_{g}"]
            assert logit(hi) - logit(max(lo, 1e-300)) > 3.0, (case, g, lo, hi)       # pre-sigmoid logits span several (> 3) units
        assert np.abs(out[f"{case}/range_raw_wh"]).max() <= 4.0, out[f"{case}/range_raw_wh"]   # exp neither flattens nor explodes
        assert np.isfinite(d64).all() and np.isfinite(d32).all()
        if not c["rows"]:
            conf, nms, e_score, sm, im, k32 = handoff(d32, d64, c["num_classes"])
            out[f"{case}/conf_thre"], out[f"{case}/nms_thre"] = np.float32(conf), np.float32(nms)
            out[f"{case}/e_ref_score"], out[f"{case}/score_margin"], out[f"{case}/iou_margin"] = np.float64(e_score), np.float64(sm), np.float64(im)
            assert sm > 8 * e_score and im > 1e-4
            out[f"{case}/kept_counts"] = np.array([0 if a is None else len(a) for a in k32], np.int32)
            out[f"{case}/kept32"] = np.concatenate([a for a in k32 if a is not None], 0)
            print(f"{case:9s} hand-off conf_thre {conf:.6f} nms_thre {nms} kept {out[f'{case}/kept_counts']} score margin {sm:.3e} "
                  f"(e_ref_score {e_score:.3e}) iou margin {im:.3e}")
        path = os.path.join(HERE, f"yolox_net_golden_{case}.npz")
        np.savez_compressed(path, **out)
        print("wrote", path, os.path.getsize(path), "bytes")
        assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
