"""Image in, poses out: what the reference's ``predictor_yolo.py:142-171`` + ``predictor_gdrn.py`` give, as one stream of this
library's own launches.

    u8[B,H,W,3] BGR (device)
      -> gdrnpp_yolox_letterbox      (resize + pad, written in the Focus stem's layout)
      -> YOLOX forward               (det/yolox/models/hip_forward.py, csrc/yolox_net.hip)
      -> gdrnpp_yolox_postprocess    (decode, confidence filter, NMS)
      -> gdrnpp_rois_from_dets       (boxes / ratio, selection, the per-ROI table)
      -> read back n_rois and the per-image counts: ONE pinned asynchronous copy and an event — the only host read-back
      -> batch_from_uploaded         (GPU crops from the very images the detector read)
      -> inference_step              (GDRN forward, pose, refine, records)

There is no CPU fallback: with the HIP layers disabled, or a detector / input size outside ``hip_forward.supported_size``, the
predictor raises."""
from __future__ import annotations

import torch

from .. import hip_lib
from ..det.yolox.models import hip_forward
from . import hip_layers
from .roi_stream import batch_from_uploaded
from .streams import inference_step


class YoloGdrnPredictor:
    def __init__(self, yolox, gdrn_model, post, cfg, *, test_size=(640, 640), num_classes: int, conf_thr: float, nms_thr: float,
                 class_agnostic: bool = False, cam, extents, top_k_per_obj: int = 0, score_thr: float = 0.0, max_det: int = 64,
                 roi_cap: int = 256):
        self.yolox, self.model, self.post, self.cfg = yolox, gdrn_model, post, cfg
        self.test_size = (int(test_size[0]), int(test_size[1]))
        self.num_classes, self.conf_thr, self.nms_thr, self.class_agnostic = int(num_classes), float(conf_thr), float(nms_thr), bool(class_agnostic)
        self.top_k_per_obj, self.score_thr, self.max_det, self.roi_cap = int(top_k_per_obj), float(score_thr), int(max_det), int(roi_cap)
        if yolox.head.num_classes != self.num_classes:
            raise ValueError(f"YoloGdrnPredictor: the detector has {yolox.head.num_classes} classes, num_classes={self.num_classes}")
        if self.max_det < 1 or self.roi_cap < 1 or self.top_k_per_obj < 0:
            raise ValueError("YoloGdrnPredictor: max_det and roi_cap must be positive, top_k_per_obj >= 0")
        dev = next(yolox.parameters()).device
        self.device = dev
        self.cam = torch.as_tensor(cam, dtype=torch.float32).to(dev).contiguous()              # [3,3] or [B,3,3] (per image)
        self.extents = torch.as_tensor(extents, dtype=torch.float32).to(dev).contiguous()      # [C,3]
        if self.extents.shape != (self.num_classes, 3):
            raise ValueError(f"YoloGdrnPredictor: extents must be [{self.num_classes},3], got {tuple(self.extents.shape)}")
        self._counts_host = None               # pinned i32[1 + B]

    @staticmethod
    def sizes(H: int, W: int, test_size) -> tuple:
        """(r, rh, rw) of the reference's ``preproc`` for an H x W image: Python floats, ``int()`` of the products."""
        return hip_lib.letterbox_sizes(H, W, test_size)

    def _require_hip(self, images_u8) -> None:
        if not isinstance(images_u8, torch.Tensor) or not images_u8.is_cuda or images_u8.dtype != torch.uint8 or images_u8.dim() != 4 \
                or images_u8.shape[-1] != 3:
            raise RuntimeError("YoloGdrnPredictor: images must be a u8[B,H,W,3] BGR tensor on the device")
        if not hip_layers.is_enabled():
            raise RuntimeError("YoloGdrnPredictor: the HIP layers are disabled and the predictor has no CPU / operator fallback")
        if self.yolox.training or not hip_forward.supported_size(self.yolox, *self.test_size):
            raise RuntimeError(f"YoloGdrnPredictor: detector / test_size {self.test_size} outside the HIP forward "
                               "(eval mode, three levels, sizes multiples of 32); there is no fallback")

    @torch.no_grad()
    def detect(self, images_u8):
        """u8[B,H,W,3] -> (dets f32[B,max_det,7], count i32[B], ratio): boxes in LETTERBOX pixels, as ``yolox_postprocess`` gives them."""
        self._require_hip(images_u8)
        images_u8 = images_u8.contiguous()
        b = images_u8.shape[0]
        ht, wt = self.test_size
        foc = hip_forward.focus_buffer(self.yolox, b, ht, wt, images_u8.device)
        _, ratio = hip_lib.yolox_letterbox(images_u8, self.test_size, out=foc, focus=True)
        out = hip_forward.forward(self.yolox, None, focus=foc)
        det = out["det_preds"] if isinstance(out, dict) else out
        dets, count = hip_lib.yolox_postprocess(det, self.num_classes, self.conf_thr, self.nms_thr, self.class_agnostic, self.max_det)
        return dets, count, ratio

    @torch.no_grad()
    def rois(self, images_u8):
        """detect + ``rois_from_dets`` + the one read-back: -> (table views sliced to n_rois, per-image counts as a list)."""
        dets, count, ratio = self.detect(images_u8)
        b, H, W, _ = images_u8.shape
        if self.cam.dim() == 3 and self.cam.shape[0] != b:
            raise RuntimeError(f"YoloGdrnPredictor: cam holds {self.cam.shape[0]} matrices for {b} images")
        table, counts = hip_lib.rois_from_dets(
            dets, count, ratio, H, W, self.cam, self.extents, self.cfg.INPUT.DZI_PAD_SCALE, self.cfg.MODEL.POSE_NET.OUTPUT_RES,
            self.score_thr, self.top_k_per_obj, self.roi_cap)
        if self._counts_host is None or self._counts_host.numel() != 1 + b:
            self._counts_host = torch.empty((1 + b,), dtype=torch.int32, pin_memory=True)
        self._counts_host.copy_(counts, non_blocking=True)
        done = torch.cuda.Event()
        done.record()
        done.synchronize()
        host = self._counts_host.tolist()
        n = host[0]
        return {k: v[:n] for k, v in table.items()}, host[1:]

    @torch.no_grad()
    def __call__(self, images_u8, depths=None):
        """u8[B,H,W,3] BGR (device), depths f32[B,H,W] or None -> (records f32[n,16] on the device, per-image ROI counts); the
        ``roi_id`` column is the ROI's position in the stream (image order, then the selection's order)."""
        up, per_image = self.rois(images_u8)
        if up["scale"].shape[0] == 0:
            return torch.zeros((0, 16), dtype=torch.float32, device=images_u8.device), per_image
        batch = batch_from_uploaded(self.cfg, images_u8.contiguous(), depths, up)
        return inference_step(self.model, self.post, batch), per_image
