"""Host-side ROI preparation (detections -> the batch a step consumes, through one packed upload) and the scheduler that
turns a stream of images into steps of the size the kernels want."""
from __future__ import annotations

from typing import TYPE_CHECKING

import torch

from .. import hip_lib
from . import hip_layers
from .records import sort_detections_by_class
from .streams import (GraphedInference, StepStreams, _step_closure, default_compute_streams, default_graph_streams,
                      inference_step_async)

if TYPE_CHECKING:      # annotations only (they are never evaluated): no import at run time
    from .post import GdrnHipPost


# --------------------------------------------------------------------------------------------------
# ROI preparation on the device (rows a1 + a2): detections -> ROI tensors, no CPU crop, no H2D of crops
# --------------------------------------------------------------------------------------------------
def rois_from_detections(bboxes_xyxy, im_H: int, im_W: int, dzi_pad_scale: float = 1.5, out_res: int = 64):
    """Per-detection ROI parameters exactly as read_data_test derives them (data_loader.py:754-769), float64 like
    the reference's NumPy/Python scalars: centre, (bw, bh) clamped to >= 1, scale = min(max(bw,bh)*DZI_PAD_SCALE,
    max(im_H, im_W)), resize_ratio = out_res / scale."""
    import numpy as np

    bb = np.asarray(bboxes_xyxy, np.float64).reshape(-1, 4)
    x1, y1, x2, y2 = bb[:, 0], bb[:, 1], bb[:, 2], bb[:, 3]
    center = np.stack([0.5 * (x1 + x2), 0.5 * (y1 + y2)], 1)
    bw = np.maximum(x2 - x1, 1)
    bh = np.maximum(y2 - y1, 1)
    scale = np.minimum(np.maximum(bh, bw) * dzi_pad_scale, max(im_H, im_W)) * 1.0
    return dict(bbox_center=center, scale=scale, roi_wh=np.stack([bw, bh], 1).astype(np.float32),
                resize_ratio=(out_res / scale))


def detections_from_yolox(dets: torch.Tensor, count: torch.Tensor, cam, extents, ratio: float = 1.0, max_per_image: int = 0) -> dict:
    """Hand-off from the detector to the pose path without the JSON file of the reference (dataset_utils.py:146-239):
    ``hip_lib.yolox_postprocess`` output (dets f32[B,max_det,7], count i32[B]) -> the ``detections`` dict of
    ``batch_data_test_gpu``.  Boxes are divided by ``ratio`` (YOLOX's test-time resize, predictor_yolo.py:170-176), the
    score is obj_conf * class_conf and the class column becomes ``roi_cls``; rows keep NMS order within an image."""
    import numpy as np

    counts = count.tolist()
    rows, im_idx = [], []
    for i, n in enumerate(counts):
        n = min(n, dets.shape[1], max_per_image or n)
        if n > 0:
            rows.append(dets[i, :n])
            im_idx += [i] * n
    if not rows:
        return dict(bbox=np.zeros((0, 4), np.float32), im_idx=np.zeros((0,), np.int64), roi_cls=np.zeros((0,), np.int64),
                    score=np.zeros((0,), np.float32), cam=cam, extents=extents)
    d = torch.cat(rows, 0).cpu().numpy()
    return dict(bbox=d[:, :4] / np.float32(ratio), im_idx=np.asarray(im_idx, np.int64), roi_cls=d[:, 6].astype(np.int64),
                score=d[:, 4] * d[:, 5], cam=cam, extents=extents)


def detections_from_bop_json(detections: dict, scene_im_ids, obj_ids, cam, extents, top_k_per_obj: int = 1,
                             score_thr: float = 0.0, train_obj_ids=None) -> dict:
    """The offline hand-off of the reference: a BOP detection file ``{scene_im_id: [{"obj_id", "bbox_est": [x, y, w, h],
    "score", "time"}]}`` -> the ``detections`` dict of ``batch_data_test_gpu``, with the selection rules of
    ``load_detections_into_dataset`` (core/utils/dataset_utils.py:146-227): drop score < score_thr and objects the model
    was not trained on, keep the ``top_k_per_obj`` highest scores per object (stable for ties), objects in the dataset's
    class order, images without detections skipped.  ``scene_im_ids[i]`` names image ``i`` of the batch; ``obj_ids`` is
    the dataset's object-id list in class order.  Also returns ``time`` (detector time per ROI) for the BOP results."""
    import numpy as np

    obj_ids = [int(o) for o in obj_ids]
    keep = set(obj_ids if train_obj_ids is None else [int(o) for o in train_obj_ids])
    bbox, im_idx, cls, score, times = [], [], [], [], []
    for i, key in enumerate(scene_im_ids):
        per_obj = {o: [] for o in obj_ids}
        for det in detections.get(key, []):
            o, sc = int(det["obj_id"]), float(det.get("score", 1.0))
            if sc < score_thr or o not in per_obj or o not in keep:
                continue
            per_obj[o].append((sc, det))
        for o in obj_ids:
            for sc, det in sorted(per_obj[o], key=lambda pair: pair[0], reverse=True)[:top_k_per_obj]:
                x, y, w, h = [float(v) for v in det["bbox_est"]]
                bbox.append([x, y, x + w, y + h])           # BoxMode.XYWH_ABS -> XYXY_ABS
                im_idx.append(i)
                cls.append(obj_ids.index(o))
                score.append(sc)
                times.append(float(det.get("time", 0.0)))
    return dict(bbox=np.asarray(bbox, np.float32).reshape(-1, 4), im_idx=np.asarray(im_idx, np.int64),
                roi_cls=np.asarray(cls, np.int64), score=np.asarray(score, np.float32), cam=cam, extents=extents,
                time=np.asarray(times, np.float32))


def packed_layout(arrays: dict):
    """Byte layout of ``upload_packed``'s staging buffer: -> ({key: (offset, nbytes, numpy dtype, shape)}, total bytes); every
    array starts on a 16-byte boundary, dict order."""
    import numpy as np

    lay, total = {}, 0
    for k, a in arrays.items():
        a = np.asarray(a)
        total = (total + 15) & ~15
        lay[k] = (total, a.nbytes, a.dtype, a.shape)
        total += a.nbytes
    return lay, max(total, 16)


def fill_packed(host_u8, arrays: dict, layout: dict) -> None:
    """Write ``arrays`` into a staging buffer (a uint8 NumPy view) laid out by ``packed_layout``."""
    import numpy as np

    for k, (off, nbytes, dt, shape) in layout.items():
        a = np.ascontiguousarray(arrays[k], dtype=dt)
        if a.shape != tuple(shape):
            raise ValueError(f"fill_packed: {k!r} has shape {a.shape}, the layout holds {tuple(shape)}")
        if nbytes:
            host_u8[off:off + nbytes] = a.reshape(-1).view(np.uint8)


def packed_views(dev_u8: torch.Tensor, layout: dict) -> dict:
    """Typed tensor views of a device copy of the staging buffer."""
    import numpy as np

    out = {}
    for k, (off, nbytes, dt, shape) in layout.items():
        tdt = torch.from_numpy(np.empty((0,), dt)).dtype
        out[k] = dev_u8[off:off + nbytes].view(tdt).reshape(tuple(shape))
    return out


def upload_packed(arrays: dict, dev) -> dict:
    """The small per-ROI host arrays of a step -> device tensors through ONE pinned staging buffer and ONE asynchronous copy on the
    current stream.  A ``torch.from_numpy(a).to(dev)`` per array is a blocking pageable copy queued behind everything already on
    the stream: the host would sit out the step that is still running there before it could prepare the next one."""
    dev = torch.device(dev)
    layout, total = packed_layout(arrays)
    host = torch.empty((total,), dtype=torch.uint8, pin_memory=dev.type == "cuda")
    fill_packed(host.numpy(), arrays, layout)
    return packed_views(host.to(dev, non_blocking=True), layout)


def roi_host_arrays(cfg, detections: dict, H: int, W: int, sort_by_class: bool = False, roi_id_base: int = 0, extra_per_roi_keys=(),
                    extra_global_keys=()) -> dict:
    """The HOST half of ``batch_data_test_gpu``: detections -> the per-ROI NumPy arrays of a step (ROI parameters exactly as
    read_data_test derives them, data_loader.py:754-769; class sort; ids), in the order ``upload_packed`` lays them out."""
    import numpy as np

    roi_id = None
    if sort_by_class:
        detections, roi_id = sort_detections_by_class(detections, roi_id_base, extra_per_roi_keys, extra_global_keys)
    if "roi_id" in detections:        # the caller's own ids (RoiStreamScheduler: global stream ids), permuted with the rest
        roi_id = np.asarray(detections["roi_id"], np.int32)
    r = rois_from_detections(detections["bbox"], H, W, cfg.INPUT.DZI_PAD_SCALE, cfg.MODEL.POSE_NET.OUTPUT_RES)
    n = len(r["scale"])
    cls = np.asarray(detections["roi_cls"], np.int64)
    cam = np.asarray(detections["cam"], np.float32)
    cam = np.repeat(cam[None], n, 0) if cam.ndim == 2 else cam
    host = dict(center64=r["bbox_center"], scale64=r["scale"], im_idx=np.asarray(detections["im_idx"], np.int32), roi_cls=cls, roi_cam=cam,
                roi_center=np.asarray(r["bbox_center"], np.float32), roi_wh=r["roi_wh"], scale=np.asarray(r["scale"], np.float32),
                resize_ratio=np.asarray(r["resize_ratio"], np.float32), roi_extent=np.asarray(detections["extents"], np.float32)[cls],
                score=np.asarray(detections.get("score", np.ones(n)), np.float32))
    if roi_id is not None:
        host["roi_id"] = np.asarray(roi_id, np.int32)
    return host


def batch_from_uploaded(cfg, images: torch.Tensor, depths, up: dict, dev=None) -> dict:
    """The DEVICE half: the uploaded per-ROI arrays (``upload_packed`` / ``packed_views`` of ``roi_host_arrays``) + the images ->
    GPU crops (``gdrnpp_crop_resize_roi``) and the batch dict ``GDRN_Net.forward`` / ``GdrnHipPost`` consume.  Launches and tensor
    views only — no host data: this half can be captured into a hipGraph (``RoiStreamScheduler(graph_steps=True)``)."""
    dev = dev or images.device
    net_cfg = cfg.MODEL.POSE_NET
    n_im, H, W, _ = images.shape
    n = up["scale"].shape[0]
    centers64, scales64 = up["center64"], up["scale64"]
    roi_img, roi_depth, roi_c2d = hip_lib.crop_resize_roi(
        images, depths, up["im_idx"], centers64, scales64,
        out_res=net_cfg.INPUT_RES, out_res_small=net_cfg.OUTPUT_RES, pixel_mean=cfg.MODEL.PIXEL_MEAN,
        pixel_std=cfg.MODEL.PIXEL_STD)
    batch = dict(
        roi_img=roi_img, roi_coord_2d=roi_c2d, roi_cls=up["roi_cls"], roi_cam=up["roi_cam"], roi_center=up["roi_center"],
        roi_wh=up["roi_wh"], scale=up["scale"], resize_ratio=up["resize_ratio"], roi_extent=up["roi_extent"], score=up["score"],
        im_H=torch.full((n,), float(H), device=dev), im_W=torch.full((n,), float(W), device=dev))
    if roi_depth is not None:
        batch["roi_depth"] = roi_depth
    if "roi_id" in up:
        batch["roi_id"] = up["roi_id"]
    if net_cfg.PNP_NET.COORD_2D_TYPE == "rel":
        # data_loader.py:799-804: (bbox_center - roi_coord_2d * (im_W, im_H)) / scale, float64 like NumPy, stored float32
        hip_layers.note_foreign_launch("batch_data_test_gpu: COORD_2D_TYPE='rel' computed with torch operators")
        wh = torch.tensor([float(W), float(H)], dtype=torch.float64, device=dev).view(1, 2, 1, 1)
        batch["roi_coord_2d_rel"] = ((centers64.view(n, 2, 1, 1) - roi_c2d.double() * wh) / scales64.view(n, 1, 1, 1)).float()
    return batch


def batch_data_test_gpu(cfg, images: torch.Tensor, depths, detections: dict, device=None, sort_by_class: bool = False,
                        roi_id_base: int = 0, extra_per_roi_keys=(), extra_global_keys=()) -> dict:
    """``read_data_test`` + ``batch_data_test`` (data_loader.py:647-818, engine_utils.py:213-241) with the crops made
    on the GPU.  images u8[n_im,H,W,3] (BGR, device), depths f32[n_im,H,W] or None, detections:
    {"bbox": [n,4] xyxy, "im_idx": [n], "roi_cls": [n], "score": [n], "cam": [n,3,3] or [3,3], "extents": [C,3]}.
    Returns the batch dict ``GDRN_Net.forward`` / ``GdrnHipPost`` consume (all tensors on the device).
    ``sort_by_class``: ROIs are laid out in class order and ``batch["roi_id"]`` = ``roi_id_base`` + the
    detection's original position (or the caller's ``detections["roi_id"]``), which ``inference_step`` writes into the records
    (``records_in_roi_order`` restores it).  = ``roi_host_arrays`` -> ``upload_packed`` (one pinned buffer, one asynchronous copy:
    the host never waits for the stream) -> ``batch_from_uploaded``."""
    dev = device or images.device
    n_im, H, W, _ = images.shape
    host = roi_host_arrays(cfg, detections, H, W, sort_by_class, roi_id_base, extra_per_roi_keys, extra_global_keys)
    return batch_from_uploaded(cfg, images, depths, upload_packed(host, dev), dev)


# --------------------------------------------------------------------------------------------------
# ROI packing: the reference's image loop (one image per forward, gdrn_evaluator.py:702, data_loader.py:901 batch_size=1)
# feeds the network 3-30 ROIs at a time; the kernels of this library reach their rate from ~128 ROIs per step on.  The packer
# sits between the two: ROIs of consecutive images are dealt into steps of EXACTLY ``rois_per_step`` (an image's ROIs may
# straddle two steps), every ROI carries a stream-wide id into its record, and records are dealt back to their images.
# --------------------------------------------------------------------------------------------------
class RoiPacker:
    """Host-side bookkeeping of the packing (no device, no tensors): which ROI of which image goes into which step, and which
    images are complete once a step's records are back.  ROI ids wrap at 2^24 (they travel as float32 in the records)."""

    ID_WRAP = 1 << 24

    def __init__(self, rois_per_step: int, roi_id_base: int = 0):
        import collections

        if rois_per_step < 1:
            raise ValueError("rois_per_step must be positive")
        self.rois_per_step = int(rois_per_step)
        self._queue = collections.deque()      # [key, n, next local index] of images with ROIs not yet dealt into a step
        self._pending = 0
        self._next_id = int(roi_id_base) % self.ID_WRAP
        self._where = {}                       # roi id -> (key, local index) of ROIs dealt into a step whose records are not back
        self._open = {}                        # key -> [n, records f32[n,16], number still missing]
        self._done = []

    def add_image(self, key, n_rois: int) -> None:
        import numpy as np

        if key in self._open:
            raise KeyError(f"image key {key!r} is already in flight")
        n = int(n_rois)
        if n == 0:
            self._done.append((key, np.zeros((0, 16), np.float32)))      # the reference skips images without detections
            return
        self._open[key] = [n, np.full((n, 16), np.nan, np.float32), n]
        self._queue.append([key, n, 0])
        self._pending += n

    @property
    def pending(self) -> int:
        return self._pending

    def ready(self) -> bool:
        return self._pending >= self.rois_per_step

    def next_pack(self, flush: bool = False):
        """-> [(key, local indices i64[k], roi ids i32[k]), ...] covering exactly ``rois_per_step`` ROIs in arrival order (fewer
        only with ``flush`` = the tail of the stream), or None when there is nothing to launch yet."""
        import numpy as np

        if self._pending == 0 or (not flush and not self.ready()):
            return None
        want = min(self.rois_per_step, self._pending)
        pack = []
        while want > 0:
            ent = self._queue[0]
            key, n, nxt = ent
            k = min(want, n - nxt)
            local = np.arange(nxt, nxt + k, dtype=np.int64)
            ids = ((self._next_id + np.arange(k, dtype=np.int64)) % self.ID_WRAP).astype(np.int32)
            for j, i in zip(local.tolist(), ids.tolist()):
                self._where[i] = (key, j)
            self._next_id = (self._next_id + k) % self.ID_WRAP
            pack.append((key, local, ids))
            ent[2] += k
            if ent[2] == n:
                self._queue.popleft()
            want -= k
            self._pending -= k
        return pack

    def last_roi_dealt(self, key) -> bool:
        """True once every ROI of image ``key`` has been dealt into a step (its pixels are no longer needed)."""
        return all(e[0] != key for e in self._queue)

    def deliver(self, records) -> None:
        """Records f32[m,16] of one step (any order) -> their images.  A record is delivered when its id is one this packer dealt
        and is still waiting for — whatever its ``valid`` column says: the refine kernel marks a ROI whose object id lies outside
        the mesh set invalid, and that ROI's image must still complete (the row keeps valid = 0 for the consumer; a record that
        is zero in every column is still the record of ROI id 0).  The only rows skipped are ``gather_records``' padding
        (roi_id = PAD_ROI_ID < 0: marked, not guessed) and ids that are not in flight."""
        import numpy as np

        rec = np.asarray(records, np.float32).reshape(-1, 16)
        for r in rec:
            if not r[14] >= 0:                   # padding (or a NaN id): never a ROI of this stream
                continue
            rid = int(r[14])
            if rid not in self._where:
                continue
            key, j = self._where.pop(rid)
            ent = self._open[key]
            ent[1][j] = r
            ent[2] -= 1
            if ent[2] == 0:
                self._done.append((key, ent[1]))
                del self._open[key]

    def pop_completed(self):
        """-> [(key, records f32[n,16] in the image's own detection order), ...] of the images completed since the last call."""
        done, self._done = self._done, []
        return done


def h2d_overlap(copies, steps, detail: bool = False) -> dict:
    """Device timeline of host-to-device copies against compute: ``copies`` = (start, end) timing events on copy streams,
    ``steps`` = (start, end) timing events around the steps' kernels on the compute stream (of one or several schedulers feeding
    the same device); one clock (elapsed time from the first copy's start).  -> h2d_ms (summed copy durations), overlapped_ms
    (the part of them during which some step's kernels were executing) and overlapped_frac = overlapped_ms / h2d_ms."""
    torch.cuda.synchronize()
    out = {"h2d_ms": sum(a.elapsed_time(b) for a, b in copies), "overlapped_ms": 0.0, "overlapped_frac": None,
           "images": len(copies), "steps": len(steps)}
    if copies and steps:
        origin = copies[0][0]
        busy, merged = sorted((origin.elapsed_time(a), origin.elapsed_time(b)) for a, b in steps), []
        for s0, s1 in busy:                      # union of the step intervals
            if merged and s0 <= merged[-1][1]:
                merged[-1][1] = max(merged[-1][1], s1)
            else:
                merged.append([s0, s1])
        for a, b in copies:
            c0, c1 = origin.elapsed_time(a), origin.elapsed_time(b)
            for s0, s1 in merged:
                lo, hi = max(c0, s0), min(c1, s1)
                if hi > lo:
                    out["overlapped_ms"] += hi - lo
        if out["h2d_ms"] > 0:
            out["overlapped_frac"] = min(1.0, out["overlapped_ms"] / out["h2d_ms"])
        if detail:
            out["steps_ms"] = busy
            out["copies_ms"] = [(origin.elapsed_time(a), origin.elapsed_time(b)) for a, b in copies]
    return out


class RoiStreamScheduler:
    """detections -> pose records for a STREAM of images, at the step size the kernels want.

        push(key, image u8[H,W,3] (device, BGR), depth f32[H,W] | None, detections)      one image and its detections
          -> the packer deals ROIs into steps of exactly ``rois_per_step``; every full step is launched at once:
             GPU crop (gdrnpp_crop_resize_roi, ROIs class-sorted within the step) -> inference_step_async
          -> steps are resolved one launch late (the range check of the three-product kernels and the 8 KB record copy never
             stall the device), their records dealt back to the images
          -> returns the images that became complete: [(key, records f32[n,16] in detection order, seconds since push)]
        flush()  launches the tail (a short step) and returns everything still open.

    ``detections`` = the dict of ``batch_data_test_gpu`` for ONE image (bbox [n,4] xyxy, roi_cls [n], score [n], cam [3,3],
    extents [C,3]).  All images of a stream share H x W (a BOP dataset's resolution).

    Host-fed streams (the reference's loader hands over HOST arrays, data_loader.py:754-797, and ``batch_data_test`` moves the
    ROI crops to the device, engine_utils.py:213-241): ``image`` / ``depth`` may be CPU tensors — pinned, or the copy is not
    asynchronous.  They are copied to the device on the scheduler's own copy stream the moment they are admitted (the FULL
    image once, 0.9 + 1.2 MB, not a 1 MB crop per ROI), an event per image orders the step's crop kernel behind its copies, and
    since admission runs one step ahead of the device the copies overlap the previous step's kernels.  ``time_h2d=True``
    brackets every image's copies with timing events (``h2d_ms()``).

    ``graph_steps``: every FULL step replays a captured hipGraph of (GPU crop -> forward -> post-processing) instead of ~150 eager
    launches — for small ``rois_per_step`` (the reference's own regime: a few ROIs at a time, low latency), where the host's launches
    bound the eager schedule; the graphs sit in 2 x streams slots with static image / per-ROI buffers, ``default_graph_streams``
    (4) steps in flight; records bit-equal to the eager scheduler with the same kernel rule; the tail step of ``flush`` runs eagerly.

    ``compute_streams`` (default: ``default_compute_streams(model)`` = 2 for the ConvNeXt configurations, whose every kernel is
    this library's): consecutive steps are launched on alternating HIP streams (``StepStreams``), so that with
    ``max_in_flight`` >= 2 two steps really are in flight on the device — one step's narrow tail under the next one's GEMMs —
    instead of queued behind each other; 1 = everything on the caller's current stream (rounds 1-4); a ``StepStreams`` object =
    that dealer, shared by several schedulers of one device (bench.py's seven-dataset stream)."""

    def __init__(self, cfg, model, post: GdrnHipPost, rois_per_step: int = 128, max_in_flight: int = 2, roi_id_base: int = 0,
                 device=None, time_h2d: bool = False, compute_streams=None, graph_steps: bool = False):
        import collections

        self.device = device
        self.graph_steps = bool(graph_steps)    # full steps replay a captured hipGraph (crop + forward + post): small rois_per_step
        self._slots = []                        # graph slots: static inputs + GraphedInference, bound to a compute stream each
        if compute_streams is None:
            compute_streams = default_graph_streams(model) if graph_steps else default_compute_streams(model)
        if isinstance(compute_streams, StepStreams):     # shared with other schedulers feeding the same device
            self._n_compute, self._dealer = len(compute_streams.streams), compute_streams
        else:
            self._n_compute = max(1, int(compute_streams))
            self._dealer = None                 # StepStreams, made at the first launch (the device is known then)
        self._copy_stream = None
        self._h2d_ready = {}                    # key -> event: the image's pixels are on the device
        self._time_h2d = bool(time_h2d)
        self._h2d_timing = []                   # (start, end) events per image, copy stream
        self._step_timing = []                  # (start, end) events per step, compute stream (time_h2d only)
        self.h2d_bytes = 0

        self.cfg, self.model, self.post = cfg, model, post
        self.packer = RoiPacker(rois_per_step, roi_id_base)
        self.max_in_flight = max(1, int(max_in_flight))
        if self.graph_steps:                    # a graph replay costs the host ~0.1 ms: as many steps in flight as there are streams
            self.max_in_flight = max(self.max_in_flight, self._n_compute)
        self._images = {}                       # key -> (image, depth, detections, arrival time)
        self._arrival = {}
        self._in_flight = collections.deque()   # (StepHandle, batch, done event) — the batch stays alive for a six-product repeat
        self._with_depth = None                 # fixed by the first image that has ROIs
        self._d2h_stream = None                 # side stream of the 8 KB record copies
        self.latencies = collections.deque(maxlen=1 << 16)   # seconds from push to completed records, per image (newest 65 536)
        self.steps_launched = 0

    # -- one step ----------------------------------------------------------------------------------
    def _launch(self, pack) -> None:
        import numpy as np

        def per_roi(key, loc, name, dtype, default=None):
            d = self._images[key][2]
            a = np.asarray(d[name] if name in d else default(len(d["roi_cls"])), dtype)
            return a.reshape((len(d["roi_cls"]),) + a.shape[1:])[loc]

        def cams(key, loc):
            c = np.asarray(self._images[key][2]["cam"], np.float32)
            return np.broadcast_to(c, (len(loc), 3, 3)) if c.ndim == 2 else c[loc]

        keys = [k for k, _, _ in pack]
        if self._dealer is None:
            dev = self.device if self.device is not None else self._images[keys[0]][0].device
            self._dealer = StepStreams(self._n_compute, dev)
        caller = torch.cuda.current_stream(self._dealer.device)
        n_rois = sum(len(loc) for _, loc, _ in pack)
        if self.graph_steps and n_rois == self.packer.rois_per_step:
            n_slots = 2 * self._n_compute       # twice the streams: consecutive steps alternate streams, a slot is reused only after
            k = self.steps_launched % n_slots   # max_in_flight (<= streams) younger steps were launched, i.e. after it was resolved
            with self._dealer.on(k):
                self._launch_graph_step(k, pack, keys, per_roi, cams, caller)
        else:                                   # eager (the default; in graph mode: the short tail step of flush())
            with self._dealer.next():           # this step's crop, forward and post-processing: the next compute stream
                self._launch_on_current_stream(pack, keys, per_roi, cams, caller)
        for k in keys:                          # pixels are only read by the crop kernel just enqueued
            if self.packer.last_roi_dealt(k):
                del self._images[k]
                self._h2d_ready.pop(k, None)

    def _step_detections(self, pack, keys, per_roi, cams) -> dict:
        import numpy as np

        return dict(
            bbox=np.concatenate([per_roi(k, loc, "bbox", np.float32) for k, loc, _ in pack]),
            roi_cls=np.concatenate([per_roi(k, loc, "roi_cls", np.int64) for k, loc, _ in pack]),
            score=np.concatenate([per_roi(k, loc, "score", np.float32, np.ones) for k, loc, _ in pack]),
            im_idx=np.concatenate([np.full(len(loc), i, np.int64) for i, (_, loc, _) in enumerate(pack)]),
            roi_id=np.concatenate([ids for _, _, ids in pack]),
            cam=np.concatenate([cams(k, loc) for k, loc, _ in pack]),
            extents=self._images[keys[0]][2]["extents"])

    def _launch_graph_step(self, k, pack, keys, per_roi, cams, caller) -> None:
        """A full step as a hipGraph replay: the step's images are copied into the slot's static image block, its per-ROI arrays
        through the slot's pinned buffer into the slot's packed device buffer (one asynchronous copy), then the slot's graph —
        GPU crop, forward, post-processing, records — is replayed on the slot's stream.  The first use of a slot captures it."""
        dev = self._dealer.device
        cur = torch.cuda.current_stream(dev)
        if cur != caller:
            cur.wait_stream(caller)
        for key in keys:
            ev = self._h2d_ready.get(key)
            if ev is not None:
                cur.wait_event(ev)
        im0, dp0 = self._images[keys[0]][0], self._images[keys[0]][1]
        H, W = int(im0.shape[0]), int(im0.shape[1])
        det = self._step_detections(pack, keys, per_roi, cams)
        host = roi_host_arrays(self.cfg, det, H, W, sort_by_class=True)
        while len(self._slots) <= k:
            self._slots.append(None)
        slot = self._slots[k]
        if slot is None:
            P = self.packer.rois_per_step       # a step of P ROIs touches at most P images
            layout, total = packed_layout(host)
            slot = dict(images=torch.zeros((P, H, W, 3), dtype=torch.uint8, device=dev),
                        depths=torch.zeros((P, H, W), dtype=torch.float32, device=dev) if self._with_depth else None,
                        packed=torch.zeros((total,), dtype=torch.uint8, device=dev),
                        pinned=torch.zeros((total,), dtype=torch.uint8, pin_memory=True), layout=layout, graph=None)
            self._slots[k] = slot
        if slot["graph"] is not None and slot["graph"]._pending is not None:
            slot["graph"]._pending.result()     # (cannot happen with max_in_flight <= streams; the pinned buffer must be free)
        for i, key in enumerate(keys):          # device-to-device copies on the slot's stream (the images were produced / copied elsewhere)
            im, dp = self._images[key][0], self._images[key][1]
            im.record_stream(cur)
            slot["images"][i].copy_(im, non_blocking=True)
            if slot["depths"] is not None:
                dp.record_stream(cur)
                slot["depths"][i].copy_(dp, non_blocking=True)
        fill_packed(slot["pinned"].numpy(), host, slot["layout"])
        slot["packed"].copy_(slot["pinned"], non_blocking=True)
        if self._time_h2d:
            t0 = torch.cuda.Event(enable_timing=True)
            t0.record()
        if slot["graph"] is None:
            cfg, model, post = self.cfg, self.model, self.post

            def body(static):
                up = packed_views(static["packed"], slot["layout"])
                batch = batch_from_uploaded(cfg, static["images"], static["depths"], up, dev)
                return _step_closure(model, post, batch, batch["roi_id"])()

            multi = len(self._dealer.streams) > 1
            rule, rows = ((self._dealer.shared_min_tiles(), self._dealer.shared_min_rows()) if multi and hip_lib.shared_min_tiles() == 0
                          else (None, None))
            slot["graph"] = GraphedInference(model, post, dict(images=slot["images"], depths=slot["depths"], packed=slot["packed"]), None,
                                             warmup=2, stream=cur, shared_min_tiles=rule, shared_min_rows=rows,
                                             sharing=self._dealer.sharing(), body=body)
        handle = slot["graph"].replay_async()
        done = torch.cuda.Event()
        done.record()
        self._in_flight.append((handle, None, done))
        if self._time_h2d:
            t1 = torch.cuda.Event(enable_timing=True)
            t1.record()
            self._step_timing.append((t0, t1))
        self.steps_launched += 1

    def _launch_on_current_stream(self, pack, keys, per_roi, cams, caller) -> None:
        import numpy as np

        cur = torch.cuda.current_stream(self._dealer.device)
        if cur != caller:
            cur.wait_stream(caller)             # device images handed over by the caller were produced on ITS stream
        for k in keys:                          # host-fed images: the crop kernel waits for their copies (device-side wait)
            ev = self._h2d_ready.get(k)
            if ev is not None:
                cur.wait_event(ev)
        for k in keys:                          # allocated on the caller's / the copy stream, read by this stream's crop kernel:
            for t in self._images[k][:2]:       # their memory must not be handed out again before that kernel has run
                if isinstance(t, torch.Tensor) and t.is_cuda:
                    t.record_stream(cur)
        images = torch.stack([self._images[k][0] for k in keys])
        depths = torch.stack([self._images[k][1] for k in keys]) if self._with_depth else None
        det = self._step_detections(pack, keys, per_roi, cams)
        if self._time_h2d:
            t0 = torch.cuda.Event(enable_timing=True)
            t0.record()
        batch = batch_data_test_gpu(self.cfg, images, depths, det, sort_by_class=True)
        handle = inference_step_async(self.model, self.post, batch)
        done = torch.cuda.Event()               # everything of this step, on the compute stream
        done.record()
        self._in_flight.append((handle, batch, done))
        if self._time_h2d:
            t1 = torch.cuda.Event(enable_timing=True)
            t1.record()
            self._step_timing.append((t0, t1))
        self.steps_launched += 1

    def _resolve_oldest(self):
        """Records of the OLDEST step in flight -> their images.  The 8 KB device-to-host copy runs on a side stream behind that
        step's own event: a ``rec.cpu()`` on the compute stream would queue behind the NEWER steps already launched there and
        stall the host until they finish — no step would ever be prepared while another runs (measured: every image copy of a
        host-fed stream landed in the idle gap between two steps, profiles/r05d_h2d_timeline_before_fix.txt)."""
        handle, _batch, done = self._in_flight.popleft()
        rec = handle.result()                   # waits for that step's range-word event only (and repeats a flagged step)
        if rec.is_cuda:
            if self._d2h_stream is None:
                # high priority = the other hardware-queue pool: a default-priority stream may share a queue with a compute stream, and
                # a record copy queued there behind the NEWEST step's kernels would hold the host until that step is done
                self._d2h_stream = torch.cuda.Stream(device=rec.device, priority=-1)
            compute = handle.stream if handle.stream is not None else torch.cuda.current_stream(rec.device)   # the step's own stream (looked up OUTSIDE the side stream's context)
            with torch.cuda.stream(self._d2h_stream):
                if handle.reran:                # a six-product repeat ran on the step's stream just now: its records are the newest work there
                    self._d2h_stream.wait_stream(compute)
                else:
                    self._d2h_stream.wait_event(done)
                host = rec.to("cpu", non_blocking=False)
            rec.record_stream(self._d2h_stream)
        else:
            host = rec
        self.packer.deliver(host.numpy())
        return rec

    def _finished(self):
        import time

        now = time.perf_counter()
        done = [(k, r, now - self._arrival.pop(k)) for k, r in self.packer.pop_completed()]
        self.latencies.extend(lat for _, r, lat in done if len(r))       # push -> records back on the host, images with ROIs
        return done

    def _admit(self, key, image, depth, detections) -> None:
        import time

        n = len(detections["roi_cls"])
        if n and self._with_depth is not None and (depth is not None) != self._with_depth:
            raise ValueError("RoiStreamScheduler: a stream is either with depth or without, not mixed "
                             f"(image {key!r} {'has' if depth is not None else 'lacks'} a depth map)")
        self.packer.add_image(key, n)           # raises for a key still in flight BEFORE any state of that image is touched
        if n:
            if self._with_depth is None:
                self._with_depth = depth is not None
            if isinstance(image, torch.Tensor) and image.device.type == "cpu":
                image, depth = self._to_device(key, image, depth)
            self._images[key] = (image, depth, detections)
        self._arrival[key] = time.perf_counter()

    def _to_device(self, key, image, depth):
        """Host image (+ depth) -> device on the copy stream; the event is what ``_launch`` waits for."""
        dev = self.device if self.device is not None else torch.device("cuda", torch.cuda.current_device())
        if self._copy_stream is None:
            # high priority = a hardware queue of its own: a default-priority stream may be mapped onto the compute stream's queue
            # (HIP multiplexes its streams over a few hardware queues) and its copies would then wait for the step in front of them —
            # measured: 3.5 % of the copy time under compute with a default stream (profiles/r05b_bench_stream_hostfed.json)
            self._copy_stream = torch.cuda.Stream(device=dev, priority=-1)
        with torch.cuda.stream(self._copy_stream):
            if self._time_h2d:
                t0 = torch.cuda.Event(enable_timing=True)
                t0.record()
            image_d = image.to(dev, non_blocking=True)
            depth_d = depth.to(dev, non_blocking=True) if depth is not None else None
            ev = torch.cuda.Event(enable_timing=self._time_h2d)
            ev.record()
        self._h2d_ready[key] = ev               # (_launch marks the tensors as used by the compute stream that crops them)
        self.h2d_bytes += image.numel() * image.element_size() + (depth.numel() * depth.element_size() if depth is not None else 0)
        if self._time_h2d:
            self._h2d_timing.append((t0, ev))
        return image_d, depth_d

    def h2d_done_event(self, key):
        """The event behind the host-to-device copies of image ``key`` (a host-fed image admitted by ``push`` / ``launch_next``), or
        None once every ROI of the image has been dealt into a step (the copies are long done then) or for a device image.  The
        copies are asynchronous (``non_blocking``) reads of the caller's PINNED buffers: a caller that recycles those buffers must
        ``event.synchronize()`` (or make its producer stream wait for it) before overwriting them."""
        return self._h2d_ready.get(key)

    def h2d_ms(self, reset: bool = True) -> float:
        """Summed device-side duration of the host-to-device copies admitted so far (``time_h2d=True``), in ms."""
        return self.h2d_timeline(reset)["h2d_ms"]

    def h2d_timeline(self, reset: bool = True) -> dict:
        """Device timeline of this scheduler's copies against its steps (``time_h2d=True``), see ``h2d_overlap``."""
        out = h2d_overlap(self._h2d_timing, self._step_timing)
        if reset:
            self._h2d_timing, self._step_timing = [], []
        return out

    # -- the stream --------------------------------------------------------------------------------
    def push(self, key, image: torch.Tensor, depth, detections: dict):
        self._admit(key, image, depth, detections)
        while self.packer.ready():
            self._launch(self.packer.next_pack())
            while len(self._in_flight) > self.max_in_flight:
                self._resolve_oldest()
        return self._finished()

    def launch_next(self, feeder):
        """bench.py's step: pull (key, image, depth, detections) tuples from ``feeder`` until one more step is launched;
        returns a callable that resolves the OLDEST step in flight (-> its records f32[rois_per_step,16] on the device).  Call
        it one launch late and the host never waits for the device."""
        while not self.packer.ready():
            self._admit(*next(feeder))
        self._launch(self.packer.next_pack())

        def resolve():
            rec = self._resolve_oldest()
            self._finished()
            return rec
        return resolve

    def flush(self):
        while self.packer.pending:
            self._launch(self.packer.next_pack(flush=True))
        while self._in_flight:
            self._resolve_oldest()
        return self._finished()
