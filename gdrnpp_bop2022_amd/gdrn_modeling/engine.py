"""Inference engine: the reference's ``gdrn_inference_on_dataset`` + ``GDRN_Evaluator.process*`` hot loop
(core/gdrn_modeling/engine/gdrn_evaluator.py:155-239,461-573,575-585,668-809) re-scheduled for MI355X.

Reference schedule per image: forward -> D2H of all maps -> per-ROI Python loop (cv2.resize, vispy GL
render x2, NumPy compare) -> pickle all-gather.  Here, per batch of ROIs resident in HBM:

    forward (PyTorch-ROCm, no host sync)                                 a3
      -> gdrnpp_zoom_K                         (K_crop for the 64x64 maps)   a8.2
      -> gdrnpp_depth_refine                   (all iterations on chip)      a8 / a8.1
      -> gdrnpp_pack_pose_records              ([n,16] f32 records)          a13
      -> one RCCL all_gather of the fixed-shape records (multi-GPU only)

Nothing is copied to the host until the caller asks for the records.

This module is the public NAMESPACE of the engine and nothing else: no def, no class, no state (tests/test_engine_namespace.py).
The code lives in five modules, each importing only from those above it:

    records.py      sharding, record ordering, the one collective, the BOP writers (torch only)
    post.py         GdrnHipPost and the xyz / uPnP / RLE helpers
    range_check.py  the range-check policy of the three-product GEMM kernels and its process-wide counters
    streams.py      the step entry points, the stream dealer, the hipGraph forms
    roi_stream.py   host-side ROI preparation, RoiPacker, RoiStreamScheduler

The mutable counters of range_check.py are deliberately NOT re-exported: an imported int is a copy, and assigning to it here
would reset nothing.  Read them (``range_reruns()``) or reset them in ``range_check`` itself.
"""
from .records import (BOP_CSV_HEADER, GLOBAL_DETECTION_KEYS, PAD_ROI_ID, PER_ROI_DETECTION_KEYS, class_sorted_order,
                      gather_records, records_in_roi_order, records_to_bop, save_bop_csv, shard_range, sort_detections_by_class)
from .post import (GdrnHipPost, coor_planes, mask_rles, pose_from_upnp, render_roi_xyz_batch, upnp_weights_from_cov,
                   xyz_back_projection)
from .range_check import (X3_OVERFLOW_STEPS_TO_GIVE_UP, StepHandle, launch_with_range_check, range_reruns,
                          run_with_range_check)
from .streams import (GraphedInference, GraphedStepStreams, GraphHandle, StepStreams, default_compute_streams,
                      default_graph_streams, inference_step, inference_step_async, streams_overlap_ratio)
from .roi_stream import (RoiPacker, RoiStreamScheduler, batch_data_test_gpu, batch_from_uploaded, detections_from_bop_json,
                         detections_from_yolox, fill_packed, h2d_overlap, packed_layout, packed_views, roi_host_arrays,
                         rois_from_detections, upload_packed)

__all__ = [
    # records
    "BOP_CSV_HEADER", "GLOBAL_DETECTION_KEYS", "PAD_ROI_ID", "PER_ROI_DETECTION_KEYS", "class_sorted_order", "gather_records",
    "records_in_roi_order", "records_to_bop", "save_bop_csv", "shard_range", "sort_detections_by_class",
    # post
    "GdrnHipPost", "coor_planes", "mask_rles", "pose_from_upnp", "render_roi_xyz_batch", "upnp_weights_from_cov",
    "xyz_back_projection",
    # range_check
    "X3_OVERFLOW_STEPS_TO_GIVE_UP", "StepHandle", "launch_with_range_check", "range_reruns", "run_with_range_check",
    # streams
    "GraphHandle", "GraphedInference", "GraphedStepStreams", "StepStreams", "default_compute_streams", "default_graph_streams",
    "inference_step", "inference_step_async", "streams_overlap_ratio",
    # roi_stream
    "RoiPacker", "RoiStreamScheduler", "batch_data_test_gpu", "batch_from_uploaded", "detections_from_bop_json",
    "detections_from_yolox", "fill_packed", "h2d_overlap", "packed_layout", "packed_views", "roi_host_arrays",
    "rois_from_detections", "upload_packed",
]
