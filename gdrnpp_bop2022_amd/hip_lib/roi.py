"""ROI preparation: crop + resize of the detections' boxes, ROIAlign / RoIPool, and the device-side ROI table filled from
detections."""
from __future__ import annotations

import ctypes

import torch

from .abi import dev_ptr, f32_ptr, gdrnpp_roi_table, launch, load, opt_f32_ptr


def crop_resize_roi(images, depths, im_idx, centers, scales, out_res: int = 256, out_res_small: int = 64,
                    pixel_mean=(0.0, 0.0, 0.0), pixel_std=(255.0, 255.0, 255.0), want_img=True, want_coord2d=True):
    """GPU ROI preparation (read_data_test, data_loader.py:754-797).  images u8[n_im,H,W,3] BGR, depths f32[n_im,H,W]
    or None, im_idx i32[b] or None, centers f64[b,2], scales f64[b] ->
    (roi_img f32[b,3,out,out] | None, roi_depth f32[b,1,out,out] | None, roi_coord_2d f32[b,2,os,os] | None)."""
    n_im, H, W, _ = images.shape
    b = centers.shape[0]
    dev = images.device
    roi_img = torch.empty((b, 3, out_res, out_res), dtype=torch.float32, device=dev) if want_img else None
    roi_depth = torch.empty((b, 1, out_res, out_res), dtype=torch.float32, device=dev) if depths is not None else None
    roi_c2d = (torch.empty((b, 2, out_res_small, out_res_small), dtype=torch.float32, device=dev)
               if want_coord2d else None)
    mean = (ctypes.c_double * 3)(*[float(v) for v in pixel_mean])
    std = (ctypes.c_double * 3)(*[float(v) for v in pixel_std])
    launch("gdrnpp_crop_resize_roi", dev_ptr(images, torch.uint8, "images"), opt_f32_ptr(depths, "depths"),
           n_im, H, W, dev_ptr(im_idx, torch.int32, "im_idx") if im_idx is not None else None,
           dev_ptr(centers, torch.float64, "centers"), dev_ptr(scales, torch.float64, "scales"),
           roi_img.data_ptr() if want_img else None, roi_depth.data_ptr() if roi_depth is not None else None,
           roi_c2d.data_ptr() if want_coord2d else None, b, out_res, out_res_small,
           ctypes.cast(mean, ctypes.c_void_p), ctypes.cast(std, ctypes.c_void_p))
    return roi_img, roi_depth, roi_c2d


def roi_align(x, rois, output_size, spatial_scale: float = 1.0, sampling_ratio: int = 0, aligned: bool = True):
    """detectron2.layers.ROIAlign(output_size, spatial_scale, sampling_ratio, aligned)(x, rois): x f32[B,C,H,W] (NCHW
    contiguous), rois f32[N,5] -> f32[N,C,oh,ow]."""
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else output_size
    bsz, c, h, w = x.shape
    n = rois.shape[0]
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    launch("gdrnpp_roi_align", f32_ptr(x, "x"), f32_ptr(rois, "rois"), out.data_ptr(), n, c, h, w, oh, ow, float(spatial_scale),
           int(sampling_ratio), 1 if aligned else 0)
    return out


def roi_pool(x, rois, output_size, spatial_scale: float = 1.0):
    """torchvision.ops.RoIPool(output_size, spatial_scale)(x, rois): x f32[B,C,H,W] (NCHW contiguous), rois f32[N,5] ->
    f32[N,C,oh,ow] (max over integer pixel bins)."""
    oh, ow = (output_size, output_size) if isinstance(output_size, int) else output_size
    bsz, c, h, w = x.shape
    n = rois.shape[0]
    out = torch.empty((n, c, oh, ow), dtype=torch.float32, device=x.device)
    launch("gdrnpp_roi_pool", f32_ptr(x, "x"), f32_ptr(rois, "rois"), out.data_ptr(), n, c, h, w, oh, ow, float(spatial_scale))
    return out


# column -> (torch dtype, trailing shape): the keys and dtypes of roi_stream.roi_host_arrays, in its order
ROI_TABLE_COLUMNS = {
    "center64": (torch.float64, (2,)), "scale64": (torch.float64, ()), "im_idx": (torch.int32, ()), "roi_cls": (torch.int64, ()),
    "roi_cam": (torch.float32, (3, 3)), "roi_center": (torch.float32, (2,)), "roi_wh": (torch.float32, (2,)),
    "scale": (torch.float32, ()), "resize_ratio": (torch.float32, ()), "roi_extent": (torch.float32, (3,)),
    "score": (torch.float32, ()), "roi_id": (torch.int32, ()),
}


def roi_table(cap: int, device) -> dict:
    """An empty ROI table of ``cap`` rows: one device allocation, every column a 16-byte aligned typed view of it."""
    sizes, total = {}, 0
    for k, (dt, tail) in ROI_TABLE_COLUMNS.items():
        n = cap * torch.empty((), dtype=dt).element_size()
        for t in tail:
            n *= t
        total = (total + 15) & ~15
        sizes[k] = (total, n)
        total += n
    raw = torch.zeros((total,), dtype=torch.uint8, device=device)
    return {k: raw[off:off + n].view(ROI_TABLE_COLUMNS[k][0]).reshape((cap,) + ROI_TABLE_COLUMNS[k][1]) for k, (off, n) in sizes.items()}


def rois_from_dets(dets, count, ratio: float, H: int, W: int, cam, extents, dzi_pad_scale: float = 1.5, out_res: int = 64,
                   score_thr: float = 0.0, top_k_per_obj: int = 0, cap: int = 256, table: dict | None = None, counts=None):
    """``gdrnpp_rois_from_dets``: ``yolox_postprocess`` output -> (table, counts).  ``table`` = {column: tensor of ``cap`` rows}
    (``roi_table``; the keys and dtypes of ``roi_stream.roi_host_arrays``), ``counts`` i32[1 + B] = (n_rois, per-image counts);
    rows from n_rois on are not written.  cam f32[3,3] or f32[B,3,3], extents f32[C,3], all on the device."""
    b, max_det, seven = dets.shape
    if seven != 7 or count.numel() != b:
        raise RuntimeError(f"rois_from_dets: dets f32[B,max_det,7] and count i32[B], got {tuple(dets.shape)} and {tuple(count.shape)}")
    if cam.numel() not in (9, 9 * b) or extents.dim() != 2 or extents.shape[1] != 3:
        raise RuntimeError(f"rois_from_dets: cam f32[3,3] or f32[B,3,3], extents f32[C,3], got {tuple(cam.shape)} and {tuple(extents.shape)}")
    table = table if table is not None else roi_table(cap, dets.device)
    if any(table[k].shape[0] != cap for k in ROI_TABLE_COLUMNS):
        raise RuntimeError(f"rois_from_dets: every table column must hold cap = {cap} rows")
    counts = counts if counts is not None else torch.zeros((1 + b,), dtype=torch.int32, device=dets.device)
    nbytes = load().gdrnpp_rois_from_dets_workspace_bytes(b, max_det)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dets.device)
    ctab = gdrnpp_roi_table(**{k: dev_ptr(table[k], ROI_TABLE_COLUMNS[k][0], k) for k in ROI_TABLE_COLUMNS})
    cnt = dev_ptr(counts, torch.int32, "counts")
    launch("gdrnpp_rois_from_dets", f32_ptr(dets, "dets"), dev_ptr(count, torch.int32, "count"), b, max_det, extents.shape[0], float(ratio),
           int(H), int(W), float(dzi_pad_scale), int(out_res), f32_ptr(cam, "cam"), 1 if cam.dim() == 3 else 0,
           f32_ptr(extents, "extents"), float(score_thr), int(top_k_per_obj), int(cap), ctypes.byref(ctab), cnt, cnt + 4,
           ws.data_ptr(), nbytes)
    return table, counts
