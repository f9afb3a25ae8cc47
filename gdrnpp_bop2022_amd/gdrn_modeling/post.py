"""Device post-processing: the batched replacement of ``GDRN_Evaluator.process*`` (``GdrnHipPost``) and the xyz / uPnP / RLE
helpers around the same kernels."""
from __future__ import annotations

import torch

from .. import hip_lib
from . import hip_layers


def coor_planes(cfg, out_dict: dict):
    """``get_out_coor`` (engine_utils.py:295-312) as three single-channel planes.  Regression heads (one channel per axis)
    pass through; the classification flavour (``XYZ_LOSS_TYPE`` CE / CE_coor: XYZ_BIN + 1 logits per axis) becomes
    argmax-bin / (XYZ_BIN - 1) with the background bin mapped to 0, as the reference does before any post-processing."""
    planes = [out_dict["coor_x"], out_dict["coor_y"], out_dict["coor_z"]]
    if all(p.shape[1] == 1 for p in planes):
        return [p.contiguous() for p in planes]
    nbin = int(cfg.MODEL.POSE_NET.GEO_HEAD.XYZ_BIN)
    hip_layers.note_foreign_launch("coor_planes: classification xyz decoded with torch argmax / where")
    out = []
    for p in planes:
        idx = torch.argmax(p, dim=1, keepdim=True)
        idx = torch.where(idx == nbin, torch.zeros_like(idx), idx)
        out.append((idx.to(torch.float32) / float(nbin - 1)).contiguous())
    return out


class GdrnHipPost:
    """Batched, device-resident replacement of ``GDRN_Evaluator.process / process_depth_refine``."""

    def __init__(self, cfg, meshes: "hip_lib.MeshSet | None" = None, z_near: float = 0.1, z_far: float = 100.0):
        self.cfg = cfg
        self.meshes = meshes
        self.z_near, self.z_far = z_near, z_far  # Renderer.set_cam defaults (render_vispy/renderer.py:126)
        net_cfg = cfg.MODEL.POSE_NET
        self.out_res = net_cfg.OUTPUT_RES
        mlt = net_cfg.LOSS_CFG.MASK_LOSS_TYPE
        if mlt == "L1":
            self.mask_type = 0
        elif mlt in ("BCE", "RW_BCE", "dice"):
            self.mask_type = 1
        elif mlt == "CE":        # two logits per pixel: get_out_mask takes the argmax (engine_utils.py:329-330)
            self.mask_type = 2
        else:
            raise NotImplementedError(f"MASK_LOSS_TYPE={mlt}")
        if cfg.TEST.USE_DEPTH_REFINE and meshes is None:
            raise ValueError("TEST.USE_DEPTH_REFINE needs the object meshes (gdrn_evaluator.py:64-84)")

    def mask_plane(self, out_dict: dict) -> torch.Tensor:
        """The mask map the kernels consume: raw logits for L1 / BCE (normalised / squashed inside the kernels), the argmax
        label for the CE flavour (``get_out_mask``, engine_utils.py:315-333)."""
        m = out_dict["mask"]
        if self.mask_type == 2:
            hip_layers.note_foreign_launch("GdrnHipPost.mask_plane: CE mask decoded with torch argmax")
            m = torch.argmax(m, dim=1, keepdim=True).to(torch.float32)
        return m.contiguous()

    def process_depth_refine(self, batch: dict, out_dict: dict) -> torch.Tensor:
        """-> refined translation f64[b,3]; rotation is unchanged (gdrn_evaluator.py:559-561)."""
        cfg = self.cfg
        b = out_dict["trans"].shape[0]
        K_crop = hip_lib.zoom_K(batch["roi_cam"].reshape(b, 9).contiguous(), batch["roi_center"].contiguous(),
                                batch["scale"].reshape(b).contiguous(), self.out_res)
        cx, cy, cz = coor_planes(cfg, out_dict)
        return hip_lib.depth_refine(
            self.meshes, batch["roi_cls"].to(torch.int32), cx, cy, cz, self.mask_plane(out_dict),
            batch["roi_depth"].contiguous(), K_crop, out_dict["rot"].reshape(b, 9).contiguous(),
            out_dict["trans"].contiguous(), res=self.out_res, iters=cfg.TEST.DEPTH_REFINE_ITER,
            threshold=cfg.TEST.DEPTH_REFINE_THRESHOLD, mask_type=self.mask_type,
            use_coor_z=bool(cfg.TEST.USE_COOR_Z_REFINE), z_near=self.z_near, z_far=self.z_far)

    def process_correspondences(self, batch: dict, out_dict: dict, max_num_points: int = -1, generator=None):
        """2D-3D correspondences for the PnP variants (gdrn_evaluator.py:115-153,255-311), all ROIs at once.
        ``max_num_points >= 4`` keeps a uniformly random subset of that size per ROI, in random order (:146-152; the
        reference shuffles with Python's unseeded ``random``, here a device permutation from ``generator``)."""
        imwh = torch.stack([batch["im_W"], batch["im_H"]], 1).float().contiguous()
        cx, cy, cz = coor_planes(self.cfg, out_dict)
        if max_num_points >= 4:
            hip_layers.note_foreign_launch("GdrnHipPost.process_correspondences(max_num_points): torch rand / argsort / gather")
            count, sel_idx, img_pts, mdl_pts, m = self.process_correspondences(batch, out_dict)
            b, hw = sel_idx.shape
            keys = torch.rand((b, hw), device=count.device, generator=generator)
            keys = torch.where(torch.arange(hw, device=count.device)[None] < count[:, None], keys, torch.full_like(keys, 2.0))
            order = torch.argsort(keys, dim=1)[:, :max_num_points]                   # the first `count` entries are a permutation
            take = lambda t: torch.gather(t, 1, order[..., None].expand(-1, -1, t.shape[2])).contiguous()  # noqa: E731
            pad = hw - order.shape[1]
            padded = lambda t: torch.cat([t, t.new_zeros((b, pad) + t.shape[2:])], 1).contiguous() if pad > 0 else t  # noqa: E731
            return (torch.clamp(count, max=max_num_points), padded(torch.gather(sel_idx, 1, order)), padded(take(img_pts)),
                    padded(take(mdl_pts)), m)
        return hip_lib.decode_correspondences(
            cx, cy, cz, self.mask_plane(out_dict), batch["roi_coord_2d"].contiguous(), batch["roi_extent"].contiguous(), imwh,
            mask_type=self.mask_type, mask_thr=self.cfg.MODEL.POSE_NET.GEO_HEAD.MASK_THR_TEST)

    def process_net_and_pnp(self, batch: dict, out_dict: dict):
        """``TEST.USE_PNP`` with ``PNP_TYPE="net_iter_pnp"`` (gdrn_evaluator.py:241-371, pnp_type="iter"): decode the
        maps, compact the 2D-3D correspondences and run the net-initialised LM for every ROI on the device."""
        b = out_dict["trans"].shape[0]
        count, _, img_pts, mdl_pts, _ = self.process_correspondences(batch, out_dict)
        return hip_lib.pnp_iter_from_correspondences(
            img_pts, mdl_pts, count, batch["roi_cam"].reshape(b, 9).contiguous(),
            out_dict["rot"].reshape(b, 9).contiguous(), out_dict["trans"].contiguous())

    def process_pnp_ransac(self, batch: dict, out_dict: dict, iters: int = 100, draws=None):
        """``TEST.USE_PNP`` with ``PNP_TYPE="ransac_pnp"`` (gdrn_evaluator.py:373-459): decode, compact, then
        ``misc.pnp_v2(..., method=EPNP, ransac=True, ransac_reprojErr=3, ransac_iter=100)`` for every ROI on the device.
        ROIs with fewer than 4 correspondences get the reference's sentinel pose -100 (:445-447); a RANSAC that finds no
        model leaves R = I, t = 0 (status 0).  Exactly 4 correspondences: one P3P solve like OpenCV's (csrc/epnp_ransac.hip,
        p3p_4points).  -> (R f32[b,3,3], t f32[b,3], status i32[b])."""
        b = out_dict["trans"].shape[0]
        count, _, img_pts, mdl_pts, _ = self.process_correspondences(batch, out_dict)
        R, t, _, status, _ = hip_lib.epnp_ransac(img_pts, mdl_pts, count, batch["roi_cam"].reshape(b, 9).contiguous(),
                                                 iters=iters, reproj_err=3.0, draws=draws)
        hip_layers.note_foreign_launch("GdrnHipPost.process_pnp_ransac: torch where / full_like around the RANSAC kernels")
        few = (count < 4).view(b, 1)
        R = torch.where(few.view(b, 1, 1), torch.full_like(R, -100.0), R)
        t = torch.where(few, torch.full_like(t, -100.0), t)
        return R, t, status

    def process_net_and_ransac(self, batch: dict, out_dict: dict, rot_only: bool = False, draws=None):
        """``PNP_TYPE="net_ransac_pnp"`` (gdrn_evaluator.py:241-371 with pnp_type "ransac"): solvePnPRansac(EPNP, reprojErr 3, 20
        iterations) on the correspondences (the extrinsic guess is ignored by EPnP); the translation falls back to the network's
        when it moved by more than 1 m (:347-351); fewer than 4 correspondences or no model: the network pose (:355-358).
        ``rot_only``: RANSAC rotation with the network's translation — what the NAME ``net_ransac_pnp_rot`` suggests; NOT what the
        reference does under that name (``process_net_and_rot_pnp`` below is), kept for callers that want it."""
        b = out_dict["trans"].shape[0]
        count, _, img_pts, mdl_pts, _ = self.process_correspondences(batch, out_dict)
        R, t, _, status, _ = hip_lib.epnp_ransac(img_pts, mdl_pts, count, batch["roi_cam"].reshape(b, 9).contiguous(),
                                                 iters=20, reproj_err=3.0, draws=draws)
        hip_layers.note_foreign_launch("GdrnHipPost.process_net_and_ransac: torch norm / where around the RANSAC kernels")
        R_net, t_net = out_dict["rot"].reshape(b, 3, 3).float(), out_dict["trans"].float()
        use = ((count >= 4) & (status == 1)).view(b, 1)
        far = (t - t_net).norm(dim=1, keepdim=True) > 1.0
        t = t_net if rot_only else torch.where(use & ~far, t, t_net)
        R = torch.where(use.view(b, 1, 1), R, R_net)
        return R, t

    def process_net_and_rot_pnp(self, batch: dict, out_dict: dict):
        """``PNP_TYPE="net_ransac_pnp_rot"`` exactly as the reference runs it: ``process`` passes pnp_type "ransac_rot"
        (gdrn_evaluator.py:171-173), and ``process_net_and_pnp`` only takes its RANSAC branch for ``pnp_type == "ransac"`` (:319)
        — "ransac_rot" falls through to the ITERATIVE solvePnP seeded with the network pose, after which the network's translation
        is kept (:341-348).  So: rotation of the net-initialised LM, translation of the network (pinned by eval_pnp_golden.npz)."""
        R, _ = self.process_net_and_pnp(batch, out_dict)
        return R, out_dict["trans"].float()

    def process(self, batch: dict, out_dict: dict, roi_ids: torch.Tensor | None = None) -> torch.Tensor:
        """-> pose records f32[b,16] = R(9) | t(3, metres) | score | obj | roi_id | valid."""
        if out_dict["trans"].shape[0] == 0:       # an image / a rank without detections: nothing to launch (the reference
            return torch.zeros((0, 16), dtype=torch.float32, device=out_dict["trans"].device)   # skips such images)
        if self.cfg.TEST.USE_PNP:      # gdrn_evaluator.py:165-176 (the PnP variants return without the depth refinement)
            pnp_type = self.cfg.TEST.PNP_TYPE.lower()
            if pnp_type == "ransac_pnp":
                R, t, _ = self.process_pnp_ransac(batch, out_dict)
            elif pnp_type == "net_iter_pnp":
                R, t = self.process_net_and_pnp(batch, out_dict)
            elif pnp_type == "net_ransac_pnp":
                R, t = self.process_net_and_ransac(batch, out_dict)
            elif pnp_type == "net_ransac_pnp_rot":
                R, t = self.process_net_and_rot_pnp(batch, out_dict)
            else:
                raise NotImplementedError(f"TEST.PNP_TYPE={self.cfg.TEST.PNP_TYPE}")
            b = t.shape[0]
            return hip_lib.pack_pose_records(
                R.reshape(b, 9).contiguous(), None, t.contiguous(),
                batch["score"].float().contiguous() if "score" in batch else None,
                batch["roi_cls"].to(torch.int32).contiguous(), roi_ids)
        b = out_dict["trans"].shape[0]
        if self.cfg.TEST.USE_DEPTH_REFINE:
            # zoom_K -> refine -> pack in ONE launch (the reference: batch_data_inference_roi + the per-ROI loop +
            # pose_prediction_to_json, gdrn_evaluator.py:461-573)
            cfg = self.cfg
            cx, cy, cz = coor_planes(cfg, out_dict)
            return hip_lib.refine_to_records(
                self.meshes, batch["roi_cls"].to(torch.int32), cx, cy, cz, self.mask_plane(out_dict),
                batch["roi_depth"].contiguous(), batch["roi_cam"].reshape(b, 9).contiguous(), batch["roi_center"].contiguous(),
                batch["scale"].reshape(b).contiguous(), out_dict["rot"].reshape(b, 9).contiguous(), out_dict["trans"].contiguous(),
                score=batch["score"].float().contiguous() if "score" in batch else None, roi_id=roi_ids, res=self.out_res,
                iters=cfg.TEST.DEPTH_REFINE_ITER, threshold=cfg.TEST.DEPTH_REFINE_THRESHOLD, mask_type=self.mask_type,
                use_coor_z=bool(cfg.TEST.USE_COOR_Z_REFINE), z_near=self.z_near, z_far=self.z_far)
        t_ref = None
        return hip_lib.pack_pose_records(
            out_dict["rot"].reshape(b, 9).contiguous(), t_ref, out_dict["trans"].contiguous(),
            batch["score"].float().contiguous() if "score" in batch else None,
            batch["roi_cls"].to(torch.int32).contiguous(), roi_ids)


def xyz_back_projection(depth: torch.Tensor, ego_rot: torch.Tensor, trans: torch.Tensor, K: torch.Tensor) -> torch.Tensor:
    """``calc_xyz_bp_batch(..., fmt="BHWC")`` (lib/pysixd/misc.py:412-448): rendered depth f32[b,h,w] -> object-space points
    f32[b,h,w,3] = R^T ((x - cx) z / fx, (y - cy) z / fy, z) - t), zero where the depth is zero; integer pixel coordinates like the
    reference.  Plain tensor arithmetic on whatever device the depth lives on; pinned by tests/golden/xyz_bp_golden.npz (the
    reference's function executed from its source)."""
    bs, h, w = depth.shape
    dev = depth.device
    gy, gx = torch.meshgrid(torch.arange(h, device=dev, dtype=torch.float32), torch.arange(w, device=dev, dtype=torch.float32), indexing="ij")
    X = gx.expand(bs, h, w) - K[:, 0, 2].view(bs, 1, 1)
    Y = gy.expand(bs, h, w) - K[:, 1, 2].view(bs, 1, 1)
    cam = torch.stack((X * depth / K[:, 0, 0].view(bs, 1, 1), Y * depth / K[:, 1, 1].view(bs, 1, 1), depth), dim=-1)
    mask = (depth != 0).to(depth).unsqueeze(-1)
    return torch.einsum("bij,bhwj->bhwi", ego_rot.transpose(1, 2), cam - trans.view(bs, 1, 1, 3)) * mask


def render_roi_xyz_batch(meshes: hip_lib.MeshSet, roi_cls, ego_rot, trans, roi_zoom_K, out_res: int = 64, xyz_bp: bool = False,
                         z_near: float = 0.25, z_far: float = 6.0):
    """Online XYZ targets of the training-side ``batch_data`` (engine_utils.py:131-172) in ONE launch instead of a Python
    loop of GL renders + CUDA-GL copies: object-space surface points per ROI pixel (``pc_obj_tensor[:, :, :3]``) or, with
    ``xyz_bp`` (``XYZ_BP``), the rendered depth back-projected through ``calc_xyz_bp_batch`` (lib/pysixd/misc.py:412-448;
    integer pixel coordinates like the reference).  Returns (roi_xyz f32[bs,res,res,3], roi_mask_obj f32[bs,res,res]):
    the mask is the reference's "all three coordinates non-zero" test.  z_near / z_far default to the EGL renderer's."""
    bs = ego_rot.shape[0]
    dev = ego_rot.device
    out = hip_lib.render_depth(meshes, roi_cls.to(torch.int32).contiguous(), roi_zoom_K.reshape(bs, 3, 3).contiguous().float(),
                               ego_rot.contiguous().float(), trans.contiguous().float(), out_res, z_near, z_far,
                               want_xyz=not xyz_bp)
    depth, xyz = (out, None) if xyz_bp else out
    roi_xyz = xyz_back_projection(depth, ego_rot.float(), trans.float(), roi_zoom_K.reshape(bs, 3, 3).float()) if xyz_bp else xyz
    roi_mask_obj = ((roi_xyz[..., 0] != 0) & (roi_xyz[..., 1] != 0) & (roi_xyz[..., 2] != 0)).to(torch.float32)
    return roi_xyz, roi_mask_obj


def upnp_weights_from_cov(covar) -> "np.ndarray":
    """Weights of ``GDRN_Evaluator.pose_from_upnp`` (gdrn_evaluator.py:612-629): W = inv(sqrtm(C)) per 2x2 keypoint
    covariance, returned as (w_xx, w_xy, w_yy) f32[pn,3]; degenerate covariances (C[0,0] < 1e-6 or NaN) get zero weight.
    The reference calls ``scipy.linalg.sqrtm``; a symmetric positive-definite 2x2 matrix has the closed form
    sqrtm(C) = (C + s I) / t with s = sqrt(det C), t = sqrt(trace C + 2 s) (Cayley-Hamilton), used here so that no per-keypoint
    SciPy call is needed.  tests/ pin it against scipy.linalg.sqrtm."""
    import numpy as np

    c = np.asarray(covar, np.float64).reshape(-1, 2, 2)
    bad = (c[:, 0, 0] < 1e-6) | np.isnan(c).any(axis=(1, 2))
    cs = np.where(bad[:, None, None], np.eye(2)[None], c)
    det = cs[:, 0, 0] * cs[:, 1, 1] - cs[:, 0, 1] * cs[:, 1, 0]
    s = np.sqrt(np.maximum(det, 0.0))
    t = np.sqrt(cs[:, 0, 0] + cs[:, 1, 1] + 2.0 * s)
    root = (cs + s[:, None, None] * np.eye(2)[None]) / t[:, None, None]
    inv = np.linalg.inv(root)
    inv[bad] = 0.0
    # the reference stacks float32 zeros with float64 inverses and keeps columns (0, 1, 3) of the flattened 2x2
    return inv.reshape(-1, 4)[:, (0, 1, 3)]


def pose_from_upnp(mean_pts2d, covar, points_3d, K, init_rt=None):
    """``GDRN_Evaluator.pose_from_upnp`` (gdrn_evaluator.py:612-629): covariance -> weights -> uncertainty-PnP (HIP, fp64)."""
    from ..core.csrc.uncertainty_pnp.un_pnp_utils import uncertainty_pnp

    return uncertainty_pnp(mean_pts2d, upnp_weights_from_cov(covar), points_3d, K, init_rt=init_rt)


def mask_rles(cfg, batch: dict, out_dict: dict, key: str = "mask", compressed: bool = True) -> list:
    """SAVE_RESULTS_ONLY instance masks (gdrn_evaluator.py:914-945): ``get_out_mask`` (engine_utils.py:315-333) on the raw
    ``out_dict[key]`` maps, boxes = roi_center -/+ scale/2, then paste + threshold + COCO RLE fused on the device
    (``gdrnpp_paste_masks_rle``).  Returns one ``{"counts", "size"}`` dict per ROI like ``binary_mask_to_rle``."""
    from ..lib.utils.mask_utils import rle_from_counts

    net_cfg = cfg.MODEL.POSE_NET
    raw = out_dict[key]
    loss_type = net_cfg.LOSS_CFG.MASK_LOSS_TYPE
    bs = raw.shape[0]
    if loss_type == "L1":                     # per-ROI (m - min) / (max - min), no epsilon (reference behaviour)
        flat = raw.reshape(bs, -1)
        mn, mx = flat.min(1).values.view(bs, 1, 1, 1), flat.max(1).values.view(bs, 1, 1, 1)
        prob = (raw - mn) / (mx - mn)
    elif loss_type in ("BCE", "RW_BCE", "dice"):
        prob = torch.sigmoid(raw)
    elif loss_type == "CE":
        prob = torch.argmax(raw, dim=1, keepdim=True).to(torch.float32)
    else:
        raise NotImplementedError(f"unknown mask loss type: {loss_type}")
    scale = batch["scale"].view(bs, 1).to(torch.float32)
    boxes = torch.cat([batch["roi_center"] - scale / 2, batch["roi_center"] + scale / 2], 1).contiguous()
    im_h, im_w = int(batch["im_H"][0]), int(batch["im_W"][0])
    counts = hip_lib.paste_masks_rle(prob[:, 0].contiguous(), boxes, im_h, im_w, float(net_cfg.GEO_HEAD.MASK_THR_TEST))
    return [rle_from_counts(c, im_h, im_w, compressed) for c in counts]
