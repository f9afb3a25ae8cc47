"""GDRN's training losses: ``gdrn_loss`` of core/gdrn_modeling/models/GDRN_double_mask.py:287-536 (and the single-mask GDRN.py) with
the terms every shipped config uses on HIP kernels (csrc/gdrn_loss.hip) behind two ``torch.autograd.Function``s:

* ``DenseLosses``: the xyz terms (L1 / CE_coor), the mask and full-mask terms (L1 / BCE) and the region cross-entropy in one pass over
  the head's maps; its backward is a kernel of its own that recomputes from the same inputs;
* ``PoseLosses``: per ROI the closest symmetric ground-truth rotation (``get_closest_rot_batch``, which the reference runs on the host
  in a Python loop), the point-matching term (L1 / Smooth_L1 / MSE) and the centroid and z terms (L1), in fp64; its backward scales the
  gradients the forward wrote.

Nothing between the network's outputs and ``loss.backward()`` reads a value back to the host.  Terms outside that set (``loss_plan``
names them) run on torch operators written here and are differentiated by autograd, so every LOSS_CFG the reference accepts gets its
loss.  Not carried: ``PM_DISENTANGLE_T`` / ``PM_DISENTANGLE_Z`` and ``USE_MTL`` (the models hold no ``log_var_*`` parameters)."""
from __future__ import annotations

import functools

import numpy as np
import torch
import torch.nn.functional as F

from .. import hip_lib

# configs/_base_/gdrn_base.py:108-152; config.py's LOSS_CFG carries the three keys that shape the network, the others default here
LOSS_DEFAULTS = dict(
    XYZ_LOSS_TYPE="L1", XYZ_LOSS_MASK_GT="visib", XYZ_LW=1.0,
    FULL_MASK_LOSS_TYPE="BCE", FULL_MASK_LW=0.0,
    MASK_LOSS_TYPE="L1", MASK_LOSS_GT="trunc", MASK_LW=1.0,
    REGION_LOSS_TYPE="CE", REGION_LOSS_MASK_GT="visib", REGION_LW=1.0,
    NUM_PM_POINTS=3000, PM_LOSS_TYPE="L1", PM_SMOOTH_L1_BETA=1.0, PM_LOSS_SYM=False, PM_NORM_BY_EXTENT=False, PM_R_ONLY=True,
    PM_DISENTANGLE_T=False, PM_DISENTANGLE_Z=False, PM_T_USE_POINTS=True, PM_LW=1.0,
    ROT_LOSS_TYPE="angular", ROT_LW=0.0,
    CENTROID_LOSS_TYPE="L1", CENTROID_LW=1.0,
    Z_LOSS_TYPE="L1", Z_LW=1.0,
    TRANS_LOSS_TYPE="L1", TRANS_LOSS_DISENTANGLE=True, TRANS_LW=0.0,
    BIND_LOSS_TYPE="L1", BIND_LW=0.0,
)

_PM_KERNEL_TYPES = {"l1": "L1", "smooth_l1": "Smooth_L1", "mse": "MSE"}


def loss_cfg(cfg) -> dict:
    """cfg.MODEL.POSE_NET.LOSS_CFG over ``LOSS_DEFAULTS``."""
    lc = dict(LOSS_DEFAULTS)
    lc.update(dict(cfg["MODEL"]["POSE_NET"]["LOSS_CFG"]))
    return lc


def loss_plan(cfg) -> dict:
    """Which terms ``gdrn_loss`` forms for ``cfg`` and where: {"terms": {loss_dict key: "kernel" | "torch"}, "dense_kernel": bool,
    "pose_kernel": bool}.  Raises what ``gdrn_loss`` would raise for the keys that are not carried."""
    net = cfg["MODEL"]["POSE_NET"]
    lc = loss_cfg(cfg)
    if net.get("USE_MTL", False):
        raise NotImplementedError("MODEL.POSE_NET.USE_MTL: the models carry no log_var_* parameters")
    for key in ("PM_DISENTANGLE_T", "PM_DISENTANGLE_Z"):
        if lc["PM_LW"] > 0 and lc[key]:
            raise NotImplementedError(f"LOSS_CFG.{key} is not carried")
    terms = {}
    if not net["GEO_HEAD"].get("FREEZE", False):
        if lc["XYZ_LOSS_TYPE"] not in hip_lib.DENSE_XYZ_TYPES:
            raise NotImplementedError(f"unknown xyz loss type: {lc['XYZ_LOSS_TYPE']}")
        if lc["REGION_LOSS_TYPE"] != "CE":
            raise NotImplementedError(f"unknown region loss type: {lc['REGION_LOSS_TYPE']}")
        for k in ("loss_coor_x", "loss_coor_y", "loss_coor_z"):
            terms[k] = "kernel"
        double_mask = net.get("NAME", "GDRN_double_mask") != "GDRN"      # models/GDRN.py has no full-mask term
        for key, ty, on in (("loss_mask", lc["MASK_LOSS_TYPE"], True),
                            ("loss_mask_full", lc["FULL_MASK_LOSS_TYPE"], double_mask and lc["FULL_MASK_LW"] > 0)):
            if on:
                if ty not in ("L1", "BCE", "RW_BCE", "dice", "CE"):
                    raise NotImplementedError(f"unknown mask loss type: {ty}")
                terms[key] = "kernel" if ty in hip_lib.DENSE_MASK_TYPES else "torch"
        terms["loss_region"] = "kernel"
    pm_kernel = False
    if lc["PM_LW"] > 0:
        ty = lc["PM_LOSS_TYPE"].lower()
        if ty not in ("l1", "smooth_l1", "mse", "l2"):
            raise ValueError(f"loss type {ty} not supported.")
        pm_kernel = ty in _PM_KERNEL_TYPES
        terms["loss_PM_R" if lc["PM_R_ONLY"] else "loss_PM_RT"] = "kernel" if pm_kernel else "torch"
    if lc["ROT_LW"] > 0:
        terms["loss_rot"] = "torch"
    # the centroid and z terms ride in the point-matching launch
    if lc["CENTROID_LW"] > 0:
        terms["loss_centroid"] = "kernel" if pm_kernel and lc["CENTROID_LOSS_TYPE"] == "L1" else "torch"
    if lc["Z_LW"] > 0:
        terms["loss_z"] = "kernel" if pm_kernel and lc["Z_LOSS_TYPE"] == "L1" else "torch"
    if lc["TRANS_LW"] > 0:
        for k in (("loss_trans_xy", "loss_trans_z") if lc["TRANS_LOSS_DISENTANGLE"] else ("loss_trans_LPnP",)):
            terms[k] = "torch"
    if lc.get("BIND_LW", 0.0) > 0.0:
        terms["loss_bind"] = "torch"
    return {"terms": terms, "dense_kernel": any(v == "kernel" for k, v in terms.items() if k.startswith(("loss_coor", "loss_mask", "loss_region"))),
            "pose_kernel": pm_kernel or (lc["PM_LW"] > 0 and lc["PM_LOSS_SYM"])}


@functools.lru_cache(maxsize=256)
def _const(values: tuple, dtype, device):
    """A small device constant, uploaded once per (values, dtype, device)."""
    return torch.tensor(values, dtype=dtype, device=device)


# ---- the dense terms ------------------------------------------------------------------------------------------------------------------

class DenseLosses(torch.autograd.Function):
    """forward(out_x, out_y, out_z, out_mask, out_mask_full, out_region, opts) -> (losses f32[6], bad i32[1]): the weighted terms x, y, z,
    mask, full mask, region (0 for a map given as None) and the count of class targets outside [0, C).  ``opts``: gt_xyz / gt_xyz_bin /
    gt_region / masks, the selectors of ``hip_lib.gdrn_dense_losses`` and ``weights`` (six floats)."""

    @staticmethod
    def forward(ctx, out_x, out_y, out_z, out_mask, out_mask_full, out_region, opts):
        maps = (out_x, out_y, out_z, out_mask, out_mask_full, out_region)
        kw = {k: v for k, v in opts.items() if k != "weights"}
        sums, bad = hip_lib.gdrn_dense_losses(*maps, **kw)
        dev = sums.device
        n = float(next(m for m in kw["masks"].values() if m is not None).numel())
        inf = float("inf")
        den = sums.index_select(0, _const((6, 6, 6, 6, 6, 7), torch.int64, dev))
        den = torch.clamp(den, min=_const((1.0, 1.0, 1.0, n, n, 1.0), torch.float64, dev), max=_const((inf, inf, inf, n, n, inf), torch.float64, dev))
        losses = (sums[:6] / den * _const(tuple(float(w) for w in opts["weights"]), torch.float64, dev)).float()
        ctx.save_for_backward(*maps, sums)
        ctx.kw = kw
        ctx.weights = _const(tuple(float(w) for w in opts["weights"]), torch.float32, dev)
        ctx.mark_non_differentiable(bad)
        return losses, bad

    @staticmethod
    def backward(ctx, grad_losses, _grad_bad):
        *maps, sums = ctx.saved_tensors
        scale = (grad_losses.float() * ctx.weights).contiguous()
        grads = hip_lib.gdrn_dense_losses_backward(*maps, sums, scale, want=ctx.needs_input_grad[:6], **ctx.kw)
        return (*grads, None)


# ---- the per-ROI terms ----------------------------------------------------------------------------------------------------------------

class PoseLosses(torch.autograd.Function):
    """forward(R_pred, t_pred | None, pred_t_ | None, opts) -> (losses f32[3] = the weighted PM, centroid and z terms, R_gt' f32[B,3,3]).
    ``opts``: the constant arguments of ``hip_lib.gdrn_pose_losses`` and ``weights`` = (PM_LW, CENTROID_LW, Z_LW)."""

    @staticmethod
    def forward(ctx, R_pred, t_pred, pred_t_, opts):
        kw = {k: v for k, v in opts.items() if k != "weights"}
        B, P = R_pred.shape[0], kw["points"].shape[1]
        sums, R_sel, dR, dt, dpt = hip_lib.gdrn_pose_losses(R_pred.detach().contiguous(), t_pred=None if t_pred is None else t_pred.detach().contiguous(),
                                                            pred_t_=None if pred_t_ is None else pred_t_.detach().contiguous(), **kw)
        w_pm, w_c, w_z = (float(w) for w in opts["weights"])
        # mean over B P 3 times 3 PM_LW; mean over B 2; mean over B
        factors = (w_pm / (B * P), w_c / (2 * B), w_z / B)
        losses = (sums * _const(factors, torch.float64, sums.device)).float()
        ctx.save_for_backward(dR, dt, dpt if dpt is not None else dt)
        ctx.has_dpt = dpt is not None
        ctx.factors = _const(factors, torch.float32, sums.device)
        ctx.col = _const((factors[1], factors[1], factors[2]), torch.float32, sums.device)
        ctx.mark_non_differentiable(R_sel)
        return losses, R_sel

    @staticmethod
    def backward(ctx, grad_losses, _grad_sel):
        dR, dt, dpt = ctx.saved_tensors
        g = grad_losses.float()
        k_pm = g[0] * ctx.factors[0]
        gR = dR * k_pm if ctx.needs_input_grad[0] else None
        gt = dt * k_pm if ctx.needs_input_grad[1] else None
        gp = None
        if ctx.needs_input_grad[2] and ctx.has_dpt:
            gp = dpt * (g.index_select(0, _const((1, 1, 2), torch.int64, g.device)) * ctx.col)
        return gR, gt, gp, None


def sym_tables(sym_infos, device):
    """A list with one entry per object (K x 3 x 3 array / tensor, or None for an asymmetric object) -> (sym_rots f64[n_sym,9],
    sym_off i32[n_obj+1]) on ``device``: the layout ``hip_lib.pose_errors`` and ``hip_lib.gdrn_pose_losses`` take.  Built on the host, so
    build it once per dataset, not per step."""
    rots, off = [], [0]
    for s in sym_infos:
        if s is not None:
            a = np.asarray(s.detach().cpu().numpy() if isinstance(s, torch.Tensor) else s, dtype=np.float64).reshape(-1, 9)
            rots.append(a)
            off.append(off[-1] + len(a))
        else:
            off.append(off[-1])
    flat = np.concatenate(rots, 0) if rots else np.zeros((0, 9), np.float64)
    return torch.from_numpy(flat).to(device), torch.tensor(off, dtype=torch.int32, device=device)


# ---- terms on torch operators -----------------------------------------------------------------------------------------------------------

def _l2(pred, target):
    return torch.norm((pred - target).reshape(pred.shape[0], -1), p=2, dim=1, keepdim=True).mean()


def _by_type(kind, pred, target, what):
    if kind == "L1":
        return F.l1_loss(pred, target)
    if kind == "L2":
        return _l2(pred, target)
    if kind == "MSE":
        return F.mse_loss(pred, target)
    raise ValueError(f"Unknown {what} loss type: {kind}")


def _mask_term_torch(kind, out, gt):
    x = out[:, 0]
    if kind == "RW_BCE":        # weighted_ex_loss_probs(sigmoid(x), gt): positives and negatives normalised separately
        p = torch.sigmoid(x).clamp(min=1e-7, max=1 - 1e-7)
        pos = (gt > 0).to(x.dtype)
        neg = (gt == 0).to(x.dtype)
        n_pos, n_neg = pos.sum(), neg.sum()
        l_pos = 1.0 / n_pos.float().clamp(min=1.0) * (-gt * torch.log(p) * pos).sum()      # the reference's float32 reciprocal
        l_neg = 1.0 / n_neg.float().clamp(min=1.0) * (-torch.log(1 - p) * neg).sum()
        return l_pos + l_neg                # an empty class adds 0, as the reference's `if num > 0`
    if kind == "dice":          # soft_dice_loss(sigmoid(x), gt, eps=0.002)
        n = gt.shape[0]
        m1, m2 = torch.sigmoid(x).reshape(n, -1), gt.reshape(n, -1)
        return 1 - (2.0 * (m1 * m2).sum(1) / (m1.sum(1) + m2.sum(1) + 0.002)).sum() / n
    if kind == "CE":
        return F.cross_entropy(out, gt.long(), reduction="mean")
    raise NotImplementedError(f"unknown mask loss type: {kind}")


def _channel0(out):
    """[B,1,o,o] contiguous for the kernels: the map itself, or channel 0 of a 2-channel CE head whose term is L1 / BCE."""
    return out if out.shape[1] == 1 else out[:, 0:1]


def gdrn_loss(cfg, *, out_mask_vis=None, out_mask_full=None, gt_mask_trunc=None, gt_mask_visib=None, gt_mask_obj=None, gt_mask_full=None,
              out_x=None, out_y=None, out_z=None, gt_xyz=None, gt_xyz_bin=None, out_region=None, gt_region=None, out_rot=None, gt_rot=None,
              out_trans=None, gt_trans=None, out_centroid=None, out_trans_z=None, gt_trans_ratio=None, gt_points=None, sym_infos=None,
              extents=None, roi_classes=None, stats=None) -> dict:
    """The reference's ``gdrn_loss`` with its keyword names -> its ``loss_dict`` (0-dim float32 device tensors): loss_coor_x / _y / _z,
    loss_mask, loss_mask_full (FULL_MASK_LW > 0), loss_region, loss_PM_R or loss_PM_RT, loss_centroid, loss_z, and loss_rot,
    loss_trans_* and loss_bind where their weights are positive.  ``GEO_HEAD.FREEZE`` drops the terms over the maps.

    The targets come as ``train_targets.roi_train_targets`` returns them: float32 masks [B,o,o], int32 gt_region [B,o,o], uint8
    gt_xyz_bin [B,3,o,o], float32 gt_xyz [B,3,o,o].  gt_points / sym_infos / extents come either as per-object tables with
    ``roi_classes`` (gt_points f32[n_obj,P,3], extents f32[n_obj,3], sym_infos the pair of ``sym_tables`` or a list with one entry per
    object: no per-ROI copies), or in the reference's per-ROI form (gt_points [B,P,3], sym_infos a list of K x 3 x 3 or None per ROI,
    extents [B,3]).  ``stats``: a dict that receives "bad_targets" (i32[1] on the device: class targets outside [0, C), left out of
    sum and gradient) and "gt_rot_closest" (f32[B,3,3])."""
    plan = loss_plan(cfg)
    terms = plan["terms"]
    net = cfg["MODEL"]["POSE_NET"]
    lc = loss_cfg(cfg)
    loss = {}
    masks = {"trunc": gt_mask_trunc, "visib": gt_mask_visib, "obj": gt_mask_obj, "full": gt_mask_full}

    if plan["dense_kernel"]:
        k_mask = terms["loss_mask"] == "kernel"
        k_full = terms.get("loss_mask_full") == "kernel"
        opts = dict(gt_xyz=gt_xyz, gt_xyz_bin=gt_xyz_bin, gt_region=gt_region, masks=masks, xyz_type=lc["XYZ_LOSS_TYPE"],
                    xyz_mask=lc["XYZ_LOSS_MASK_GT"], mask_type=lc["MASK_LOSS_TYPE"] if k_mask else "L1", mask_gt=lc["MASK_LOSS_GT"],
                    full_type=lc["FULL_MASK_LOSS_TYPE"] if k_full else "L1", region_mask=lc["REGION_LOSS_MASK_GT"],
                    weights=(lc["XYZ_LW"], lc["XYZ_LW"], lc["XYZ_LW"], lc["MASK_LW"], lc["FULL_MASK_LW"], lc["REGION_LW"]))
        if lc["XYZ_LOSS_TYPE"] == "L1":
            opts["gt_xyz_bin"] = None
        else:
            opts["gt_xyz"] = None
        dense, bad = DenseLosses.apply(out_x.contiguous(), out_y.contiguous(), out_z.contiguous(),
                                       _channel0(out_mask_vis).contiguous() if k_mask else None,
                                       _channel0(out_mask_full).contiguous() if k_full else None, out_region.contiguous(), opts)
        if stats is not None:
            stats["bad_targets"] = bad
        for i, key in enumerate(("loss_coor_x", "loss_coor_y", "loss_coor_z", "loss_mask", "loss_mask_full", "loss_region")):
            if terms.get(key) == "kernel":
                loss[key] = dense[i]
    if terms.get("loss_mask") == "torch":
        loss["loss_mask"] = _mask_term_torch(lc["MASK_LOSS_TYPE"], out_mask_vis, masks[lc["MASK_LOSS_GT"]]) * lc["MASK_LW"]
    if terms.get("loss_mask_full") == "torch":
        loss["loss_mask_full"] = _mask_term_torch(lc["FULL_MASK_LOSS_TYPE"], out_mask_full, gt_mask_full) * lc["FULL_MASK_LW"]
    if "loss_coor_x" in loss:       # the reference's key order
        loss = {k: loss[k] for k in ("loss_coor_x", "loss_coor_y", "loss_coor_z", "loss_mask", "loss_mask_full", "loss_region") if k in loss}

    z_type = net["PNP_NET"]["Z_TYPE"]
    pm_key = "loss_PM_R" if lc["PM_R_ONLY"] else "loss_PM_RT"
    gt_rot_sel = gt_rot
    if lc["PM_LW"] > 0:
        assert gt_points is not None and gt_trans is not None and gt_rot is not None
        dev = out_rot.device
        B = out_rot.shape[0]
        if roi_classes is not None:
            obj, points, ext_table = roi_classes.to(torch.int32), gt_points, extents
            per_obj = gt_points.shape[0]
        else:                       # the reference's per-ROI form: one object per ROI
            obj, points, ext_table = torch.arange(B, dtype=torch.int32, device=dev), gt_points, extents
            per_obj = B
        sym_rots = sym_off = None
        if lc["PM_LOSS_SYM"]:
            assert sym_infos is not None
            if isinstance(sym_infos, tuple) and len(sym_infos) == 2 and isinstance(sym_infos[1], torch.Tensor) and sym_infos[1].dtype == torch.int32:
                sym_rots, sym_off = sym_infos
            else:
                if len(sym_infos) != per_obj:
                    raise RuntimeError(f"gdrn_loss: sym_infos must hold one entry per {'object' if roi_classes is not None else 'ROI'} ({per_obj}), got {len(sym_infos)}")
                sym_rots, sym_off = sym_tables(sym_infos, dev)
        if plan["pose_kernel"]:
            pm_kernel = terms[pm_key] == "kernel"
            with_t_ = terms.get("loss_centroid") == "kernel" or terms.get("loss_z") == "kernel"
            pred_t_ = torch.cat([out_centroid, out_trans_z.reshape(-1, 1)], 1) if with_t_ else None
            opts = dict(R_gt=gt_rot.float().contiguous(), obj=obj.contiguous(), points=points.float().contiguous(),
                        t_gt=None if lc["PM_R_ONLY"] else gt_trans.float().contiguous(), sym_rots=sym_rots, sym_off=sym_off,
                        extents=ext_table.float().contiguous() if lc["PM_NORM_BY_EXTENT"] else None,
                        gt_trans_ratio=gt_trans_ratio.float().contiguous() if with_t_ else None,
                        gt_trans=gt_trans.float().contiguous() if with_t_ and z_type == "ABS" else None, symmetric=bool(lc["PM_LOSS_SYM"]),
                        r_only=bool(lc["PM_R_ONLY"]), z_type=z_type if z_type in ("REL", "ABS") else "REL",
                        pm_type=_PM_KERNEL_TYPES.get(lc["PM_LOSS_TYPE"].lower(), "L1"), beta=float(lc["PM_SMOOTH_L1_BETA"]),
                        weights=(lc["PM_LW"], lc["CENTROID_LW"], lc["Z_LW"]))
            pose, gt_rot_sel = PoseLosses.apply(out_rot.float(), None if lc["PM_R_ONLY"] else out_trans.float(), pred_t_, opts)
            if pm_kernel:
                loss[pm_key] = pose[0]
        if terms[pm_key] == "torch":        # PM_LOSS_TYPE "L2": per-ROI norms over the closest ground truth the kernel chose
            pts = points[obj.long()] if roi_classes is not None else points
            est = (out_rot[:, None] @ pts[..., None]).squeeze(-1)
            tgt = (gt_rot_sel.to(out_rot.dtype)[:, None] @ pts[..., None]).squeeze(-1)
            w = 1
            if lc["PM_NORM_BY_EXTENT"]:
                e = ext_table[obj.long()] if roi_classes is not None else ext_table
                w = (1.0 / e.max(1, keepdim=True)[0]).view(-1, 1, 1)
            if lc["PM_R_ONLY"]:
                loss[pm_key] = 3 * _l2(w * est, w * tgt) * lc["PM_LW"]
            else:
                loss[pm_key] = 3 * _l2(w * (est + out_trans.view(-1, 1, 3)), w * (tgt + gt_trans.view(-1, 1, 3))) * lc["PM_LW"]
        if stats is not None:
            stats["gt_rot_closest"] = gt_rot_sel

    if lc["ROT_LW"] > 0:
        if lc["ROT_LOSS_TYPE"] == "angular":
            tr = torch.einsum("bii->b", torch.bmm(out_rot, gt_rot.transpose(1, 2)))
            v = ((1 - (tr - 1) / 2) / 2).mean()
        elif lc["ROT_LOSS_TYPE"] == "L2":
            v = torch.pow(out_rot - gt_rot, 2).mean()
        else:
            raise ValueError(f"Unknown rot loss type: {lc['ROT_LOSS_TYPE']}")
        loss["loss_rot"] = v * lc["ROT_LW"]
    if lc["CENTROID_LW"] > 0:
        assert net["PNP_NET"]["TRANS_TYPE"] == "centroid_z", "centroid loss is only valid for predicting centroid2d_rel_delta"
        if terms["loss_centroid"] == "kernel":
            loss["loss_centroid"] = pose[1]
        else:
            loss["loss_centroid"] = _by_type(lc["CENTROID_LOSS_TYPE"], out_centroid, gt_trans_ratio[:, :2], "centroid") * lc["CENTROID_LW"]
    if lc["Z_LW"] > 0:
        if z_type not in ("REL", "ABS"):
            raise NotImplementedError(f"Z_TYPE={z_type}")
        if terms["loss_z"] == "kernel":
            loss["loss_z"] = pose[2]
        else:
            gt_z = gt_trans_ratio[:, 2] if z_type == "REL" else gt_trans[:, 2]
            loss["loss_z"] = _by_type(lc["Z_LOSS_TYPE"], out_trans_z, gt_z, "z") * lc["Z_LW"]
    if lc["TRANS_LW"] > 0:
        if lc["TRANS_LOSS_DISENTANGLE"]:
            loss["loss_trans_xy"] = _by_type(lc["TRANS_LOSS_TYPE"], out_trans[:, :2], gt_trans[:, :2], "trans") * lc["TRANS_LW"]
            loss["loss_trans_z"] = _by_type(lc["TRANS_LOSS_TYPE"], out_trans[:, 2], gt_trans[:, 2], "trans") * lc["TRANS_LW"]
        else:
            loss["loss_trans_LPnP"] = _by_type(lc["TRANS_LOSS_TYPE"], out_trans, gt_trans, "trans") * lc["TRANS_LW"]
    if lc.get("BIND_LW", 0.0) > 0.0:
        pred_bind = torch.bmm(out_rot.permute(0, 2, 1), out_trans.view(-1, 3, 1)).view(-1, 3)
        gt_bind = torch.bmm(gt_rot.permute(0, 2, 1), gt_trans.view(-1, 3, 1)).view(-1, 3)
        if lc["BIND_LOSS_TYPE"] in ("L1", "L2"):
            v = _by_type(lc["BIND_LOSS_TYPE"], pred_bind, gt_bind, "bind")
        elif lc["CENTROID_LOSS_TYPE"] == "MSE":          # the reference tests CENTROID_LOSS_TYPE for its MSE branch (:525)
            v = F.mse_loss(pred_bind, gt_bind)
        else:
            raise ValueError(f"Unknown bind loss (R^T@t) type: {lc['BIND_LOSS_TYPE']}")
        loss["loss_bind"] = v * lc["BIND_LW"]
    return loss


# ---- the differentiable pose of the training forward --------------------------------------------------------------------------------------

def pose_from_pred_train(pred_rot_, pred_t_, roi_cams, roi_centers, roi_whs, resize_ratios, z_type: str = "REL", is_allo: bool = True):
    """rot6d -> R, the ``centroid_z`` translation (Z_TYPE REL or ABS) and allocentric -> egocentric on torch operators, differentiable:
    the arithmetic of ``hip_lib.pose_from_pred`` (csrc/pose_maps.hip), which has no gradient -> (R_ego [B,3,3], t [B,3]).  The
    allocentric-to-egocentric rotation takes the ray to the object onto the optical axis about (0,0,1) x ray; with the unit ray
    (ox, oy, oz), which the kernel forms in fp32, its cosine is oz and its sine sqrt(1 - oz^2), and the axis is (-oy, ox, 0) normalised
    by itself: the matrix is formed in fp64 as the kernel forms it, without the kernel's acos / cos / sin round trip."""
    a, b = pred_rot_[:, 0:3], pred_rot_[:, 3:6]
    x = F.normalize(a, p=2, dim=1)
    z = F.normalize(torch.cross(x, b, dim=1), p=2, dim=1)
    y = torch.cross(z, x, dim=1)
    rot = torch.stack([x, y, z], dim=2)
    K = roi_cams.reshape(-1, 3, 3)
    cx = pred_t_[:, 0] * roi_whs[:, 0] + roi_centers[:, 0]
    cy = pred_t_[:, 1] * roi_whs[:, 1] + roi_centers[:, 1]
    if z_type == "REL":
        tz = pred_t_[:, 2] * resize_ratios.reshape(-1)
    elif z_type == "ABS":
        tz = pred_t_[:, 2]
    else:
        raise NotImplementedError(f"Z_TYPE={z_type}")
    trans = torch.stack([tz * (cx - K[:, 0, 2]) / K[:, 0, 0], tz * (cy - K[:, 1, 2]) / K[:, 1, 1], tz], dim=1)
    if not is_allo:
        return rot, trans
    tx, ty = trans[:, 0], trans[:, 1]
    nt = torch.sqrt((tx * tx + ty * ty) + tz * tz)
    ox, oy, c = (tx / nt).double(), (ty / nt).double(), (tz / nt).double()
    n = torch.sqrt(ox * ox + oy * oy)
    on_axis = (n == 0) | (c >= 1)
    n_safe = torch.where(on_axis, torch.ones_like(n), n)
    ux, uy = -oy / n_safe, ox / n_safe
    s = torch.sqrt(torch.where(on_axis, torch.ones_like(c), 1 - c * c))      # (an on-axis ROI takes the identity below)
    C = 1 - c
    M = torch.stack([ux * ux * C + c, ux * uy * C, uy * s,
                     ux * uy * C, uy * uy * C + c, -ux * s,
                     -uy * s, ux * s, c], dim=1).reshape(-1, 3, 3)
    eye = torch.eye(3, dtype=M.dtype, device=M.device).expand_as(M)
    M = torch.where(on_axis.view(-1, 1, 1), eye, M)
    return (M @ rot.double()).to(rot.dtype), trans
