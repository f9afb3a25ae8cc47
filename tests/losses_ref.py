"""The yardstick of the training losses: this project's own restatement of the reference's ``gdrn_loss``
(core/gdrn_modeling/models/GDRN_double_mask.py:287-536, losses/pm_loss.py, core/utils/pose_utils.py:472-528) on torch operators, in
the dtype of its inputs (the tests run it in fp64 on the CPU; tools/loss_microbench.py runs it in fp32 on the device) and
differentiable by autograd.  tests/test_losses_cpu.py ties it to values and gradients recorded from the reference's own code.

``lc`` is a fully populated LOSS_CFG (every key of ``gdrn_modeling.losses.LOSS_DEFAULTS``).  The per-ROI form of the reference is
kept: gt_points [B,P,3], sym_infos a list of [K,3,3] or None, extents [B,3]."""
import numpy as np
import torch
import torch.nn.functional as F


def closest_rots(pred_rots, gt_rots, sym_infos):
    """``get_closest_rot_batch`` in fp64: per ROI the R_gt S_k with the smallest re(R_pred, R_gt S_k); R_gt itself is the first
    candidate and the earliest of equal candidates wins (np.argmin's first occurrence = the sequential scan with a strict <).
    Through the host, as the reference does it.  Each element of R_gt S is (a0 s0 + a1 s1) + a2 s2, the expression of
    csrc/gdrn_loss.hip, so that the chosen matrix can be compared bit for bit.  -> float64 ndarray [B,3,3]."""
    pr = pred_rots.detach().cpu().double().numpy()
    gt = gt_rots.detach().cpu().double().numpy()
    out = gt.copy()
    for i in range(len(gt)):
        sym = sym_infos[i]
        if sym is None:
            continue
        S = np.asarray(sym.detach().cpu().numpy() if isinstance(sym, torch.Tensor) else sym, dtype=np.float64).reshape(-1, 3, 3)
        if len(S) == 0:
            continue
        Rg = gt[i]
        X = (Rg[None, :, 0, None] * S[:, None, 0, :] + Rg[None, :, 1, None] * S[:, None, 1, :]) + Rg[None, :, 2, None] * S[:, None, 2, :]
        cand = np.concatenate([Rg[None], X], 0)
        out[i] = cand[int(np.argmin(re_deg(pr[i], cand)))]
    return out


def re_deg(R_est, R_gts):
    """lib/pysixd/pose_error.py:359-374 for K ground truths at once: float64 [K] degrees."""
    tr = (R_est[None] * R_gts).sum((1, 2))
    tr = np.minimum(tr, 3.0)
    return np.rad2deg(np.arccos(np.clip(0.5 * (tr - 1.0), -1.0, 1.0)))


def _l2(pred, target):
    return torch.norm((pred - target).reshape(pred.shape[0], -1), p=2, dim=1, keepdim=True).mean()


def _by_type(kind, pred, target, what):
    if kind == "L1":
        return (pred - target).abs().mean()
    if kind == "L2":
        return _l2(pred, target)
    if kind == "MSE":
        return ((pred - target) ** 2).mean()
    raise ValueError(f"Unknown {what} loss type: {kind}")


def _masked_ce(out, target, mask):
    """sum over ALL pixels of CE(out * m, target * m.long()) / max(sum m, 1): a masked-out pixel adds log C."""
    logp = F.log_softmax(out * mask[:, None], dim=1)
    t = target.long() * mask.long()
    return -logp.gather(1, t[:, None]).sum() / mask.sum().clamp(min=1.0)


def _mask_term(kind, out, gt):
    x = out[:, 0]
    if kind == "L1":
        return (x - gt).abs().mean()
    if kind == "BCE":
        return F.binary_cross_entropy_with_logits(x, gt, reduction="mean")
    if kind == "RW_BCE":
        p = torch.sigmoid(x).clamp(min=1e-7, max=1 - 1e-7)
        pos, neg = gt > 0, gt == 0
        loss = 0.0
        if pos.any():
            loss = loss + 1.0 / pos.sum().float() * (-gt[pos] * torch.log(p[pos])).sum()     # the reference's float32 reciprocal
        if neg.any():
            loss = loss + 1.0 / neg.sum().float() * (-torch.log(1 - p[neg])).sum()
        return loss
    if kind == "dice":
        n = gt.shape[0]
        m1, m2 = torch.sigmoid(x).reshape(n, -1), gt.reshape(n, -1)
        score = 2.0 * (m1 * m2).sum(1) / (m1.sum(1) + m2.sum(1) + 0.002)
        return 1 - score.sum() / n
    if kind == "CE":
        return F.cross_entropy(out, gt.long(), reduction="mean")
    raise NotImplementedError(f"unknown mask loss type: {kind}")


def _pm_elem(kind, beta, d):
    kind = kind.lower()
    if kind == "l1":
        return d.abs().mean()
    if kind == "mse":
        return (d ** 2).mean()
    if kind == "smooth_l1":
        if beta < 1e-5:
            return d.abs().mean()
        n = d.abs()
        return torch.where(n < beta, 0.5 * n ** 2 / beta, n - 0.5 * beta).mean()
    raise ValueError(f"loss type {kind} not supported.")


def gdrn_loss_ref(lc, *, out_mask_vis=None, out_mask_full=None, gt_mask_trunc=None, gt_mask_visib=None, gt_mask_obj=None, gt_mask_full=None,
                  out_x=None, out_y=None, out_z=None, gt_xyz=None, gt_xyz_bin=None, out_region=None, gt_region=None, out_rot=None, gt_rot=None,
                  out_trans=None, gt_trans=None, out_centroid=None, out_trans_z=None, gt_trans_ratio=None, gt_points=None, sym_infos=None,
                  extents=None, freeze=False, trans_type="centroid_z", z_type="REL"):
    """-> (loss_dict, R_gt' float64 ndarray [B,3,3] or None)."""
    loss = {}
    masks = {"trunc": gt_mask_trunc, "visib": gt_mask_visib, "obj": gt_mask_obj, "full": gt_mask_full}
    if not freeze:
        m = masks[lc["XYZ_LOSS_MASK_GT"]]
        den = m.sum().clamp(min=1.0)
        for c, (name, out) in enumerate((("x", out_x), ("y", out_y), ("z", out_z))):
            if lc["XYZ_LOSS_TYPE"] == "L1":
                v = (out * m[:, None] - gt_xyz[:, c:c + 1] * m[:, None]).abs().sum() / den
            elif lc["XYZ_LOSS_TYPE"] == "CE_coor":
                v = _masked_ce(out, gt_xyz_bin[:, c], m)
            else:
                raise NotImplementedError(f"unknown xyz loss type: {lc['XYZ_LOSS_TYPE']}")
            loss[f"loss_coor_{name}"] = v * lc["XYZ_LW"]
        loss["loss_mask"] = _mask_term(lc["MASK_LOSS_TYPE"], out_mask_vis, masks[lc["MASK_LOSS_GT"]]) * lc["MASK_LW"]
        if lc["FULL_MASK_LW"] > 0:
            loss["loss_mask_full"] = _mask_term(lc["FULL_MASK_LOSS_TYPE"], out_mask_full, gt_mask_full) * lc["FULL_MASK_LW"]
        if lc["REGION_LOSS_TYPE"] != "CE":
            raise NotImplementedError(f"unknown region loss type: {lc['REGION_LOSS_TYPE']}")
        loss["loss_region"] = _masked_ce(out_region, gt_region, masks[lc["REGION_LOSS_MASK_GT"]]) * lc["REGION_LW"]

    R_sel = None
    if lc["PM_LW"] > 0:
        if lc["PM_DISENTANGLE_T"] or lc["PM_DISENTANGLE_Z"]:
            raise NotImplementedError("PM_DISENTANGLE_T / PM_DISENTANGLE_Z")
        gt_rots = gt_rot
        if lc["PM_LOSS_SYM"]:
            R_sel = closest_rots(out_rot, gt_rot, sym_infos)
            gt_rots = torch.from_numpy(R_sel).to(device=gt_rot.device, dtype=gt_rot.dtype)
        est = (out_rot[:, None] @ gt_points[..., None]).squeeze(-1)
        tgt = (gt_rots[:, None] @ gt_points[..., None]).squeeze(-1)
        w = (1.0 / extents.max(1, keepdim=True)[0]).view(-1, 1, 1) if lc["PM_NORM_BY_EXTENT"] else 1
        if lc["PM_LOSS_TYPE"].lower() == "l2":
            pm = lambda a, b: _l2(a, b)                                                # noqa: E731
        else:
            pm = lambda a, b: _pm_elem(lc["PM_LOSS_TYPE"], lc["PM_SMOOTH_L1_BETA"], a - b)      # noqa: E731
        if lc["PM_R_ONLY"]:
            loss["loss_PM_R"] = 3 * pm(w * est, w * tgt) * lc["PM_LW"]
        else:
            loss["loss_PM_RT"] = 3 * pm(w * (est + out_trans.view(-1, 1, 3)), w * (tgt + gt_trans.view(-1, 1, 3))) * lc["PM_LW"]

    if lc["ROT_LW"] > 0:
        if lc["ROT_LOSS_TYPE"] == "angular":
            tr = torch.einsum("bii->b", out_rot @ gt_rot.transpose(1, 2))
            v = ((1 - (tr - 1) / 2) / 2).mean()
        elif lc["ROT_LOSS_TYPE"] == "L2":
            v = ((out_rot - gt_rot) ** 2).mean()
        else:
            raise ValueError(f"Unknown rot loss type: {lc['ROT_LOSS_TYPE']}")
        loss["loss_rot"] = v * lc["ROT_LW"]
    if lc["CENTROID_LW"] > 0:
        assert trans_type == "centroid_z"
        loss["loss_centroid"] = _by_type(lc["CENTROID_LOSS_TYPE"], out_centroid, gt_trans_ratio[:, :2], "centroid") * lc["CENTROID_LW"]
    if lc["Z_LW"] > 0:
        gt_z = gt_trans_ratio[:, 2] if z_type == "REL" else gt_trans[:, 2]
        loss["loss_z"] = _by_type(lc["Z_LOSS_TYPE"], out_trans_z, gt_z, "z") * lc["Z_LW"]
    if lc["TRANS_LW"] > 0:
        if lc["TRANS_LOSS_DISENTANGLE"]:
            loss["loss_trans_xy"] = _by_type(lc["TRANS_LOSS_TYPE"], out_trans[:, :2], gt_trans[:, :2], "trans") * lc["TRANS_LW"]
            loss["loss_trans_z"] = _by_type(lc["TRANS_LOSS_TYPE"], out_trans[:, 2], gt_trans[:, 2], "trans") * lc["TRANS_LW"]
        else:
            loss["loss_trans_LPnP"] = _by_type(lc["TRANS_LOSS_TYPE"], out_trans, gt_trans, "trans") * lc["TRANS_LW"]
    if lc.get("BIND_LW", 0.0) > 0.0:
        pb = torch.bmm(out_rot.permute(0, 2, 1), out_trans.view(-1, 3, 1)).view(-1, 3)
        gb = torch.bmm(gt_rot.permute(0, 2, 1), gt_trans.view(-1, 3, 1)).view(-1, 3)
        if lc["BIND_LOSS_TYPE"] in ("L1", "L2"):
            v = _by_type(lc["BIND_LOSS_TYPE"], pb, gb, "bind")
        elif lc["CENTROID_LOSS_TYPE"] == "MSE":      # the reference tests CENTROID_LOSS_TYPE here (:525)
            v = ((pb - gb) ** 2).mean()
        else:
            raise ValueError(f"Unknown bind loss (R^T@t) type: {lc['BIND_LOSS_TYPE']}")
        loss["loss_bind"] = v * lc["BIND_LW"]
    return loss, R_sel


# ---- tests/golden/losses_golden.npz ---------------------------------------------------------------------------------------------------------
VARIANTS = ("shipped", "ce_bce", "pm_rt", "fallback", "fallback_ce", "single")
NET_INPUTS = ("out_mask_vis", "out_mask_full", "out_x", "out_y", "out_z", "out_region", "out_rot", "out_trans", "out_centroid", "out_trans_z")


def variant_inputs(z, meta, name, dtype=torch.float64, device="cpu", grad=True):
    """-> (lc, kwargs of gdrn_loss_ref / gdrn_loss in the reference's per-ROI form, z_type)."""
    from gdrnpp_bop2022_amd.gdrn_modeling.losses import LOSS_DEFAULTS

    m = meta[name]
    lc = dict(LOSS_DEFAULTS)
    lc.update(m["loss_cfg"])
    kw = {}
    for key in z.files:
        if not key.startswith(f"{name}/in/"):
            continue
        k, a = key.split("/")[-1], z[key]
        t = torch.from_numpy(a)
        if a.dtype == np.float32:
            t = t.to(dtype)
            if grad and k in NET_INPUTS:
                t.requires_grad_(True)
        kw[k] = t.to(device) if device != "cpu" else t
        if grad and k in NET_INPUTS and device != "cpu":
            kw[k] = kw[k].detach().requires_grad_(True)
    kw["sym_infos"] = [z[f"sym_{j}"] if f"sym_{j}" in z.files else None for j in range(3)]
    if m["model"] == "GDRN":
        kw.pop("out_mask_full"), kw.pop("gt_mask_full")
    return lc, kw, m["z_type"]
