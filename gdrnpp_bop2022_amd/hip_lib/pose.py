"""Pose post-processing: the resident meshes, sampling and nearest-neighbour kernels, correspondence decoding, the PnP solvers,
pose decoding, the depth renderer and refinement, pose records, flow and mask pasting."""
from __future__ import annotations

import ctypes

import torch

from .abi import dev_ptr, f32_ptr, gdrnpp_meshes, launch, load, opt_f32_ptr
from .net import ROT_MODES, T_MODES


class MeshSet:
    """All object models of a dataset, flat and resident in HBM (``gdrnpp_meshes``)."""

    def __init__(self, vertices: list, faces: list, device="cuda"):
        import numpy as np

        assert len(vertices) == len(faces) and len(vertices) > 0
        v_off, f_off = [0], [0]
        for v, f in zip(vertices, faces):
            v_off.append(v_off[-1] + int(len(v)))
            f_off.append(f_off[-1] + int(len(f)))
        self.n_obj = len(vertices)
        self.verts = torch.from_numpy(np.ascontiguousarray(np.concatenate(vertices, 0), np.float32)).to(device)
        self.faces = torch.from_numpy(np.ascontiguousarray(np.concatenate(faces, 0), np.int32)).to(device)
        self.vert_off = torch.tensor(v_off, dtype=torch.int32, device=device)
        self.face_off = torch.tensor(f_off, dtype=torch.int32, device=device)
        self.n_verts = v_off[1:]
        self.n_faces = f_off[1:]
        self._c = gdrnpp_meshes(self.verts.data_ptr(), self.faces.data_ptr(), self.vert_off.data_ptr(),
                                self.face_off.data_ptr(), self.n_obj, max(len(v) for v in vertices),
                                max(len(f) for f in faces))

    @property
    def c(self):
        return ctypes.byref(self._c)

    def bytes_per_render(self, obj: int) -> int:
        return 12 * (self.n_verts[obj] - (self.n_verts[obj - 1] if obj else 0)) + 12 * (
            self.n_faces[obj] - (self.n_faces[obj - 1] if obj else 0))


def fps(pts: torch.Tensor, sn: int, init_center: bool = True, start_idx: torch.Tensor | None = None) -> torch.Tensor:
    """pts f32[b,pn,3] -> idxs i32[b,sn]."""
    lib = load()
    assert pts.dim() == 3 and pts.shape[2] == 3
    b, pn, _ = pts.shape
    idxs = torch.empty((b, sn), dtype=torch.int32, device=pts.device)
    ws_bytes = lib.gdrnpp_fps_workspace_bytes(b, pn)
    ws = torch.empty((max(ws_bytes, 4),), dtype=torch.uint8, device=pts.device)
    sp = dev_ptr(start_idx, torch.int32, "start_idx") if start_idx is not None else None
    launch("gdrnpp_fps", f32_ptr(pts, "pts"), idxs.data_ptr(), sp, b, pn, sn, 1 if init_center else 0, ws.data_ptr())
    return idxs


def nnd_forward(xyz1, xyz2, dist1, dist2, idx1, idx2) -> int:
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    launch("gdrnpp_nnd_forward", f32_ptr(xyz1, "xyz1"), f32_ptr(xyz2, "xyz2"), f32_ptr(dist1, "dist1"), f32_ptr(dist2, "dist2"),
           dev_ptr(idx1, torch.int32, "idx1"), dev_ptr(idx2, torch.int32, "idx2"), b, n, m)
    return 1


def nnd_backward(xyz1, xyz2, gradxyz1, gradxyz2, graddist1, graddist2, idx1, idx2) -> int:
    b, n, _ = xyz1.shape
    m = xyz2.shape[1]
    launch("gdrnpp_nnd_backward", f32_ptr(xyz1, "xyz1"), f32_ptr(xyz2, "xyz2"), f32_ptr(gradxyz1, "gradxyz1"), f32_ptr(gradxyz2, "gradxyz2"),
           f32_ptr(graddist1, "graddist1"), f32_ptr(graddist2, "graddist2"), dev_ptr(idx1, torch.int32, "idx1"),
           dev_ptr(idx2, torch.int32, "idx2"), b, n, m)
    return 1


def uncertainty_pnp_batched(pts2d, pts3d, wgt2d, K, init_rt, return_info: bool = False):
    b, pn, _ = pts2d.shape
    out = torch.empty((b, 6), dtype=torch.float64, device=pts2d.device)
    info = torch.zeros((b, 2), dtype=torch.int32, device=pts2d.device)
    launch("gdrnpp_uncertainty_pnp_batched", dev_ptr(pts2d, torch.float64, "pts2d"), dev_ptr(pts3d, torch.float64, "pts3d"),
           dev_ptr(wgt2d, torch.float64, "wgt2d"), dev_ptr(K, torch.float64, "K"), dev_ptr(init_rt, torch.float64, "init_rt"),
           out.data_ptr(), info.data_ptr(), b, pn)
    return (out, info) if return_info else out


def decode_correspondences(coor_x, coor_y, coor_z, mask_raw, coord2d, extent, im_wh, mask_type: int = 0,
                           mask_thr: float = 0.5, want_mask: bool = True):
    """Maps [b,1,h,w] (or [b,h,w]) -> (count i32[b], sel_idx i32[b,hw], img_pts f32[b,hw,2], mdl_pts f32[b,hw,3],
    out_mask f32[b,1,h,w] | None).  Rows >= count[b] are undefined."""
    b = coor_x.shape[0]
    hw = coor_x[0].numel()
    dev = coor_x.device
    count = torch.empty((b,), dtype=torch.int32, device=dev)
    sel_idx = torch.empty((b, hw), dtype=torch.int32, device=dev)
    img_pts = torch.empty((b, hw, 2), dtype=torch.float32, device=dev)
    mdl_pts = torch.empty((b, hw, 3), dtype=torch.float32, device=dev)
    out_mask = torch.empty_like(mask_raw) if want_mask else None
    launch("gdrnpp_decode_correspondences", f32_ptr(coor_x, "coor_x"), f32_ptr(coor_y, "coor_y"), f32_ptr(coor_z, "coor_z"),
           f32_ptr(mask_raw, "mask"), f32_ptr(coord2d, "coord2d"), f32_ptr(extent, "extent"), f32_ptr(im_wh, "im_wh"),
           out_mask.data_ptr() if want_mask else None, count.data_ptr(), sel_idx.data_ptr(), img_pts.data_ptr(), mdl_pts.data_ptr(),
           b, hw, mask_type, float(mask_thr))
    return count, sel_idx, img_pts, mdl_pts, out_mask


def pose_from_pred_centroid_z(rot6d, t_, cams, centers, whs, resize_ratios, z_type: str = "REL", is_allo: bool = True):
    b = rot6d.shape[0]
    rot = torch.empty((b, 3, 3), dtype=torch.float32, device=rot6d.device)
    trans = torch.empty((b, 3), dtype=torch.float32, device=rot6d.device)
    launch("gdrnpp_pose_from_pred_centroid_z", f32_ptr(rot6d, "rot6d"), f32_ptr(t_, "t_"), f32_ptr(cams, "cams"), f32_ptr(centers, "centers"),
           f32_ptr(whs, "whs"), f32_ptr(resize_ratios, "resize_ratios"), rot.data_ptr(), trans.data_ptr(), b,
           {"REL": 0, "ABS": 1}[z_type], 1 if is_allo else 0)
    return rot, trans


def pose_from_pred(rot_in, t_, cams, centers=None, whs=None, resize_ratios=None, rot_mode: str = "rot6d",
                   t_mode: str = "centroid_z_rel", is_allo: bool = True):
    """``gdrnpp_pose_from_pred``: every ROT_TYPE (rot6d / quat / log_quat / lie_vec / matrix) x TRANS_TYPE (centroid_z REL or
    ABS, centroid_z_abs, trans) combination of GDRN_double_mask.py:162-200 -> (R_ego f32[b,3,3], t f32[b,3])."""
    b = rot_in.shape[0]
    rot = torch.empty((b, 3, 3), dtype=torch.float32, device=rot_in.device)
    trans = torch.empty((b, 3), dtype=torch.float32, device=rot_in.device)
    rm, tm = ROT_MODES[rot_mode], T_MODES[t_mode]
    launch("gdrnpp_pose_from_pred", f32_ptr(rot_in, "rot_in"), rm, f32_ptr(t_, "t_"), tm, f32_ptr(cams, "cams"), opt_f32_ptr(centers, "centers"),
           opt_f32_ptr(whs, "whs"), opt_f32_ptr(resize_ratios, "resize_ratios"), rot.data_ptr(), trans.data_ptr(), b, 1 if is_allo else 0)
    return rot, trans


def zoom_K(K, centers, scales, out_res: float):
    b = K.shape[0]
    out = torch.empty_like(K)
    launch("gdrnpp_zoom_K", f32_ptr(K, "K"), f32_ptr(centers, "centers"), f32_ptr(scales, "scales"), out.data_ptr(), b, float(out_res))
    return out


def render_depth(meshes: MeshSet, obj, K, R, t, res: int, z_near: float = 0.1, z_far: float = 100.0,
                 want_xyz: bool = False):
    b = obj.shape[0]
    depth = torch.empty((b, res, res), dtype=torch.float32, device=obj.device)
    xyz = torch.empty((b, res, res, 3), dtype=torch.float32, device=obj.device) if want_xyz else None
    launch("gdrnpp_render_depth", meshes.c, dev_ptr(obj, torch.int32, "obj"), f32_ptr(K, "K"), f32_ptr(R, "R"), f32_ptr(t, "t"), depth.data_ptr(),
           xyz.data_ptr() if want_xyz else None, b, res, z_near, z_far)
    return (depth, xyz) if want_xyz else depth


_REFINE_EVENT_SINK = None


def set_refine_event_sink(sink):
    """bench.py's roofline pass: a list that receives one (start, stop) HIP event pair per depth-refine launch, recorded
    on the launch stream (torch's current stream); None switches it off."""
    global _REFINE_EVENT_SINK
    _REFINE_EVENT_SINK = sink


def refine_kernel_name() -> str:
    return "depth_refine_kernel"


def _launch_refine(name: str, meshes: MeshSet, b: int, device, *args) -> None:
    """Launch a depth-refine entry point with ``args`` + the workspace it asks for; between two events when a sink is set."""
    nbytes = load().gdrnpp_depth_refine_workspace_bytes(meshes.c, b)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=device) if nbytes else None
    sink = _REFINE_EVENT_SINK
    if sink is not None:
        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
        ev[0].record()
    launch(name, meshes.c, *args, ws.data_ptr() if ws is not None else None, nbytes)
    if sink is not None:
        ev[1].record()
        sink.append(ev)


def depth_refine(meshes: MeshSet, obj, coor_x, coor_y, coor_z, mask_raw, roi_depth, K_crop, R, t, res: int = 64,
                 iters: int = 2, threshold: float = 0.8, mask_type: int = 0, use_coor_z: bool = False,
                 z_near: float = 0.1, z_far: float = 100.0, debug: bool = False, out: torch.Tensor | None = None):
    """-> t_refined f64[b,3] (and the per-iteration renders f32[b,iters,res,res] when debug)."""
    b = obj.shape[0]
    t_out = out if out is not None else torch.empty((b, 3), dtype=torch.float64, device=obj.device)
    dbg = torch.zeros((b, iters, res, res), dtype=torch.float32, device=obj.device) if debug else None
    if roi_depth.shape[-1] != roi_depth.shape[-2]:
        raise RuntimeError(f"depth_refine: roi_depth must be square, got {tuple(roi_depth.shape[-2:])}")
    _launch_refine(
        "gdrnpp_depth_refine", meshes, b, obj.device, dev_ptr(obj, torch.int32, "obj"), f32_ptr(coor_x, "coor_x"), f32_ptr(coor_y, "coor_y"), f32_ptr(coor_z, "coor_z"),
        f32_ptr(mask_raw, "mask"), f32_ptr(roi_depth, "roi_depth"), f32_ptr(K_crop, "K_crop"), f32_ptr(R, "R"), f32_ptr(t, "t"),
        dev_ptr(t_out, torch.float64, "t_out"), dbg.data_ptr() if debug else None,
        b, res, int(roi_depth.shape[-1]), iters, float(threshold), mask_type, 1 if use_coor_z else 0, z_near, z_far)
    return (t_out, dbg) if debug else t_out


def refine_to_records(meshes: MeshSet, obj, coor_x, coor_y, coor_z, mask_raw, roi_depth, cam, center, scale, R, t, score=None,
                      roi_id=None, res: int = 64, iters: int = 2, threshold: float = 0.8, mask_type: int = 0,
                      use_coor_z: bool = False, z_near: float = 0.1, z_far: float = 100.0):
    """The refine configuration's post-processing tail in ONE launch (``gdrnpp_refine_to_records``): K_crop from cam /
    center / scale, the depth refinement, and the f32[b,16] pose records."""
    b = obj.shape[0]
    rec = torch.empty((b, 16), dtype=torch.float32, device=obj.device)
    if b == 0:
        return rec
    _launch_refine(
        "gdrnpp_refine_to_records", meshes, b, obj.device, dev_ptr(obj, torch.int32, "obj"), f32_ptr(coor_x, "coor_x"), f32_ptr(coor_y, "coor_y"), f32_ptr(coor_z, "coor_z"),
        f32_ptr(mask_raw, "mask"), f32_ptr(roi_depth, "roi_depth"), f32_ptr(cam, "cam"), f32_ptr(center, "center"), f32_ptr(scale, "scale"),
        f32_ptr(R, "R"), f32_ptr(t, "t"), opt_f32_ptr(score, "score"),
        dev_ptr(roi_id, torch.int32, "roi_id") if roi_id is not None else None, rec.data_ptr(),
        b, res, int(roi_depth.shape[-1]), iters, float(threshold), mask_type, 1 if use_coor_z else 0, z_near, z_far)
    return rec


def pack_pose_records(R, t_refined, t_net, score, obj_id, roi_id):
    b = R.shape[0]
    rec = torch.empty((b, 16), dtype=torch.float32, device=R.device)
    launch("gdrnpp_pack_pose_records", f32_ptr(R, "R"), dev_ptr(t_refined, torch.float64, "t_refined") if t_refined is not None else None,
           opt_f32_ptr(t_net, "t_net"), opt_f32_ptr(score, "score"), dev_ptr(obj_id, torch.int32, "obj_id") if obj_id is not None else None,
           dev_ptr(roi_id, torch.int32, "roi_id") if roi_id is not None else None, rec.data_ptr(), b)
    return rec


def _pair_args(what: str, meshes: MeshSet, obj, R_est, t_est, R_gt, t_gt, K, k_optional: bool = False):
    """The checks every pair-error wrapper makes -> (obj pointer, [R_est, t_est, R_gt, t_gt, K pointers]): obj is i32 and lies in the
    mesh set (the read-back of two integers), each tensor is f64 and holds b x cols values.  ``K`` may be None only where ``k_optional``."""
    b = int(obj.shape[0])
    op = dev_ptr(obj, torch.int32, "obj")
    lo, hi = torch.aminmax(obj)
    if int(lo) < 0 or int(hi) >= meshes.n_obj:
        raise RuntimeError(f"{what}: obj must lie in [0, {meshes.n_obj}), got [{int(lo)}, {int(hi)}]")
    ptrs = []
    for t, name, cols in ((R_est, "R_est", 9), (t_est, "t_est", 3), (R_gt, "R_gt", 9), (t_gt, "t_gt", 3), (K, "K", 9)):
        if t is None and name == "K" and k_optional:
            ptrs.append(None)
            continue
        ptrs.append(dev_ptr(t, torch.float64, name))
        if t.numel() != b * cols:
            raise RuntimeError(f"{what}: {name} must hold {b} x {cols} values, got {tuple(t.shape)}")
    return op, ptrs


def pose_errors(meshes: MeshSet, obj, R_est, t_est, R_gt, t_gt, K, sym_rots=None, sym_off=None, symmetric=None) -> torch.Tensor:
    """``gdrnpp_pose_errors``: the custom evaluator's errors of b (estimate, ground truth) pairs -> f64[b,4] = ad (ADD, or ADI for
    a class flagged in ``symmetric``), re (degrees, against the closest symmetric ground-truth rotation), te, proj (pixels).
    obj i32[b]; R_est, R_gt, K f64[b,3,3|9]; t_est, t_gt f64[b,3] (metres); sym_rots f64[n_sym_total,3,3|9] with sym_off
    i32[n_obj+1]; symmetric u8[n_obj].  All device tensors; ``obj`` is checked against the mesh set here (one read-back of two
    integers), so that a class index without a model is an error and not a NaN row."""
    dev = meshes.verts.device
    b = int(obj.shape[0])
    out = torch.empty((b, 4), dtype=torch.float64, device=dev)
    if b == 0:
        return out
    op, ptrs = _pair_args("pose_errors", meshes, obj, R_est, t_est, R_gt, t_gt, K)
    if (sym_rots is None) != (sym_off is None):
        raise RuntimeError("pose_errors: sym_rots and sym_off come together")
    sp = so = fp = None
    if sym_rots is not None:
        sp, so = dev_ptr(sym_rots, torch.float64, "sym_rots"), dev_ptr(sym_off, torch.int32, "sym_off")
        if sym_off.numel() != meshes.n_obj + 1:
            raise RuntimeError(f"pose_errors: sym_off must hold n_obj + 1 = {meshes.n_obj + 1} offsets")
    if symmetric is not None:
        fp = dev_ptr(symmetric, torch.uint8, "symmetric")
        if symmetric.numel() != meshes.n_obj:
            raise RuntimeError(f"pose_errors: symmetric must hold n_obj = {meshes.n_obj} flags")
    nbytes = load().gdrnpp_pose_errors_workspace_bytes(meshes.c, b)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    launch("gdrnpp_pose_errors", meshes.c, op, *ptrs, sp, so, fp, out.data_ptr(), b, ws.data_ptr(), nbytes)
    return out


def _pair_sym_errors(what: str, cols: int, k_optional: bool, meshes: MeshSet, obj, R_est, t_est, R_gt, t_gt, K, sym_R, sym_t, sym_off):
    """``bop_errors`` and ``sym_errors``: the checks, the host copy of sym_off, the workspace and the launch of ``gdrnpp_<what>``
    -> f64[b,cols]."""
    import numpy as np

    dev = meshes.verts.device
    b = int(obj.shape[0])
    out = torch.empty((b, cols), dtype=torch.float64, device=dev)
    if b == 0:
        return out
    op, ptrs = _pair_args(what, meshes, obj, R_est, t_est, R_gt, t_gt, K, k_optional)
    off = np.ascontiguousarray(sym_off.cpu().numpy() if isinstance(sym_off, torch.Tensor) else sym_off).reshape(-1)
    if off.dtype.kind not in "iu" or off.size != meshes.n_obj + 1:
        raise RuntimeError(f"{what}: sym_off must hold n_obj + 1 = {meshes.n_obj + 1} integer offsets")
    off = off.astype(np.int32)          # a contiguous host array, alive across the launch
    n_sym = int(off[-1])
    if off[0] != 0 or (np.diff(off) <= 0).any():
        raise RuntimeError(f"{what}: sym_off must start at 0 and give every object at least one transformation (the identity)")
    for t, name, c in ((sym_R, "sym_R", 9), (sym_t, "sym_t", 3)):
        ptrs.append(dev_ptr(t, torch.float64, name))
        if t.numel() != n_sym * c:
            raise RuntimeError(f"{what}: {name} must hold sym_off[-1] x {c} = {n_sym} x {c} values, got {tuple(t.shape)}")
    offp = off.ctypes.data
    nbytes = getattr(load(), f"gdrnpp_{what}_workspace_bytes")(meshes.c, offp, b)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    launch(f"gdrnpp_{what}", meshes.c, op, *ptrs, offp, out.data_ptr(), b, ws.data_ptr(), nbytes)
    return out


def bop_errors(meshes: MeshSet, obj, R_est, t_est, R_gt, t_gt, K, sym_R, sym_t, sym_off) -> torch.Tensor:
    """``gdrnpp_bop_errors``: BOP19 MSSD and MSPD of b (estimate, ground truth) pairs -> f64[b,2] = mssd, mspd (pixels).
    obj i32[b]; R_est, R_gt, K f64[b,3,3|9]; t_est, t_gt f64[b,3], in the unit of the meshes' vertices (millimetres for a BOP results
    file); sym_R f64[n_sym_total,3,3|9] and sym_t f64[n_sym_total,3|3,1]: every object's symmetry transformations
    (``lib.pysixd.misc.get_symmetry_transformations``), object after object; sym_off: n_obj + 1 offsets into them (a sequence, an
    array or a tensor; it is read on the host, where it sizes the launch).  The other arguments are device tensors; ``obj`` is
    checked against the mesh set here (one read-back of two integers)."""
    return _pair_sym_errors("bop_errors", 2, False, meshes, obj, R_est, t_est, R_gt, t_gt, K, sym_R, sym_t, sym_off)


def sym_errors(meshes: MeshSet, obj, R_est, t_est, R_gt, t_gt, K, sym_R, sym_t, sym_off) -> torch.Tensor:
    """``gdrnpp_sym_errors``: the symmetry-aware reS, teS and projS of b (estimate, ground truth) pairs -> f64[b,3] = reS (degrees), teS
    (the unit of the translations), projS (pixels): each the minimum over the object's symmetry transformations of re, te and the mean
    projected distance of the model points.  Arguments and checks as ``bop_errors``, except that ``K`` may be None: projS is then not
    computed (the third column is NaN), nothing runs over the model points and the call costs O(symmetries) per pair; the first two
    columns are the same bits either way."""
    return _pair_sym_errors("sym_errors", 3, True, meshes, obj, R_est, t_est, R_gt, t_gt, K, sym_R, sym_t, sym_off)


VSD_WORKSPACE_BUDGET = 256 << 20        # bytes of projected vertices one ``gdrnpp_vsd_counts`` launch may stage


def _launch_chunked(what: str, meshes: MeshSet, count: int, ints, f64s, workspace_budget: int, rest) -> None:
    """Launch ``gdrnpp_<what>`` over ``count`` items in chunks whose workspace (``gdrnpp_<what>_workspace_bytes``) stays under
    ``workspace_budget`` bytes, on the current stream.  ints: (tensor, name) i32[count]; f64s: (tensor, name, cols) f64[count,cols]: both
    are checked here and passed as each chunk's slice.  ``rest(i0, n)``: the arguments between those pointers and the chunk's n."""
    for t, name in ints:
        dev_ptr(t, torch.int32, name)
        if t.numel() != count:
            raise RuntimeError(f"{what}: {name} must hold {count} values, got {tuple(t.shape)}")
    for t, name, cols in f64s:
        dev_ptr(t, torch.float64, name)
        if t.numel() != count * cols:
            raise RuntimeError(f"{what}: {name} must hold {count} x {cols} values, got {tuple(t.shape)}")
    query = getattr(load(), f"gdrnpp_{what}_workspace_bytes")
    per_item = query(meshes.c, 1)
    if per_item == 0:
        raise RuntimeError(f"{what}: the mesh set does not say its largest vertex count")
    chunk = max(1, min(count, int(workspace_budget) // per_item))
    nbytes = query(meshes.c, chunk)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=meshes.verts.device)
    for i0 in range(0, count, chunk):                      # stream order keeps one workspace safe across the chunks
        n = min(chunk, count - i0)
        launch(f"gdrnpp_{what}", meshes.c, *[t.reshape(-1)[i0:i0 + n].data_ptr() for t, _ in ints],
               *[t.reshape(-1)[cols * i0:cols * (i0 + n)].data_ptr() for t, _, cols in f64s], *rest(i0, n), n, ws.data_ptr(), nbytes)


def vsd_counts(meshes: MeshSet, obj, im_idx, R_est, t_est, R_gt, t_gt, K, diameter, depth_test, taus, delta, z_near: float = 1.0,
               z_far: float = 1e6, workspace_budget: int = VSD_WORKSPACE_BUDGET) -> torch.Tensor:
    """``gdrnpp_vsd_counts``: the pixel counts behind BOP19 VSD of b (estimate, ground truth) pairs -> i32[b, 2 + n_tau] = union, inter,
    cost_0 .. (a row of -1 for a pair whose obj or im_idx is out of range or whose object has no faces).  obj, im_idx i32[b]; R_est,
    R_gt, K f64[b,3,3|9]; t_est, t_gt f64[b,3] in the unit of the meshes' vertices (mm); diameter f64[b] (1.0 = not normalised);
    depth_test f32[n_im,H,W] in mm, 0 = missing: all device tensors.  taus: 1..16 floats (a sequence, an array or a tensor); delta: the
    visibility tolerance.  The meshes need faces.  A launch stages 80 bytes per vertex of the largest model per pair, so the pairs run
    in chunks that keep that workspace under ``workspace_budget`` bytes, on the current stream, into one output tensor."""
    dev = meshes.verts.device
    b = int(obj.shape[0])
    tau_t = torch.as_tensor(taus, dtype=torch.float64).reshape(-1).to(dev).contiguous()
    n_tau = int(tau_t.numel())
    out = torch.empty((b, 2 + n_tau), dtype=torch.int32, device=dev)
    if b == 0:
        return out
    if depth_test.dim() != 3:
        raise RuntimeError(f"vsd_counts: depth_test must be f32[n_im,H,W], got {tuple(depth_test.shape)}")
    n_im, H, W = (int(s) for s in depth_test.shape)
    dp = f32_ptr(depth_test, "depth_test")
    _launch_chunked("vsd_counts", meshes, b, [(obj, "obj"), (im_idx, "im_idx")],
                    [(R_est, "R_est", 9), (t_est, "t_est", 3), (R_gt, "R_gt", 9), (t_gt, "t_gt", 3), (K, "K", 9), (diameter, "diameter", 1)],
                    workspace_budget, lambda i0, n: (dp, n_im, H, W, tau_t.data_ptr(), n_tau, float(delta), float(z_near), float(z_far),
                                                     out[i0:i0 + n].data_ptr()))
    return out


def vsd_errors(meshes: MeshSet, obj, im_idx, R_est, t_est, R_gt, t_gt, K, diameter, depth_test, taus, delta, z_near: float = 1.0,
               z_far: float = 1e6, workspace_budget: int = VSD_WORKSPACE_BUDGET) -> torch.Tensor:
    """BOP19 VSD of b pairs -> f64[b, n_tau]: ``(cost_k + (union - inter)) / float(union)`` of ``vsd_counts`` as pose_error.py:110-126
    forms it (integers below 2^31, one fp64 division), 1.0 for every tau where union is 0, NaN where the row is -1."""
    c = vsd_counts(meshes, obj, im_idx, R_est, t_est, R_gt, t_gt, K, diameter, depth_test, taus, delta, z_near, z_far, workspace_budget)
    union, inter = c[:, 0:1].to(torch.int64), c[:, 1:2].to(torch.int64)
    e = (c[:, 2:].to(torch.int64) + (union - inter)).to(torch.float64) / union.to(torch.float64)
    e = torch.where(union == 0, torch.ones_like(e), e)
    return torch.where(union < 0, torch.full_like(e, float("nan")), e)


GT_INFO_COLUMNS = ("px_count_all", "px_count_valid", "px_count_visib", "obj_x_min", "obj_y_min", "obj_x_max", "obj_y_max",
                   "visib_x_min", "visib_y_min", "visib_x_max", "visib_y_max")


def gt_visibility(meshes: MeshSet, obj, im_idx, R, t, K, depth, delta, *, canvas_offset=(0, 0), want_masks: bool = False,
                  z_near: float = 1.0, z_far: float = 1e6, workspace_budget: int = VSD_WORKSPACE_BUDGET):
    """``gdrnpp_gt_visibility``: what calc_gt_info.py / calc_gt_masks.py compute for n ground-truth poses -> (info i32[n,11], mask,
    mask_visib).  info columns are ``GT_INFO_COLUMNS``: the three pixel counts, then the inclusive extents of the whole silhouette and of
    its visible part in image coordinates (empty: INT_MAX, INT_MAX, INT_MIN, INT_MIN; a row of -1 for a pose whose obj or im_idx is out of
    range or whose object has no faces).  mask, mask_visib: u8[n,H,W] of 0 / 255 when ``want_masks``, else None.  obj, im_idx i32[n]; R, K
    f64[n,3,3|9]; t f64[n,3] in the unit of the meshes' vertices (mm); depth f32[n_im,H,W] in mm, 0 = missing: all device tensors.
    canvas_offset (ox, oy): the render covers (W + 2 ox) x (H + 2 oy) pixels around the image — (W, H) is calc_gt_info.py's canvas, on
    which px_count_all and the silhouette's extents include the truncated part.  A launch stages 40 bytes per vertex of the largest model
    per pose, so the poses run in chunks that keep that workspace under ``workspace_budget`` bytes, on the current stream."""
    dev = meshes.verts.device
    n = int(obj.shape[0])
    if depth.dim() != 3:
        raise RuntimeError(f"gt_visibility: depth must be f32[n_im,H,W], got {tuple(depth.shape)}")
    n_im, H, W = (int(s) for s in depth.shape)
    ox, oy = (int(v) for v in canvas_offset)
    info = torch.empty((n, 11), dtype=torch.int32, device=dev)
    mask = torch.empty((n, H, W), dtype=torch.uint8, device=dev) if want_masks else None
    mask_visib = torch.empty((n, H, W), dtype=torch.uint8, device=dev) if want_masks else None
    if n == 0:
        return info, mask, mask_visib
    dp = f32_ptr(depth, "depth")
    _launch_chunked("gt_visibility", meshes, n, [(obj, "obj"), (im_idx, "im_idx")], [(R, "R", 9), (t, "t", 3), (K, "K", 9)], workspace_budget,
                    lambda i0, m: (dp, n_im, H, W, ox, oy, float(delta), float(z_near), float(z_far), info[i0:i0 + m].data_ptr(),
                                   mask[i0:i0 + m].data_ptr() if want_masks else None,
                                   mask_visib[i0:i0 + m].data_ptr() if want_masks else None))
    return info, mask, mask_visib


XYZ_CROP_COLUMNS = ("status", "px_count", "x1", "y1", "x2", "y2", "box_x1", "box_x2", "box_y1", "box_y2", "offset")
XYZ_CROP_CAPACITY_PX = 4 << 20          # pixels (6 bytes each) of the packed buffer one ``gdrnpp_gt_xyz_crop`` launch may fill by default
_XYZ_ROW = 12                           # i32 per pose on the device: the eleven columns, the offset in two words
_XYZ_PX_PER_POSE = {}                   # (W, H) -> the largest share of the packed buffer a pose has used: sizes the next call's first copy


def gt_xyz_crops(meshes: MeshSet, obj, R, t, K, im_size, *, z_near: float = 0.01, z_far: float = 6.5, capacity_px: int | None = None,
                 out: torch.Tensor | None = None, workspace_budget: int = VSD_WORKSPACE_BUDGET):
    """``gdrnpp_gt_xyz_crop``: the xyz_crop targets of n ground-truth poses, what the reference's ``*_1_gen_xyz.py`` tools compute per pose
    -> (packed f16[total_px,3] host array, table i64[n,11] host array).  table columns are ``XYZ_CROP_COLUMNS``: status (0, or -1 for a pose
    whose obj is out of range or whose object has no faces: the whole row is -1), the covered-pixel count, the inclusive extents of coverage
    (empty: INT_MAX, INT_MAX, INT_MIN, INT_MIN), the conservative box the pose occupies in ``packed`` (inclusive; empty when box_x1 >
    box_x2) and its offset there in pixels: pixel (x, y) of the box is ``packed[offset + (y - box_y1) * (box_x2 - box_x1 + 1) + (x - box_x1)]``,
    zeros where it is not covered.  obj i32[n]; R, K f64[n,3,3|9]; t f64[n,3] in the unit of the meshes' vertices (the tools: metres): device
    tensors.  im_size (W, H).

    The poses run in launches of at most ``workspace_budget`` bytes of staged vertices (40 per vertex of the largest model per pose) and
    ``capacity_px`` packed pixels (>= W * H; default ``XYZ_CROP_CAPACITY_PX`` or one image per pose, whichever is less).  A launch defers
    the poses that do not fit; the next one starts at the first of them.  The rows and the packed pixels of a launch share one device
    allocation and come back in ONE device-to-host copy; its length is a guess (the whole capacity for the first launch at an image
    size in this process, then twice the largest share a pose has used so far) and only a launch that used more costs a second copy
    for the rest.  ``out``: a caller's f16 device
    buffer of at least 3 * capacity_px elements to render into (then the rows come in a copy of their own); nothing at or beyond the
    pixels a launch used is written there."""
    import numpy as np

    what = "gt_xyz_crop"
    dev = meshes.verts.device
    n = int(obj.shape[0])
    W, H = int(im_size[0]), int(im_size[1])
    dev_ptr(obj, torch.int32, "obj")
    for x, name, cols in ((R, "R", 9), (t, "t", 3), (K, "K", 9)):
        dev_ptr(x, torch.float64, name)
        if x.numel() != n * cols:
            raise RuntimeError(f"{what}: {name} must hold {n} x {cols} values, got {tuple(x.shape)}")
    if n == 0:
        return np.zeros((0, 3), np.float16), np.zeros((0, len(XYZ_CROP_COLUMNS)), np.int64)
    query = load().gdrnpp_gt_xyz_crop_workspace_bytes
    per_item = query(meshes.c, 1)
    if per_item == 0:
        raise RuntimeError(f"{what}: the mesh set does not say its largest vertex count")
    chunk = max(1, min(n, int(workspace_budget) // per_item))
    if capacity_px is None:
        capacity_px = out.numel() // 3 if out is not None else max(H * W, min(chunk * H * W, XYZ_CROP_CAPACITY_PX))
    capacity_px = int(capacity_px)
    if out is not None:
        dev_ptr(out, torch.float16, "out")
        if out.numel() < 3 * capacity_px:
            raise RuntimeError(f"{what}: out must hold 3 x capacity_px = {3 * capacity_px} values, got {out.numel()}")
    nbytes = query(meshes.c, chunk)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    head = (16 + 4 * _XYZ_ROW * chunk + 15) // 16 * 16                      # totals i64[2], rows i32[chunk,12]; then the packed pixels
    buf = torch.empty((head + (0 if out is not None else 6 * capacity_px),), dtype=torch.uint8, device=dev)
    out_ptr = out.data_ptr() if out is not None else buf.data_ptr() + head
    obj1, R1, t1, K1 = obj.reshape(-1), R.reshape(-1), t.reshape(-1), K.reshape(-1)
    tables, packs, i0, total, per_pose = [], [], 0, 0, _XYZ_PX_PER_POSE.get((W, H))
    while i0 < n:                                                           # the copy below waits for the launch: one workspace serves all
        m = min(chunk, n - i0)
        launch("gdrnpp_gt_xyz_crop", meshes.c, obj1[i0:i0 + m].data_ptr(), R1[9 * i0:9 * (i0 + m)].data_ptr(), t1[3 * i0:3 * (i0 + m)].data_ptr(),
               K1[9 * i0:9 * (i0 + m)].data_ptr(), H, W, float(z_near), float(z_far), out_ptr, capacity_px, buf.data_ptr() + 16, buf.data_ptr(),
               m, ws.data_ptr(), nbytes)
        guess = 0 if out is not None else capacity_px if per_pose is None else min(capacity_px, 2 * per_pose * m)
        host = buf[:head + 6 * guess].cpu().numpy()
        n_done, used = (int(v) for v in host[:16].view(np.int64))
        if n_done <= 0:
            raise RuntimeError(f"{what}: a launch served no pose (capacity {capacity_px} px, image {W} x {H})")
        rows = host[16:16 + 4 * _XYZ_ROW * m].view(np.int32).reshape(m, _XYZ_ROW)[:n_done].astype(np.int64)
        if out is not None:
            pixels = out.reshape(-1)[:3 * used].cpu().numpy()
        elif used <= guess:
            pixels = host[head:head + 6 * used].view(np.float16)
        else:
            pixels = np.concatenate([host[head:], buf[head + 6 * guess:head + 6 * used].cpu().numpy()]).view(np.float16)
        table = rows[:, :len(XYZ_CROP_COLUMNS)].copy()
        table[:, 10] = np.where(rows[:, 0] == 0, (rows[:, 10] & 0xffffffff) | (rows[:, 11] << 32), 0) + total
        table[rows[:, 0] < 0] = -1
        tables.append(table)
        packs.append(pixels.reshape(-1, 3))
        per_pose = _XYZ_PX_PER_POSE[(W, H)] = max(per_pose or 0, -(-used // n_done))
        total += used
        i0 += n_done
    return (packs[0] if len(packs) == 1 else np.concatenate(packs)), np.concatenate(tables)


def pnp_iter_from_correspondences(img_pts, mdl_pts, count, K, R_net, t_net, return_info: bool = False):
    """Net-initialised iterative PnP (gdrn_evaluator.py:241-371, pnp_type="iter") for all ROIs at once."""
    b, stride, _ = img_pts.shape
    R_out = torch.empty((b, 3, 3), dtype=torch.float32, device=img_pts.device)
    t_out = torch.empty((b, 3), dtype=torch.float32, device=img_pts.device)
    info = torch.zeros((b, 2), dtype=torch.int32, device=img_pts.device)
    launch("gdrnpp_pnp_iter_from_correspondences", f32_ptr(img_pts, "img_pts"), f32_ptr(mdl_pts, "mdl_pts"), dev_ptr(count, torch.int32, "count"),
           stride, f32_ptr(K, "K"), f32_ptr(R_net, "R_net"), f32_ptr(t_net, "t_net"), R_out.data_ptr(), t_out.data_ptr(), info.data_ptr(), b)
    return (R_out, t_out, info) if return_info else (R_out, t_out)


def epnp_ransac(img_pts, mdl_pts, count, K, iters: int = 100, reproj_err: float = 3.0, confidence: float = 0.99,
                draws: "torch.Tensor | None" = None):
    """cv2.solvePnPRansac(flags=SOLVEPNP_EPNP) for every ROI (``gdrnpp_epnp_ransac``): img_pts f32[b,stride,2], mdl_pts
    f32[b,stride,3], count i32[b] (``decode_correspondences`` outputs), K f32[b,9|3,3]; ``draws`` i32/u32[b,n] injects the
    random words of the minimal sets (default: OpenCV's fixed-seed cv::RNG).  -> (R f32[b,3,3], t f32[b,3], n_inliers
    i32[b], status i32[b], inlier_mask u8[b,stride])."""
    b, stride, _ = img_pts.shape
    dev = img_pts.device
    Rm = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((b, 3), dtype=torch.float32, device=dev)
    n_inl = torch.empty((b,), dtype=torch.int32, device=dev)
    status = torch.empty((b,), dtype=torch.int32, device=dev)
    mask = torch.empty((b, stride), dtype=torch.uint8, device=dev)
    if b == 0:
        return Rm, t, n_inl, status, mask
    nbytes = load().gdrnpp_epnp_ransac_workspace_bytes(b, stride, iters)
    ws = torch.empty((nbytes,), dtype=torch.uint8, device=dev)
    n_draws = 0
    if draws is not None:
        if draws.dtype not in (torch.int32, torch.uint32) or not draws.is_cuda or not draws.is_contiguous() or draws.shape[0] != b:
            raise RuntimeError("draws must be a contiguous 32-bit integer CUDA(HIP) tensor [b, n_words]")
        n_draws = int(draws.shape[1])
    launch("gdrnpp_epnp_ransac", f32_ptr(img_pts, "img_pts"), f32_ptr(mdl_pts, "mdl_pts"), dev_ptr(count, torch.int32, "count"),
           stride, f32_ptr(K.reshape(b, 9), "K"), draws.data_ptr() if draws is not None else None, n_draws, int(iters),
           float(reproj_err), float(confidence), Rm.data_ptr(), t.data_ptr(), n_inl.data_ptr(), status.data_ptr(), mask.data_ptr(),
           b, ws.data_ptr(), nbytes)
    return Rm, t, n_inl, status, mask


def epnp_batched(img_pts, mdl_pts, K):
    """Plain EPnP on all n >= 4 points of each problem: img_pts f32[b,n,2], mdl_pts f32[b,n,3], K f32[b,9|3,3]
    -> (R f32[b,3,3], t f32[b,3], status i32[b])."""
    b, n, _ = img_pts.shape
    dev = img_pts.device
    Rm = torch.empty((b, 3, 3), dtype=torch.float32, device=dev)
    t = torch.empty((b, 3), dtype=torch.float32, device=dev)
    status = torch.empty((b,), dtype=torch.int32, device=dev)
    launch("gdrnpp_epnp_batched", f32_ptr(img_pts, "img_pts"), f32_ptr(mdl_pts, "mdl_pts"), n, f32_ptr(K.reshape(b, 9), "K"), Rm.data_ptr(),
           t.data_ptr(), status.data_ptr(), b)
    return Rm, t, status


def paste_masks_rle(mask_probs, boxes_xyxy, im_h: int, im_w: int, threshold: float = 0.5, max_runs: int = 4096):
    """mask_probs f32[B,hm,wm], boxes f32[B,4] (device) -> list of B uncompressed COCO count lists (column-major, first
    run = zeros).  The launch is repeated with a larger buffer if an instance needs more than ``max_runs`` runs."""
    b, hm, wm = mask_probs.shape
    while True:
        counts = torch.empty((b, max_runs), dtype=torch.int32, device=mask_probs.device)
        n_runs = torch.empty((b,), dtype=torch.int32, device=mask_probs.device)
        launch("gdrnpp_paste_masks_rle", f32_ptr(mask_probs, "mask_probs"), f32_ptr(boxes_xyxy, "boxes"), b, hm, wm, im_h, im_w, float(threshold),
               counts.data_ptr(), n_runs.data_ptr(), max_runs)
        n = n_runs.tolist()
        if max(n) <= max_runs:
            c = counts.cpu().numpy().view("uint32")
            return [c[i, :n[i]].astype("int64").tolist() for i in range(b)]
        max_runs = max(n)


def flow_forward(depth_src, depth_tgt, KT, Kinv):
    """depth f32[B,1,H,W] x2, KT f32[B,3,4], Kinv f32[B,3,3] (device) -> flow f32[B,2,H,W], valid f32[B,1,H,W]."""
    b, _, h, w = depth_src.shape
    flow = torch.empty((b, 2, h, w), dtype=torch.float32, device=depth_src.device)
    valid = torch.empty((b, 1, h, w), dtype=torch.float32, device=depth_src.device)
    launch("gdrnpp_flow_forward", f32_ptr(depth_src, "depth_src"), f32_ptr(depth_tgt, "depth_tgt"), f32_ptr(KT, "KT"), f32_ptr(Kinv, "Kinv"),
           flow.data_ptr(), valid.data_ptr(), b, h, w)
    return flow, valid
