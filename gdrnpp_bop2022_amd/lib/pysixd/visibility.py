"""``estimate_visib_mask_gt`` of the reference's BOP-toolkit fork (lib/pysixd/visibility.py:44-54, visib_mode "bop19") on the device.

The toolkit's function takes two distance images that its callers made from a GL render and the scene's depth image.  Here the render,
the two distance images and the visibility test are one kernel (``hip_lib.gt_visibility``, csrc/gt_visib.hip), so the function takes what
those callers start from: ``d_test`` is the scene's DEPTH image in millimetres (0 = missing), and ``d_gt`` is a ``GtPose`` in place of the
rendered distance image.  The mask returned is the one the toolkit's callers get, pixel for pixel."""
from __future__ import annotations

import numpy as np
import torch


class GtPose:
    """What stands in for the rendered distance image of an object in its ground-truth pose: a ``pose_error.VsdRenderer`` (the models
    with faces on the device, BOP object id -> index), the object id, R 3x3, t 3 (mm) and the camera matrix K."""

    def __init__(self, renderer, obj_id, R, t, K):
        self.renderer, self.obj_id, self.R, self.t, self.K = renderer, int(obj_id), R, t, K


def estimate_visib_mask_gt(d_test, d_gt, delta, visib_mode="bop19"):
    """The visible part of the object's silhouette: bool[H,W].  d_test: the scene's depth image f32[H,W] in mm; d_gt: a ``GtPose``."""
    if visib_mode != "bop19":
        if visib_mode == "bop18":
            raise NotImplementedError("pysixd.visibility: visib_mode 'bop18' is not computed here (the BOP19 scripts use 'bop19')")
        raise ValueError("Unknown visibility mode.")
    if not isinstance(d_gt, GtPose):
        raise TypeError("pysixd.visibility.estimate_visib_mask_gt: d_gt must be a GtPose (the render runs on the device, see the module's docstring)")
    if not torch.cuda.is_available():
        raise RuntimeError("pysixd.visibility: needs a HIP device (no CPU fallback)")
    from ... import hip_lib

    meshes = d_gt.renderer.meshes
    dev = meshes.verts.device

    def T(a, n):
        return torch.from_numpy(np.ascontiguousarray(np.asarray(a, np.float64).reshape(1, n))).to(dev)

    depth = torch.from_numpy(np.ascontiguousarray(np.asarray(d_test, np.float32))[None]).to(dev)
    _, _, visib = hip_lib.gt_visibility(meshes, torch.full((1,), d_gt.renderer.obj_index[d_gt.obj_id], dtype=torch.int32, device=dev),
                                        torch.zeros(1, dtype=torch.int32, device=dev), T(d_gt.R, 9), T(d_gt.t, 3), T(d_gt.K, 9), depth,
                                        float(delta), want_masks=True)
    return visib[0].cpu().numpy() > 0


def estimate_visib_mask_est(d_test, d_est, visib_gt, delta, visib_mode="bop19"):
    raise NotImplementedError("pysixd.visibility.estimate_visib_mask_est is not served on its own: the estimate's visibility is part of "
                              "pysixd.pose_error.vsd (hip_lib.vsd_counts)")


def _estimate_visib_mask(d_test, d_model, delta, visib_mode="bop19"):
    raise NotImplementedError("pysixd.visibility._estimate_visib_mask is not served on distance images: use estimate_visib_mask_gt with a GtPose")
