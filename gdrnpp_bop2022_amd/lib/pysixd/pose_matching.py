"""Matching of pose estimates to ground-truth poses, with the signatures and results of the reference's
lib/pysixd/pose_matching.py:9-159 (host code; written from the behaviour: greedy by falling score)."""
from __future__ import annotations


def match_poses(errs, error_ths, max_ests_count=0, gt_valid_mask=None):
    """errs: list of ``{"est_id", "score", "errors": {gt_id: [error elements]}}`` of one object in one image -> list of matches
    ``{"est_id", "gt_id", "score", "error", "error_norm"}``, one per estimate that found a ground truth.

    The estimates are visited by falling score (a stable sort: equal scores keep their order in ``errs``), the first
    ``max_ests_count`` of them when that is positive.  An estimate takes, among the valid ground truths nobody has taken yet,
    visited in the order of its ``errors``, the one whose EVERY error element is strictly below the best so far, which starts
    at the thresholds; a ground truth is taken at most once."""
    order = sorted(errs, key=lambda e: e["score"], reverse=True)
    if max_ests_count > 0:
        order = order[:max_ests_count]
    n_elems = len(list(error_ths))
    matches, taken = [], []
    for est in order:
        best_gt, best = -1, list(error_ths)
        for gt_id, error in est["errors"].items():
            valid = not gt_valid_mask or gt_valid_mask[gt_id]
            if valid and gt_id not in taken and all(error[i] < best[i] for i in range(n_elems)):
                best_gt, best = gt_id, error
        if best_gt >= 0:
            taken.append(best_gt)
            matches.append({"est_id": est["est_id"], "gt_id": best_gt, "score": est["score"], "error": best,
                            "error_norm": [best[i] / float(error_ths[i]) for i in range(n_elems)]})
    return matches


def match_poses_scene(scene_id, scene_gt, scene_gt_valid, scene_errs, correct_th, n_top):
    """One record per ground truth of the scene's images (``scene_gt``: {im_id: [{"obj_id"}, ...]}), in image and annotation order:
    ``{"scene_id", "im_id", "obj_id", "gt_id", "est_id", "score", "error", "error_norm", "valid"}`` with -1 in the four estimate
    fields of a ground truth no estimate was matched to.  Objects are matched one by one with ``match_poses``."""
    by_im_obj = {}
    for e in scene_errs:
        by_im_obj.setdefault(e["im_id"], {}).setdefault(e["obj_id"], []).append(e)
    out = []
    for im_id, im_gts in scene_gt.items():
        im_matches = [{"scene_id": scene_id, "im_id": im_id, "obj_id": gt["obj_id"], "gt_id": gt_id, "est_id": -1, "score": -1,
                       "error": -1, "error_norm": -1, "valid": scene_gt_valid[im_id][gt_id]} for gt_id, gt in enumerate(im_gts)]
        for obj_id in set(gt["obj_id"] for gt in im_gts):
            errs = by_im_obj.get(im_id, {}).get(obj_id)
            if errs is None:
                continue
            for m in match_poses(errs, correct_th, n_top, scene_gt_valid[im_id]):
                g = im_matches[m["gt_id"]]
                g["est_id"], g["score"], g["error"], g["error_norm"] = m["est_id"], m["score"], m["error"], m["error_norm"]
        out += im_matches
    return out
