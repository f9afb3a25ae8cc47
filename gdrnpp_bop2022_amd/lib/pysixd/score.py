"""Recall of the 6D object localization task, with the signature and the result fields of the reference's
lib/pysixd/score.py:49-155 (host code)."""
from __future__ import annotations

import logging

import numpy as np

logger = logging.getLogger(__name__)


def calc_recall(tp_count, targets_count):
    return 0.0 if targets_count == 0 else tp_count / float(targets_count)


def calc_localization_scores(scene_ids, obj_ids, matches, n_top, do_print=True):
    """matches: the records of ``pose_matching.match_poses_scene`` -> ``{"recall", "obj_recalls", "mean_obj_recall", "scene_recalls",
    "mean_scene_recall", "gt_count", "targets_count", "tp_count"}``.

    Targets are the valid ground truths, counted per (object, scene, image); with ``n_top`` > 0 an image contributes at most
    ``n_top`` of an object (one target per image in the single-instance task, however many instances it shows).  True positives are
    the valid ground truths with a matched estimate."""
    insts = {o: {s: {} for s in scene_ids} for o in obj_ids}
    for m in matches:
        if m["valid"]:
            per_im = insts[m["obj_id"]][m["scene_id"]]
            per_im[m["im_id"]] = per_im.get(m["im_id"], 0) + 1

    tars, obj_tars, scene_tars = 0, {o: 0 for o in obj_ids}, {s: 0 for s in scene_ids}
    for o, per_scene in insts.items():
        for s, per_im in per_scene.items():
            counts = list(per_im.values())
            count = sum(np.minimum(n_top, counts)) if n_top > 0 else sum(counts)
            tars += count
            obj_tars[o] += count
            scene_tars[s] += count

    tps, obj_tps, scene_tps = 0, {o: 0 for o in obj_ids}, {s: 0 for s in scene_ids}
    for m in matches:
        if m["valid"] and m["est_id"] != -1:
            tps += 1
            obj_tps[m["obj_id"]] += 1
            scene_tps[m["scene_id"]] += 1

    obj_recalls = {o: calc_recall(obj_tps[o], obj_tars[o]) for o in obj_ids}
    scene_recalls = {s: float(calc_recall(scene_tps[s], scene_tars[s])) for s in scene_ids}
    scores = {
        "recall": float(calc_recall(tps, tars)),
        "obj_recalls": obj_recalls,
        "mean_obj_recall": float(np.mean(list(obj_recalls.values()))),
        "scene_recalls": scene_recalls,
        "mean_scene_recall": float(np.mean(list(scene_recalls.values()))),
        "gt_count": len(matches),
        "targets_count": int(tars),
        "tp_count": int(tps),
    }
    if do_print:
        logger.info("GT count: %d, target count: %d, TP count: %d, recall: %.4f, mean object recall: %.4f, mean scene recall: %.4f",
                    scores["gt_count"], scores["targets_count"], scores["tp_count"], scores["recall"], scores["mean_obj_recall"],
                    scores["mean_scene_recall"])
    return scores
