"""Sharding, record ordering, the one collective and the BOP writers: everything that touches pose records f32[n,16]
(R(9) | t(3, metres) | score | obj | roi_id | valid) or the order of the ROIs behind them, and nothing of the device library."""
from __future__ import annotations

import torch
import torch.distributed as dist


def shard_range(n: int, rank: int, world: int):
    """Contiguous ROI shard of rank ``rank`` — InferenceSampler's rule (core/utils/my_distributed_sampler.py:
    181-194) at ROI granularity: ceil(n/world)-sized blocks, the last ranks may get fewer (or none)."""
    shard = (n - 1) // world + 1 if n > 0 else 0
    begin = min(shard * rank, n)
    end = min(shard * (rank + 1), n)
    return begin, end


def class_sorted_order(roi_cls):
    """within a rank ROIs run sorted by class (consecutive 256-row tiles of the class-sliced output layer
    then share a weight slice, consecutive refine workgroups a mesh), the original index travels in the record.  Returns the
    STABLE permutation ``order`` with ``roi_cls[order]`` non-decreasing — ROIs of one class keep their detection order, like
    the reference's per-object ordering of load_detections_into_dataset (dataset_utils.py:202-227)."""
    import numpy as np

    if isinstance(roi_cls, torch.Tensor):
        return torch.sort(roi_cls.reshape(-1), stable=True).indices
    return np.argsort(np.asarray(roi_cls).reshape(-1), kind="stable")


# The detections dict of ``batch_data_test_gpu`` — which entries are per ROI and which are not is a CONTRACT, not a guess:
PER_ROI_DETECTION_KEYS = ("bbox", "im_idx", "roi_cls", "score", "time", "roi_id", "det_id", "scene_im_id", "inst_id")
GLOBAL_DETECTION_KEYS = ("extents", "obj_ids", "model_points", "sym_infos")   # per class / per dataset: never permuted


def sort_detections_by_class(detections: dict, roi_id_base: int = 0, extra_per_roi_keys=(), extra_global_keys=()):
    """-> (detections with every per-ROI entry permuted into class order, roi_id i32[n] = ``roi_id_base`` + the position the
    ROI had before).

    Per-ROI entries: ``PER_ROI_DETECTION_KEYS`` + ``extra_per_roi_keys`` (arrays, tensors or lists whose leading dimension is
    the number of ROIs — anything else under such a key raises) and ``cam`` when it is [n,3,3].  Passed through untouched:
    ``GLOBAL_DETECTION_KEYS`` + ``extra_global_keys``, a shared ``cam`` [3,3], scalars, strings, None.  Any OTHER entry whose
    leading dimension happens to equal the number of ROIs is ambiguous (a per-class table when n == number of classes?) and
    raises ``KeyError`` naming the two arguments that resolve it — nothing is reordered on a guess.  Sorting the DETECTIONS
    costs nothing on the device: the crop kernel reads its ROI parameters in the new order, no ROI tensor is ever permuted."""
    import numpy as np

    order = class_sorted_order(np.asarray(detections["roi_cls"]))
    out = dict(detections)
    n = len(order)
    per_roi = set(PER_ROI_DETECTION_KEYS) | set(extra_per_roi_keys)
    glob = set(GLOBAL_DETECTION_KEYS) | set(extra_global_keys)

    def lead(v):
        if isinstance(v, torch.Tensor):
            return v.shape[0] if v.dim() >= 1 else None
        if isinstance(v, (str, bytes)) or v is None or np.isscalar(v):
            return None
        if isinstance(v, (list, tuple)):
            return len(v)
        a = np.asarray(v)
        return a.shape[0] if a.ndim >= 1 else None

    def permuted(v):
        if isinstance(v, torch.Tensor):
            return v[torch.as_tensor(order, device=v.device)]
        if isinstance(v, (list, tuple)) and not isinstance(v, np.ndarray) and any(isinstance(e, (str, bytes)) for e in v):
            return [v[i] for i in order]
        return np.asarray(v)[order]

    for k, v in detections.items():
        if k in glob:
            continue
        if k == "cam":
            nd = v.dim() if isinstance(v, torch.Tensor) else np.asarray(v).ndim
            if nd == 3:
                if lead(v) != n:
                    raise ValueError(f"detections['cam'] is per ROI ([n,3,3]) but has {lead(v)} entries for {n} ROIs")
                out[k] = permuted(v)
            continue
        if k in per_roi:
            if v is None:
                continue
            if lead(v) != n:
                raise ValueError(f"detections[{k!r}] is a per-ROI entry but has leading dimension {lead(v)} for {n} ROIs")
            out[k] = permuted(v)
        elif lead(v) == n:
            raise KeyError(f"detections[{k!r}] has as many entries as there are ROIs ({n}) but is neither a known per-ROI key nor a "
                           "known global one: pass it in extra_per_roi_keys (to be permuted with the ROIs) or extra_global_keys")
    return out, (roi_id_base + order).astype(np.int32)


def records_in_roi_order(rec: torch.Tensor) -> torch.Tensor:
    """Valid records of a (gathered) block ordered by their ``roi_id`` column — undoes the per-rank class sort and drops the
    padding rows of ``gather_records``."""
    rec = rec[rec[:, 15] > 0.5]
    return rec[torch.sort(rec[:, 14], stable=True).indices]


PAD_ROI_ID = -1.0       # roi_id column of gather_records' padding rows


def gather_records(rec: torch.Tensor, n_local_max: int, group=None, dst: int | None = None, single_rank_collective: bool = False):
    """The one collective of the inference path (gdrn_evaluator.py:575-585 / my_comm.py:70-171): instead of
    pickling Python dicts into byte tensors (size all-gather + padded byte all-gather), every rank contributes a
    fixed-shape f32[n_local_max,16] block (``valid`` = 0 on padding rows) to ONE all_gather — 64 B per ROI,
    latency-bound on xGMI.  Returns f32[world*n_local_max,16] on every rank.

    Padding rows carry ``roi_id`` = ``PAD_ROI_ID`` (-1) and ``valid`` = 0.  ``dst`` is a rank of ``group`` (group-local).

    ``single_rank_collective``: run the collective even in a one-rank group (``bench.py --force-dist``: what a 1-GPU box can show
    of the path).  ``dst``: gather to that rank only (``my_comm.gather``, my_comm.py:119-171; the reference's ``evaluate`` lets only the main
    process go on to write the results, gdrn_evaluator.py:581-582): rank ``dst`` gets the block, every other rank ``None``."""
    if rec.shape[0] < n_local_max:
        pad = torch.zeros((n_local_max - rec.shape[0], 16), dtype=rec.dtype, device=rec.device)
        pad[:, 14] = PAD_ROI_ID                  # padding says so itself: no real ROI has a negative id
        rec = torch.cat([rec, pad], 0)
    if not (dist.is_available() and dist.is_initialized()):
        return rec
    world = dist.get_world_size(group)
    if world == 1 and not single_rank_collective:     # bench.py --force-dist sends a one-rank group's records through the collective
        return rec
    rec = rec.contiguous()
    if dst is not None:                                    # dst = a rank OF ``group`` (group-local, like every index of this function)
        mine = dist.get_rank(group) == dst
        parts = [torch.empty_like(rec) for _ in range(world)] if mine else None
        dst_global = dist.get_global_rank(group, dst) if group is not None else dst      # dist.gather's dst is a GLOBAL rank
        dist.gather(rec, parts, dst=dst_global, group=group)      # RCCL: world - 1 point-to-point receives on rank dst
        return torch.cat(parts, 0) if mine else None
    if dist.get_backend(group) == "gloo":  # CPU tests: list form
        parts = [torch.empty_like(rec) for _ in range(world)]
        dist.all_gather(parts, rec, group=group)
        return torch.cat(parts, 0)
    out = torch.empty((world * n_local_max, 16), dtype=rec.dtype, device=rec.device)
    dist.all_gather_into_tensor(out, rec, group=group)  # RCCL ncclAllGather over xGMI
    return out


def records_to_bop(rec: torch.Tensor, scene_im_ids, obj_ids, times=None):
    """BOP result dicts as ``pose_prediction_to_json`` writes them (gdrn_evaluator.py:636-665): R flattened row-major
    (``to_list(rot)``), t in mm."""
    rec = rec.detach().cpu()
    results = []
    for r in rec:
        if r[15] < 0.5:
            continue
        i = int(r[14])
        scene_id, im_id = scene_im_ids[i].split("/")
        results.append({
            "scene_id": scene_id, "im_id": int(im_id), "obj_id": int(obj_ids[int(r[13])]), "score": float(r[12]),
            "R": r[:9].tolist(), "t": (1000.0 * r[9:12]).tolist(),
            "time": float(times[i]) if times is not None else -1.0,
        })
    return results


BOP_CSV_HEADER = "scene_id,im_id,obj_id,score,R,t,time"


def save_bop_csv(results, path: str) -> None:
    """The BOP results file of ``save_and_eval_results`` (core/gdrn_modeling/engine/test_utils.py:33-52): one header line,
    then one line per estimate with R (9 values) and t (3 values, mm) space-separated inside their comma fields, every
    value formatted with ``"{}".format`` like the reference's ``_to_str``."""
    keys = BOP_CSV_HEADER.split(",")

    def to_str(item):
        return " ".join("{}".format(e) for e in item) if isinstance(item, (list, tuple)) else "{}".format(item)

    with open(path, "w") as f:
        f.write(BOP_CSV_HEADER + "\n")
        for res in results:
            f.write(",".join(to_str(res[k]) for k in keys) + "\n")
