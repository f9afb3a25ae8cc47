"""``GDRN_EvaluatorCustom`` — the reference's default evaluator (core/gdrn_modeling/engine/gdrn_custom_evaluator.py; chosen at
engine.py:98 unless ``VAL.USE_BOP``): every prediction is compared with its ground-truth pose and a recall (or precision) table of
``ad_2/5/10``, ``rete_*``, ``re_*``, ``te_*``, ``proj_*`` per object is written.

Same protocol and the same result dicts as the reference class; built the way ``GDRN_Evaluator`` is here:

    reference, per (object, image) pair:  te / get_closest_rot / re / arp_2d / add — or adi, a scipy cKDTree built and
                                          queried per prediction — in CPU NumPy
    here, per dataset:                    every pair that has a ground truth and a prediction -> flat arrays -> ONE
                                          ``hip_lib.pose_errors`` call (csrc/pose_error.hip) -> ONE read-back of f64[pairs,4]
                                          -> the table, a host-only function of those errors (``summarize_errors``)

The dataset registry is not rebuilt: its facts are constructor arguments.  Deviations, on purpose: (1) the batch is indexed with the
running ROI index — the reference's ``out_rots[inst_i]`` (:221) equals it only because its batches hold one image; (2) ``score``
is a float; (3) the ``_preds.pkl`` cache of ``VAL.EVAL_CACHED / EVAL_PRINT_ONLY`` is not kept; (4) pickles are plain ``pickle``.
"""
from __future__ import annotations

import logging
import os
import pickle
import time
from collections import OrderedDict

import numpy as np
import torch

from .. import hip_lib
from .gdrn_evaluator import GDRN_Evaluator

logger = logging.getLogger(__name__)

ERROR_NAMES = ("ad", "re", "te", "proj")
# yapf: disable
METRIC_NAMES = (
    "ad_2", "ad_5", "ad_10",
    "rete_2", "rete_5", "rete_10",
    "re_2", "re_5", "re_10",
    "te_2", "te_5", "te_10",
    "proj_2", "proj_5", "proj_10",
)
# yapf: enable


def reorganize_preds(predictions):
    """gdrn_custom_evaluator.py:607-620: list of result dicts -> ``preds[obj_name][file_name] = [dict without the two keys]``."""
    res = OrderedDict()
    for d in predictions:
        per_file = res.setdefault(d["cls_name"], OrderedDict())
        per_file.setdefault(d["file_name"], []).append({k: v for k, v in d.items() if k not in ("cls_name", "file_name")})
    return res


def match_pairs(gts, predictions, obj_names):
    """The walk of ``_eval_predictions`` (:655-682) without its arithmetic: for every object of ``gts`` that has predictions, its
    ground truths in order, each paired with the FIRST prediction of that object in that image.
    -> (slots, pairs): ``slots[obj_name]`` lists, per ground-truth image, the index into ``pairs`` or None (no prediction);
    ``pairs`` lists (label, R_est, t_est, R_gt, t_gt, K)."""
    slots, pairs = OrderedDict(), []
    for obj_name in gts:
        if obj_name not in predictions:
            continue
        label = obj_names.index(obj_name)
        cur = slots[obj_name] = []
        obj_preds = predictions[obj_name]
        for file_name, gt in gts[obj_name].items():
            if file_name not in obj_preds:
                cur.append(None)
                continue
            pred = obj_preds[file_name][0]      # assume only one instance for each object in an image (:678)
            cur.append(len(pairs))
            pairs.append((label, pred["R"], pred["t"], gt["R"], gt["t"], gt["K"]))
    return slots, pairs


def summarize_errors(slots, pair_errors, diameters, obj_names, eval_precision=False):
    """Host-only tail of ``_eval_predictions`` (:727-793) / ``_eval_predictions_precision`` (:915-982): ``pair_errors`` f64[pairs,4]
    = ad, re, te, proj in the order of ``match_pairs`` -> (errors, rates, table text).  Strict ``<`` everywhere; an image without a
    prediction counts 0.0 for every recall and is skipped for precision."""
    pair_errors = np.asarray(pair_errors, np.float64).reshape(-1, 4)
    errors, rates = OrderedDict(), OrderedDict()
    for obj_name, obj_slots in slots.items():
        diameter = diameters[obj_names.index(obj_name)]
        rate = rates[obj_name] = OrderedDict((m, []) for m in METRIC_NAMES)
        err = errors[obj_name] = OrderedDict((e, []) for e in ERROR_NAMES)
        for slot in obj_slots:
            if slot is None:
                if not eval_precision:
                    for m in METRIC_NAMES:
                        rate[m].append(0.0)
                continue
            ad, r_error, t_error, proj = pair_errors[slot]
            for name, value in zip(ERROR_NAMES, (ad, r_error, t_error, proj)):
                err[name].append(value)
            for pct, deg_px, metres in ((2, 2, 0.02), (5, 5, 0.05), (10, 10, 0.1)):
                rate[f"ad_{pct}"].append(float(ad < metres * diameter))
                rate[f"rete_{pct}"].append(float(r_error < deg_px and t_error < metres))
                rate[f"re_{pct}"].append(float(r_error < deg_px))
                rate[f"te_{pct}"].append(float(t_error < metres))
                rate[f"proj_{pct}"].append(float(proj < deg_px))
    return errors, rates, format_table(errors, rates)


def format_table(errors, rates):
    """:752-793 — the table of the rates in percent and the mean re / te rows, ``tabulate(..., tablefmt="plain")``."""
    from tabulate import tabulate

    names = sorted(rates.keys())
    big_tab = [["objects"] + names + [f"Avg({len(names)})"]]
    for metric_name in METRIC_NAMES:
        line, this_line_res = [metric_name], []
        for obj_name in names:
            res = rates[obj_name][metric_name]
            if len(res) > 0:
                line.append(f"{100 * np.mean(res):.2f}")
                this_line_res.append(np.mean(res))
            else:
                line.append(0.0)
                this_line_res.append(0.0)
        if len(names) > 0:
            line.append(f"{100 * np.mean(this_line_res):.2f}")
        big_tab.append(line)
    for error_name in ("re", "te"):
        line, this_line_res = [error_name], []
        for obj_name in names:
            res = errors[obj_name][error_name]
            if len(res) > 0:
                line.append(f"{np.mean(res):.2f}")
                this_line_res.append(np.mean(res))
            else:
                line.append(float("nan"))
                this_line_res.append(float("nan"))
        if len(names) > 0:
            line.append(f"{np.mean(this_line_res):.2f}")
        big_tab.append(line)
    return tabulate(big_tab, tablefmt="plain")


class GDRN_EvaluatorCustom(GDRN_Evaluator):
    """Drop-in for the reference class of the same name.  What the reference reads from the dataset registry is passed in:
    ``obj_names`` / ``obj2id`` as for ``GDRN_Evaluator``; ``models`` — the EVAL models (``data_ref.model_eval_dir``) as a
    ``hip_lib.MeshSet`` in class order; ``diameters`` in metres, class order; ``gts`` — ``{obj_name: {file_name: {"R", "t",
    "K"}}}``, what ``get_gts`` builds (:588-605); ``sym_infos`` — per class None or K x 3 x 3 (``_metadata.sym_infos``);
    ``meshes`` — the render models of the depth refinement, handed to ``GdrnHipPost``."""

    def __init__(self, cfg, dataset_name=None, distributed=False, output_dir=None, train_objs=None, *, obj_names, obj2id, models,
                 diameters, gts, sym_infos=None, meshes: "hip_lib.MeshSet | None" = None):
        super().__init__(cfg, dataset_name, distributed, output_dir, train_objs, obj_names=obj_names, obj2id=obj2id, meshes=meshes)
        self.models = models
        self.diameters = [float(d) for d in diameters]
        self.gts = gts
        self.sym_infos = list(sym_infos) if sym_infos is not None else [None] * len(self.obj_names)
        assert models.n_obj == len(self.obj_names) == len(self.diameters) == len(self.sym_infos)
        val = cfg.get("VAL", {})
        self.eval_precision = bool(val.get("EVAL_PRECISION", False))
        self.sym_objs = list(cfg.get("DATASETS", {}).get("SYM_OBJS", []))

    def process(self, inputs, outputs, out_dict):
        """Appends the reference's result dict ``{"cls_name", "file_name", "score", "R", "t", "time"}`` per ROI (:555-567): R 3x3, t
        in metres.  The poses come from ``GdrnHipPost.process`` exactly as in ``GDRN_Evaluator.process``."""
        start = time.perf_counter()
        rec = self._pose_records(inputs, out_dict)
        if rec is None:
            return
        spent = time.perf_counter() - start
        out_i = -1
        for _input, output in zip(inputs, outputs):
            results = []
            for inst_i in range(len(_input["roi_cls"])):
                out_i += 1
                _, cls_name = self._maybe_adapt_label_cls_name(_input["roi_cls"][inst_i])
                if cls_name is None:
                    continue
                r = rec[out_i]
                results.append({"cls_name": cls_name, "file_name": _input["file_name"][inst_i], "score": float(_input["score"][inst_i]),
                                "R": r[:9].reshape(3, 3).copy(), "t": r[9:12].copy(), "time": output["time"]})
            output["time"] += spent
            for item in results:
                item["time"] = output["time"]
            self._predictions.extend(results)

    def evaluate(self):
        """:569-585."""
        if not self._gather_predictions():
            return
        if isinstance(self._predictions, list):
            self._predictions = reorganize_preds(self._predictions)
        return self._eval_predictions(self.eval_precision)

    def _symmetry_tables(self, device):
        """``symmetric`` u8[n_obj] from ``DATASETS.SYM_OBJS``; the symmetry lists flat, with offsets (None, None when all are empty)."""
        flags = [1 if name in self.sym_objs else 0 for name in self.obj_names]
        rots, off = [], [0]
        for flag, info in zip(flags, self.sym_infos):
            if flag and info is not None:
                if isinstance(info, torch.Tensor):
                    info = info.cpu().numpy()
                rots.append(np.asarray(info, np.float64).reshape(-1, 3, 3))     # a single 3x3 is one symmetry (pose_utils.py:483)
            off.append(off[-1] + (len(rots[-1]) if flag and info is not None else 0))
        symmetric = torch.tensor(flags, dtype=torch.uint8, device=device)
        if off[-1] == 0:
            return symmetric, None, None
        return (symmetric, torch.from_numpy(np.concatenate(rots, 0).reshape(-1, 9)).to(device),
                torch.tensor(off, dtype=torch.int32, device=device))

    def pair_errors(self, pairs) -> np.ndarray:
        """All pairs of ``match_pairs`` in one kernel call and one read-back -> f64[pairs,4]."""
        if not pairs:
            return np.zeros((0, 4), np.float64)
        device = self.models.verts.device
        cols = [np.stack([np.asarray(p[k], np.float64).reshape(-1) for p in pairs]) for k in range(1, 6)]
        obj = torch.tensor([p[0] for p in pairs], dtype=torch.int32, device=device)
        R_est, t_est, R_gt, t_gt, K = (torch.from_numpy(np.ascontiguousarray(c)).to(device) for c in cols)
        symmetric, sym_rots, sym_off = self._symmetry_tables(device)
        out = hip_lib.pose_errors(self.models, obj, R_est, t_est, R_gt, t_gt, K, sym_rots, sym_off, symmetric)
        return out.cpu().numpy()

    def _eval_predictions(self, eval_precision=False):
        """:622-809 (recall) / :811-1004 (precision)."""
        slots, pairs = match_pairs(self.gts, self._predictions, self.obj_names)
        errors, rates, table = summarize_errors(slots, self.pair_errors(pairs), self.diameters, self.obj_names, eval_precision)
        logger.info("%s\n%s", "precisions" if eval_precision else "recalls", table)
        if self._output_dir:
            os.makedirs(self._output_dir, exist_ok=True)
            stem = os.path.join(self._output_dir, f"{self.cfg.EXP_ID.replace('_', '-')}_{self.dataset_name}")
            with open(stem + "_errors.pkl", "wb") as f:
                pickle.dump(errors, f)
            with open(stem + ("_precisions.pkl" if eval_precision else "_recalls.pkl"), "wb") as f:
                pickle.dump(rates, f)
            with open(stem + ("_tab_precisions.txt" if eval_precision else "_tab.txt"), "w") as f:     # :800, :994-997
                f.write("{}\n".format(table))
        if self._distributed:
            logger.warning("\n The current evaluation on multi-gpu might be incorrect, run with single-gpu instead.")
        return {}

    def _eval_predictions_precision(self):
        return self._eval_predictions(True)


def build_evaluator(cfg, dataset_name=None, distributed=False, output_dir=None, train_objs=None, *, obj_names, obj2id, meshes=None,
                    **custom):
    """The reference's selection rule (engine.py:98): ``GDRN_Evaluator`` when ``VAL.USE_BOP``, else ``GDRN_EvaluatorCustom`` (which
    needs ``models``, ``diameters``, ``gts`` and optionally ``sym_infos`` in ``custom``)."""
    if cfg.get("VAL", {}).get("USE_BOP", False):
        return GDRN_Evaluator(cfg, dataset_name, distributed, output_dir, train_objs, obj_names=obj_names, obj2id=obj2id, meshes=meshes)
    return GDRN_EvaluatorCustom(cfg, dataset_name, distributed, output_dir, train_objs, obj_names=obj_names, obj2id=obj2id,
                                meshes=meshes, **custom)
