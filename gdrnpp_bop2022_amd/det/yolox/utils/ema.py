"""``ModelEMA``: the exponential moving average of everything in a model's state dict, the model every shipped detector config evaluates
and checkpoints (``train.ema=True``: ``ModelEMA(model, 0.9998)``).

``update(model)`` has two paths with the same arithmetic, ``v *= d; v += (1.0 - d) * m`` per floating-point state entry.  Pairs of dense
fp32 tensors of one layout on a GPU are updated by ONE launch per device of the multi-tensor kernel (``hip_lib.ema_update``,
csrc/model_ema.hip): ``e = fadd(fmul(e, d32), fmul(omd32, m))`` with ``d32 = float32(d)`` and ``omd32 = float32(1.0 - d)``, the subtraction
in double, which is what torch's two statements compute on fp32 tensors bit for bit.  The device tables are built once and reused; the
two coefficients travel as launch arguments.  Every other floating-point pair (fp16, fp64, CPU, differing layouts) runs the two statements
on torch operators; on a GPU those are counted in ``torch_path_tensors`` the way ``solver.Ranger`` counts its own.  Entries that are not
floating point (``num_batches_tracked``) keep the copy's value, as in the reference.

What is not here: hipGraph capture of the update (the decay is a launch argument, a captured graph would freeze it)."""
from __future__ import annotations

import math
from copy import deepcopy

import torch
import torch.nn as nn

from .... import hip_lib

__all__ = ["ModelEMA", "is_parallel", "torch_path_tensors", "last_torch_path"]

_TORCH_PATH_TENSORS = 0
_LAST_TORCH_PATH = None


def torch_path_tensors() -> int:
    """State entries updated on torch operators although the EMA's tensor lives on a GPU, so far in this process."""
    return _TORCH_PATH_TENSORS


def last_torch_path():
    return _LAST_TORCH_PATH


def _note_torch_path(key, v, m):
    global _TORCH_PATH_TENSORS, _LAST_TORCH_PATH
    _TORCH_PATH_TENSORS += 1
    _LAST_TORCH_PATH = (f"ModelEMA.update: {key} {tuple(v.shape)} {v.dtype} on {v.device} updated with torch operators (the pair is not two dense "
                        f"fp32 tensors of one layout on one GPU: the model's is {m.dtype} on {m.device}, strides {tuple(v.stride())} / {tuple(m.stride())})")


def is_parallel(model) -> bool:
    """Whether ``model`` is a DataParallel / DistributedDataParallel wrapper (its ``.module`` is the model)."""
    return isinstance(model, (nn.parallel.DataParallel, nn.parallel.DistributedDataParallel))


def _copy_without_caches(model):
    """``deepcopy(model)`` without the library's per-module attachments (``weight_cache.module_cache`` entries: folded and packed weights
    tagged with the ORIGINAL parameters' storage, stale on arrival; the detector's activation buffers): the copy gets none and fills
    its own on its first forward.  They are kept out of the copy through deepcopy's memo, so no device tensor is cloned to be dropped."""
    memo = {}
    for mod in model.modules():
        for k, v in mod.__dict__.items():
            if k.startswith("_gdrnpp_"):
                memo[id(v)] = None
    ema = deepcopy(model, memo)
    for mod in ema.modules():
        for k in [k for k in mod.__dict__ if k.startswith("_gdrnpp_")]:
            del mod.__dict__[k]
    return ema


class ModelEMA:
    """The reference's class: ``ema`` (the averaged copy, eval mode, no gradients), ``updates`` (set it to the start iteration on resume),
    ``decay`` (``x -> decay * (1 - exp(-x / 2000))``, the ramp that helps early epochs) and ``update(model)``.

    ``use_kernel``: None (default) = the HIP kernel wherever a pair qualifies; False = torch operators everywhere, nothing counted (the
    reference's own statements: the baseline of tools/model_ema_microbench.py and of the two-path tests)."""

    def __init__(self, model, decay=0.9999, updates=0, use_kernel=None):
        self.ema = _copy_without_caches(model.module if is_parallel(model) else model).eval()
        self.updates = updates
        self.decay = lambda x: decay * (1 - math.exp(-x / 2000))
        for p in self.ema.parameters():
            p.requires_grad_(False)
        self.use_kernel = use_kernel
        self._tables = {}        # device -> hip_lib.EmaTables

    def update(self, model):
        with torch.no_grad():
            self.updates += 1
            d = self.decay(self.updates)
            # keep_vars: the parameters and buffers themselves, not a detached alias of each (a third of the walk's host time, which is
            # what an update costs once the device's share is one launch)
            msd = (model.module if is_parallel(model) else model).state_dict(keep_vars=True)
            batches = {}         # device -> (EMA tensors, model tensors)
            for k, v in self.ema.state_dict(keep_vars=True).items():
                if not v.dtype.is_floating_point:
                    continue
                m = msd[k]           # under no_grad: nothing below records a graph, so no detach() either
                if self.use_kernel is not False and v.is_cuda:
                    if hip_lib.ema_tensor_ok(v, m):
                        b = batches.get(v.device)
                        if b is None:
                            b = batches[v.device] = ([], [])
                        b[0].append(v), b[1].append(m)
                        continue
                    _note_torch_path(k, v, m)
                v *= d
                v += (1.0 - d) * m
            for device, (es, ms) in batches.items():
                tables = self._tables.get(device)
                if tables is None:
                    tables = self._tables[device] = hip_lib.EmaTables(device)
                with torch.cuda.device(device):
                    hip_lib.ema_update(tables, es, ms, d, 1.0 - d, validate=False)      # every pair has just passed ema_tensor_ok
                # the kernel wrote through raw pointers: advance the version counters that weight_cache.weight_tag keys on (es holds the
                # copy's parameters and buffers themselves)
                torch.autograd.graph.increment_version(es)

    def close(self):
        """Release the kernel path's device tables and pinned staging buffers now, with the device idle.  The next ``update()`` builds
        them again."""
        for tables in self._tables.values():
            tables.close()
        self._tables = {}
