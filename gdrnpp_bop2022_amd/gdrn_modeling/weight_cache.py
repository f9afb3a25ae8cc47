"""Eval-time caches of derived weights (packed GEMM images, folded BatchNorm, re-laid-out kernels): one dict per module, every
entry tagged with the identity of the parameters it was built from and filled in a way that is safe for every compute stream."""
from __future__ import annotations

import torch


def module_cache(mod) -> dict:
    """The derived-weight cache dict of ``mod`` (kept in its ``__dict__``: no parameter, no buffer, not in the state dict)."""
    return mod.__dict__.setdefault("_gdrnpp_cache", {})


def weight_tag(*tensors):
    """Identity of parameter values for the eval-time derived-weight caches: storage, in-place version counter (bumped by
    load_state_dict / optimiser steps) and device of every tensor the cached form is derived from."""
    return tuple((t.data_ptr(), t._version, t.device) for t in tensors if t is not None)


_CACHE_FILLS = 0


def cache_fills() -> int:
    """Derived-weight cache entries built so far by this process (tests: a warm model fills none)."""
    return _CACHE_FILLS


def cached(cache: dict, key: str, tag, build, on: torch.Tensor | None = None):
    """``cache[key]`` = (tag, *build()) — rebuilt when ``tag`` (weight_tag of the parameters it derives from) changed.

    Consecutive steps run on DIFFERENT compute streams (engine.StepStreams) and share these per-module entries, so a fill is
    made safe for every stream, not just the one that happens to touch the layer first: the device is drained before the old
    entry is dropped (its memory goes back to the filling stream's pool while another stream's step might still read it) and the
    filling stream is drained before the new entry becomes visible (the pack kernels are complete when the next step, on the
    other stream, hits the cache).  Two host waits per weight per process lifetime (+ one per load_state_dict); never inside a
    hipGraph capture (engine.GraphedInference fills the caches with eager passes first; a fill under capture is captured as is)."""
    global _CACHE_FILLS
    hit = cache.get(key)
    if hit is not None and hit[0] == tag:
        return hit
    gpu = on is not None and on.is_cuda and not torch.cuda.is_current_stream_capturing()
    if gpu:
        torch.cuda.synchronize(on.device)
    hit = cache[key] = (tag,) + tuple(build())
    if gpu:
        torch.cuda.current_stream(on.device).synchronize()
    _CACHE_FILLS += 1
    return hit
