"""The training side behind ``loss.backward()``: the Ranger optimiser (RAdam + Lookahead + gradient centralisation, the optimiser of every
shipped GDRN config), the ``flat_and_anneal`` learning-rate schedule and the builders that read ``cfg.SOLVER``.

``Ranger.step()`` has two paths with the same arithmetic.  Contiguous fp32 parameters on the GPU are updated by ONE launch of the
multi-tensor kernel (``hip_lib.ranger_step``, csrc/ranger.hip): the per-tensor table of pointers, row lengths, flags and coefficients is
rebuilt on the host every step (gradient pointers change with ``zero_grad(set_to_none=True)``) and uploaded with one asynchronous copy;
nothing is read back.  Everything else (CPU tensors, other dtypes, non-contiguous parameters) runs the same step on torch operators, one
tensor at a time; on a GPU those are counted in ``torch_path_tensors`` the way ``hip_layers`` counts launches outside the library.

``build_model_ema`` reads ``cfg.MODEL.EMA`` and returns the loop's ``ModelEMA`` (lib/torch_utils/torch_utils.py, the detector's class).

What is not here: the ``do_train`` loop, data loading and augmentation, DDP and AMP, gradient clipping
(``CLIP_GRADIENTS.ENABLED`` raises), the reference's other optimisers and schedulers, and hipGraph capture of the step."""
from __future__ import annotations

import copy
import math
import warnings
from bisect import bisect_right

import torch

from .. import hip_lib

_TORCH_PATH_TENSORS = 0
_LAST_TORCH_PATH = None


def torch_path_tensors() -> int:
    """Parameter updates that ran on torch operators although the parameter lives on a GPU, so far in this process."""
    return _TORCH_PATH_TENSORS


def last_torch_path():
    return _LAST_TORCH_PATH


def _note_torch_path(p, why):
    global _TORCH_PATH_TENSORS, _LAST_TORCH_PATH
    _TORCH_PATH_TENSORS += 1
    _LAST_TORCH_PATH = f"Ranger.step: {tuple(p.shape)} {p.dtype} updated with torch operators ({why})"


def radam_coefficients(step: int, beta1: float, beta2: float, threshold: float):
    """(N_sma, step_size) of RAdam at ``step``, in Python floats: the length of the approximated simple moving average and the step's
    scale — the variance rectification over the bias correction of the first moment where N_sma exceeds the threshold, the bias
    correction alone where not."""
    beta2_t = beta2 ** step
    n_sma_max = 2 / (1 - beta2) - 1
    n_sma = n_sma_max - 2 * step * beta2_t / (1 - beta2_t)
    if n_sma > threshold:
        step_size = math.sqrt((1 - beta2_t) * (n_sma - 4) / (n_sma_max - 4) * (n_sma - 2) / n_sma * n_sma_max / (n_sma_max - 2)) / (1 - beta1 ** step)
    else:
        step_size = 1.0 / (1 - beta1 ** step)
    return n_sma, step_size


class Ranger(torch.optim.Optimizer):
    """Ranger with the reference's arguments, defaults, checks and state keys (``step``, ``exp_avg``, ``exp_avg_sq``, ``slow_buffer``), so
    that ``state_dict`` / ``load_state_dict`` are torch's own and a reference checkpoint's optimiser state resumes.

    ``use_kernel``: None (default) = the HIP kernel wherever a parameter qualifies; False = torch operators everywhere (the baseline of
    tools/ranger_microbench.py and the two-path tests).  ``nan_to_num``: ``SOLVER.SET_NAN_GRAD_TO_ZERO`` folded into the step —
    ``nan_to_num(grad, nan=0, posinf=1e5, neginf=-1e5)`` on the gradient as read, the gradient tensor rewritten.

    ``use_gc`` is stored and, as in the reference's ``step()``, not consulted: centralisation depends on ``gc_conv_only`` and the gradient's
    rank alone.  Unlike the reference, a centralised fp32 gradient is not written back into ``p.grad``: nothing reads it after the step."""

    def __init__(self, params, lr=1e-3, alpha=0.5, k=6, N_sma_threshhold=5, betas=(0.95, 0.999), eps=1e-5, weight_decay=0, use_gc=True,
                 gc_conv_only=False, use_kernel=None, nan_to_num=False):
        if not 0.0 <= alpha <= 1.0:
            raise ValueError(f"Invalid slow update rate: {alpha}")
        if not 1 <= k:
            raise ValueError(f"Invalid lookahead steps: {k}")
        if not lr > 0:
            raise ValueError(f"Invalid Learning Rate: {lr}")
        if not eps > 0:
            raise ValueError(f"Invalid eps: {eps}")
        defaults = dict(lr=lr, alpha=alpha, k=k, step_counter=0, betas=betas, N_sma_threshhold=N_sma_threshhold, eps=eps, weight_decay=weight_decay)
        super().__init__(params, defaults)
        self.N_sma_threshhold = N_sma_threshhold
        self.alpha = alpha
        self.k = k
        self.use_gc = use_gc
        self.gc_gradient_threshold = 3 if gc_conv_only else 1
        self.use_kernel = use_kernel
        self.nan_to_num = bool(nan_to_num)
        self._tables = {}        # device -> hip_lib.RangerTables

    def _on_kernel(self, p, grad, state):
        """Whether the kernel takes this update: the parameter dense fp32 on a GPU (``hip_lib.ranger_tensor_ok``), gradient and state laid
        out as it is.  Spelled out on attributes: this runs once per tensor per step and is most of the host's share of ``step()``.
        A refusal is counted in ``torch_path_tensors`` — except with ``use_kernel=False``, where the torch operators are what the caller
        asked for.  A fp32 state tensor that only differs in layout (a resumed checkpoint's contiguous state beside a channels_last
        weight) is copied into the parameter's layout once and stays on the kernel from then on."""
        if self.use_kernel is False or not p.is_cuda:
            return False
        f32, stride, shape, dev = torch.float32, p.stride(), p.shape, p.device
        ok = p.dtype is f32 and (p.is_contiguous() or (p.dim() == 4 and p.is_contiguous(memory_format=torch.channels_last)))
        if ok:
            for key in ("exp_avg", "exp_avg_sq", "slow_buffer"):
                t = state[key]
                if t.dtype is not f32 or t.shape != shape or t.device != dev:
                    ok = False
                    break
                if t.stride() != stride and not hip_lib.ranger_same_layout(t, p):
                    state[key] = torch.empty_like(p.data).copy_(t)
            ok = ok and grad.dtype is f32 and grad.shape == shape and grad.device == dev and (grad.stride() == stride or hip_lib.ranger_same_layout(grad, p))
        if not ok:
            _note_torch_path(p, "parameter, gradient and state are not dense fp32 tensors of one layout")
        return ok

    def _torch_step(self, p, grad, state, group, n_sma, step_size, centralise):
        if self.nan_to_num:
            torch.nan_to_num(grad, nan=0, posinf=1e5, neginf=-1e5, out=grad)
        beta1, beta2 = group["betas"]
        g32 = grad.float()
        p32 = p.data.float()
        state["exp_avg"] = state["exp_avg"].type_as(p32)
        state["exp_avg_sq"] = state["exp_avg_sq"].type_as(p32)
        exp_avg, exp_avg_sq = state["exp_avg"], state["exp_avg_sq"]
        if centralise:
            g32 = g32 - g32.mean(dim=tuple(range(1, g32.dim())), keepdim=True)
        exp_avg_sq.mul_(beta2).addcmul_(g32, g32, value=1 - beta2)
        exp_avg.mul_(beta1).add_(g32, alpha=1 - beta1)
        if group["weight_decay"] != 0:
            p32.add_(p32, alpha=-group["weight_decay"] * group["lr"])
        if n_sma > self.N_sma_threshhold:
            p32.addcdiv_(exp_avg, exp_avg_sq.sqrt().add_(group["eps"]), value=-step_size * group["lr"])
        else:
            p32.add_(exp_avg, alpha=-step_size * group["lr"])
        p.data.copy_(p32)
        if state["step"] % group["k"] == 0:
            slow = state["slow_buffer"]
            slow.add_(p.data - slow, alpha=self.alpha)
            p.data.copy_(slow)

    @torch.no_grad()
    def step(self, closure=None):
        loss = None          # as the reference: a closure is accepted and not called
        batches = {}         # device -> the lists of hip_lib.ranger_step
        on_torch = []        # parameters updated by _torch_step
        for group in self.param_groups:
            beta1, beta2 = group["betas"]
            wd_lr = -group["weight_decay"] * group["lr"] if group["weight_decay"] != 0 else 0.0
            per_step = {}        # step count -> (N_sma, step_size, flags, coefficients): tensors of a group mostly share their count
            for p in group["params"]:
                if p.grad is None:
                    continue
                grad = p.grad.data
                if grad.is_sparse:
                    raise RuntimeError("Ranger optimizer does not support sparse gradients")
                state = self.state[p]
                if len(state) == 0:
                    state["step"] = 0
                    state["exp_avg"] = torch.zeros_like(p.data, dtype=torch.float32)
                    state["exp_avg_sq"] = torch.zeros_like(p.data, dtype=torch.float32)
                    state["slow_buffer"] = torch.empty_like(p.data)
                    state["slow_buffer"].copy_(p.data)
                state["step"] += 1
                step = int(state["step"])
                hit = per_step.get(step)
                if hit is None:
                    n_sma, step_size = radam_coefficients(step, beta1, beta2, self.N_sma_threshhold)
                    flags = (hip_lib.RANGER_RECTIFIED if n_sma > self.N_sma_threshhold else 0) | (hip_lib.RANGER_LOOKAHEAD if step % group["k"] == 0 else 0) \
                        | (hip_lib.RANGER_NAN_TO_NUM if self.nan_to_num else 0)
                    hit = per_step[step] = (n_sma, step_size, flags,
                                            (beta1, beta2, 1 - beta1, 1 - beta2, group["eps"], self.alpha, wd_lr, -step_size * group["lr"]))
                centralise = grad.dim() > self.gc_gradient_threshold      # as in the reference, use_gc is kept but does not gate the step
                if not self._on_kernel(p, grad, state):
                    self._torch_step(p, grad, state, group, hit[0], hit[1], centralise)
                    on_torch.append(p)
                    continue
                row_len = p.numel() // p.shape[0] if centralise and p.numel() else 0
                b = batches.get(p.device)
                if b is None:
                    b = batches[p.device] = ([], [], [], [], [], [], [], [], [])
                b[0].append(p.data), b[1].append(grad), b[2].append(state["exp_avg"]), b[3].append(state["exp_avg_sq"])
                b[4].append(state["slow_buffer"]), b[5].append(row_len), b[6].append(hit[2]), b[7].append(hit[3]), b[8].append(p)
        for device, b in batches.items():
            tables = self._tables.get(device)
            if tables is None:
                tables = self._tables[device] = hip_lib.RangerTables(device)
            with torch.cuda.device(device):
                hip_lib.ranger_step(tables, *b[:8], validate=False)       # _on_kernel has just held every tensor to the same conditions
            # the kernel wrote through raw pointers: advance the version counters that weight_cache.weight_tag keys on (the parameter's own:
            # p.data is an alias with a counter of its own)
            torch.autograd.graph.increment_version(b[8])
        if on_torch:         # _torch_step writes through p.data, as the reference does: the parameter's own counter has not moved either
            torch.autograd.graph.increment_version(on_torch)
        return loss

    def close(self):
        """Release the kernel path's device tables and pinned staging buffers now, with the device idle, instead of whenever the collector
        frees this optimiser (an optimiser is cyclic garbage; e.g. before a hipGraph capture).  The next ``step()`` builds them again."""
        for tables in self._tables.values():
            tables.close()
        self._tables = {}


def flat_and_anneal_lr_scheduler(optimizer, total_iters, warmup_iters=0, warmup_factor=0.1, warmup_method="linear", warmup_pow=2, anneal_point=0.72,
                                 anneal_method="cosine", target_lr_factor=0, poly_power=1.0, step_gamma=0.1, steps=(2 / 3.0, 8 / 9.0), cyclic=False,
                                 return_function=False):
    """Warm up from ``warmup_factor``, stay flat at the base rate until ``anneal_point * total_iters`` (``steps[0] * total_iters`` with the
    ``step`` method), anneal to ``target_lr_factor`` at ``total_iters``; ``cyclic`` repeats the cycle.  Returns a ``LambdaLR`` (and the
    factor function with ``return_function``)."""
    if warmup_method not in ("constant", "linear", "pow", "exp"):
        raise ValueError("Only 'constant', 'linear', 'pow' or 'exp' warmup_method accepted, got {}".format(warmup_method))
    if anneal_method not in ("cosine", "linear", "poly", "exp", "step", "none"):
        raise ValueError("Only 'cosine', 'linear', 'poly', 'exp', 'step' or 'none' anneal_method accepted, got {}".format(anneal_method))
    if anneal_method == "step":
        if any(s < warmup_iters / total_iters or s > 1 for s in steps):
            raise ValueError("error in steps: {}. warmup_iters: {} total_iters: {}. steps should be in ({},1)".format(
                steps, warmup_iters, total_iters, warmup_iters / total_iters))
        if list(steps) != sorted(steps):
            raise ValueError("steps {} is not in ascending order.".format(steps))
        warnings.warn("ignore anneal_point when using step anneal_method")
        anneal_start = steps[0] * total_iters
    else:
        if anneal_point > 1 or anneal_point < 0:
            raise ValueError("anneal_point should be in [0,1], got {}".format(anneal_point))
        anneal_start = anneal_point * total_iters

    def f(x):
        x = x % total_iters if cyclic else x
        if x < warmup_iters:
            alpha = float(x) / warmup_iters
            if warmup_method == "linear":
                return (1 - warmup_factor) * alpha + warmup_factor
            if warmup_method == "pow":
                return (1 - warmup_factor) * pow(alpha, warmup_pow) + warmup_factor
            if warmup_method == "exp":
                assert warmup_factor > 0, warmup_factor
                return warmup_factor ** (1 - alpha)
            return warmup_factor
        if x < anneal_start:
            return 1
        if x >= total_iters:
            return target_lr_factor
        rel = (float(x) - anneal_start) / (total_iters - anneal_start)
        if anneal_method == "step":
            return step_gamma ** bisect_right([s * total_iters for s in steps], float(x))
        if anneal_method == "cosine":
            return target_lr_factor + 0.5 * (1 - target_lr_factor) * (1 + math.cos(math.pi * rel))
        if anneal_method == "linear":
            return target_lr_factor + (1 - target_lr_factor) * (total_iters - float(x)) / (total_iters - anneal_start)
        if anneal_method == "poly":
            return target_lr_factor + (1 - target_lr_factor) * ((total_iters - float(x)) / (total_iters - anneal_start)) ** poly_power
        if anneal_method == "exp":
            return max(target_lr_factor, 5e-3) ** rel
        return 1

    sched = torch.optim.lr_scheduler.LambdaLR(optimizer, f)
    return (sched, f) if return_function else sched


def _get(node, key, default):
    try:
        v = node.get(key, default) if hasattr(node, "get") else getattr(node, key, default)
    except (KeyError, AttributeError):
        return default
    return default if v is None else v


def build_optimizer_with_params(cfg, params):
    """``cfg.SOLVER.OPTIMIZER_CFG`` (a dict, or its text) -> the optimiser over ``params`` (a list of parameter groups): ``type="Ranger"`` is
    this module's, any other type names a class of ``torch.optim``."""
    spec = cfg.SOLVER.OPTIMIZER_CFG
    if isinstance(spec, str):
        if spec == "":
            raise RuntimeError("please provide cfg.SOLVER.OPTIMIZER_CFG to build optimizer")
        spec = eval(spec, {"__builtins__": {}, "dict": dict})
    spec = copy.deepcopy(dict(spec))
    clip = _get(cfg.SOLVER, "CLIP_GRADIENTS", None)
    if clip is not None and _get(clip, "ENABLED", False):
        raise NotImplementedError("SOLVER.CLIP_GRADIENTS.ENABLED: gradient clipping is not carried")
    kind = spec.pop("type")
    if kind == "Ranger":
        return Ranger(params, nan_to_num=bool(_get(cfg.SOLVER, "SET_NAN_GRAD_TO_ZERO", False)), **spec)
    cls = getattr(torch.optim, kind, None) if isinstance(kind, str) else None
    if not (isinstance(cls, type) and issubclass(cls, torch.optim.Optimizer) and cls is not torch.optim.Optimizer):
        raise ValueError(f"Unknown optimizer name: {kind}")
    return cls(params, **spec)


def build_lr_scheduler(cfg, optimizer, total_iters, return_function=False):
    """``cfg.SOLVER.LR_SCHEDULER_NAME`` -> the scheduler; ``flat_and_anneal`` is the one every shipped config names."""
    s = cfg.SOLVER
    name = s.LR_SCHEDULER_NAME
    if name.lower() != "flat_and_anneal":
        raise ValueError("Unknown LR scheduler: {}".format(name))
    return flat_and_anneal_lr_scheduler(
        optimizer, total_iters=total_iters, warmup_factor=s.WARMUP_FACTOR, warmup_iters=s.WARMUP_ITERS, warmup_method=s.WARMUP_METHOD,
        anneal_method=s.ANNEAL_METHOD, anneal_point=s.ANNEAL_POINT, steps=_get(s, "REL_STEPS", [2 / 3.0, 8 / 9.0]),
        target_lr_factor=_get(s, "TARGET_LR_FACTOR", 0), poly_power=_get(s, "POLY_POWER", 1.0), step_gamma=s.GAMMA, return_function=return_function)


def build_model_ema(cfg, model):
    """``cfg.MODEL.EMA`` -> ``ModelEMA(model, **INIT_CFG)`` (``decay``, ``updates``), or None unless ``ENABLED`` is set.  The keys are read
    with defaults: a config without the block trains without an EMA, as the reference's base config does.  Build it after the weights
    are loaded, and set ``ema.updates`` to the start iteration on resume (engine.py:234-237 of the reference)."""
    from ..lib.torch_utils.torch_utils import ModelEMA

    block = _get(_get(cfg, "MODEL", {}), "EMA", None)
    if block is None or not _get(block, "ENABLED", False):
        return None
    return ModelEMA(model, **dict(_get(block, "INIT_CFG", {})))


def model_param_groups(cfg, backbone, geo_head, pnp_net):
    """The reference's parameter groups, in its order: backbone at BASE_LR, geometry head and PnP net at BASE_LR x LR_MULT.  A FREEZEd part
    gets ``requires_grad=False`` and no group; only parameters that require a gradient are listed."""
    net = cfg.MODEL.POSE_NET
    base_lr = _get(cfg.SOLVER, "BASE_LR", None)
    if base_lr is None:          # main_gdrn.py:103: BASE_LR is the optimiser block's lr
        spec = cfg.SOLVER.OPTIMIZER_CFG
        base_lr = (eval(spec, {"__builtins__": {}, "dict": dict}) if isinstance(spec, str) else spec)["lr"]
    base_lr = float(base_lr)
    groups = []
    for part, mod, mult in ((net.BACKBONE, backbone, 1.0), (net.GEO_HEAD, geo_head, float(_get(net.GEO_HEAD, "LR_MULT", 1.0))),
                            (net.PNP_NET, pnp_net, float(_get(net.PNP_NET, "LR_MULT", 1.0)))):
        if _get(part, "FREEZE", False):
            for p in mod.parameters():
                p.requires_grad = False
        else:
            groups.append({"params": [p for p in mod.parameters() if p.requires_grad], "lr": base_lr * mult})
    return groups
