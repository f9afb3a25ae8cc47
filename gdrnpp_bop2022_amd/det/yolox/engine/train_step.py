"""One YOLOX training iteration, the statements of the reference's ``run_step`` (det/yolox/engine/yolox_trainer.py:358-396) in their
order, and the two builders its configs ask for: the learning-rate schedule and the parameter groups.

What is not here: AMP and the GradScaler, ``all_reduce_norm``, the data prefetcher, hooks and writers, DDP, hipGraph capture of the EMA
update, and ``preprocess`` / ``random_resize``: multi-scale training is dead code in the reference (``run_step`` hands ``preprocess`` the
very size it then divides by, so both scales are 1 and nothing is resized; the loader is never told the drawn size)."""
from __future__ import annotations

import torch.nn as nn

from ....gdrn_modeling.solver import flat_and_anneal_lr_scheduler
from ..utils.ema import ModelEMA

NORM_MODULE_TYPES = (nn.BatchNorm1d, nn.BatchNorm2d, nn.BatchNorm3d, nn.SyncBatchNorm, nn.GroupNorm, nn.InstanceNorm1d, nn.InstanceNorm2d,
                     nn.InstanceNorm3d, nn.LayerNorm, nn.LocalResponseNorm)


class YoloxTrainStep:
    """``run_step(inps, targets)`` on a train-mode model: forward with the losses, ``zero_grad``, backward, optimiser step, EMA update,
    scheduler step.  ``ema`` is ``ModelEMA(model, ema_decay)`` (the trainer's 0.9998) or None with ``use_ema=False``; ``eval_model`` is
    what evaluation and the checkpointer take: the EMA's copy when there is one, else the model.  On resume call ``resume(start_iter)``."""

    def __init__(self, model, optimizer, scheduler=None, ema_decay=0.9998, use_ema=True):
        self.model, self.optimizer, self.scheduler = model, optimizer, scheduler
        self.ema = ModelEMA(model, ema_decay) if use_ema else None
        self.iter = 0

    @property
    def eval_model(self):
        return self.ema.ema if self.ema is not None else self.model

    def resume(self, start_iter: int):
        """The reference's ``train()`` on resume: the EMA's ramp continues from the start iteration (yolox_trainer.py:309-310)."""
        self.iter = int(start_iter)
        if self.ema is not None:
            self.ema.updates = int(start_iter)

    def run_step(self, inps, targets):
        """inps f32[B,3,H,W], targets f32[B,G,5] = (class, cx, cy, w, h) -> (out_dict, loss_dict) of this iteration's forward."""
        if not self.model.training:
            raise RuntimeError("YoloxTrainStep.run_step: the model was changed to eval mode")
        out_dict, loss_dict = self.model(inps, targets)
        losses = sum(loss_dict.values())
        self.optimizer.zero_grad()
        losses.backward()
        self.optimizer.step()
        if self.ema is not None:
            self.ema.update(self.model)
        if self.scheduler is not None:
            self.scheduler.step()
        self.iter += 1
        return out_dict, loss_dict


def yolox_lr_scheduler(optimizer, lr_config, train_cfg):
    """The reference's ``build_lr_scheduler`` (yolox_trainer.py:520-536): ``flat_and_anneal_lr_scheduler`` over ``lr_config``'s keywords
    with ``total_iters = max_iter - no_aug_iters`` (the iterations without augmentation run at the final rate), ``warmup_iters`` from
    ``train_cfg``, and, with ``anneal_after_warmup``, the anneal point moved behind the warm-up:
    ``min(anneal_point + warmup_epochs / (total_epochs - no_aug_epochs), 1.0)``.  Both arguments are mappings."""
    kw = {k: v for k, v in dict(lr_config).items() if k not in ("optimizer", "total_iters", "warmup_iters", "anneal_point")}
    anneal_point = lr_config.get("anneal_point", 0)
    if train_cfg.get("anneal_after_warmup", False):
        anneal_point = min(anneal_point + train_cfg["warmup_epochs"] / (train_cfg["total_epochs"] - train_cfg["no_aug_epochs"]), 1.0)
    return flat_and_anneal_lr_scheduler(optimizer, total_iters=train_cfg["max_iter"] - train_cfg["no_aug_iters"],
                                        warmup_iters=train_cfg["warmup_iters"], anneal_point=anneal_point, **kw)


def yolox_param_groups(model, weight_decay, weight_decay_norm=0.0, weight_decay_bias=0.0):
    """The parameter groups the shipped configs ask detectron2's ``get_default_optimizer_params(weight_decay_norm=0.0,
    weight_decay_bias=0.0)`` for: parameters of normalisation layers get ``weight_decay_norm``, parameters named ``bias`` get
    ``weight_decay_bias`` (the later rule wins for a norm layer's bias), everything else ``weight_decay``; every parameter that requires
    a gradient appears once (a shared one under its first owner), and parameters of one decay share a group, in order of first
    appearance.  detectron2 is not installed where this was written: this is a restatement of its documented behaviour, not its code."""
    decays, seen = {}, set()
    for module in model.modules():
        for name, p in module.named_parameters(recurse=False):
            if not p.requires_grad or id(p) in seen:
                continue
            seen.add(id(p))
            wd = weight_decay
            if isinstance(module, NORM_MODULE_TYPES) and weight_decay_norm is not None:
                wd = weight_decay_norm
            if name == "bias" and weight_decay_bias is not None:
                wd = weight_decay_bias
            decays.setdefault(wd, []).append(p)
    return [{"params": ps, "weight_decay": wd} for wd, ps in decays.items()]
