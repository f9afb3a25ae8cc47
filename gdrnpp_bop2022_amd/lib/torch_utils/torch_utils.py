"""The part of the reference's ``lib/torch_utils/torch_utils.py`` that GDRN's training loop imports: ``ModelEMA`` (behind
``MODEL.EMA.ENABLED``), ``copy_attr`` and ``is_parallel``.  The class is the detector's (``det/yolox/utils/ema.py``: one update path, the
multi-tensor HIP kernel wherever a pair of tensors qualifies) with the reference's ``update_attr`` on top."""
from ...det.yolox.utils.ema import ModelEMA as _ModelEMA, is_parallel

__all__ = ["ModelEMA", "copy_attr", "is_parallel"]


def copy_attr(a, b, include=(), exclude=()):
    """Copy the attributes of ``b``'s ``__dict__`` onto ``a``: only those in ``include`` when it is not empty, none that starts with an
    underscore (a module's parameters, buffers and submodules live under such names) and none in ``exclude``."""
    wanted = set(include) if len(include) else None
    for name, value in vars(b).items():
        if name[:1] != "_" and name not in exclude and (wanted is None or name in wanted):
            setattr(a, name, value)


class ModelEMA(_ModelEMA):
    def update_attr(self, model, include=(), exclude=("process_group", "reducer")):
        """Bring the averaged copy's plain attributes up to the model's (``copy_attr``)."""
        copy_attr(self.ema, model, include, exclude)
