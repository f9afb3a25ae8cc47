"""What the ModelEMA tests and tests/golden/make_golden_model_ema.py share: the small seeded model, the seeded perturbation between
updates, the runs of the fixture, its loader, and the oracle of the GPU tests — the reference's two statements on CPU tensors."""
import os

import numpy as np
import torch
import torch.nn as nn

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "model_ema_golden.npz")
DECAYS = (0.9998, 0.9999)
CLASSES = ("yolox", "gdrn")                                   # det/yolox/utils/ema.py and lib/torch_utils/torch_utils.py
RUNS = {"fresh": dict(updates=0, steps=5), "resume": dict(updates=1999, steps=2)}
TRACKED_AT_COPY = 7                                           # num_batches_tracked when the EMA is made; the model's moves on by 3 per step


class Tiny(nn.Module):
    """Conv2d + BatchNorm2d (running statistics and the int64 ``num_batches_tracked``), a Linear and one fp64 buffer."""

    def __init__(self):
        super().__init__()
        self.conv = nn.Conv2d(3, 5, 3)
        self.bn = nn.BatchNorm2d(5)
        self.fc = nn.Linear(7, 4)
        self.register_buffer("scale64", torch.linspace(0.5, 1.5, 3, dtype=torch.float64))

    def forward(self, x):
        return self.fc(self.bn(self.conv(x)).mean((2, 3)).repeat(1, 2)[:, :7]) * self.scale64[0].float()


def build_tiny():
    gen = torch.Generator().manual_seed(20221)
    model = Tiny()
    with torch.no_grad():
        for v in model.state_dict().values():
            if v.dtype.is_floating_point:
                v.copy_(torch.randn(v.shape, generator=gen, dtype=torch.float64).to(v.dtype))
        model.bn.running_var.abs_().add_(0.5)
        model.bn.num_batches_tracked.fill_(TRACKED_AT_COPY)
    return model


def perturb(model, run: str, t: int):
    """What stands in for an optimiser step before update ``t`` (1-based) of ``run``: seeded noise on every floating-point state entry,
    three more batches tracked.  Works on any device: the noise is drawn on the CPU in fp64 and rounded to the entry's type."""
    gen = torch.Generator().manual_seed(1000 * (1 + list(RUNS).index(run)) + t)
    with torch.no_grad():
        for v in model.state_dict().values():
            if v.dtype.is_floating_point:
                v.add_((0.05 * torch.randn(v.shape, generator=gen, dtype=torch.float64)).to(v.dtype).to(v.device))
            else:
                v.add_(3)


def float_keys(model):
    return [k for k, v in model.state_dict().items() if v.dtype.is_floating_point]


def unflatten(vector, keys, dtypes, shapes):
    """A recorded state (one fp64 vector, entries in key order; every recorded type is exact in fp64) -> {key: array of its own type}."""
    out, at = {}, 0
    for k, dt, shape in zip(keys, dtypes, shapes):
        shape = tuple(int(s) for s in str(shape).split(",") if s)
        n = int(np.prod(shape, dtype=np.int64))
        out[str(k)] = vector[at:at + n].astype(np.dtype(str(dt))).reshape(shape)
        at += n
    assert at == len(vector)
    return out


class Golden:
    """model_ema_golden.npz: ``model(run, t)`` = the model's state before update t, ``ema(cls, decay, run, t)`` = the reference's EMA state
    after it, ``d(cls, decay, run, t)`` = the decay it used, as fp64."""

    def __init__(self):
        self.z = np.load(GOLDEN)
        self.keys = [str(k) for k in self.z["keys"]]

    def _state(self, name):
        return unflatten(self.z[name], self.keys, self.z["dtypes"], self.z["shapes"])

    def model(self, run, t):
        return self._state(f"model/{run}/{t}")

    def ema(self, cls, decay, run, t):
        return self._state(f"ema/{cls}/{decay}/{run}/{t}")

    def d(self, cls, decay, run, t):
        return float(self.z[f"d/{cls}/{decay}/{run}/{t}"])


def load_state(model, arrays):
    """Write a recorded state into ``model``'s own tensors (on whatever device they live)."""
    with torch.no_grad():
        for k, v in model.state_dict().items():
            v.copy_(torch.from_numpy(np.asarray(arrays[k])).to(v.dtype))


def reference_update(e: torch.Tensor, m: torch.Tensor, d: float) -> torch.Tensor:
    """The reference's two statements on CPU copies -> the updated EMA tensor (``d`` a Python float, as ``ModelEMA.decay`` returns it)."""
    v = e.detach().cpu().clone()
    v *= d
    v += (1.0 - d) * m.detach().cpu()
    return v


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Equal bit patterns, except that any NaN equals any NaN."""
    a, b = a.detach().cpu(), b.detach().cpu()
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if not a.dtype.is_floating_point:
        return bool(torch.equal(a, b))
    nan = torch.isnan(a)
    if not torch.equal(nan, torch.isnan(b)):
        return False
    view = {torch.float32: torch.int32, torch.float64: torch.int64, torch.float16: torch.int16}[a.dtype]
    return bool(torch.equal(a.contiguous().view(view)[~nan.contiguous()], b.contiguous().view(view)[~nan.contiguous()]))
