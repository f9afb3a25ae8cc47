"""Seeded parameters and inputs of the YOLOX fixture (tests/golden/yolox_net_golden_<case>.npz).

Shared by the generator (make_golden_yolox_net.py, authoring container) and the tests: YOLOX-x has 99 M parameters, so the .npz
stores seeds, case descriptions, digests and recorded outputs only; the state dict is refilled here key by key from a
``torch.Generator`` seeded with PARAM_SEED + crc32(key), so the values do not depend on the order of the keys.

Distributions (chosen so that 155 stacked convolutions neither die nor explode and the outputs exercise the decode):
  conv weights      uniform(+-1.3 sqrt(3 / fan_in)): output variance 1.69 x the input's mean square — contracts both where SiLU
                    halves small signals (x 0.25) and where it passes the positive half of large ones (x 0.5)
                    (the 3x3 of a Bottleneck, whose output is added to its input up to twelve times in a row: gain 0.6)
  BatchNorm         weight uniform[0.8, 1.2), bias uniform[-1, 1), running_mean uniform[-0.5, 0.5), running_var
                    uniform[0.5, 2.0): far from the identity; the shifts keep feeding the signal the contraction removes
  cls / obj preds   weights uniform(+-3 sqrt(3 / fan_in)), bias uniform[-3, -1): logits span several units
  reg preds         weights uniform(+-sqrt(3 / fan_in)), bias uniform[-0.5, 0.5): |pre-exp w, h| stays below 4
  image             uniform[-1.7, 1.7), unit variance
"""
import hashlib
import zlib

import numpy as np
import torch

PARAM_SEED, INPUT_SEED = 20221101, 20221102

# case -> model size, input shape, number of anchor rows stored (0 = all)
CASES = {
    "x320": dict(depth=1.33, width=1.25, num_classes=21, shape=(1, 3, 320, 320), rows=0),
    "s256x384": dict(depth=0.33, width=0.50, num_classes=21, shape=(2, 3, 256, 384), rows=0),
    "x640": dict(depth=1.33, width=1.25, num_classes=21, shape=(1, 3, 640, 640), rows=1024),
}
SIZES = {"x": (1.33, 1.25), "s": (0.33, 0.50)}

DISTRIBUTIONS = ("per key torch.Generator(PARAM_SEED + crc32(key)): conv weights U(+-1.3 sqrt(3/fan_in)), 0.6 for Bottleneck conv2; bn weight U[0.8,1.2), bias "
                 "U[-1,1), running_mean U[-0.5,0.5), running_var U[0.5,2.0), num_batches_tracked 1000; cls/obj preds weight "
                 "U(+-3 sqrt(3/fan_in)) bias U[-3,-1); reg preds weight U(+-sqrt(3/fan_in)) bias U[-0.5,0.5); image "
                 "torch.Generator(INPUT_SEED + crc32(case)) U[-1.7,1.7)")


def _gen(seed: int, key: str) -> torch.Generator:
    g = torch.Generator(device="cpu")
    g.manual_seed(seed + zlib.crc32(key.encode()))
    return g


def _uniform(g, shape, lo, hi):
    return torch.rand(tuple(shape), generator=g, dtype=torch.float32) * (hi - lo) + lo


def fill(key: str, shape) -> torch.Tensor:
    g = _gen(PARAM_SEED, key)
    leaf = key.rsplit(".", 1)[-1]
    pred = next((p for p in ("cls_preds", "obj_preds", "reg_preds") if p in key), None)
    if leaf == "num_batches_tracked":
        return torch.tensor(1000, dtype=torch.int64)
    if leaf == "weight" and len(shape) == 4:
        fan_in = shape[1] * shape[2] * shape[3]
        gain = {None: 1.3, "cls_preds": 3.0, "obj_preds": 3.0, "reg_preds": 1.0}[pred]
        if pred is None and ".m." in key and ".conv2." in key:
            gain = 0.6          # the 3x3 of a Bottleneck: its output is ADDED to its input, twelve times in a row in dark3 / dark4
        bound = gain * (3.0 / fan_in) ** 0.5
        return _uniform(g, shape, -bound, bound)
    if pred is not None and leaf == "bias":
        return _uniform(g, shape, -0.5, 0.5) if pred == "reg_preds" else _uniform(g, shape, -3.0, -1.0)
    lo, hi = {"weight": (0.8, 1.2), "bias": (-1.0, 1.0), "running_mean": (-0.5, 0.5), "running_var": (0.5, 2.0)}[leaf]
    return _uniform(g, shape, lo, hi)


def state_dict_for(model) -> dict:
    """A full state dict for ``model`` (this repository's YOLOX or the reference's): every key refilled."""
    return {k: fill(k, v.shape) for k, v in model.state_dict().items()}


def image(case: str) -> torch.Tensor:
    return _uniform(_gen(INPUT_SEED, case), CASES[case]["shape"], -1.7, 1.7)


def stored_rows(case: str, n_anchors: int) -> np.ndarray:
    """Sorted anchor rows the fixture keeps for ``case`` (all of them when CASES[case]['rows'] == 0)."""
    n = CASES[case]["rows"]
    if not n:
        return np.arange(n_anchors)
    return np.sort(np.random.RandomState(INPUT_SEED).permutation(n_anchors)[:n])


def digest(tensors: dict) -> str:
    """sha256 over a few values of every tensor in key order: tells a machine whose generator draws differently from a kernel error."""
    h = hashlib.sha256()
    for k in sorted(tensors):
        t = tensors[k].detach().reshape(-1)
        h.update(k.encode())
        h.update(t[:: max(1, t.numel() // 64)].contiguous().numpy().tobytes())
    return h.hexdigest()


# output groups of det_preds[..., 5 + C] and their columns
GROUPS = {"xy": slice(0, 2), "wh": slice(2, 4), "obj": slice(4, 5), "cls": slice(5, None)}


def yolox_x_conv_shapes():
    """The distinct (Cin, Cout, k, stride) of YOLOX-x's convolutions with 21 classes."""
    from gdrnpp_bop2022_amd.det.yolox.models import build_yolox
    import torch.nn as nn

    net = build_yolox(1.33, 1.25, 21)
    return sorted({(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0]) for m in net.modules() if isinstance(m, nn.Conv2d)})
