"""Seeded parameters and inputs of the SimplePointPnPNet fixture (tests/golden/point_pnp_golden.npz).

Shared by the generator (make_golden_point_pnp.py, authoring container) and the tests: the .npz stores seeds, case descriptions
and recorded outputs only; everything else is redrawn here from ``numpy.random.RandomState`` — the legacy generator, whose
streams are bit-stable across NumPy versions and machines.

Distributions (also written into the .npz as text):
  parameters   weights uniform(-1/sqrt(fan_in), 1/sqrt(fan_in)), biases uniform(-0.1, 0.1), drawn in the order of PARAM_SHAPES
  inputs       xyz, coord2d uniform[0, 1); region = softmax over 64 channels of 3 * N(0, 1) logits (float64, then cast);
               extents uniform[0.05, 0.3); mask attention (concat case) uniform[0, 1)
"""
import hashlib

import numpy as np

B, RES, NUM_REGIONS = 8, 64, 64
PARAM_SEED, INPUT_SEED = 20221017, 20221018

# case -> constructor / input description
CASES = {
    "rot6": dict(rot_dim=6, mask_attention_type="none", region=True),
    "rot4": dict(rot_dim=4, mask_attention_type="none", region=True),
    "concat": dict(rot_dim=6, mask_attention_type="concat", region=False),
}

DISTRIBUTIONS = ("weights uniform(+-1/sqrt(fan_in)), biases uniform(+-0.1), RandomState(PARAM_SEED + 1000 * rot_dim + nIn) in "
                 "state_dict order; inputs RandomState(INPUT_SEED): xyz|coord2d uniform[0,1) [8,5,64,64], region softmax(3*N(0,1)) "
                 "over 64 channels [8,64,64,64], extents uniform[0.05,0.3) [8,3], mask attention uniform[0,1) [8,1,64,64]")


def n_in(case: str) -> int:
    c = CASES[case]
    return 5 + (NUM_REGIONS if c["region"] else 0) + (1 if c["mask_attention_type"] == "concat" else 0)


def param_shapes(nIn: int, rot_dim: int):
    """(key, shape, fan_in) in the reference's state_dict order."""
    return [("conv1.weight", (128, nIn, 1), nIn), ("conv1.bias", (128,), 0), ("conv2.weight", (128, 128, 1), 128),
            ("conv2.bias", (128,), 0), ("conv3.weight", (1024, 128, 1), 128), ("conv3.bias", (1024,), 0),
            ("fc1.weight", (512, 1024), 1024), ("fc1.bias", (512,), 0), ("fc2.weight", (256, 512), 512), ("fc2.bias", (256,), 0),
            ("fc_pose.weight", (rot_dim + 3, 256), 256), ("fc_pose.bias", (rot_dim + 3,), 0)]


def params(nIn: int, rot_dim: int, seed: int = PARAM_SEED) -> dict:
    rng = np.random.RandomState(seed + 1000 * rot_dim + nIn)
    out = {}
    for key, shape, fan_in in param_shapes(nIn, rot_dim):
        bound = 1.0 / np.sqrt(fan_in) if fan_in else 0.1
        out[key] = rng.uniform(-bound, bound, size=shape).astype(np.float32)
    return out


def inputs(seed: int = INPUT_SEED, b: int = B, res: int = RES) -> dict:
    rng = np.random.RandomState(seed)
    coor_feat = rng.uniform(0.0, 1.0, size=(b, 5, res, res)).astype(np.float32)
    logits = 3.0 * rng.standard_normal(size=(b, NUM_REGIONS, res, res))
    e = np.exp(logits - logits.max(axis=1, keepdims=True))
    region = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    extents = rng.uniform(0.05, 0.3, size=(b, 3)).astype(np.float32)
    mask_attention = rng.uniform(0.0, 1.0, size=(b, 1, res, res)).astype(np.float32)
    return dict(coor_feat=coor_feat, region=region, extents=extents, mask_attention=mask_attention)


def digest(arrays: dict) -> str:
    """sha256 over the arrays' bytes in key order: the fixture stores it, so a machine whose libm rounds the softmax differently
    is reported as such instead of as a kernel error."""
    h = hashlib.sha256()
    for k in sorted(arrays):
        h.update(k.encode())
        h.update(np.ascontiguousarray(arrays[k]).tobytes())
    return h.hexdigest()


def case_inputs(case: str, inp: dict) -> dict:
    """The keyword arguments of the head's ``forward`` for ``case`` (fresh copies: forward de-normalises xyz in place)."""
    c = CASES[case]
    kw = dict(coor_feat=inp["coor_feat"].copy(), extents=inp["extents"].copy())
    if c["region"]:
        kw["region"] = inp["region"].copy()
    if c["mask_attention_type"] != "none":
        kw["mask_attention"] = inp["mask_attention"].copy()
    return kw
