"""Golden vectors of the point-wise PnP head from the reference's own module (authoring container only: needs the
reference checkout that tests/golden/_refimport.py imports from).

What runs here is the reference's ``SimplePointPnPNet`` (core/gdrn_modeling/models/heads/point_pnp_net.py:208-293), imported from
its file through tests/golden/_refimport.py, in fp32 and in fp64 on the same seeded parameters and inputs
(tests/golden/point_pnp_seeded.py).  Recorded per case of ``point_pnp_seeded.CASES`` in point_pnp_golden.npz:

  <case>/rot32, t32, pooled32      the reference's fp32 outputs; ``pooled`` = max over the points of conv3's output (forward hook)
  <case>/rot64, t64, pooled64      the same module and inputs in fp64
  <case>/e_ref_rot, e_ref_t, e_ref_pooled     max |fp32 - fp64|: the reference's own error, the unit of the tests' bars
  <case>/keys, shapes              the reference's state_dict manifest
  param_seed, input_seed, distributions, input_digest
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import _refimport  # noqa: E402

_refimport.install()

import point_pnp_seeded as PS  # noqa: E402
from core.gdrn_modeling.models.heads.point_pnp_net import SimplePointPnPNet  # noqa: E402


def run(case, inp, dtype):
    c = PS.CASES[case]
    nIn = PS.n_in(case)
    net = SimplePointPnPNet(nIn, rot_dim=c["rot_dim"], mask_attention_type=c["mask_attention_type"])
    sd = {k: torch.from_numpy(v) for k, v in PS.params(nIn, c["rot_dim"]).items()}
    assert list(sd) == list(net.state_dict()) and all(sd[k].shape == v.shape for k, v in net.state_dict().items())
    net.load_state_dict(sd, strict=True)
    net = net.to(dtype).eval()
    pooled = {}
    net.conv3.register_forward_hook(lambda m, i, o: pooled.__setitem__("v", o.max(dim=2)[0].detach().clone()))
    kw = {k: torch.from_numpy(v).to(dtype) for k, v in PS.case_inputs(case, inp).items()}
    with torch.no_grad():
        rot, t = net(**kw)
    manifest = [(k, tuple(v.shape)) for k, v in net.state_dict().items()]
    return rot.numpy().copy(), t.numpy().copy(), pooled["v"].numpy().copy(), manifest


def main():
    torch.manual_seed(0)
    inp = PS.inputs()
    out = dict(param_seed=np.int64(PS.PARAM_SEED), input_seed=np.int64(PS.INPUT_SEED), distributions=np.array(PS.DISTRIBUTIONS),
               input_digest=np.array(PS.digest(inp)))
    for case in PS.CASES:
        r32, t32, p32, manifest = run(case, inp, torch.float32)
        r64, t64, p64, _ = run(case, inp, torch.float64)
        out[f"{case}/keys"] = np.array([k for k, _ in manifest])
        out[f"{case}/shapes"] = np.array([",".join(map(str, s)) for _, s in manifest])
        for name, a32, a64 in (("rot", r32, r64), ("t", t32, t64), ("pooled", p32, p64)):
            out[f"{case}/{name}32"], out[f"{case}/{name}64"] = a32, a64
            e = float(np.abs(a32.astype(np.float64) - a64).max())
            out[f"{case}/e_ref_{name}"] = np.float64(e)
            print(f"{case:7s} {name:7s} e_ref = {e:.3e}   max |value| = {np.abs(a64).max():.3e}")
    path = os.path.join(HERE, "point_pnp_golden.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
