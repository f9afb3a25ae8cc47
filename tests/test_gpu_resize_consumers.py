"""-m gpu: the three kernels that restate an 8-bit ``cv2.resize(INTER_LINEAR)`` take their pixel from one place (csrc/resize_u8.hpp), so
from one source and one request they give the same bytes: the detector's letterbox (``yolox_letterbox``), the training backgrounds
(``replace_bg``) and the plain branch of the YOLOX training batches (``yolox_train_inputs``).  EQUALITY among the three and with
tests/replace_bg_ref.py's ``cv2_resize``; outside the resized region each keeps its own padding (114, 0, 114)."""
import numpy as np
import pytest
import torch

from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd.gdrn_modeling import train_inputs as TI
from tests import replace_bg_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"

# form -> (source H x W, letterbox target); the linear case clamps its last column tap and its last row tap
CASES = {"copy": ((32, 64), (32, 64)), "area": ((64, 128), (32, 64)), "linear": ((37, 50), (64, 64))}


@pytest.mark.parametrize("form", list(CASES))
def test_letterbox_replace_bg_and_train_inputs_resize_to_the_same_bytes(form):
    (H, W), (Ht, Wt) = CASES[form]
    src = np.random.RandomState(H * W).randint(0, 256, (H, W, 3)).astype(np.uint8)
    _, rh, rw = hip_lib.letterbox_sizes(H, W, (Ht, Wt))
    req = TI.resize_request(W, H, dsize=(rw, rh))
    assert (req["dw"], req["dh"]) == (rw, rh) and hip_lib.RESIZE_MODES[req["mode"]] == form
    if form == "linear":
        assert (rh, rw) == (47, 64)
    want = R.cv2_resize(src, dsize=(rw, rh))
    assert want.shape == (rh, rw, 3)
    dev_src = torch.from_numpy(src).to(DEV)

    def padded(value):
        canvas = np.full((Ht, Wt, 3), value, np.uint8)
        canvas[:rh, :rw] = want
        return canvas

    boxed, _ = hip_lib.yolox_letterbox(dev_src[None], (Ht, Wt))
    boxed = boxed[0].permute(1, 2, 0).cpu().numpy()

    image = torch.full((1, Ht, Wt, 3), 255, dtype=torch.uint8, device=DEV)
    row = dict(do=1, bg_off=0, bg_stride=W, x0=0, y0=0, cw=W, ch=H, cut=0, u=0.0, **req)
    mask_trunc, flags = hip_lib.replace_bg(image, torch.zeros((1, Ht, Wt), dtype=torch.uint8, device=DEV), dev_src.reshape(-1),
                                           hip_lib.replace_bg_table([row]))
    assert not mask_trunc.any() and not flags.any()
    background = image[0].cpu().numpy()

    plain = dict(branch=hip_lib.YOLOX_AUG_BRANCHES.index("plain"), flags=0, s0_off=0, s0_w=W, s0_h=H, s0_pw=rw, s0_ph=rh,
                 **{f"s0_{k}": v for k, v in req.items()})
    lut = torch.zeros((1, 2, 3, 256), dtype=torch.uint8, device=DEV)
    batch, flags = hip_lib.yolox_train_inputs(dev_src.reshape(-1), hip_lib.yolox_aug_table([plain]), lut, Ht, Wt)
    assert not flags.any()
    batch = batch[0].permute(1, 2, 0).cpu().numpy()

    for name, got, pad in (("letterbox", boxed, 114), ("replace_bg", background, 0), ("yolox_train_inputs", batch, 114)):
        ref = padded(pad).astype(got.dtype)
        bad = got != ref
        assert got.shape == ref.shape and not bad.any(), (form, name, int(bad.sum()), np.argwhere(bad)[:4].tolist())
    assert boxed[:rh, :rw].astype(np.uint8).tobytes() == background[:rh, :rw].tobytes() == batch[:rh, :rw].astype(np.uint8).tobytes()
