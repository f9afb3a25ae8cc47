"""-m gpu: gdrnpp_yolox_letterbox against the NumPy restatement of cv2.resize's 8-bit path (tests/letterbox_ref.py) and the
fixture written by the reference's own ``preproc`` (tests/golden/letterbox_golden.npz): bit-exact, in both output forms; the
Focus form is also bit-equal to gdrnpp_yolox_focus of the NCHW form.

Cases (H x W -> Ht x Wt) and what each reaches:
  copy_96x128    96x128 -> 128x128    r = 1 (copy), bottom pad
  up_60x80       60x80 -> 128x128     upscale, source-index clamps at the right and bottom
  area_256x256   256x256 -> 128x128   OpenCV's 2:1 area shortcut
  hbound_100x60  100x60 -> 128x96     height-bound, right pad, non-square target
  down_135x180   135x180 -> 160x160   fractional downscale
  batch3_w81     3 x 57x81 -> 96x128  rows of 243 bytes (unaligned), batch stride
  wide_50x200    50x200 -> 128x224    112 cell columns: a full wave and a partial one per row (Python gives rw = 224 here)
  rw200_64x100   64x100 -> 128x224    rw = 200: the image ends inside a wave, 24 columns of pad behind it"""
import os

import numpy as np
import pytest
import torch

import letterbox_ref as LR
from conftest import GOLDEN

from gdrnpp_bop2022_amd import hip_lib

pytestmark = pytest.mark.gpu
DEV = "cuda"


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "letterbox_golden.npz"))


@pytest.mark.parametrize("name", list(LR.CASES))
def test_both_forms_are_bit_exact(hip, golden, name):
    b, h, w, t = LR.CASES[name]
    imgs = LR.case_images(name)
    want = np.stack([LR.preproc(im, t)[0] for im in imgs])
    assert np.array_equal(want, golden[f"{name}/out_u8"].astype(np.float32)), "restatement and fixture disagree"
    dev = torch.from_numpy(imgs).to(DEV)
    nchw, r = hip_lib.yolox_letterbox(dev, t)
    assert r == float(golden[f"{name}/r"]) and nchw.shape == (b, 3) + t and nchw.dtype == torch.float32
    got = nchw.cpu().numpy()
    bad = np.argwhere(got != want)
    assert len(bad) == 0, (name, len(bad), bad[:4], got[tuple(bad[0])] if len(bad) else None, want[tuple(bad[0])] if len(bad) else None)
    # Focus form into a slice of a wider NaN-filled buffer; against gdrnpp_yolox_focus of the NCHW form
    ld, off = 20, 4
    foc = torch.full((b, t[0] // 2, t[1] // 2, ld), float("nan"), device=DEV)
    out, _ = hip_lib.yolox_letterbox(dev, t, out=foc, y_off=off, focus=True)
    assert out is foc
    ref = torch.full_like(foc, float("nan"))
    hip_lib.yolox_focus(nchw, ref, off)
    assert torch.equal(foc[..., off:off + 12].view(torch.int32), ref[..., off:off + 12].view(torch.int32))
    assert torch.isnan(foc[..., :off]).all() and torch.isnan(foc[..., off + 12:]).all(), "written outside the Focus slice"
    fresh, _ = hip_lib.yolox_letterbox(dev, t, focus=True)
    assert fresh.shape == (b, t[0] // 2, t[1] // 2, 12) and torch.equal(fresh, ref[..., off:off + 12])


def test_the_plans_focus_buffer_feeds_the_forward_bit_equal(hip):
    """hip_forward.forward(None, focus=...) on the letterbox's Focus output == YOLOX.forward on its NCHW output."""
    import sys

    sys.path.insert(0, GOLDEN)
    import yolox_seeded as YS

    from gdrnpp_bop2022_amd.det.yolox import models as M
    from gdrnpp_bop2022_amd.det.yolox.models import hip_forward

    net = M.build_yolox(0.33, 0.50, 5)
    net.load_state_dict(YS.state_dict_for(net), strict=True)
    net = net.to(DEV).eval()
    dev = torch.from_numpy(LR.case_images("batch3_w81")).to(DEV)
    with torch.no_grad():
        x, _ = hip_lib.yolox_letterbox(dev, (96, 128))
        want = net(x)["det_preds"]
        foc = hip_forward.focus_buffer(net, 3, 96, 128, dev.device)
        hip_lib.yolox_letterbox(dev, (96, 128), out=foc, focus=True)
        got = hip_forward.forward(net, None, focus=foc)["det_preds"]
        with pytest.raises(RuntimeError, match="focus_buffer"):
            hip_forward.forward(net, None, focus=foc.clone())
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_bad_target_sizes_return_a_status_and_launch_nothing(hip):
    lib = hip_lib.load()
    img = torch.zeros((1, 50, 50, 3), dtype=torch.uint8, device=DEV)
    out = torch.full((1, 3, 128, 128), float("nan"), device=DEV)
    for ht, wt, rh, rw in [(100, 128, 100, 100), (128, 100, 100, 100), (0, 128, 50, 50), (128, 128, 129, 50), (128, 128, 50, 0)]:
        rc = lib.gdrnpp_yolox_letterbox(img.data_ptr(), 1, 50, 50, rh, rw, out.data_ptr(), ht, wt, 0, 0, 0, None)
        assert rc < 0 and lib.gdrnpp_last_error(), (ht, wt, rh, rw, rc)
    rc = lib.gdrnpp_yolox_letterbox(img.data_ptr(), 1, 50, 50, 128, 128, out.data_ptr(), 128, 128, 1, 14, 4, None)     # ldy not a multiple of 4
    assert rc < 0
    torch.cuda.synchronize()
    assert torch.isnan(out).all(), "an argument error must not launch"
    with pytest.raises(RuntimeError, match="multiples of 32"):
        hip_lib.yolox_letterbox(img, (100, 128))
    rc = lib.gdrnpp_yolox_letterbox(img.data_ptr(), 1, 50, 50, 128, 128, out.data_ptr(), 128, 128, 0, 0, 0, None)
    torch.cuda.synchronize()
    assert rc == 0 and torch.isfinite(out).all()
