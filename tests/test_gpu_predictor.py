"""-m gpu: YoloGdrnPredictor (image -> letterbox -> YOLOX -> NMS -> ROI table -> crop -> GDRN -> records) against the same
chain staged with the pieces that existed before it: the NumPy letterbox (tests/letterbox_ref.py) uploaded -> YOLOX.forward ->
yolox_postprocess -> detections_from_yolox (host) -> batch_data_test_gpu -> inference_step.  Records must be bit-equal.

Detector: YOLOX-s with the seeding of tests/golden/yolox_seeded.py; the stem's BatchNorm statistics are rescaled by
STEM_INPUT_SCALE (running_mean * s, running_var * s^2), i.e. the seeded network sees the 8-bit image divided by s — its seeded
weights are drawn for unit-variance input and saturate every score on 0..255 pixels otherwise.

IMAGE_SEED and CONF_THR were chosen on the CPU module path (restated letterbox -> the plain-PyTorch modules -> the reference's
decode / class-aware NMS restated in torch): two 96 x 128 images of RandomState(IMAGE_SEED) at test_size (128, 128) give
CPU_COUNTS = (9, 8) detections; the nearest scores on either side of CONF_THR are 0.05926 / 0.05613 (image 0) and
0.05881 / 0.05644 (image 1), margins of 8e-4 and more against an fp32 forward error near 1e-6."""
import sys

import numpy as np
import pytest
import torch

import letterbox_ref as LR
from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import yolox_seeded as YS  # noqa: E402

from gdrnpp_bop2022_amd import hip_lib, synthetic as S  # noqa: E402
from gdrnpp_bop2022_amd.det.yolox import models as M  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling import YoloGdrnPredictor, engine, hip_layers  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling.GDRN_double_mask import build_model_optimizer  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
IMAGE_SEED, CONF_THR, NMS_THR, CPU_COUNTS = 1, 0.058, 0.45, (9, 8)
STEM_INPUT_SCALE = 73.6          # the standard deviation of uniform 0..255
TEST_SIZE, NUM_CLASSES, MAX_DET = (128, 128), 21, 64


def seeded_yolox_s():
    net = M.build_yolox(0.33, 0.50, NUM_CLASSES)
    net.load_state_dict(YS.state_dict_for(net), strict=True)
    bn = net.backbone.backbone.stem.conv.bn
    with torch.no_grad():
        bn.running_var.mul_(STEM_INPUT_SCALE ** 2)
        bn.running_mean.mul_(STEM_INPUT_SCALE)
    return net.eval()


@pytest.fixture(scope="module")
def setup(hip):
    cfg = get_cfg("ycbv_convnext_a6", opts=["TEST.USE_DEPTH_REFINE=True", "INPUT.WITH_DEPTH=True"])
    torch.manual_seed(0)
    model, _ = build_model_optimizer(cfg)
    model.load_state_dict(S.seeded_state_dict([(k, tuple(v.shape)) for k, v in model.state_dict().items()], 5), strict=True)
    with torch.no_grad():
        model.pnp_net.fc_t.bias.copy_(torch.tensor([0.0, 0.0, 1.5 * float(S.YCBV_K[0, 0]) * 0.19 / 64.0]))
    rng = np.random.default_rng(9)
    verts, faces, ext = S.make_models(NUM_CLASSES, rng, 2)
    post = engine.GdrnHipPost(cfg, hip_lib.MeshSet(verts, faces, DEV))
    yolox = seeded_yolox_s().to(DEV)
    images = np.random.RandomState(IMAGE_SEED).randint(0, 256, (2, 96, 128, 3)).astype(np.uint8)
    depths = torch.rand((2, 96, 128), device=DEV, generator=torch.Generator(device=DEV).manual_seed(1)) + 0.5
    cam = S.YCBV_K.astype(np.float32)
    return cfg, model, post, yolox, images, depths, cam, ext.astype(np.float32)


def predictor(setup, **kw):
    cfg, model, post, yolox, _, _, cam, ext = setup
    args = dict(test_size=TEST_SIZE, num_classes=NUM_CLASSES, conf_thr=CONF_THR, nms_thr=NMS_THR, cam=cam, extents=ext, max_det=MAX_DET)
    args.update(kw)
    return YoloGdrnPredictor(yolox, model, post, cfg, **args)


def staged(setup, images_dev, depths):
    cfg, model, post, yolox, images, _, cam, ext = setup
    x = torch.from_numpy(np.stack([LR.preproc(im, TEST_SIZE)[0] for im in images])).to(DEV)
    ratio = LR.sizes(96, 128, TEST_SIZE)[0]
    with torch.no_grad():
        det = yolox(x)["det_preds"]
    dets, count = hip_lib.yolox_postprocess(det, NUM_CLASSES, CONF_THR, NMS_THR, False, MAX_DET)
    d = engine.detections_from_yolox(dets, count, cam, ext, ratio)
    batch = engine.batch_data_test_gpu(cfg, images_dev, depths, d)
    return engine.inference_step(model, post, batch), dets, count, d


def test_records_are_bit_equal_to_the_staged_chain(setup):
    images_dev = torch.from_numpy(setup[4]).to(DEV)
    depths = setup[5]
    want, dets_s, count_s, d = staged(setup, images_dev, depths)
    p = predictor(setup)
    dets, count, ratio = p.detect(images_dev)
    assert ratio == 1.0 and torch.equal(count, count_s) and torch.equal(dets.view(torch.int32), dets_s.view(torch.int32))
    n0 = hip_layers.fallback_launches()
    rec, per_image = p(images_dev, depths)
    torch.cuda.synchronize()
    assert hip_layers.fallback_launches() == n0, hip_layers.last_fallback()
    print(f"predictor: {per_image} ROIs per image (CPU module path: {CPU_COUNTS})")
    assert sum(per_image) >= 3, "the detector found fewer than 3 ROIs: the comparison would be empty"
    assert per_image == count_s.cpu().tolist() == list(CPU_COUNTS)
    assert rec.shape == (sum(per_image), 16) and rec.dtype == torch.float32 and torch.isfinite(rec).all()
    assert torch.equal(rec.view(torch.int32), want.view(torch.int32)), (rec - want).abs().max()
    assert torch.equal(rec[:, 14], torch.arange(len(rec), device=DEV, dtype=torch.float32)), "roi_id is the stream position"
    assert np.array_equal(rec[:, 13].cpu().numpy(), d["roi_cls"].astype(np.float32)) and np.array_equal(rec[:, 12].cpu().numpy(), d["score"])
    again, _ = p(images_dev, depths)
    assert torch.equal(again.view(torch.int32), rec.view(torch.int32)), "two calls differ bit for bit"


def test_no_detections_give_an_empty_result(setup):
    """No image reaches the confidence bar (the seeded scores top out near 0.1): nothing is launched behind the ROI table."""
    images_dev = torch.from_numpy(setup[4]).to(DEV)
    rec, per_image = predictor(setup, conf_thr=0.5)(images_dev, setup[5])
    assert rec.shape == (0, 16) and rec.dtype == torch.float32 and rec.is_cuda and per_image == [0, 0]


def test_top_k_and_cap_shape_the_stream(setup):
    images_dev = torch.from_numpy(setup[4]).to(DEV)
    up, per_image = predictor(setup, top_k_per_obj=1).rois(images_dev)
    cls, im = up["roi_cls"].cpu().numpy(), up["im_idx"].cpu().numpy()
    for b in range(2):
        c = cls[im == b]
        assert len(c) == per_image[b] == len(set(c.tolist())) and (np.diff(c) > 0).all(), "one ROI per class, class order"
    rec, per_image = predictor(setup, roi_cap=5)(images_dev, setup[5])
    assert rec.shape == (5, 16) and per_image == [5, 0]


def test_there_is_no_fallback(setup):
    images_dev = torch.from_numpy(setup[4]).to(DEV)
    hip_layers.set_enabled(False)
    try:
        with pytest.raises(RuntimeError, match="no CPU / operator fallback"):
            predictor(setup)(images_dev, setup[5])
    finally:
        hip_layers.set_enabled(True)
    with pytest.raises(RuntimeError, match="outside the HIP forward"):
        predictor(setup, test_size=(100, 128))(images_dev, setup[5])
    with pytest.raises(RuntimeError, match="on the device"):
        predictor(setup)(torch.from_numpy(setup[4]), None)
