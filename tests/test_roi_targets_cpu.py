"""-m "not gpu": the per-ROI training targets without a device.

tests/golden/readdata_train_golden.npz holds what the reference's ``read_data_train`` returned, executed from its source
(tests/golden/make_golden_readdata_train.py).  Here: the NumPy restatement tests/roi_targets_ref.py reproduces every array and scalar of
it exactly, ``train_targets.aug_bbox_dzi`` reproduces its centres and scales under its seeds, the restatement's explicit distance
expression picks what scipy's ``cdist`` picks, and ``train_targets.roi_train_targets`` — with the kernel call replaced by the restatement —
applies the reference's config-to-outputs rules and reproduces the fixture through the host API."""
import numpy as np
import pytest
import torch

from gdrnpp_bop2022_amd import hip_lib
from gdrnpp_bop2022_amd.gdrn_modeling import train_targets as TT
from tests import roi_targets_golden as RG
from tests import roi_targets_ref as RR

VARIANTS = ("l1_visib", "ce_trunc", "ce_obj", "ce_only_full")


def test_fixture_covers_what_it_should():
    g = RG.load()
    W, H = g["im_size"]
    assert (W, H) == (200, 136) and tuple(g["variants"]) == VARIANTS and len(g["keys"]) == 12
    v = g["variants"]
    assert v["l1_visib"][:2] == ("L1", "visib") and {v[t][:3] for t in ("ce_trunc", "ce_obj")} == {("CE_coor/L1", "trunc", 64), ("CE_coor/L1", "obj", 64)}
    assert {v[t][3] for t in VARIANTS} >= {64, 4} and {v[t][4] for t in VARIANTS} == {"VISIB", "AMODAL_CLIP"}
    assert {v[t][5] for t in VARIANTS} == {"uniform", "none"}
    invisible = [k for k in g["keys"] if not g["records"][k]["xyz_crop"].any()]
    assert len(invisible) == 2
    for tag in VARIANTS:
        for k in invisible:
            # the tools' record of an invisible instance is the whole image: 199 px plain, and the DZI's >= 0.75 x 1.5 x 199 is clamped to 200
            assert not RG.recorded(tag, k, "roi_mask_obj").any() and float(RG.recorded(tag, k, "scale")) <= 200.0
            if v[tag][4] == "VISIB":
                assert float(RG.recorded(tag, k, "scale")) == (200.0 if v[tag][5] == "uniform" else 199.0)
        # only the "syn" instance went through replace_bg: its truncated mask differs from the visible one
        differs = [k for k in g["keys"] if not np.array_equal(RG.recorded(tag, k, "roi_mask_trunc"), RG.recorded(tag, k, "roi_mask_visib"))]
        assert differs == [g["syn_key"]], (tag, differs)
    assert (RG.recorded("l1_visib", g["keys"][0], "roi_xyz") == 0.5).any()                 # the background of an unclipped roi_xyz
    clipped = [RG.recorded("ce_obj", k, "roi_xyz") for k in g["keys"]]
    assert max(c.max() for c in clipped) == np.float32(0.999999) and min(c.min() for c in clipped) == 0.0      # the clipping had work


def restate(tag, key):
    """One fixture instance through the restatement -> its maps and host scalars."""
    g = RG.load()
    W, H = g["im_size"]
    loss_type, mask_gt, n_bin, num_regions, bbox_type, dzi_type = g["variants"][tag]
    bbox = RG.bbox_of(tag, key)
    center, scale = RR.aug_bbox_dzi_ref(bbox, H, W, dzi_type, 1.5, 0.25, 0.25, RG.rng_of(tag, key))
    ce = "CE" in loss_type
    cls = int(RG.given(key, "roi_cls"))
    out = RR.roi_targets_ref(RR.paste(g["records"][key], W, H), center, scale, 64, visib=RG.given(key, "segmentation"),
                             trunc=RG.given(key, "mask_trunc") if key == g["syn_key"] else None, full=RG.given(key, "mask_full"),
                             extent=g["extents"][cls], fps=g["fps"][num_regions][cls] if num_regions > 1 else None, n_bin=n_bin if ce else 0,
                             bin_mask=mask_gt)
    if ce and not ("/" in loss_type and loss_type.split("/")[1]):
        del out["roi_xyz"]
    bw, bh = max(bbox[2] - bbox[0], 1), max(bbox[3] - bbox[1], 1)
    resize_ratio = 64 / scale
    delta_c = RG.given(key, "centroid_2d") - center
    out.update(bbox_center=center.astype(np.float32), scale=np.float64(scale), roi_wh=np.array([bw, bh], np.float32), resize_ratio=np.float64(resize_ratio),
               trans_ratio=np.array([delta_c[0] / bw, delta_c[1] / bh, float(RG.given(key, "trans")[2]) / resize_ratio]).astype(np.float32))
    return out


@pytest.mark.parametrize("tag", VARIANTS)
def test_restatement_reproduces_the_reference(tag):
    for key in RG.load()["keys"]:
        RG.assert_same(restate(tag, key), tag, key, "restatement")


@pytest.mark.parametrize("tag", VARIANTS)
def test_aug_bbox_dzi_under_the_fixture_seeds(tag):
    g = RG.load()
    W, H = g["im_size"]
    cfg = RG.cfg_of(tag)
    for key in g["keys"]:
        center, scale = TT.aug_bbox_dzi(cfg, RG.bbox_of(tag, key), H, W, RG.rng_of(tag, key))
        assert center.dtype == np.float64 and isinstance(scale, float)
        assert np.array_equal(center.astype(np.float32), RG.recorded(tag, key, "bbox_center")), (tag, key)
        assert scale == float(RG.recorded(tag, key, "scale")) and scale <= max(H, W), (tag, key)


def test_aug_bbox_dzi_draw_order_clamp_and_refusals():
    cfg = RG.cfg_of("l1_visib")
    rng = np.random.RandomState(7)
    s, sh = rng.random_sample(), rng.random_sample(2)
    center, scale = TT.aug_bbox_dzi(cfg, [10, 20, 50, 100], 136, 200, np.random.RandomState(7))
    assert np.array_equal(center, [30 + 40 * (0.25 * (2 * sh[0] - 1)), 60 + 80 * (0.25 * (2 * sh[1] - 1))])
    assert scale == 80 * (1 + 0.25 * (2 * s - 1)) * 1.5
    assert TT.aug_bbox_dzi(cfg, [0, 0, 199, 135], 136, 200, np.random.RandomState(1))[1] == 200.0       # clamped to max(H, W)
    cfg.INPUT.DZI_TYPE = "none"
    center, scale = TT.aug_bbox_dzi(cfg, [10, 20, 50, 100], 136, 200, None)                           # the plain box draws nothing
    assert center.tolist() == [30.0, 60.0] and scale == 80.0
    for t in ("roi10d", "truncnorm"):
        cfg.INPUT.DZI_TYPE = t
        with pytest.raises(NotImplementedError):
            TT.aug_bbox_dzi(cfg, [10, 20, 50, 100], 136, 200, np.random.RandomState(1))


def test_region_equals_scipy_cdist():
    cdist = pytest.importorskip("scipy.spatial.distance").cdist
    g = RG.load()
    for key in g["keys"]:
        cls = int(RG.given(key, "roi_cls"))
        center, scale = RR.aug_bbox_dzi_ref(RG.bbox_of("l1_visib", key), 136, 200, "uniform", 1.5, 0.25, 0.25, RG.rng_of("l1_visib", key))
        roi_xyz = RR.P.warp_affine(RR.paste(g["records"][key], 200, 136), RR.P.get_affine_transform(center, scale, 64), 64, nearest=True)
        for F in (4, 64):
            d = cdist(roi_xyz.reshape(-1, 3), g["fps"][F][cls])
            want = (np.argmin(d, axis=1).reshape(64, 64) + 1) * (roi_xyz != 0).any(-1)
            assert np.array_equal(RR.region_of(roi_xyz, g["fps"][F][cls]), want), (key, F)


def fake_kernel(packed, table, centers, scales, im_size, **kw):
    """``hip_lib.roi_train_targets`` served by the restatement on the host."""
    host = lambda x: x.cpu().numpy() if isinstance(x, torch.Tensor) else x          # noqa: E731
    res = RR.batch_ref(host(packed), table, host(centers), host(scales), im_size, **{k: host(v) for k, v in kw.items()})
    return {k: torch.from_numpy(v) for k, v in res.items()}


@pytest.mark.parametrize("tag", VARIANTS)
def test_host_api_reproduces_the_reference_with_the_kernel_restated(tag, monkeypatch):
    monkeypatch.setattr(hip_lib, "roi_train_targets", fake_kernel)
    g = RG.load()
    masks, _ = RG.host_masks()
    num_regions = g["variants"][tag][3]
    out = TT.roi_train_targets(RG.cfg_of(tag), RG.instances(), [g["records"][k] for k in g["keys"]], g["im_size"], g["extents"],
                               g["fps"][num_regions] if num_regions > 1 else None, masks=masks, rng=[RG.rng_of(tag, k) for k in g["keys"]], device="cpu")
    assert np.array_equal(out["roi_cls"], [int(RG.given(k, "roi_cls")) for k in g["keys"]])
    for i, key in enumerate(g["keys"]):
        RG.assert_same({k: (v[i].numpy() if isinstance(v, torch.Tensor) else v[i]) for k, v in out.items() if k in RG.MAPS + RG.HOST}, tag, key, "host api")


@pytest.mark.parametrize("loss_type,num_regions,keys", [
    ("L1", 64, {"roi_region", "roi_xyz"}), ("L1", 1, {"roi_xyz"}), ("L1", 0, {"roi_xyz"}), ("CE_coor", 4, {"roi_region", "roi_xyz_bin"}),
    ("CE_coor/", 1, {"roi_xyz_bin"}), ("CE_coor/L1", 64, {"roi_region", "roi_xyz_bin", "roi_xyz"}), ("MSE", 4, {"roi_region", "roi_xyz"})])
def test_config_to_outputs_rules(loss_type, num_regions, keys, monkeypatch):
    calls = []

    def spy(*a, **kw):
        calls.append(kw)
        return fake_kernel(*a, **kw)

    monkeypatch.setattr(hip_lib, "roi_train_targets", spy)
    g = RG.load()
    cfg = RG.cfg_of("l1_visib")
    cfg.MODEL.POSE_NET.LOSS_CFG.XYZ_LOSS_TYPE = loss_type
    cfg.MODEL.POSE_NET.GEO_HEAD.NUM_REGIONS = num_regions
    cfg.MODEL.POSE_NET.GEO_HEAD.XYZ_BIN = 32
    cfg.MODEL.POSE_NET.OUTPUT_RES = 16
    fps = g["fps"][num_regions] if num_regions > 1 else None
    insts = RG.instances()[:2]
    for i in insts:
        del i["full_idx"]
    out = TT.roi_train_targets(cfg, insts, [g["records"][k] for k in g["keys"]], g["im_size"], g["extents"], fps, masks=RG.host_masks()[0],
                               rng=np.random.RandomState(3), device="cpu")
    masks = {"roi_mask_trunc", "roi_mask_visib", "roi_mask_obj"}                     # no instance has a full mask: no roi_mask_full
    assert {k for k in out if k.startswith("roi_") and k not in ("roi_wh", "roi_cls")} == masks | keys
    assert len(calls) == 1 and calls[0]["out_res"] == 16 and calls[0]["n_bin"] == (32 if "CE" in loss_type else 0) and calls[0]["bin_mask"] == "visib"
    assert out["roi_mask_obj"].shape == (2, 16, 16) and out["roi_wh"].dtype == torch.float32 and out["trans_ratio"].shape == (2, 3)
    if "roi_xyz_bin" in keys:
        assert out["roi_xyz_bin"].dtype == torch.uint8 and int(out["roi_xyz_bin"].max()) <= 32
    if "roi_region" in keys:
        assert out["roi_region"].dtype == torch.int32 and int(out["roi_region"].max()) <= num_regions


def test_host_api_refusals(monkeypatch):
    monkeypatch.setattr(hip_lib, "roi_train_targets", fake_kernel)
    g = RG.load()
    recs = [g["records"][k] for k in g["keys"]]
    call = lambda cfg, insts, fps=g["fps"][64]: TT.roi_train_targets(cfg, insts, recs, g["im_size"], g["extents"], fps, masks=RG.host_masks()[0],    # noqa: E731
                                                                     rng=np.random.RandomState(3), device="cpu")
    cfg = RG.cfg_of("l1_visib")
    with pytest.raises(ValueError, match="NUM_REGIONS"):
        call(cfg, RG.instances()[:1], g["fps"][4])
    cfg.MODEL.BBOX_TYPE = "nonsense"
    with pytest.raises(ValueError, match="BBOX_TYPE"):
        call(cfg, RG.instances()[:1])
    cfg = RG.cfg_of("ce_only_full")
    insts = RG.instances()[:1]
    del insts[0]["full_idx"]
    with pytest.raises(ValueError, match="full"):
        call(cfg, insts, None)
    cfg = RG.cfg_of("l1_visib")
    cfg["TRAIN"] = dict(VIS=True)
    with pytest.raises(NotImplementedError):
        call(cfg, RG.instances()[:1])
