"""NumPy restatement of the training loader's background replacement — ``replace_bg``, ``trunc_mask``, ``get_bg_image``,
``get_bg_image_v2`` (reference core/base_data_loader.py:413-579) and ``resize_short_edge`` (core/utils/data_utils.py:208-235) — the
yardstick of ``hip_lib.replace_bg`` and ``gdrn_modeling.train_inputs``.  tests/test_replace_bg_cpu.py ties it to what the reference's
own methods returned (tests/golden/replace_bg_golden.npz, written by tests/golden/make_golden_replace_bg.py).

It materialises what the reference materialises: the resized background as an image of its own, pasted top-left onto zeros of the
image's size; the boolean mask with a block of rows or columns cleared; one boolean-mask copy.

``cv2.resize`` is restated for 8-bit INTER_LINEAR in both of its calling forms from OpenCV's modules/imgproc/src/resize.cpp AS RECALLED:
cv2 is not installed where these tests run and was not run.  ``cv2.resize(im, None, None, fx=, fy=)`` makes
dsize = (cvRound(W fx), cvRound(H fy)), halves to even, and interpolates with the scale 1. / fx — not src / dst, which differs (a 37 x 28
crop with fx = 48 / 28 comes out 63 x 48 with the scale 0.58333 against 37 / 63 = 0.58730); ``cv2.resize(im, dsize)`` interpolates with
1. / (dst / src).  Then: dsize == ssize is a copy; a scale within DBL_EPSILON of exactly 2 on both axes is the area mean
``(a + b + c + d + 2) >> 2``; otherwise per axis ``f = (float)((d + 0.5) * scale - 0.5)``, ``s = floor(f)``, ``f -= s``; columns with s < 0
or s >= src - 1 are clamped and lose the fraction, row indices are clipped and keep it; coefficients ``saturate_cast<short>(c * 2048)``;
horizontal pass in int; vertical pass ``uchar((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2)`` — the arithmetic of
tests/letterbox_ref.py, with the scale handed in."""
import zlib

import numpy as np

COEF_ONE = 1 << 11
DBL_EPSILON = float(np.finfo(np.float64).eps)
CUTS = ("none", "upper", "bottom", "left", "right")


def cv_round(x):
    return int(np.rint(np.float64(x)))


def _axis(dst, src, scale, clamp_fraction):
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * np.float64(scale) - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp_fraction:
        lo = s < 0
        f[lo], s[lo] = 0.0, 0
        hi = s >= src - 1
        f[hi], s[hi] = 0.0, src - 1
    c0 = np.rint((np.float32(1.0) - f) * np.float32(COEF_ONE)).astype(np.int64)
    c1 = np.rint(f * np.float32(COEF_ONE)).astype(np.int64)
    return np.clip(s, 0, src - 1), np.clip(s + 1, 0, src - 1), c0, c1


def resize_request(w, h, dsize=None, fx=None, fy=None):
    """-> (dw, dh, scale_x, scale_y, form) of cv2.resize on a w x h image; form is "copy", "area" or "linear"."""
    if dsize is None:
        inv_x, inv_y = float(fx), float(fy)
        dw, dh = cv_round(w * inv_x), cv_round(h * inv_y)
    else:
        dw, dh = int(dsize[0]), int(dsize[1])
        inv_x, inv_y = float(dw) / w, float(dh) / h
    assert dw > 0 and dh > 0
    scale_x, scale_y = 1.0 / inv_x, 1.0 / inv_y
    if (dw, dh) == (w, h):
        return dw, dh, scale_x, scale_y, "copy"
    if all(abs(s - cv_round(s)) < DBL_EPSILON and cv_round(s) == 2 for s in (scale_x, scale_y)):
        return dw, dh, scale_x, scale_y, "area"
    return dw, dh, scale_x, scale_y, "linear"


def cv2_resize(img, dsize=None, fx=None, fy=None):
    """cv2.resize(img, dsize, fx=fx, fy=fy, interpolation=cv2.INTER_LINEAR) for uint8 [H,W,C]."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    H, W, _ = img.shape
    dw, dh, scale_x, scale_y, form = resize_request(W, H, dsize, fx, fy)
    if form == "copy":
        return img.copy()
    s = img.astype(np.int64)
    if form == "area":
        assert 2 * dw <= W and 2 * dh <= H, "the ragged last cell of OpenCV's area mean is not restated"
        e = s[:2 * dh, :2 * dw]
        return ((e[0::2, 0::2] + e[0::2, 1::2] + e[1::2, 0::2] + e[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    x0, x1, a0, a1 = _axis(dw, W, scale_x, True)
    y0, y1, b0, b1 = _axis(dh, H, scale_y, False)
    hor = s[:, x0] * a0[None, :, None] + s[:, x1] * a1[None, :, None]
    r0, r1 = hor[y0], hor[y1]
    out = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return (out & 255).astype(np.uint8)


def keep_aspect_crop(bg_h, bg_w, im_H, im_W):
    """get_bg_image's four aspect branches -> (cw, ch) of the crop [0:ch, 0:cw] (a slice beyond the image clips)."""
    ratio = float(im_H) / float(im_W)
    same = (ratio < 1 and float(bg_h) / float(bg_w) < 1) or (ratio >= 1 and float(bg_h) / float(bg_w) >= 1)
    if same:
        if bg_h >= bg_w:
            new = int(np.ceil(bg_w * ratio))
            return (bg_w, new) if new < bg_h else (bg_w, bg_h)
        new = int(np.ceil(bg_h / ratio))
        return (new, bg_h) if new < bg_w else (bg_w, bg_h)
    if bg_h >= bg_w:
        return bg_w, len(range(bg_h)[0:int(np.ceil(bg_w * ratio))])
    return len(range(bg_w)[0:int(np.ceil(bg_h / ratio))]), bg_h


def short_edge_scale(h, w, target_size, max_size):
    """resize_short_edge's im_scale."""
    im_scale = float(target_size) / float(min(h, w))
    if np.round(im_scale * max(h, w)) > max_size:
        im_scale = float(max_size) / float(max(h, w))
    return im_scale


def bg_image(bg, im_H, im_W, v2_crop=None):
    """get_bg_image (v2_crop None) or get_bg_image_v2 with its drawn (x1, y1, x2, y2) -> the im_H x im_W background."""
    bg = np.asarray(bg)
    if v2_crop is not None:
        x1, y1, x2, y2 = v2_crop
        return cv2_resize(bg[y1:y2, x1:x2], dsize=(im_W, im_H))
    cw, ch = keep_aspect_crop(bg.shape[0], bg.shape[1], im_H, im_W)
    s = short_edge_scale(ch, cw, min(im_H, im_W), max(im_H, im_W))
    small = cv2_resize(bg[0:ch, 0:cw], fx=s, fy=s)
    out = np.zeros((im_H, im_W, 3), np.uint8)
    out[0:small.shape[0], 0:small.shape[1]] = small          # raises where the reference's paste raises
    return out


def trunc_mask(mask, cut, u):
    """trunc_mask with its branch (index into CUTS) and the random.random() behind its random.uniform given.  An empty mask under a cut,
    where the reference raises in np.min, is returned as it is — the rule of the kernel, which sets a flag instead."""
    mask = np.asarray(mask) != 0
    if cut == 0 or not mask.any():
        return mask
    rows, cols = np.nonzero(mask)
    x1, x2, y1, y2 = int(rows.min()), int(rows.max()), int(cols.min()), int(cols.max())
    c_h, c_w = 0.5 * (x1 + x2), 0.5 * (y1 + y2)
    a, b = {1: (x1, c_h), 2: (c_h, x2), 3: (y1, c_w), 4: (c_w, y2)}[cut]
    line = int(a + (b - a) * float(u))
    mask = mask.copy()
    if cut == 1:
        mask[:line, :] = False
    elif cut == 2:
        mask[line:, :] = False
    elif cut == 3:
        mask[:, :line] = False
    else:
        mask[:, line:] = False
    return mask


def replace_bg_ref(im, mask, bg, cut=0, u=0.0, v2_crop=None):
    """replace_bg(im, mask, return_mask=True, truncate_fg=cut is drawn) on one image with one chosen background -> (composite u8[H,W,3],
    mask_trunc bool[H,W])."""
    im = np.array(im, np.uint8)
    H, W = im.shape[:2]
    keep = trunc_mask(mask, cut, u)
    back = bg_image(bg, H, W, v2_crop)
    im[~keep] = back[~keep]
    return im, keep


# ---- the fixture's cases: inputs are re-drawn from the name, nothing of them is stored ---------------------------------------------------
# name -> dict(H, W, bgs [(h, w)], mask kind, keep_aspect, truncate, img_type, prob, py_seed, np_seed)
def _case(H, W, bgs, mask, py_seed, *, keep_aspect=True, truncate=True, img_type="syn", prob=0.5, np_seed=0):
    return dict(H=H, W=W, bgs=bgs, mask=mask, keep_aspect=keep_aspect, truncate=truncate, img_type=img_type, prob=prob, py_seed=py_seed, np_seed=np_seed)


CASES = {
    # the four aspect branches of get_bg_image over three image shapes; seeds chosen to reach trunc_mask's five branches
    "h48w64_bg50x37_box": _case(48, 64, [(50, 37)], "box", 0),            # dw = 63: column 63 stays zero
    "h48w64_bg37x50_border": _case(48, 64, [(37, 50)], "border", 1),
    "h64w48_bg50x37_blob": _case(64, 48, [(50, 37)], "blob", 2),
    "h64w48_bg37x50_box": _case(64, 48, [(37, 50)], "box", 3),
    "h40w40_bg50x37_blob": _case(40, 40, [(50, 37)], "blob", 4),
    "h40w40_bg37x50_border": _case(40, 40, [(37, 50)], "border", 5),
    "pixel_bottom_h40w40": _case(40, 40, [(50, 37)], "pixel", 4),         # x1 == x2: "block bottom" empties the mask
    "pixel_upper_h40w40": _case(40, 40, [(37, 50)], "pixel", 2),
    "area_h24w32_bg48x64": _case(24, 32, [(48, 64)], "box", 0),           # fx = 0.5: the 2 x 2 mean
    "copy_h40w56_bg40x56": _case(40, 56, [(40, 56)], "blob", 3),          # dsize == ssize
    "w67_h33_bg45x90": _case(33, 67, [(45, 90)], "border", 5),            # the last wave of a row is partial
    "rows_h70w36_bg90x45": _case(70, 36, [(90, 45)], "blob", 4),          # more rows than one workgroup of either phase covers
    "pool3_h48w64": _case(48, 64, [(50, 37), (37, 50), (48, 64)], "blob", 7),
    "empty_notrunc_h40w40": _case(40, 40, [(37, 50)], "empty", 0, truncate=False),   # all background (with a cut the reference raises)
    "v2_h48w64_bg60x80": _case(48, 64, [(60, 80)], "box", 1, keep_aspect=False, np_seed=11),
    "v2_h40w40_bg37x50": _case(40, 40, [(37, 50)], "blob", 5, keep_aspect=False, np_seed=12),
    "real_replaced_h40w40": _case(40, 40, [(50, 37)], "box", 0, img_type="real", np_seed=1),
    "real_kept_h40w40": _case(40, 40, [(50, 37)], "box", 0, img_type="real", np_seed=0),
}
INPUT_SEED = 20221020


def case_inputs(name):
    """-> (image u8[H,W,3], mask u8[H,W], [background u8[h,w,3]])."""
    c = CASES[name]
    H, W = c["H"], c["W"]
    rng = np.random.RandomState((INPUT_SEED + zlib.crc32(name.encode())) % (1 << 31))
    image = rng.randint(0, 256, (H, W, 3)).astype(np.uint8)
    bgs = []
    for h, w in c["bgs"]:
        bg = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
        # a smooth half keeps neighbouring taps close, noise keeps them far apart: both ends of the rounding
        bg[:, : w // 2, 1] = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 256).astype(np.uint8)[:, : w // 2]
        bgs.append(bg)
    return image, make_mask(c["mask"], H, W, rng), bgs


def make_mask(kind, H, W, rng):
    """The instance masks: bytes 0, 1 and 255 (non-zero counts)."""
    m = np.zeros((H, W), np.uint8)
    if kind == "box":                                  # in the interior
        m[H // 4: H // 4 + H // 3, W // 5: W // 5 + W // 2] = 1
    elif kind == "border":                             # touches all four image borders
        m[H // 2 - 2: H // 2 + 3, :] = 1
        m[:, W // 3: W // 3 + 4] = 255
    elif kind == "pixel":
        m[H // 3, 2 * W // 3] = 1
    elif kind == "blob":                               # ragged, with holes
        m[H // 6: H - H // 5, W // 7: W - W // 4] = rng.choice(np.array([0, 1, 1, 255], np.uint8), (H - H // 5 - H // 6, W - W // 4 - W // 7))
    elif kind != "empty":
        raise KeyError(kind)
    return m
