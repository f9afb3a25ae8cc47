"""NumPy restatement of ``cv2.resize(img, (dw, dh), interpolation=cv2.INTER_LINEAR)`` for 8-bit images and of the
reference's ``preproc`` (det/yolox/data/data_augment.py:161-177) on top of it.

cv2 is not installed where these tests run, so the resize is restated from OpenCV's source (modules/imgproc/src/resize.cpp,
the generic fixed-point path every 8-bit INTER_LINEAR call takes):

  * ``dsize == ssize``: a copy;
  * INTER_LINEAR with an exact 2:1 reduction in both axes becomes INTER_AREA's fast path: ``(a + b + c + d + 2) >> 2``;
  * otherwise, per axis, ``scale = 1. / (dst / src)`` (double), ``f = (float)((d + 0.5) * scale - 0.5)``, ``s = floor(f)``,
    ``f -= s`` (float); columns: ``s < 0 -> s = 0, f = 0`` and ``s >= src - 1 -> s = src - 1, f = 0``; rows: the indices ``s`` and
    ``s + 1`` are clipped to the image, the fraction stays; coefficients ``saturate_cast<short>(c * 2048)`` (round half to even)
    of ``1.f - f`` and ``f``; horizontal pass ``S[s] * a0 + S[s + 1] * a1`` in int; vertical pass
    ``uchar((((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2)``.

``bilinear_f64`` is the yardstick the restatement is measured against: half-pixel-centre bilinear interpolation in float64
with replicated borders, unrounded."""
import numpy as np

COEF_BITS = 11
COEF_ONE = 1 << COEF_BITS
PAD = 114


def sizes(H, W, test_size):
    """preproc's own arithmetic: (r, rh, rw)."""
    r = min(test_size[0] / H, test_size[1] / W)
    return r, int(H * r), int(W * r)


def _axis(dst, src, clamp_fraction):
    scale = 1.0 / (np.float64(dst) / np.float64(src))
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp_fraction:
        lo = s < 0
        f[lo], s[lo] = 0.0, 0
        hi = s >= src - 1
        f[hi], s[hi] = 0.0, src - 1
    c0 = np.rint((np.float32(1.0) - f) * np.float32(COEF_ONE)).astype(np.int64)
    c1 = np.rint(f * np.float32(COEF_ONE)).astype(np.int64)
    i0 = np.clip(s, 0, src - 1)
    i1 = np.clip(s + 1, 0, src - 1)
    return i0, i1, c0, c1


def resize_linear_u8(img, dw, dh):
    """cv2.resize(img, (dw, dh), interpolation=cv2.INTER_LINEAR) for uint8 [H,W,C]."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    H, W, _ = img.shape
    if (dh, dw) == (H, W):
        return img.copy()
    if H == 2 * dh and W == 2 * dw:
        s = img.astype(np.int64)
        return ((s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2).astype(np.uint8)
    x0, x1, a0, a1 = _axis(dw, W, True)
    y0, y1, b0, b1 = _axis(dh, H, False)
    s = img.astype(np.int64)
    hor = s[:, x0] * a0[None, :, None] + s[:, x1] * a1[None, :, None]              # [H, dw, C]
    r0, r1 = hor[y0], hor[y1]
    out = (((b0[:, None, None] * (r0 >> 4)) >> 16) + ((b1[:, None, None] * (r1 >> 4)) >> 16) + 2) >> 2
    return (out & 255).astype(np.uint8)


class _Cv2:
    """What ``preproc`` asks of cv2, served by the restatement."""
    INTER_LINEAR = 1

    @staticmethod
    def resize(img, dsize, interpolation=1):
        assert interpolation == _Cv2.INTER_LINEAR
        return resize_linear_u8(img, int(dsize[0]), int(dsize[1]))


def preproc(img, input_size, swap=(2, 0, 1)):
    """The reference's preproc, restated: -> (f32[3,Ht,Wt], r)."""
    padded = np.full((input_size[0], input_size[1], 3), PAD, np.uint8)
    r, rh, rw = sizes(img.shape[0], img.shape[1], input_size)
    padded[:rh, :rw] = resize_linear_u8(img, rw, rh)
    return np.ascontiguousarray(padded.transpose(swap), dtype=np.float32), r


def bilinear_f64(img, dw, dh):
    """Half-pixel-centre bilinear in float64, borders replicated, unrounded: the yardstick of the fixed-point path."""
    H, W, _ = img.shape
    s = img.astype(np.float64)

    def axis(dst, src):
        f = (np.arange(dst) + 0.5) * (src / dst) - 0.5
        i = np.floor(f)
        return np.clip(i, 0, src - 1).astype(int), np.clip(i + 1, 0, src - 1).astype(int), f - i

    x0, x1, fx = axis(dw, W)
    y0, y1, fy = axis(dh, H)
    hor = s[:, x0] * (1 - fx)[None, :, None] + s[:, x1] * fx[None, :, None]
    return hor[y0] * (1 - fy)[:, None, None] + hor[y1] * fy[:, None, None]


# the fixture's cases: name -> (B, H, W, (Ht, Wt)); images are seeded per case (tests/golden/make_golden_letterbox.py)
CASES = {
    "copy_96x128": (1, 96, 128, (128, 128)),
    "up_60x80": (1, 60, 80, (128, 128)),
    "area_256x256": (1, 256, 256, (128, 128)),
    "hbound_100x60": (1, 100, 60, (128, 96)),
    "down_135x180": (1, 135, 180, (160, 160)),
    "batch3_w81": (3, 57, 81, (96, 128)),
    "wide_50x200": (1, 50, 200, (128, 224)),
    "rw200_64x100": (1, 64, 100, (128, 224)),
}
# size arithmetic only (no pixels stored)
SIZE_CASES = [(540, 720, (640, 640)), (480, 640, (640, 640)), (100, 60, (128, 96)), (1080, 1920, (640, 640)), (400, 640, (416, 416))]
IMAGE_SEED = 20221103


def case_images(name):
    import zlib

    b, h, w, _ = CASES[name]
    rng = np.random.RandomState((IMAGE_SEED + zlib.crc32(name.encode())) % (1 << 31))
    img = rng.randint(0, 256, (b, h, w, 3)).astype(np.uint8)
    # smooth half: a ramp keeps neighbouring taps close, noise keeps them far apart — both ends of the rounding
    ramp = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 256).astype(np.uint8)
    img[:, :, : w // 2, 1] = ramp[:, : w // 2]
    return img
