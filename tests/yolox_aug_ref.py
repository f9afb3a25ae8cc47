"""NumPy restatement of YOLOX's training augmentation — the yardstick of ``hip_lib.yolox_train_inputs`` (csrc/yolox_aug.hip) and
``det.yolox.data``.  Two layers:

``Cv2``        the cv2 calls ``MosaicDetection`` and ``TrainTransform`` make (det/yolox/data/datasets/mosaicdetection.py,
               det/yolox/data/data_augment.py), restated for 8-bit images from OpenCV's published source AS RECALLED — cv2 is not installed
               where these tests run and was not run: ``resize`` (tests/replace_bg_ref.py), ``warpAffine`` (``warp_affine_u8``: the
               arithmetic of oracle/warp_oracle.c with a border value), ``getRotationMatrix2D``, ``cvtColor`` for the four HSV codes
               (the scalar path of modules/imgproc/src/color_hsv.simd.hpp: integer RGB -> HSV with the two division tables, hue range
               180; fp32 HSV -> RGB with every operation rounded on its own — OpenCV's SIMD builds may contract those products, so
               equality with a given cv2 binary is NOT measured), ``LUT``, ``split``, ``merge``.  Every call is logged.
``run_item``   the pipeline, driven by a plan (``det.yolox.data.mosaic.draw_mosaic_item``) instead of generators.

tests/test_yolox_aug_cpu.py ties both to what the reference's own code returned (tests/golden/yolox_aug_golden.npz, written by
tests/golden/make_golden_yolox_aug.py with this ``Cv2`` serving the reference)."""
import math
import zlib

import numpy as np

from tests import replace_bg_ref as RB

INTER_BITS, INTER_TAB = 5, 32
OPS = ("resize", "warpAffine", "cvtColor", "LUT", "split", "merge", "getRotationMatrix2D")


def invert_affine(M):
    """cv::warpAffine's inversion of the 2x3 map, in Python floats (oracle/warp_oracle.c ``invert_affine``)."""
    M = [float(v) for v in np.asarray(M, np.float64).reshape(6)]
    D = M[0] * M[4] - M[1] * M[3]
    D = 1.0 / D if D != 0 else 0.0
    A11, A22 = M[4] * D, M[0] * D
    M[0] = A11
    M[1] *= -D
    M[3] *= -D
    M[4] = A22
    b1 = -M[0] * M[2] - M[1] * M[5]
    b2 = -M[3] * M[2] - M[4] * M[5]
    M[2], M[5] = b1, b2
    return M


def warp_affine_u8(img, M, dsize, border=0):
    """cv2.warpAffine(img u8[H,W,C], M, dsize=(ow, oh), flags=INTER_LINEAR, borderValue=border)."""
    img = np.asarray(img)
    assert img.dtype == np.uint8 and img.ndim == 3
    H, W, _ = img.shape
    ow, oh = int(dsize[0]), int(dsize[1])
    Mi = invert_affine(M)
    x, y = np.arange(ow, dtype=np.float64), np.arange(oh, dtype=np.float64)
    adelta = np.rint(Mi[0] * x * 1024).astype(np.int64)
    bdelta = np.rint(Mi[3] * x * 1024).astype(np.int64)
    X0 = np.rint((Mi[1] * y + Mi[2]) * 1024).astype(np.int64) + 16
    Y0 = np.rint((Mi[4] * y + Mi[5]) * 1024).astype(np.int64) + 16
    X = (X0[:, None] + adelta[None, :]) >> 5
    Y = (Y0[:, None] + bdelta[None, :]) >> 5
    sx, sy = np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767)
    fx, fy = X & 31, Y & 31
    w = np.stack([(32 - fy) * (32 - fx) * 32, (32 - fy) * fx * 32, fy * (32 - fx) * 32, fy * fx * 32])
    zero = (fx == 0) & (fy == 0)              # the table's entry 0: saturate_cast<short>(32768) and the sum fix-up
    w[0][zero], w[3][zero] = 32767, 1
    acc = np.full((oh, ow, img.shape[2]), 1 << 14, np.int64)
    for t in range(4):
        xx, yy = sx + (t & 1), sy + (t >> 1)
        inside = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
        tap = np.where(inside[:, :, None], img[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)].astype(np.int64), int(border))
        acc += tap * w[t][:, :, None]
    return np.clip(acc >> 15, 0, 255).astype(np.uint8)


def div_tables():
    """OpenCV's sdiv_table / hdiv_table for hue range 180: round-half-even of (255 << 12) / i and (180 << 12) / (6 i), entry 0 = 0."""
    sdiv, hdiv = np.zeros(256, np.int64), np.zeros(256, np.int64)
    for i in range(1, 256):
        sdiv[i] = int(np.rint((255 << 12) / (1.0 * i)))
        hdiv[i] = int(np.rint((180 << 12) / (6.0 * i)))
    return sdiv, hdiv


SDIV, HDIV = div_tables()


def to_hsv_u8(img, rgb):
    """cv2.cvtColor(img, COLOR_RGB2HSV if rgb else COLOR_BGR2HSV) for uint8 [...,3]."""
    img = np.asarray(img).astype(np.int64)
    b, g, r = (img[..., 2], img[..., 1], img[..., 0]) if rgb else (img[..., 0], img[..., 1], img[..., 2])
    v = np.maximum(b, np.maximum(g, r))
    diff = v - np.minimum(b, np.minimum(g, r))
    s = (diff * SDIV[v] + (1 << 11)) >> 12
    h = np.where(v == r, g - b, np.where(v == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * HDIV[diff] + (1 << 11)) >> 12
    h = h + np.where(h < 0, 180, 0)
    return np.stack([h, s, v], -1).astype(np.uint8)


SECTORS = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])


def from_hsv_u8(img, rgb):
    """cv2.cvtColor(img, COLOR_HSV2RGB if rgb else COLOR_HSV2BGR) for uint8 [...,3]: float32, one rounding per operation."""
    img = np.asarray(img)
    f32 = np.float32
    h, s, v = img[..., 0], img[..., 1], img[..., 2]
    hf = h.astype(f32) * (f32(6.0) / f32(180.0))
    sf = s.astype(f32) * (f32(1.0) / f32(255.0))
    vf = v.astype(f32) * (f32(1.0) / f32(255.0))
    while (hf >= 6).any():
        hf = np.where(hf >= 6, hf - f32(6.0), hf).astype(f32)
    sector = np.floor(hf).astype(np.int64)
    f = hf - sector.astype(f32)
    one = f32(1.0)
    tab = np.stack([vf, vf * (one - sf), vf * (one - sf * f), vf * (one - sf * (one - f))], -1)
    assert tab.dtype == np.float32
    bgr = np.take_along_axis(tab, SECTORS[sector], -1)
    bgr = np.where((s == 0)[..., None], vf[..., None], bgr).astype(f32)
    out = np.clip(np.rint(bgr * f32(255.0)), 0, 255).astype(np.uint8)
    return out[..., ::-1].copy() if rgb else out


def getRotationMatrix2D(center, angle, scale):
    angle = angle * (math.pi / 180)
    a, b = math.cos(angle) * scale, math.sin(angle) * scale
    cx, cy = float(center[0]), float(center[1])
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], np.float64)


class Cv2:
    """The cv2 namespace the reference's two files use, with a log of [op, a, b, c, d] rows: resize / warpAffine (source w, h,
    destination w, h), cvtColor (code, w, h), LUT / split / merge (w, h)."""
    INTER_LINEAR, INTER_NEAREST = 1, 0
    COLOR_BGR2HSV, COLOR_RGB2HSV, COLOR_HSV2BGR, COLOR_HSV2RGB = 40, 41, 54, 55

    def __init__(self):
        self.log = []

    def _note(self, op, *v):
        self.log.append([OPS.index(op)] + [int(x) for x in v] + [0] * (4 - len(v)))

    def resize(self, src, dsize, interpolation=1):
        assert interpolation == 1
        out = RB.cv2_resize(src, dsize=dsize)
        self._note("resize", src.shape[1], src.shape[0], out.shape[1], out.shape[0])
        return out

    def warpAffine(self, src, M, dsize, borderValue=(0, 0, 0)):
        assert len(set(borderValue)) == 1
        self._note("warpAffine", src.shape[1], src.shape[0], dsize[0], dsize[1])
        return warp_affine_u8(src, M, dsize, borderValue[0])

    def getRotationMatrix2D(self, center, angle, scale):
        return getRotationMatrix2D(center, angle, scale)

    def cvtColor(self, src, code, dst=None):
        self._note("cvtColor", code, src.shape[1], src.shape[0])
        assert src.dtype == np.uint8
        if code in (self.COLOR_BGR2HSV, self.COLOR_RGB2HSV):
            out = to_hsv_u8(src, code == self.COLOR_RGB2HSV)
        else:
            assert code in (self.COLOR_HSV2BGR, self.COLOR_HSV2RGB), code
            out = from_hsv_u8(src, code == self.COLOR_HSV2RGB)
        if dst is not None:
            dst[...] = out
            return dst
        return out

    def LUT(self, src, lut):
        self._note("LUT", src.shape[1], src.shape[0])
        assert src.dtype == np.uint8 and lut.shape == (256,)
        return lut[src]

    def split(self, m):
        self._note("split", m.shape[1], m.shape[0])
        return [np.ascontiguousarray(m[..., k]) for k in range(m.shape[2])]

    def merge(self, mv):
        self._note("merge", mv[0].shape[1], mv[0].shape[0])
        return np.stack(mv, -1)


# ---- the pipeline, driven by a plan -----------------------------------------------------------------------------------------------------

def augment_hsv(cv2, img, luts, rgb):
    """augment_hsv with its three LUTs given, in place."""
    hue, sat, val = cv2.split(cv2.cvtColor(img, cv2.COLOR_RGB2HSV if rgb else cv2.COLOR_BGR2HSV))
    img_hsv = cv2.merge((cv2.LUT(hue, luts[0]), cv2.LUT(sat, luts[1]), cv2.LUT(val, luts[2]))).astype(np.uint8)
    cv2.cvtColor(img_hsv, cv2.COLOR_HSV2RGB if rgb else cv2.COLOR_HSV2BGR, dst=img)


def preproc(cv2, img, input_size):
    padded = np.ones((input_size[0], input_size[1], 3), dtype=np.uint8) * 114
    r = min(input_size[0] / img.shape[0], input_size[1] / img.shape[1])
    resized = cv2.resize(img, (int(img.shape[1] * r), int(img.shape[0] * r)), interpolation=cv2.INTER_LINEAR).astype(np.uint8)
    padded[: int(img.shape[0] * r), : int(img.shape[1] * r)] = resized
    return np.ascontiguousarray(padded.transpose(2, 0, 1), dtype=np.float32)


def run_item(item, luts_of, cv2=None):
    """The image f32[3,H,W] of one item's plan.  ``luts_of(r)`` -> the three LUTs of the gains r (``data_augment.hsv_luts``)."""
    cv2 = Cv2() if cv2 is None else cv2
    H, W = item["input_dim"]
    src = item["sources"]
    if item["branch"] == "plain":
        img = np.array(src[0]["image"])
    else:
        canvas = np.full((2 * H, 2 * W, 3), 114, np.uint8)
        for s in src[:4]:
            tile = cv2.resize(s["image"], (s["dw"], s["dh"]), interpolation=cv2.INTER_LINEAR)
            canvas[s["l_y"]: s["l_y"] + s["ph"], s["l_x"]: s["l_x"] + s["pw"]] = tile[s["s_y"]: s["s_y"] + s["ph"], s["s_x"]: s["s_x"] + s["pw"]]
        img = cv2.warpAffine(canvas, item["M"], dsize=(W, H), borderValue=(114, 114, 114))
        if item["branch"] == "mixup":
            s, mix = src[4], item["mix"]
            cp = np.ones((H, W, 3), np.uint8) * 114
            cp[: s["dh"], : s["dw"]] = cv2.resize(s["image"], (s["dw"], s["dh"]), interpolation=cv2.INTER_LINEAR)
            cp = cv2.resize(cp, (mix["jw"], mix["jh"]))
            if mix["flip"]:
                cp = cp[:, ::-1, :]
            padded = np.zeros((max(mix["jh"], H), max(mix["jw"], W), 3), np.uint8)
            padded[: mix["jh"], : mix["jw"]] = cp
            crop = padded[mix["y_off"]: mix["y_off"] + H, mix["x_off"]: mix["x_off"] + W]
            img = (0.5 * img.astype(np.float32) + 0.5 * crop.astype(np.float32)).astype(np.uint8)
    if item["empty"]:
        out = preproc(cv2, img, (H, W))
    else:
        image_o = img.copy()
        if item["hsv"]:
            augment_hsv(cv2, img, luts_of(item["hsv_r"]), False)
        out = preproc(cv2, img[:, ::-1] if item["mirror"] else img, (H, W))
        if item["fallback"]:
            out = preproc(cv2, image_o, (H, W))
    if item["branch"] != "plain" and item["hsv2"]:
        t = out.transpose(2, 1, 0).astype(np.uint8).copy()
        augment_hsv(cv2, t, luts_of(item["hsv2_r"]), item["hsv2_rgb"])
        out = t.transpose(2, 1, 0).astype(np.float32).copy()
    return out


# ---- the fixture's cases: datasets are re-drawn from the case, nothing of them is stored ---------------------------------------------------

class StubDataset:
    """What ``MosaicDetection`` asks of its dataset: ``pull_item``, ``load_anno``, ``__len__``, ``input_dim`` — seeded synthetic images of the
    given (h, w) with ``boxes[k]`` boxes each, sides in ``box_px``.  ``pull_item`` hands out copies: the reference's HSV pass writes into
    the image it was given."""

    def __init__(self, sizes, boxes, input_dim, seed, box_px=(6, 20)):
        rng = np.random.RandomState(seed % (1 << 31))
        self.input_dim = input_dim
        self.images, self.annos, self.anno_calls = [], [], 0
        for (h, w), n in zip(sizes, boxes):
            im = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
            # a smooth half keeps neighbouring taps close, noise keeps them far apart; a grey band has s == 0
            im[:, : w // 2, 1] = (np.add.outer(np.arange(h) * 3, np.arange(w) * 2) % 256).astype(np.uint8)[:, : w // 2]
            im[h // 2: h // 2 + 3] = im[h // 2: h // 2 + 3, :, :1]
            self.images.append(im)
            res = np.zeros((n, 5))
            for k in range(n):
                bw, bh = rng.uniform(*box_px, 2)
                x1, y1 = rng.uniform(0, max(w - bw, 1)), rng.uniform(0, max(h - bh, 1))
                res[k] = [x1, y1, min(x1 + bw, w), min(y1 + bh, h), rng.randint(0, 5)]
            self.annos.append(res)

    def __len__(self):
        return len(self.images)

    def load_anno(self, index):
        self.anno_calls += 1
        return self.annos[index]

    def pull_item(self, index):
        im = self.images[index]
        return im.copy(), self.annos[index].copy(), f"{index}/{index}", (im.shape[0], im.shape[1]), index


SIZES = [(32, 48), (64, 96), (40, 50), (20, 30), (24, 48)]      # copy, 2:1 area, linear down, linear up, copy with rows to spare
HSV2 = dict(AUG_HSV_PROB=1.0, HSV_H=0.3, HSV_S=0.5, HSV_V=0.4)


def _case(py_seed, np_seed=0, *, dim=(32, 48), boxes=(2, 3, 1, 2, 4), idx=0, enable_mosaic=True, box_px=(6, 20), expect=None, **kw):
    return dict(py_seed=py_seed, np_seed=np_seed, dim=dim, boxes=list(boxes), idx=idx, enable_mosaic=enable_mosaic, box_px=box_px,
                expect=expect or {}, kw=kw)


# expect: what the case is named for; make_golden_yolox_aug.py asserts it of the reference's run, test_yolox_aug_cpu.py of the plan
CASES = {
    "mixup_down_flip": _case(0, 1, mixup_scale=(0.5, 0.9), hsv_prob=1.0, expect=dict(branch="mixup", jit_up=False, flip=True, hsv=True)),
    "mixup_down_noflip": _case(105, 2, idx=1, mixup_scale=(0.5, 0.9), hsv_prob=0.0, expect=dict(branch="mixup", jit_up=False, flip=False, hsv=False)),
    "mixup_up_flip": _case(54, 3, idx=2, mixup_scale=(1.1, 1.5), hsv_prob=1.0, **HSV2, FORMAT="RGB",
                           expect=dict(branch="mixup", jit_up=True, flip=True, hsv=True, hsv2=True)),
    "mixup_up_noflip": _case(3, 4, idx=3, mixup_scale=(1.1, 1.5), hsv_prob=0.0, **HSV2, FORMAT="RGB",
                             expect=dict(branch="mixup", jit_up=True, flip=False, hsv=False, hsv2=True)),
    "mixup_redraw": _case(43, 5, idx=4, boxes=(0, 0, 0, 1, 0), expect=dict(branch="mixup", redraw=True)),
    "mosaic_nomixup": _case(5, 6, idx=1, enable_mixup=False, **HSV2, FORMAT="BGR", expect=dict(branch="mosaic", hsv2=True)),
    "mosaic_no_labels": _case(9, 7, idx=2, boxes=(0, 0, 0, 0, 0), hsv_prob=1.0, expect=dict(branch="mosaic", empty=True, hsv=False)),
    "mosaic_fallback": _case(7, 8, idx=3, mosaic_scale=(0.1, 0.1), enable_mixup=False, box_px=(2, 6), hsv_prob=1.0,
                             expect=dict(branch="mosaic", fallback=True)),
    "mosaic_max_labels": _case(21, 9, idx=4, max_labels=3, expect=dict(truncated=True)),
    "plain_mirror": _case(9, 10, idx=2, mosaic_prob=0.0, hsv_prob=1.0, expect=dict(branch="plain", mirror=True, hsv=True)),
    "plain_nomirror": _case(23, 11, idx=1, enable_mosaic=False, hsv_prob=0.0, expect=dict(branch="plain", mirror=False, hsv=False)),
    "plain_up": _case(11, 12, idx=3, enable_mosaic=False, hsv_prob=1.0, expect=dict(branch="plain", hsv=True)),
    "plain_copy": _case(13, 14, idx=0, enable_mosaic=False, hsv_prob=1.0, expect=dict(branch="plain", hsv=True)),
    "plain_rows_to_spare": _case(14, 15, idx=4, mosaic_prob=0.0, hsv_prob=0.0, expect=dict(branch="plain", hsv=False)),
    "tall_mixup": _case(12, 13, dim=(48, 32), idx=0, hsv_prob=1.0, **HSV2, FORMAT="RGB", expect=dict(branch="mixup", hsv=True, hsv2=True)),
}
INPUT_SEED = 20221021


def case_dataset(name):
    c = CASES[name]
    return StubDataset(SIZES, c["boxes"], c["dim"], INPUT_SEED + zlib.crc32(name.encode()), c["box_px"])


def observed(item):
    """The properties ``expect`` may name, read from a plan."""
    mix = item["mix"]
    return dict(branch=item["branch"], jit_up=None if mix is None else (mix["jw"] > item["input_dim"][1] and mix["jh"] > item["input_dim"][0]),
                flip=None if mix is None else mix["flip"], hsv=item["hsv"], hsv2=item["hsv2"], mirror=item["mirror"], fallback=item["fallback"],
                empty=item["empty"])
