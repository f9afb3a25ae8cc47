"""Generate tests/golden/letterbox_golden.npz: the reference's OWN ``preproc`` and ``ValTransform(legacy=False)``
(det/yolox/data/data_augment.py:161-177,230-259) executed from source through _refimport.py (authoring container only).

cv2 is not installed, so the one cv2 call of ``preproc`` — ``cv2.resize(img, (w, h), interpolation=cv2.INTER_LINEAR)`` — is
served by tests/letterbox_ref.py's restatement of OpenCV's 8-bit path.  Everything else is the reference's text: the 114 canvas,
``r = min(...)``, the two ``int(...)`` products, the top-left paste, the transpose and the float conversion.

Per case of letterbox_ref.CASES (images are re-drawn from their seed, not stored): r, rh, rw, the output as uint8 (every value
is a whole grey level; float32 in the reference) and a sha256 of the reference's float32 bytes.  SIZE_CASES store r, rh, rw only.

    python tests/golden/make_golden_letterbox.py
"""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import _refimport  # noqa: E402
import letterbox_ref as LR  # noqa: E402


def main():
    _refimport.install()
    import det.yolox.data.data_augment as DA

    asked = []          # the (w, h) the reference hands to cv2.resize: its own int() products

    class Cv2(LR._Cv2):
        @staticmethod
        def resize(img, dsize, interpolation=1):
            asked.append((int(dsize[0]), int(dsize[1])))
            return LR._Cv2.resize(img, dsize, interpolation)

    DA.cv2 = Cv2
    out = {"cases": np.array(list(LR.CASES)), "size_cases": np.array([[h, w, t[0], t[1]] for h, w, t in LR.SIZE_CASES], np.int64)}
    val = DA.ValTransform(legacy=False)
    for name, (b, h, w, tsize) in LR.CASES.items():
        imgs = LR.case_images(name)
        res = []
        for i in range(b):
            x, r = DA.preproc(imgs[i], tsize)
            xv, _ = val(imgs[i], None, tsize)
            assert x.dtype == np.float32 and np.array_equal(x, xv)
            assert np.array_equal(x, np.round(x)) and x.min() >= 0 and x.max() <= 255
            res.append(x)
        x = np.stack(res)
        out[f"{name}/r"] = np.float64(r)
        out[f"{name}/rh_rw"] = np.array([asked[-1][1], asked[-1][0]], np.int64)
        out[f"{name}/out_u8"] = x.astype(np.uint8)
        out[f"{name}/sha256_f32"] = np.array(hashlib.sha256(np.ascontiguousarray(x).tobytes()).hexdigest())
        out[f"{name}/image_sha256"] = np.array(hashlib.sha256(imgs.tobytes()).hexdigest())
    rs = []
    for h, w, t in LR.SIZE_CASES:
        _, r = DA.preproc(np.zeros((h, w, 3), np.uint8), t)
        rs.append([r, asked[-1][1], asked[-1][0]])
    out["size_r_rh_rw"] = np.array(rs, np.float64)
    path = os.path.join(HERE, "letterbox_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
