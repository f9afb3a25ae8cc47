"""The request of an 8-bit ``cv2.resize(INTER_LINEAR)``: the host half of csrc/resize_u8.hpp.  The kernels that resize (``replace_bg``,
``yolox_train_inputs``) take sizes, form and interpolation scales from their tables and derive none of them; the loaders that fill those
tables (gdrn_modeling/train_inputs.py, det/yolox/data/mosaic.py) get them here.  No library call: NumPy and arithmetic."""
import numpy as np

RESIZE_MODES = ("copy", "area", "linear")                                     # cv2.resize's forms: a table's mode column = index
MODE_COPY, MODE_AREA, MODE_LINEAR = range(len(RESIZE_MODES))
DBL_EPSILON = float(np.finfo(np.float64).eps)


def cv_round(x) -> int:
    """OpenCV's cvRound / saturate_cast<int>(double): to the nearest integer, halves to the even one."""
    return int(np.rint(np.float64(x)))


def resize_request(cw, ch, *, dsize=None, fx=None, fy=None) -> dict:
    """The sizes, form and interpolation scales of an 8-bit ``cv2.resize(crop, dsize, fx=fx, fy=fy, interpolation=INTER_LINEAR)`` of a
    cw x ch crop -> dict(dw, dh, mode, scale_x, scale_y).

    OpenCV's modules/imgproc/src/resize.cpp as recalled — OpenCV is not installed where this project is built and tested and was not
    run: without a dsize, dsize = (cvRound(cw fx), cvRound(ch fy)) and the interpolation scale is 1. / fx, NOT src / dst; with a dsize
    the scale is 1. / (dst / src).  Then, in this order: dsize == ssize is a copy; a scale within DBL_EPSILON of exactly 2 on both axes
    turns INTER_LINEAR into the 2 x 2 area mean; everything else is the fixed-point linear path with these scales."""
    if dsize is None:
        inv_x, inv_y = float(fx), float(fy)
        dw, dh = cv_round(cw * inv_x), cv_round(ch * inv_y)
    else:
        dw, dh = int(dsize[0]), int(dsize[1])
        inv_x, inv_y = float(dw) / cw, float(dh) / ch
    if dw < 1 or dh < 1:
        raise ValueError(f"resize_request: a {cw} x {ch} crop resized to {dw} x {dh}: cv2.resize refuses an empty destination")
    scale_x, scale_y = 1.0 / inv_x, 1.0 / inv_y
    if (dw, dh) == (cw, ch):
        mode = MODE_COPY
    elif all(abs(s - cv_round(s)) < DBL_EPSILON and cv_round(s) == 2 for s in (scale_x, scale_y)):
        if 2 * dw > cw or 2 * dh > ch:
            raise NotImplementedError(f"resize_request: 2:1 area mean of {cw} x {ch} into {dw} x {dh}: OpenCV's ragged last cell is not restated")
        mode = MODE_AREA
    else:
        mode = MODE_LINEAR
    return dict(dw=dw, dh=dh, mode=mode, scale_x=scale_x, scale_y=scale_y)
