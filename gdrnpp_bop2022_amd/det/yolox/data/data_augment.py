"""det/yolox/data/data_augment.py: the host half of the training augmentation — the affine matrix, the boxes, the HSV LUTs and what
``TrainTransform`` decides — in NumPy, in the reference's dtypes and order of operations.  The pixels are ``hip_lib.yolox_train_inputs``'
(csrc/yolox_aug.hip); ``mosaic.MosaicDetectionHip`` joins the two.

Every function that draws takes its generator: ``py_random`` has ``random`` / ``uniform`` / ``randint`` (the ``random`` module, or a
``random.Random``), ``np_random`` has ``rand`` / ``uniform`` (``np.random``, or a ``RandomState``)."""
import math
import random

import numpy as np


def xyxy2cxcywh(bboxes):
    """det/yolox/utils/boxes.py:131-136, in place."""
    bboxes[:, 2] = bboxes[:, 2] - bboxes[:, 0]
    bboxes[:, 3] = bboxes[:, 3] - bboxes[:, 1]
    bboxes[:, 0] = bboxes[:, 0] + bboxes[:, 2] * 0.5
    bboxes[:, 1] = bboxes[:, 1] + bboxes[:, 3] * 0.5
    return bboxes


def adjust_box_anns(bbox, scale_ratio, padw, padh, w_max, h_max):
    """det/yolox/utils/boxes.py:119-122, in place."""
    bbox[:, 0::2] = np.clip(bbox[:, 0::2] * scale_ratio + padw, 0, w_max)
    bbox[:, 1::2] = np.clip(bbox[:, 1::2] * scale_ratio + padh, 0, h_max)
    return bbox


def get_aug_params(value, center=0, py_random=None):
    py_random = random if py_random is None else py_random
    if isinstance(value, float):
        return py_random.uniform(center - value, center + value)
    if len(value) == 2:
        return py_random.uniform(value[0], value[1])
    raise ValueError(f"Affine params should be either a sequence containing two values or single float values. Got {value}")


def getRotationMatrix2D(center, angle, scale):
    """cv2.getRotationMatrix2D as published (modules/imgproc/src/imgwarp.cpp): a = cos(angle) scale, b = sin(angle) scale in double,
    rows [a, b, (1 - a) cx - b cy] and [-b, a, b cx + (1 - a) cy]."""
    angle = angle * (math.pi / 180)         # `angle *= CV_PI / 180`: the constant is formed first
    a, b = math.cos(angle) * scale, math.sin(angle) * scale
    cx, cy = float(center[0]), float(center[1])
    return np.array([[a, b, (1 - a) * cx - b * cy], [-b, a, b * cx + (1 - a) * cy]], np.float64)


def get_affine_matrix(target_size, degrees=10, translate=0.1, scales=0.1, shear=10, py_random=None):
    """-> (M f64[2,3], scale).  Draws, in this order: angle, scale, shear x, shear y, translation x, translation y."""
    twidth, theight = target_size
    angle = get_aug_params(degrees, py_random=py_random)
    scale = get_aug_params(scales, center=1.0, py_random=py_random)
    if scale <= 0.0:
        raise ValueError("Argument scale should be positive")
    R = getRotationMatrix2D(center=(0, 0), angle=angle, scale=scale)
    M = np.ones([2, 3])
    shear_x = math.tan(get_aug_params(shear, py_random=py_random) * math.pi / 180)
    shear_y = math.tan(get_aug_params(shear, py_random=py_random) * math.pi / 180)
    M[0] = R[0] + shear_y * R[1]
    M[1] = R[1] + shear_x * R[0]
    M[0, 2] = get_aug_params(translate, py_random=py_random) * twidth
    M[1, 2] = get_aug_params(translate, py_random=py_random) * theight
    return M, scale


def apply_affine_to_bboxes(targets, target_size, M, scale):
    """The four corners of every box through M, their bounding box, clipped to the target; written into targets[:, :4]."""
    num_gts = len(targets)
    twidth, theight = target_size
    corner_points = np.ones((4 * num_gts, 3))
    corner_points[:, :2] = targets[:, [0, 1, 2, 3, 0, 3, 2, 1]].reshape(4 * num_gts, 2)      # x1y1, x2y2, x1y2, x2y1
    corner_points = corner_points @ M.T
    corner_points = corner_points.reshape(num_gts, 8)
    corner_xs = corner_points[:, 0::2]
    corner_ys = corner_points[:, 1::2]
    new_bboxes = np.concatenate((corner_xs.min(1), corner_ys.min(1), corner_xs.max(1), corner_ys.max(1))).reshape(4, num_gts).T
    new_bboxes[:, 0::2] = new_bboxes[:, 0::2].clip(0, twidth)
    new_bboxes[:, 1::2] = new_bboxes[:, 1::2].clip(0, theight)
    targets[:, :4] = new_bboxes
    return targets


def hsv_luts(r, dtype=np.uint8):
    """augment_hsv's three LUTs for the gains r = uniform(-1, 1, 3) * [hgain, sgain, vgain] + 1 -> dtype[3,256] (hue, saturation, value)."""
    x = np.arange(0, 256, dtype=np.int16)
    lut_hue = ((x * r[0]) % 180).astype(dtype)
    lut_sat = np.clip(x * r[1], 0, 255).astype(dtype)
    lut_val = np.clip(x * r[2], 0, 255).astype(dtype)
    return np.stack([lut_hue, lut_sat, lut_val])


def preproc_sizes(height, width, input_size):
    """preproc's arithmetic -> (r, resized w, resized h)."""
    r = min(input_size[0] / height, input_size[1] / width)
    return r, int(width * r), int(height * r)


def train_transform_plan(targets, image_hw, input_dim, *, max_labels=50, flip_prob=0.5, hsv_prob=1.0, hsv_gains=(0.5, 0.5, 0.5),
                         py_random=None, np_random=None):
    """What ``TrainTransform(max_labels, flip_prob, hsv_prob)(image, targets, input_dim)`` decides for an image of ``image_hw`` and its
    ``targets`` [n,5] (x1, y1, x2, y2, class) -> dict(empty, hsv, hsv_r, mirror, fallback, r, padded_labels f32[max_labels,5] of
    (class, cx, cy, w, h)).

    Draws, in this order, none of them when there is no box: ``py_random.random()`` against hsv_prob; if it wins
    ``np_random.uniform(-1, 1, 3)`` (augment_hsv's gains, times ``hsv_gains``, plus 1 -> hsv_r); ``py_random.random()`` against flip_prob.
    fallback: no box is left with min(w, h) > 1 after the resize, and the transform returns the image before the HSV pass and the
    mirror with its boxes before the mirror."""
    py_random = random if py_random is None else py_random
    np_random = np.random if np_random is None else np_random
    targets = np.asarray(targets)
    boxes = targets[:, :4].copy()
    labels = targets[:, 4].copy()
    height, width = int(image_hw[0]), int(image_hw[1])
    r_, _, _ = preproc_sizes(height, width, input_dim)
    plan = dict(empty=len(boxes) == 0, hsv=False, hsv_r=None, mirror=False, fallback=False, r=r_)
    if plan["empty"]:
        plan["padded_labels"] = np.zeros((max_labels, 5), dtype=np.float32)
        return plan
    targets_o = targets.copy()
    boxes_o = xyxy2cxcywh(targets_o[:, :4])
    labels_o = targets_o[:, 4]
    if py_random.random() < hsv_prob:
        plan["hsv"] = True
        plan["hsv_r"] = np_random.uniform(-1, 1, 3) * list(hsv_gains) + 1
    if py_random.random() < flip_prob:
        plan["mirror"] = True
        boxes[:, 0::2] = width - boxes[:, 2::-2]
    boxes = xyxy2cxcywh(boxes)
    boxes *= r_
    mask_b = np.minimum(boxes[:, 2], boxes[:, 3]) > 1
    boxes_t = boxes[mask_b]
    labels_t = labels[mask_b]
    if len(boxes_t) == 0:
        plan["fallback"] = True
        boxes_o *= r_
        boxes_t = boxes_o
        labels_t = labels_o
    labels_t = np.expand_dims(labels_t, 1)
    targets_t = np.hstack((labels_t, boxes_t))
    padded_labels = np.zeros((max_labels, 5))
    padded_labels[range(len(targets_t))[:max_labels]] = targets_t[:max_labels]
    plan["padded_labels"] = np.ascontiguousarray(padded_labels, dtype=np.float32)
    return plan
