"""det/yolox/data: YOLOX's training batches — the host's draws and box arithmetic (``data_augment``, ``mosaic``) around one
``hip_lib.yolox_train_inputs`` call for the pixels."""
from .data_augment import (apply_affine_to_bboxes, get_affine_matrix, get_aug_params, getRotationMatrix2D, hsv_luts,  # noqa: F401
                           train_transform_plan)
from .mosaic import MOSAIC_DEFAULTS, MosaicDetectionHip, draw_mosaic_item, get_mosaic_coordinate  # noqa: F401
