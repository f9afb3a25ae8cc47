"""YOLOX detector modules (import-compatible with the reference's ``det.yolox.models``)."""
from .darknet import CSPDarknet
from .network_blocks import BaseConv, Bottleneck, CSPLayer, Focus, SPPBottleneck
from .yolo_head import YOLOXHead
from .yolo_pafpn import YOLOPAFPN
from .yolox import YOLOX, build_yolox

__all__ = ["YOLOX", "YOLOPAFPN", "YOLOXHead", "CSPDarknet", "BaseConv", "Bottleneck", "CSPLayer", "SPPBottleneck", "Focus", "build_yolox"]
