"""CSPDarknet, the YOLOX backbone: Focus stem, then four stages of [3x3 stride-2 BaseConv, CSPLayer]; the last stage holds
the SPP block between the two."""
import torch.nn as nn

from .network_blocks import BaseConv, CSPLayer, Focus, SPPBottleneck, _no_depthwise


class CSPDarknet(nn.Module):
    def __init__(self, dep_mul, wid_mul, out_features=("dark3", "dark4", "dark5"), depthwise=False, act="silu"):
        super().__init__()
        _no_depthwise(depthwise)
        assert out_features, "out_features must name at least one stage"
        self.out_features = out_features
        c = int(wid_mul * 64)
        n = max(round(dep_mul * 3), 1)
        self.stem = Focus(3, c, ksize=3, act=act)
        self.dark2 = nn.Sequential(BaseConv(c, 2 * c, 3, 2, act=act), CSPLayer(2 * c, 2 * c, n=n, act=act))
        self.dark3 = nn.Sequential(BaseConv(2 * c, 4 * c, 3, 2, act=act), CSPLayer(4 * c, 4 * c, n=3 * n, act=act))
        self.dark4 = nn.Sequential(BaseConv(4 * c, 8 * c, 3, 2, act=act), CSPLayer(8 * c, 8 * c, n=3 * n, act=act))
        self.dark5 = nn.Sequential(BaseConv(8 * c, 16 * c, 3, 2, act=act), SPPBottleneck(16 * c, 16 * c, activation=act),
                                   CSPLayer(16 * c, 16 * c, n=n, shortcut=False, act=act))

    def forward(self, x):
        out = {}
        for name in ("stem", "dark2", "dark3", "dark4", "dark5"):
            x = getattr(self, name)(x)
            out[name] = x
        return {k: v for k, v in out.items() if k in self.out_features}
