"""YOLOX-x forward at 640 x 640 on one MI355X: the HIP path (csrc/yolox_net.hip) against the same module with
``hip_layers.set_enabled(False)`` (PyTorch-ROCm fp32 operators), in one process on one box.

Per batch size (1 and 8): milliseconds per image, launches, GFLOP per image recomputed from the layer list and the fraction of
the f32 matrix floor (FLOP / 157 TFLOP/s); per distinct convolution shape at its natural size: milliseconds of both paths.
Method: warm-up, HIP events around ``iters`` back-to-back forwards, median of ``repeats``.

    python tools/microbench_yolox.py [--out profiles/yolox_forward_microbench.json]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gdrnpp_bop2022_amd import hip_lib  # noqa: E402
from gdrnpp_bop2022_amd.det.yolox.models import build_yolox  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers, slice_layers  # noqa: E402

F32_MATRIX_TFLOPS = 157.0
DEV = "cuda"


def timed(fn, iters, repeats, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / iters)
    return statistics.median(ms)


def layer_list(net, h, w):
    """(conv module, input height, input width) of every convolution, from forward hooks on the module path (CPU, batch 1)."""
    seen = []
    hooks = [m.register_forward_hook(lambda m, i, o: seen.append((m, i[0].shape[2], i[0].shape[3]))) for m in net.modules()
             if isinstance(m, nn.Conv2d)]
    with torch.no_grad():
        net(torch.zeros(1, 3, h, w))
    for hk in hooks:
        hk.remove()
    return seen


def conv_flop(m, h, w):
    k, s = m.kernel_size[0], m.stride[0]
    oh, ow = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
    return 2.0 * oh * ow * m.out_channels * m.in_channels * k * k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolox_forward_microbench.json"))
    ap.add_argument("--size", type=int, default=640)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    hip_lib.load()
    torch.manual_seed(0)
    net = build_yolox(1.33, 1.25, 21)
    layers = layer_list(net, args.size, args.size)
    gflop = sum(conv_flop(m, h, w) for m, h, w in layers) / 1e9
    net = net.to(DEV)
    out = dict(model="YOLOX-x, 21 classes", input=[args.size, args.size], gflop_per_image=gflop, convolutions=len(layers),
               hip_launches_per_forward=len(layers) + 4, f32_matrix_tflops=F32_MATRIX_TFLOPS,
               floor_ms_per_image=gflop / F32_MATRIX_TFLOPS, device=torch.cuda.get_device_name(0), method=dict(iters=args.iters, repeats=args.repeats),
               batches={}, conv_shapes=[])
    for b in (1, 8):
        x = torch.randn(b, 3, args.size, args.size, device=DEV)
        with torch.no_grad():
            run = lambda: net(x)  # noqa: E731
            n0 = hip_layers.fallback_launches()
            hip_ms = timed(run, args.iters, args.repeats)
            assert hip_layers.fallback_launches() == n0
            hip_layers.set_enabled(False)
            try:
                op_ms = timed(run, args.iters, args.repeats)
            finally:
                hip_layers.set_enabled(True)
        out["batches"][str(b)] = dict(hip_ms_per_image=hip_ms / b, operators_ms_per_image=op_ms / b, hip_over_operators=hip_ms / op_ms,
                                      hip_fraction_of_f32_floor=gflop / F32_MATRIX_TFLOPS / (hip_ms / b))
        print(f"batch {b}: HIP {hip_ms / b:.3f} ms/image, operators {op_ms / b:.3f} ms/image, floor {gflop / F32_MATRIX_TFLOPS:.3f} ms", flush=True)
    # per distinct convolution shape at its size in the 640 x 640 forward, batch 8: Conv2d + BatchNorm2d + SiLU against one launch
    shapes = {}
    for m, h, w in layers:
        shapes.setdefault((m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], h, w), 0)
        shapes[(m.in_channels, m.out_channels, m.kernel_size[0], m.stride[0], h, w)] += 1
    b = 8
    for (cin, cout, k, s, h, w), count in sorted(shapes.items()):
        conv = nn.Conv2d(cin, cout, k, s, k // 2, bias=False).to(DEV)
        bn = nn.BatchNorm2d(cout, eps=1e-3).to(DEV).eval()
        xb = torch.randn(b, h, w, cin, device=DEV)
        x_cl = xb.permute(0, 3, 1, 2)
        oh, ow = (h + 2 * (k // 2) - k) // s + 1, (w + 2 * (k // 2) - k) // s + 1
        yb = torch.empty(b, oh, ow, cout, device=DEV)
        with torch.no_grad():
            hip_ms = timed(lambda: slice_layers.conv_bn_act_slice(conv, bn, "silu", slice_layers.NhwcSlice(xb), slice_layers.NhwcSlice(yb)), args.iters, args.repeats)
            op_ms = timed(lambda: F.silu(bn(conv(x_cl))), args.iters, args.repeats)
        fl = 2.0 * b * oh * ow * cout * cin * k * k
        out["conv_shapes"].append(dict(cin=cin, cout=cout, k=k, stride=s, h=h, w=w, batch=b, layers=count, hip_ms=hip_ms, operators_ms=op_ms,
                                       hip_tflops=fl / hip_ms / 1e9))
        print(f"{cin:5d} -> {cout:5d} k{k} s{s} {h:3d}x{w:<3d} x{count:2d}: HIP {hip_ms:.3f} ms ({fl / hip_ms / 1e9:.1f} TFLOP/s), operators {op_ms:.3f} ms", flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
