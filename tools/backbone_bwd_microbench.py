"""Microbenchmark of the trainable ConvNeXt stem and downsample layers on one MI355X: forward + backward of ``hip_layers.StemConvLN`` and
``hip_layers.DownsampleLNConv`` (csrc/backbone_bwd.hip and the exact-f32 products around it) against the same layers on PyTorch's
operators (what ``hip_layers.stem`` / ``hip_layers.downsample`` run with the training switch off), in one process, on the same tensors.

Shapes: the stem on 256 x 256 images and the three stage entries of ConvNeXt-B behind it (64 x 64 x 128, 32 x 32 x 256, 16 x 16 x 512),
at ``--rois`` 48 (SOLVER.IMS_PER_BATCH of the reference's training configs) and 8.  The parameters and grad_y are leaves, and so is the
downsample's input; the image is not (the stem layer exists for images without a gradient).

Measured per variant: the host clock around ``--reps`` forward + backward steps that end in a device synchronise, the two variants
alternating within each of ``--rounds`` rounds after a warm-up of both; median / min / max over the rounds.  Nothing here is gated: a
ratio below 1 is reported as it is.

    python tools/backbone_bwd_microbench.py [--out profiles/backbone_bwd_microbench.json] [--rois 48 8] [--reps 20] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DOWNSAMPLES = ((64, 128, 256), (32, 256, 512), (16, 512, 1024))      # (H = W, C, Cout)
STEM_HW = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "backbone_bwd_microbench.json"))
    ap.add_argument("--rois", type=int, nargs="+", default=[48, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers
    from gdrnpp_bop2022_amd.gdrn_modeling.backbones import LayerNorm2d

    assert torch.cuda.is_available(), "backbone_bwd_microbench needs the GPU"
    hip_lib.load()
    dev = torch.device("cuda")
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "cases": []}

    def measure(case, leaves, forward, g):
        def step(train_kernels):
            for t in leaves:
                t.grad = None
            hip_layers.set_train_kernels(train_kernels)
            try:
                y = forward()
            finally:
                hip_layers.set_train_kernels(False)
            y.backward(g)
            return [y.detach()] + [t.grad for t in leaves]

        variants = (("hip", lambda: step(True)), ("torch", lambda: step(False)))
        a, b = step(True), step(False)
        case["max_relative_difference_hip_vs_torch"] = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
        for _, fn in variants:
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        times = {"hip": [], "torch": []}
        for _ in range(args.rounds):
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    fn()
                torch.cuda.synchronize()
                times[name].append((time.perf_counter() - t0) / args.reps * 1e3)
        for name, v in times.items():
            case[f"{name}_fwd_bwd_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        case["torch_over_hip"] = case["torch_fwd_bwd_ms"]["median"] / case["hip_fwd_bwd_ms"]["median"]
        result["cases"].append(case)
        print(json.dumps(case))

    for n in args.rois:
        torch.manual_seed(n)
        conv, ln = torch.nn.Conv2d(3, 128, 4, stride=4).to(dev), LayerNorm2d(128, eps=1e-6).to(dev)
        x = torch.randn(n, 3, STEM_HW, STEM_HW, device=dev)
        g = torch.randn(n, STEM_HW // 4, STEM_HW // 4, 128, device=dev).permute(0, 3, 1, 2)
        measure({"layer": "stem", "rois": n, "H": STEM_HW, "W": STEM_HW, "C": 3, "Cout": 128,
                 "workspace_bytes": int(hip_lib.load().gdrnpp_stem_conv4x4_ln_backward_workspace_bytes(n, STEM_HW, STEM_HW, 128))},
                (conv.weight, conv.bias, ln.weight, ln.bias), lambda: hip_layers.stem(conv, ln, x), g)
        del x, g
        for hw, c, cout in DOWNSAMPLES:
            torch.manual_seed(n * 10000 + c)
            ln, conv = LayerNorm2d(c, eps=1e-6).to(dev), torch.nn.Conv2d(c, cout, 2, stride=2).to(dev)
            x = torch.randn(n, c, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            g = torch.randn(n, hw // 2, hw // 2, cout, device=dev).permute(0, 3, 1, 2)
            measure({"layer": "downsample", "rois": n, "H": hw, "W": hw, "C": c, "Cout": cout},
                    (x, ln.weight, ln.bias, conv.weight, conv.bias), lambda: hip_layers.downsample(ln, conv, x), g)
            del x, g
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
