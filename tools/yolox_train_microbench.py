"""Microbenchmark of YOLOX training on one MI355X: forward + backward of one ``BaseConv`` (convolution, BatchNorm with batch statistics,
SiLU) at a few of YOLOX-x's shapes, and of the whole YOLOX-x ``model(x, targets)`` + ``backward()`` at 640 x 640, each in two variants,
in one process, on the same modules and tensors:

    hip      ``hip_layers.set_train_kernels(True)``: ``train_layers.ConvBnSilu`` — the fp32-MFMA convolution, csrc/conv_bn_bwd.hip;
    torch    the switch off: PyTorch's operators on the same commit (MIOpen convolutions and BatchNorm, ATen's SiLU and their backward).

The input of a layer and every parameter are leaves; every gradient is asked for.  The losses of the model run on csrc/yolox_loss.hip in
both variants.

Measured per variant: the host clock around ``--reps`` forward + backward steps that end in a device synchronise, the two variants
alternating within each of ``--rounds`` rounds after a warm-up of both; median / min / max over the rounds.  Nothing is gated and no
speed is promised: at narrow widths the 128 x 128 tile of the weight gradient multiplies mostly zeros.

    python tools/yolox_train_microbench.py [--out profiles/yolox_train_microbench.json] [--batch 8] [--model-batch 2] [--reps 5] [--rounds 5]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, Cin, Cout, ks, stride, H = W of the input) of YOLOX-x (width 1.25) at 640 x 640
LAYERS = (("focus 12->80 3x3", 12, 80, 3, 1, 320), ("dark2 80->160 3x3/2", 80, 160, 3, 2, 320), ("dark3 csp 160->160 1x1", 160, 160, 1, 1, 80),
          ("dark3 bottleneck 160->160 3x3", 160, 160, 3, 1, 80), ("dark4 320->640 3x3/2", 320, 640, 3, 2, 40),
          ("dark5 bottleneck 640->640 3x3", 640, 640, 3, 1, 20), ("head 320->320 3x3", 320, 320, 3, 1, 80))


def timed(variants, reps, rounds):
    """{name: [ms per step]} for alternating variants after a warm-up of each."""
    import torch

    for _, fn in variants:
        for _ in range(2):
            fn()
    torch.cuda.synchronize()
    times = {name: [] for name, _ in variants}
    for _ in range(rounds):
        for name, fn in variants:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) / reps * 1e3)
    return times


def summary(times):
    out = {f"{name}_fwd_bwd_ms": {"median": statistics.median(v), "min": min(v), "max": max(v)} for name, v in times.items()}
    out["torch_over_hip"] = out["torch_fwd_bwd_ms"]["median"] / out["hip_fwd_bwd_ms"]["median"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yolox_train_microbench.json"))
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--model-batch", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--no-model", action="store_true")
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.det.yolox.models import build_yolox
    from gdrnpp_bop2022_amd.det.yolox.models.network_blocks import BaseConv
    from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers

    assert torch.cuda.is_available(), "yolox_train_microbench needs the GPU"
    hip_lib.load()
    dev = torch.device("cuda")
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds, "layers": [], "model": None}

    def switched(flag, fn):
        hip_layers.set_train_kernels(flag)
        try:
            return fn()
        finally:
            hip_layers.set_train_kernels(False)

    for name, cin, cout, ks, stride, hw in LAYERS:
        torch.manual_seed(cin + cout)
        layer = BaseConv(cin, cout, ks, stride).to(dev).train()
        layer.bn.eps, layer.bn.momentum = 1e-3, 0.03
        x = torch.randn(args.batch, cin, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        g = torch.randn(args.batch, cout, hw // stride, hw // stride, device=dev).contiguous(memory_format=torch.channels_last)
        leaves = [x] + list(layer.parameters())

        def step(flag):
            for t in leaves:
                t.grad = None
            y = switched(flag, lambda: layer(x))
            y.backward(g)
            return [y.detach()] + [t.grad for t in leaves]

        a, b = step(True), step(False)
        agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
        del a, b
        case = {"layer": name, "batch": args.batch, "cin": cin, "cout": cout, "ks": ks, "stride": stride, "hw": hw,
                "max_relative_difference_hip_vs_torch": agree}
        case.update(summary(timed((("hip", lambda: step(True)), ("torch", lambda: step(False))), args.reps, args.rounds)))
        result["layers"].append(case)
        print(json.dumps(case))
        del x, g, leaves, layer
        torch.cuda.empty_cache()

    if not args.no_model:
        torch.manual_seed(0)
        model = build_yolox(1.33, 1.25, num_classes=21).to(dev).train()
        b = args.model_batch
        x = torch.randn(b, 3, 640, 640, device=dev)
        targets = torch.zeros(b, 4, 5, device=dev)
        targets[:, :3, 0] = torch.randint(0, 21, (b, 3), device=dev).float()
        targets[:, :3, 1:3] = 120.0 + 400.0 * torch.rand(b, 3, 2, device=dev)
        targets[:, :3, 3:5] = 40.0 + 160.0 * torch.rand(b, 3, 2, device=dev)

        def model_step(flag):
            model.zero_grad(set_to_none=True)
            _, losses = switched(flag, lambda: model(x, targets))
            total = sum(losses.values())
            total.backward()
            return total.detach()

        case = {"model": "YOLOX-x", "batch": b, "input": [640, 640], "loss_hip": float(model_step(True)), "loss_torch": float(model_step(False))}
        case.update(summary(timed((("hip", lambda: model_step(True)), ("torch", lambda: model_step(False))), max(1, args.reps // 2), args.rounds)))
        result["model"] = case
        print(json.dumps(case))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
