"""Microbenchmark of the trainable dwconv7x7 + LayerNorm on one MI355X: forward + backward of ``hip_layers.DwConvLN`` (the inference
kernel forward, csrc/dwconv_ln_bwd.hip backward) against the same layer on PyTorch's operators (Conv2d(C, C, 7, padding=3, groups=C) then
F.layer_norm over the NHWC view: what ``hip_layers.dwconv_ln`` runs with the training switch off), in one process, on the same tensors.

Shapes: the four ConvNeXt-B stages of a 256 x 256 ROI, 64 x 64 x 128 down to 8 x 8 x 1024, at ``--rois`` 48 (SOLVER.IMS_PER_BATCH of the
reference's training configs) and 8.  x, the four parameters and grad_y are leaves; every gradient is asked for.

Measured per variant: the host clock around ``--reps`` forward + backward steps that end in a device synchronise, the two variants
alternating within each of ``--rounds`` rounds after a warm-up of both; median / min / max over the rounds.  Per pass of the HIP backward:
the device time of each kernel from one separately profiled step (torch.profiler device events; "not measured" when the profiler gives
none), with the bytes and FMAs the pass needs — computed from the shape here — over that time, beside the peaks DESIGN.md uses (8 TB/s
HBM, 157.3 TFLOP/s fp32 and 78.6 TFLOP/s fp64 vector; an FMA = 2 FLOP).  Nothing here is gated.

    python tools/dwconv_ln_bwd_microbench.py [--out profiles/dwconv_ln_bwd_microbench.json] [--rois 48 8] [--reps 20] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ((64, 128), (32, 256), (16, 512), (8, 1024))      # (H = W, C)
PEAKS = {"hbm_TBps": 8.0, "fp32_vector_TFLOPs": 157.3, "fp64_vector_TFLOPs": 78.6}
PASSES = {"dwln_bwd_du_kernel": "du", "dwln_bwd_dx_kernel": "dx", "dwln_bwd_dw_kernel": "dw", "dwln_bwd_finalize_kernel": "finalize",
          "dwconv7_ln_kernel": "forward"}


def algorithmic(n, h, w, c):
    """Per pass: (bytes read once + written once, FMAs, their precision).  E = elements of one activation tensor."""
    e = n * h * w * c
    return {"forward": (8 * e, 49 * e, "fp32"),
            "du": (12 * e, 49 * e, "fp64"),           # reads x and grad_y, writes du; the convolution again, in fp64
            "dx": (8 * e, 49 * e, "fp32"),            # reads du, writes dx
            "dw": (8 * e, 49 * e, "fp32"),            # reads du and x (seven times each, out of L2), writes partials
            "finalize": (0, 0, "fp64")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dwconv_ln_bwd_microbench.json"))
    ap.add_argument("--rois", type=int, nargs="+", default=[48, 8])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers

    assert torch.cuda.is_available(), "dwconv_ln_bwd_microbench needs the GPU"
    hip_lib.load()
    dev = torch.device("cuda")
    result = {"device": torch.cuda.get_device_name(0), "peaks": PEAKS, "reps": args.reps, "rounds": args.rounds, "cases": []}
    for n in args.rois:
        for hw, c in STAGES:
            torch.manual_seed(n * 10000 + c)
            conv = torch.nn.Conv2d(c, c, 7, padding=3, groups=c).to(dev)
            ln = torch.nn.LayerNorm(c, eps=1e-6).to(dev)
            x = torch.randn(n, c, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            g = torch.randn(n, hw, hw, c, device=dev)
            leaves = (x, conv.weight, conv.bias, ln.weight, ln.bias)

            def step(train_kernels):
                for t in leaves:
                    t.grad = None
                hip_layers.set_train_kernels(train_kernels)
                try:
                    y = hip_layers.dwconv_ln(conv, ln, x, {})
                finally:
                    hip_layers.set_train_kernels(False)
                y.backward(g)
                return [y.detach()] + [t.grad for t in leaves]

            variants = (("hip", lambda: step(True)), ("torch", lambda: step(False)))
            a, b = step(True), step(False)
            agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
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
            case = {"rois": n, "H": hw, "W": hw, "C": c, "max_relative_difference_hip_vs_torch": agree,
                    "workspace_bytes": int(hip_lib.load().gdrnpp_dwconv7x7_ln_backward_workspace_bytes(n, hw, hw, c))}
            for name, v in times.items():
                case[f"{name}_fwd_bwd_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
            case["torch_over_hip"] = case["torch_fwd_bwd_ms"]["median"] / case["hip_fwd_bwd_ms"]["median"]
            # per pass: one profiled step of each variant, outside the timed rounds
            alg = algorithmic(n, hw, hw, c)
            try:
                from torch.autograd import DeviceType
                from torch.profiler import ProfilerActivity, profile

                kernels = {}
                for name, fn in variants:
                    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                        fn()
                        torch.cuda.synchronize()
                    ev = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
                    kernels[name] = ev
                passes = {}
                for e in kernels["hip"]:
                    key = next((v for k, v in PASSES.items() if k in e.name), None)
                    if key is None:
                        continue
                    us = float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0))
                    nbytes, fma, prec = alg[key]
                    passes[key] = {"us": us, "algorithmic_bytes": nbytes, "fma": fma, "fma_precision": prec,
                                   "TBps": nbytes / us * 1e-6 if us else None, "TFMAps": fma / us * 1e-6 if us else None}
                case["hip_passes"] = passes or "not measured"
                tk = {}
                for e in kernels["torch"]:
                    us = float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0))
                    tk[e.name[:80]] = tk.get(e.name[:80], 0.0) + us
                case["torch_kernels_us"] = tk or "not measured"
            except Exception as exc:      # noqa: BLE001
                case["hip_passes"] = case["torch_kernels_us"] = "not measured: " + repr(exc)[:200]
            result["cases"].append(case)
            print(json.dumps(case))
            del x, g, conv, ln, a, b
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
