"""Microbenchmark of a trainable ConvNeXt block on one MI355X: forward + backward of one ``ConvNeXtBlock`` with
``hip_layers.set_train_kernels(True)`` in two variants, in one process, on the same tensors:

    hip      this commit: dwconv7x7 + LayerNorm on ``DwConvLN`` and the MLP tail on ``ConvNeXtMlp`` (six-product split GEMMs up to a
             depth of 256, csrc/mlp_bwd.hip for the deeper products and everything else) — no kernel of the step is PyTorch's;
    parent   the behaviour before ``ConvNeXtMlp`` existed: dwconv on ``DwConvLN``, the MLP tail as torch.addcmul(shortcut, mlp(x), gamma)
             on PyTorch's operators.  Reached by a flag local to this tool that makes ``hip_layers._mlp_train_ok`` say no; the library
             has no public switch for it.

Shapes: the four ConvNeXt-B stages of a 256 x 256 ROI, 64 x 64 x 128 down to 8 x 8 x 1024, at ``--rois`` 48 (SOLVER.IMS_PER_BATCH of
the reference's training configs) and 8.  The input, the ten parameters and grad_y are leaves; every gradient is asked for.

Measured per variant: the host clock around ``--reps`` forward + backward steps that end in a device synchronise, the two variants
alternating within each of ``--rounds`` rounds after a warm-up of both; median / min / max over the rounds.  Per kernel: the device
time from one separately profiled step of each variant (torch.profiler device events; "not measured" when the profiler gives none),
summed by kernel name; for the TN GEMM also its FLOP over that time beside the 157.3 TFLOP/s of the fp32 matrix instruction.  Saved
activations per block: computed from the shape (ours: x and pre of the MLP; PyTorch's: x, pre, h and the MLP output).  Nothing is gated.

    python tools/convnext_mlp_bwd_microbench.py [--out profiles/convnext_mlp_bwd_microbench.json] [--rois 48 8] [--reps 40] [--rounds 7]
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
PEAKS = {"hbm_TBps": 8.0, "fp32_matrix_TFLOPs": 157.3, "bf16_matrix_TFLOPs": 2516.0}


def saved_bytes(m, c):
    """Activation bytes a block's MLP tail keeps for its backward: (this library, PyTorch's graph).  x is the LayerNorm output [M,C]."""
    return {"hip": 4 * m * (c + 4 * c), "torch": 4 * m * (c + 4 * c + 4 * c + c)}


def kernel_key(name):
    """A kernel's name without its namespace, template and argument lists (library kernels without any keep their last 60 characters)."""
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return name.split("(")[0].split("<")[0].strip()[-60:] or name[-60:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convnext_mlp_bwd_microbench.json"))
    ap.add_argument("--rois", type=int, nargs="+", default=[48, 8])
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import hip_layers
    from gdrnpp_bop2022_amd.gdrn_modeling.backbones import ConvNeXtBlock

    assert torch.cuda.is_available(), "convnext_mlp_bwd_microbench needs the GPU"
    hip_lib.load()
    dev = torch.device("cuda")
    mlp_train_ok = hip_layers._mlp_train_ok
    result = {"device": torch.cuda.get_device_name(0), "peaks": PEAKS, "reps": args.reps, "rounds": args.rounds, "cases": []}
    for n in args.rois:
        for hw, c in STAGES:
            torch.manual_seed(n * 10000 + c)
            block = ConvNeXtBlock(c).to(dev)
            with torch.no_grad():
                block.gamma.copy_(torch.randn(c) * 0.5 + 1.0)
            x = torch.randn(n, c, hw, hw, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
            g = torch.randn(n, c, hw, hw, device=dev).contiguous(memory_format=torch.channels_last)
            leaves = [x] + list(block.parameters())
            m = n * hw * hw

            def step(bypass_mlp):
                for t in leaves:
                    t.grad = None
                hip_layers.set_train_kernels(True)
                hip_layers._mlp_train_ok = (lambda *a: False) if bypass_mlp else mlp_train_ok      # the tool's local flag
                try:
                    y = block(x)
                finally:
                    hip_layers.set_train_kernels(False)
                    hip_layers._mlp_train_ok = mlp_train_ok
                y.backward(g)
                return [y.detach()] + [t.grad for t in leaves]

            variants = (("hip", lambda: step(False)), ("parent", lambda: step(True)))
            a, b = step(False), step(True)
            agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
            for _, fn in variants:
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            times = {"hip": [], "parent": []}
            for _ in range(args.rounds):
                for name, fn in variants:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / args.reps * 1e3)
            case = {"rois": n, "H": hw, "W": hw, "C": c, "rows": m, "max_relative_difference_hip_vs_parent": agree,
                    "saved_activation_bytes": saved_bytes(m, c),
                    "gemm_tn_workspace_bytes": int(hip_lib.load().gdrnpp_gemm_tn_f32_workspace_bytes(m, c, 4 * c))}
            for name, v in times.items():
                case[f"{name}_fwd_bwd_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
            case["parent_over_hip"] = case["parent_fwd_bwd_ms"]["median"] / case["hip_fwd_bwd_ms"]["median"]
            try:      # per kernel: one profiled step of each variant, outside the timed rounds
                from torch.autograd import DeviceType
                from torch.profiler import ProfilerActivity, profile

                for name, fn in variants:
                    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                        fn()
                        torch.cuda.synchronize()
                    tk = {}
                    for e in prof.events():
                        if e.device_type != DeviceType.CUDA:
                            continue
                        us = float(getattr(e, "device_time", 0.0) or getattr(e, "cuda_time", 0.0))
                        key = kernel_key(e.name)
                        k = tk.setdefault(key, {"us": 0.0, "launches": 0})
                        k["us"] += us
                        k["launches"] += 1
                    case[f"{name}_kernels"] = tk or "not measured"
                    if tk:
                        case[f"{name}_device_us"] = sum(k["us"] for k in tk.values())
                tn = next((v for k, v in case.get("hip_kernels", {}).items() if "gemm_tn_kernel" in k), None) if isinstance(case.get("hip_kernels"), dict) else None
                if tn and tn["us"]:
                    case["gemm_tn_TFLOPs"] = 2 * 2.0 * m * c * 4 * c / tn["us"] * 1e-6       # two products of M x C x 4C
            except Exception as exc:      # noqa: BLE001
                case["hip_kernels"] = case["parent_kernels"] = "not measured: " + repr(exc)[:200]
            result["cases"].append(case)
            print(json.dumps({k: v for k, v in case.items() if not k.endswith("_kernels")}))
            del x, g, block, a, b, leaves
            torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
