"""Microbenchmark of a trainable block of the geometry head on one MI355X: forward + backward of
``[UpsamplingBilinear2d(2), ConvModule(C, C, 3, GN, GELU), ConvModule(C, C, 3, GN, GELU)]`` through ``heads.run_features`` in two
variants, in one process, on the same tensors:

    hip      ``hip_layers.set_train_kernels(True)``: ``Upsample2x`` and ``Conv3x3GnAct`` (csrc/conv_gn_bwd.hip) — no kernel of the step
             is PyTorch's;
    torch    the switch off: the same modules on PyTorch's operators on the same device (MIOpen convolutions, ATen GroupNorm / GELU /
             bilinear kernels), which is what a forward under enable_grad runs without the switch.

Shape: C = 256, 32 x 32 -> 64 x 64 (the head's last block), at ``--rois`` 48 (SOLVER.IMS_PER_BATCH of the reference's training configs)
and 8.  The input, the six parameters and grad_y are leaves; every gradient is asked for.

Measured per variant: the host clock around ``--reps`` forward + backward steps that end in a device synchronise, the two variants
alternating within each of ``--rounds`` rounds after a warm-up of both; median / min / max over the rounds.  Per kernel: the device
time from one separately profiled step of each variant (torch.profiler device events; "not measured" when the profiler gives none),
summed by kernel name; for the weight-gradient GEMM also its FLOP over that time beside the 157.3 TFLOP/s of the fp32 matrix
instruction.  Saved activations per ConvModule: computed from the shape (ours: x and z; PyTorch's: x, z
and the GroupNorm output).  Nothing is gated.

``--engine-errors`` also measures what decided the convolution engine of the training forward and of dx: error / bar (the bar of
tests/mlp_bwd_ref.py, against fp64 and fp32 CPU runs of tests/conv_gn_bwd_ref.py) at depths 1152 and 2304 of the six-product
``conv3x3_f32_split`` as dispatched (small launches cut K) and on its 256-row tiles (what large launches run) and of
``gdrnpp_conv_bias_act_f32`` (fp32 MFMA, two-level fp32 sums; ``hip_lib.conv3x3_f32_mfma``), the engine chosen; and the engines' times on
one 64 x 64 x 256 -> 256 layer of 48 ROIs.

    python tools/head_bwd_microbench.py [--out profiles/head_bwd_microbench.json] [--rois 48 8] [--reps 10] [--rounds 7] [--engine-errors]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAKS = {"hbm_TBps": 8.0, "fp32_matrix_TFLOPs": 157.3}
C, LOW = 256, 32


def kernel_key(name):
    """A kernel's name without its namespace, template and argument lists (library kernels without any keep their last 60 characters)."""
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return name.split("(")[0].split("<")[0].strip()[-60:] or name[-60:]


def engine_errors(torch, hip_lib):
    """Error / bar of z = conv3x3(x, W) per engine, and each engine's time at the head's training shape."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import conv_gn_bwd_ref as R
    from gdrnpp_bop2022_amd.hip_lib.abi import launch

    def engines(x, wt):
        n, cin, h, w = x.shape
        cout = wt.shape[0]
        w6, wk = hip_lib.pack_conv_weight_bf16x3(wt), hip_lib.conv3x3_weight_kn(wt)
        z = torch.empty((n, cout, h, w), device="cuda").contiguous(memory_format=torch.channels_last)
        P = hip_lib.load().gdrnpp_conv3x3_gnstats_partials(h, w)
        part = torch.empty((n, max(P, 1), cout // 8, 2), dtype=torch.float64, device="cuda")

        def tiles256():      # the 256-row-tile kernel the head's convolutions run at scale (no cut of K), called directly
            launch("gdrnpp_conv3x3_f32_split_gnstats", x.data_ptr(), w6.data_ptr(), None, z.data_ptr(), part.data_ptr(), n, h, w, cin, cout, cout // 8)
            return z

        table = {"six_product_as_dispatched": lambda: hip_lib.conv3x3_f32_split(x, w6, None),
                 "conv_bias_act_f32": lambda: hip_lib.conv3x3_f32_mfma(x, wk)}
        if P > 0:
            table["six_product_256_row_tiles"] = tiles256
        return table

    rows = []
    for case in ((2, 16, 16, 128, 128), (2, 16, 16, 256, 256), (1, 32, 32, 256, 256)):
        c = R.conv_random(case)
        x = c["x"].cuda().contiguous(memory_format=torch.channels_last)
        row = {"case": case, "depth": 9 * case[3]}
        for name, fn in engines(x, c["w"].cuda()).items():
            row[name] = R.ratio_to_bar(fn(), c["ref64"]["z"], c["ref32"]["z"])
        print(json.dumps(row))
        rows.append(row)
    torch.manual_seed(0)
    n = 48
    x = torch.randn(n, C, 2 * LOW, 2 * LOW, device="cuda").contiguous(memory_format=torch.channels_last)
    wt = torch.randn(C, C, 3, 3, device="cuda") * (9 * C) ** -0.5
    flop = 2.0 * n * 4 * LOW * LOW * C * 9 * C
    times = {"case": (n, 2 * LOW, 2 * LOW, C, C), "matrix_floor_ms": flop / (PEAKS["fp32_matrix_TFLOPs"] * 1e9)}
    for name, fn in engines(x, wt).items():
        for _ in range(3):
            fn()
        ms = []
        for _ in range(7):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        times[name] = {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "fp32_TFLOPs": flop / statistics.median(ms) * 1e-9}
    print(json.dumps(times))
    return {"error_over_bar": rows, "time_at_48_rois": times}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_bwd_microbench.json"))
    ap.add_argument("--rois", type=int, nargs="+", default=[48, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--engine-errors", action="store_true")
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import heads, hip_layers

    assert torch.cuda.is_available(), "head_bwd_microbench needs the GPU"
    hip_lib.load()
    dev = torch.device("cuda")
    result = {"device": torch.cuda.get_device_name(0), "peaks": PEAKS, "reps": args.reps, "rounds": args.rounds, "cases": []}
    if args.engine_errors:
        result["conv3x3_engines"] = engine_errors(torch, hip_lib)
    for n in args.rois:
        torch.manual_seed(n)
        feats = torch.nn.ModuleList([torch.nn.UpsamplingBilinear2d(scale_factor=2)]
                                    + [heads.ConvModule(C, C, 3, padding=1, norm="GN", num_gn_groups=32, act="GELU") for _ in range(2)]).to(dev)
        with torch.no_grad():
            for m_ in feats.modules():
                if isinstance(m_, torch.nn.GroupNorm):
                    m_.weight.copy_(torch.randn(C) * 0.5 + 1.0), m_.bias.copy_(torch.randn(C) * 0.5)
                elif isinstance(m_, torch.nn.Conv2d):
                    m_.weight.copy_(torch.randn(C, C, 3, 3) * (9 * C) ** -0.5)
        x = torch.randn(n, C, LOW, LOW, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        g = torch.randn(n, C, 2 * LOW, 2 * LOW, device=dev).contiguous(memory_format=torch.channels_last)
        leaves = [x] + list(feats.parameters())
        m = n * 4 * LOW * LOW

        def step(train_kernels):
            for t in leaves:
                t.grad = None
            hip_layers.set_train_kernels(train_kernels)
            try:
                y = heads.run_features(feats, x)
            finally:
                hip_layers.set_train_kernels(False)
            y.backward(g)
            return [y.detach()] + [t.grad for t in leaves]

        variants = (("hip", lambda: step(True)), ("torch", lambda: step(False)))
        a, b = step(True), step(False)
        agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
        for _, fn in variants:
            for _ in range(3):
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
        flop = 2.0 * m * C * 9 * C      # one convolution-shaped product of the layer
        case = {"rois": n, "H": 2 * LOW, "W": 2 * LOW, "C": C, "rows": m, "max_relative_difference_hip_vs_torch": agree,
                "saved_activation_bytes_per_conv_module": {"hip": 4 * m * C * 2, "torch": 4 * m * C * 3},
                "wgrad_workspace_bytes": int(hip_lib.load().gdrnpp_conv3x3_wgrad_f32_workspace_bytes(n, 2 * LOW, 2 * LOW, C, C)),
                "matrix_floor_ms_per_product": flop / (PEAKS["fp32_matrix_TFLOPs"] * 1e9)}
        for name, v in times.items():
            case[f"{name}_fwd_bwd_ms"] = {"median": statistics.median(v), "min": min(v), "max": max(v)}
        case["torch_over_hip"] = case["torch_fwd_bwd_ms"]["median"] / case["hip_fwd_bwd_ms"]["median"]
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
                    k = tk.setdefault(kernel_key(e.name), {"us": 0.0, "launches": 0})
                    k["us"] += us
                    k["launches"] += 1
                case[f"{name}_kernels"] = tk or "not measured"
                if tk:
                    case[f"{name}_device_us"] = sum(k["us"] for k in tk.values())
            if isinstance(case.get("hip_kernels"), dict):
                for key, label in (("conv3x3_wgrad_kernel", "wgrad_TFLOPs"),):
                    hit = next((v for k, v in case["hip_kernels"].items() if k.endswith(key)), None)
                    if hit and hit["us"]:
                        case[label] = hit["launches"] * flop / hit["us"] * 1e-6
        except Exception as exc:      # noqa: BLE001
            case["hip_kernels"] = case["torch_kernels"] = "not measured: " + repr(exc)[:200]
        result["cases"].append(case)
        print(json.dumps({k: v for k, v in case.items() if not k.endswith("_kernels")}))
        del x, g, feats, a, b, leaves
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
