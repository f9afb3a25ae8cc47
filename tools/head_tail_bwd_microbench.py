"""Microbenchmark of the geometry head's tail under autograd on one MI355X: forward + backward from the trunk's result ``feat`` to the
loss-side gradients (of Patch-PnP's input, of the five map planes and of the region map), in two variants, in one process, on the same
tensors:

    hip      ``hip_layers.HeadTail``: the two launches of the inference tail forward, csrc/head_tail_bwd.hip backward;
    torch    the module path of ``GDRN_DoubleMask.forward_maps`` on PyTorch's operators: the reshape out of channels_last, baddbmm over
             the per-ROI gathered weight, softmax / cat / the in-place de-normalisation, and ATen's backward of all of them.

Shape: 64 x 64 x 256, 21 classes (YCB-V), double mask, at ``--rois`` 48 (SOLVER.IMS_PER_BATCH of the reference's training configs) and
8.  feat and the output layer's weight and bias are leaves; every gradient is asked for.

Measured per variant: the host clock around ``--reps`` forward + backward steps that end in a device synchronise, the two variants
alternating within each of ``--rounds`` rounds after a warm-up of both; median / min / max over the rounds.  Per kernel: the device
time from one separately profiled step of each variant (torch.profiler device events; "not measured" when the profiler gives none),
summed by kernel name; for the tail's adjoint also its algorithmic bytes over that time beside 8 TB/s, for the two products their FLOP
over that time beside the 157.3 TFLOP/s of the fp32 matrix instruction (the weight gradient runs 128 rows for the layer's 70: both
figures are given).  Nothing is gated.

    python tools/head_tail_bwd_microbench.py [--out profiles/head_tail_bwd_microbench.json] [--rois 48 8] [--reps 10] [--rounds 7]
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
K, RES, CLASSES, N_OUT, PITCH = 256, 64, 21, 70, 128


def kernel_key(name):
    """A kernel's name without its namespace, template and argument lists (library kernels without any keep their last 60 characters)."""
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return name.split("(")[0].split("<")[0].strip()[-60:] or name[-60:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "head_tail_bwd_microbench.json"))
    ap.add_argument("--rois", type=int, nargs="+", default=[48, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch
    import torch.nn.functional as F

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import heads, hip_layers

    assert torch.cuda.is_available(), "head_tail_bwd_microbench needs the GPU"
    hip_lib.load()
    dev = torch.device("cuda")
    head = heads.TopDownDoubleMaskXyzRegionHead(K, feat_dim=K, up_types=("bilinear",), num_conv_per_block=1, mask_num_classes=CLASSES,
                                                xyz_num_classes=CLASSES, region_num_classes=CLASSES, mask_out_dim=2)
    cls_rows = head.class_channel_index(CLASSES).to(dev)
    torch.manual_seed(0)
    ol = torch.nn.Conv2d(K, CLASSES * N_OUT, 1).to(dev)
    with torch.no_grad():
        ol.weight.copy_(torch.randn_like(ol.weight) * K ** -0.5)
        ol.bias.copy_(torch.randn_like(ol.bias) * 0.5)
    result = {"device": torch.cuda.get_device_name(0), "peaks": PEAKS, "reps": args.reps, "rounds": args.rounds,
              "shape": {"H": RES, "W": RES, "K": K, "classes": CLASSES, "n_out": N_OUT}, "cases": []}
    for n in args.rois:
        torch.manual_seed(n)
        hw, m = RES * RES, n * RES * RES
        feat = torch.randn(n, K, RES, RES, device=dev).contiguous(memory_format=torch.channels_last).requires_grad_(True)
        sel = torch.randint(0, CLASSES, (n,), device=dev)
        coord2d, extents = torch.rand(n, 2, RES, RES, device=dev), torch.rand(n, 3, device=dev) * 0.2 + 0.05
        g_pnp = torch.randn(n, hw, 96, device=dev)                      # the gradient of Patch-PnP's input, NHWC; the module path's is its NCHW copy
        g_pnp_nchw = g_pnp[..., :69].view(n, RES, RES, 69).permute(0, 3, 1, 2).contiguous()
        g_planes = torch.randn(5, n, 1, RES, RES, device=dev)
        g_region = torch.randn(n, 65, RES, RES, device=dev)
        leaves = [feat, ol.weight, ol.bias]

        def hip_step():
            hip_layers.set_train_kernels(True)
            try:
                out, pnp_in, planes = hip_layers.head_tail(ol, cls_rows, feat, sel, coord2d, extents, True)
            finally:
                hip_layers.set_train_kernels(False)
            region = out.view(n, RES, RES, PITCH)[..., 5:N_OUT].permute(0, 3, 1, 2)
            torch.autograd.backward([pnp_in, planes, region], [g_pnp, g_planes.view(5, n, hw), g_region])
            return pnp_in[..., :69].view(n, RES, RES, 69).permute(0, 3, 1, 2), planes.view(5, n, 1, RES, RES), region

        def torch_step():
            w = ol.weight.view(ol.out_channels, -1)[cls_rows]
            b = ol.bias[cls_rows]
            x = feat.reshape(n, K, hw)
            out = torch.baddbmm(b[sel].unsqueeze(-1), w[sel], x).view(n, -1, RES, RES)
            vis, full, cx, cy, cz, region = out[:, 0:1], out[:, 1:2], out[:, 2:3], out[:, 3:4], out[:, 4:5], out[:, 5:]
            coor_feat = torch.cat([torch.cat([cx, cy, cz], dim=1), coord2d], dim=1)
            region_softmax = F.softmax(region[:, 1:], dim=1)
            coor_feat[:, :3] = (coor_feat[:, :3] - 0.5) * extents.view(n, 3, 1, 1)
            pnp = torch.cat([coor_feat, region_softmax], dim=1)
            maps = [vis, full, cx, cy, cz]
            torch.autograd.backward([pnp] + maps + [region], [g_pnp_nchw] + list(g_planes) + [g_region])
            return pnp, torch.stack(maps), region

        def step(fn):
            for t in leaves:
                t.grad = None
            outs = fn()
            return [o.detach() for o in outs] + [t.grad for t in leaves]

        variants = (("hip", lambda: step(hip_step)), ("torch", lambda: step(torch_step)))
        a, b = step(hip_step), step(torch_step)
        agree = max(float((u - v).abs().max() / v.abs().max()) for u, v in zip(a, b))
        del a, b
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
        case = {"rois": n, "rows": m, "max_relative_difference_hip_vs_torch": agree,
                "wgrad_workspace_bytes": int(hip_lib.load().gdrnpp_grouped_linear_wgrad_f32_workspace_bytes(n, hw, K, N_OUT))}
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
                def us_of(key):
                    hit = next((v for k, v in case["hip_kernels"].items() if k.endswith(key)), None)
                    return hit["us"] if hit and hit["us"] else None

                tail_bytes = 4.0 * m * (72 + 96 + 5 + 72 + PITCH)      # the logits, three gradients in, d_out out
                if us_of("head_tail_bwd_kernel"):
                    case["tail_adjoint_fraction_of_hbm"] = tail_bytes / us_of("head_tail_bwd_kernel") * 1e-6 / PEAKS["hbm_TBps"]
                if us_of("grouped_dinput_kernel"):
                    case["dinput_fraction_of_matrix_peak"] = 2.0 * m * N_OUT * K / us_of("grouped_dinput_kernel") * 1e-6 / PEAKS["fp32_matrix_TFLOPs"]
                if us_of("grouped_wgrad_kernel"):
                    useful = 2.0 * m * N_OUT * K / us_of("grouped_wgrad_kernel") * 1e-6 / PEAKS["fp32_matrix_TFLOPs"]
                    case["wgrad_fraction_of_matrix_peak"] = {"useful_70_rows": useful, "executed_128_rows": useful * 128 / N_OUT}
        except Exception as exc:      # noqa: BLE001
            case["hip_kernels"] = case["torch_kernels"] = "not measured: " + repr(exc)[:200]
        result["cases"].append(case)
        print(json.dumps({k: v for k, v in case.items() if not k.endswith("_kernels")}))
        print(json.dumps({k: v for k, v in case.items() if k.endswith("_kernels")}))
        del feat, g_pnp, g_pnp_nchw, g_planes, g_region, leaves
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
