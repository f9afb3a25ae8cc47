"""Microbenchmark of Patch-PnP (ConvPnPNet) under autograd on one MI355X: forward + backward from the prepared 96-pitch input to the
gradients of the two pose heads' outputs, in two variants, in one process, on the same module and tensors:

    hip      ``hip_layers.pnp_train``: Conv3x3S2GnAct x 3, FlattenNCHW, LinearGelu x 2, PnPHeads — csrc/pnp_bwd.hip and the kernels of
             the head's and the ConvNeXt MLP's backward;
    torch    the same module with ``set_train_kernels(False)``: F.conv2d on the 69 channels (MIOpen), GroupNorm, GELU, flatten,
             nn.Linear (hipBLASLt) and ATen's backward of all of them.

Shape: 64 x 64 x 96 input, featdim 128, rot_dim 6, at ``--rois`` 48 (SOLVER.IMS_PER_BATCH of the reference's training configs) and 8.
The input and every parameter are leaves; every gradient is asked for.

Measured per variant: the host clock around ``--reps`` forward + backward steps that end in a device synchronise, the two variants
alternating within each of ``--rounds`` rounds after a warm-up of both; median / min / max over the rounds.  Per kernel: the device
time from one separately profiled step of each variant (torch.profiler device events; "not measured" when the profiler gives none),
summed by kernel name.  Nothing is gated.

    python tools/pnp_bwd_microbench.py [--out profiles/pnp_bwd_microbench.json] [--rois 48 8] [--reps 10] [--rounds 7]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RES, FEATDIM, ROT_DIM = 64, 128, 6


def kernel_key(name):
    """A kernel's name without its namespace, template and argument lists (library kernels without any keep their last 60 characters)."""
    name = name.replace("(anonymous namespace)::", "").replace("void ", "")
    return name.split("(")[0].split("<")[0].strip()[-60:] or name[-60:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pnp_bwd_microbench.json"))
    ap.add_argument("--rois", type=int, nargs="+", default=[48, 8])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=7)
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import heads, hip_layers

    assert torch.cuda.is_available(), "pnp_bwd_microbench needs the GPU"
    hip_lib.load()
    dev = torch.device("cuda")
    torch.manual_seed(0)
    net = heads.ConvPnPNet(nIn=69, num_regions=64, featdim=FEATDIM, rot_dim=ROT_DIM, norm="GN", act="gelu").to(dev)
    with torch.no_grad():      # variance-preserving weights: the initial 0.001 would leave every activation at its bias
        for p in net.parameters():
            if p.dim() > 1:
                p.copy_(torch.randn_like(p) * (p[0].numel() ** -0.5))
    params = list(net.parameters())
    result = {"device": torch.cuda.get_device_name(0), "reps": args.reps, "rounds": args.rounds,
              "shape": {"H": RES, "W": RES, "pitch": 96, "featdim": FEATDIM, "rot_dim": ROT_DIM}, "cases": []}
    for n in args.rois:
        torch.manual_seed(n)
        xyz = (torch.rand(n, RES, RES, 3, device=dev) - 0.5) * 0.2
        region = torch.softmax(torch.randn(n, RES, RES, 64, device=dev) * 3.0, dim=-1)
        x = torch.cat([xyz, torch.rand(n, RES, RES, 2, device=dev), region, torch.zeros(n, RES, RES, 27, device=dev)], -1)
        x = x.permute(0, 3, 1, 2).requires_grad_(True)      # [n,96,64,64] channels_last
        g_r, g_t = torch.randn(n, ROT_DIM, device=dev), torch.randn(n, 3, device=dev)
        leaves = [x] + params

        def run(train_kernels):
            hip_layers.set_train_kernels(train_kernels)
            try:
                rot, t = net.forward_prepared(x)
            finally:
                hip_layers.set_train_kernels(False)
            torch.autograd.backward([rot, t], [g_r, g_t])
            return rot, t

        def step(train_kernels):
            for t in leaves:
                t.grad = None
            outs = run(train_kernels)
            return [o.detach() for o in outs] + [x.grad[:, :69]] + [p.grad for p in params]

        variants = (("hip", lambda: step(True)), ("torch", lambda: step(False)))
        a, b = step(True), step(False)
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
        case = {"rois": n, "max_relative_difference_hip_vs_torch": agree}
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
        except Exception as exc:      # noqa: BLE001
            case["hip_kernels"] = case["torch_kernels"] = "not measured: " + repr(exc)[:200]
        result["cases"].append(case)
        print(json.dumps({k: v for k, v in case.items() if not k.endswith("_kernels")}))
        print(json.dumps({k: v for k, v in case.items() if k.endswith("_kernels")}))
        del x, g_r, g_t, leaves
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
