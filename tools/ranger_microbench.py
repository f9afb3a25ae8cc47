"""Microbenchmark of ``solver.Ranger.step()`` on one MI355X, on the parameters of the YCB-V ConvNeXt-B GDRN model that bench.py builds, with
seeded gradients: the multi-tensor kernel path (csrc/ranger.hip) against the class's torch-operator path (the reference's algorithm, one
tensor at a time — the only baseline there is).

Each path owns a copy of the parameters.  Measured per path, after a warm-up that takes both past the first rectified step:
  * a single ``step()`` by the host clock, ending in a device synchronise, ordinary and Lookahead steps (every 6th) apart: median / min /
    max over ``--steps`` steps;
  * the same steps back to back with one synchronise at the end (what a training loop sees), per step;
  * the host time of ``step()`` alone (the call returns before the kernel ends);
  * the device events of one profiled step (torch.profiler): launches and copies.
Computed from the shapes: elements, bytes moved (g, p, m, v read, p, m, v written: 28 B per element; + slow read and written on a
Lookahead step: 36 B) and, given ``--kernel-stats`` (the kernel_stats csv of a ``rocprofv3 --kernel-trace --stats`` run of
``--trace-only``, a run of its own), the kernel's own time and its share of the 6.3 TB/s this part streams.

    python tools/ranger_microbench.py [--out profiles/ranger_microbench.json] [--steps 60] [--kernel-stats <csv>]
    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/ranger_microbench.py --trace-only
"""
import argparse
import csv
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_STREAM_BYTES_PER_S = 6.3e12


def med(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} if v else None


def kernel_stats(path):
    """Rows of rocprofv3's kernel_stats csv whose kernel is one of ranger.hip's -> {name: {calls, mean_us, min_us, max_us}}."""
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "ranger_" in name:
                key = "ranger_long_row_means_kernel" if "long_row" in name else "ranger_step_kernel"
                out[key] = dict(calls=int(row["Calls"]), mean_us=float(row["AverageNs"]) / 1e3, min_us=float(row["MinNs"]) / 1e3,
                                max_us=float(row["MaxNs"]) / 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ranger_microbench.json"))
    ap.add_argument("--steps", type=int, default=60)
    ap.add_argument("--trace-only", action="store_true", help="30 kernel-path steps and nothing else (for a profiler run)")
    ap.add_argument("--kernel-stats", default=None)
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.gdrn_modeling import solver
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from gdrnpp_bop2022_amd.gdrn_modeling.GDRN_double_mask import build_model_optimizer

    assert torch.cuda.is_available(), "ranger_microbench needs the GPU"
    cfg = get_cfg("ycbv_convnext_a6")
    torch.manual_seed(0)
    model, opt_k = build_model_optimizer(cfg, is_test=False)
    assert isinstance(opt_k, solver.Ranger)
    gen = torch.Generator(device="cuda").manual_seed(20221020)
    for g in opt_k.param_groups:
        for p in g["params"]:
            p.grad = torch.empty_like(p).normal_(0.02, 0.05, generator=gen)
    # the torch-operator path on its own copy of every parameter and gradient, same groups
    groups_t = []
    for g in opt_k.param_groups:
        ps = []
        for p in g["params"]:
            q = torch.nn.Parameter(p.detach().clone(memory_format=torch.preserve_format))
            q.grad = p.grad.clone(memory_format=torch.preserve_format)
            ps.append(q)
        groups_t.append(dict(params=ps, lr=g["lr"]))
    opt_t = solver.build_optimizer_with_params(cfg, groups_t)
    opt_t.use_kernel = False
    params = [p for g in opt_k.param_groups for p in g["params"]]
    n_el = sum(p.numel() for p in params)
    centralised = sum(p.numel() for p in params if p.dim() > 1)
    work, long_rows = hip_lib.ranger_plan([p.numel() for p in params], [p.numel() // p.shape[0] if p.dim() > 1 else 0 for p in params])
    long_el = sum(params[int(t)].numel() for t in set(long_rows["tensor"].tolist()))

    if args.trace_only:
        for _ in range(30):
            opt_k.step()
        torch.cuda.synchronize()
        return

    counted = solver.torch_path_tensors()
    for _ in range(12):             # past the first rectified step and two Lookahead steps; the code objects and allocations are warm
        opt_k.step()
        opt_t.step()
    torch.cuda.synchronize()
    assert solver.torch_path_tensors() == counted, solver.last_torch_path()
    # the two paths computed the same thing (fp64 row means against torch's fp32 ones: last bits)
    worst = max(((p.detach() - q.detach()).abs().max() / p.detach().abs().max().clamp_min(1e-30)).item()
                for gk, gt in zip(opt_k.param_groups, opt_t.param_groups) for p, q in zip(gk["params"], gt["params"]))
    result = {"device": torch.cuda.get_device_name(0), "config": "ycbv_convnext_a6", "tensors": len(params), "elements": n_el,
              "centralised_elements": centralised, "elements_in_rows_longer_than_a_tile": long_el, "work_items": len(work), "long_rows": len(long_rows),
              "tile": hip_lib.RANGER_TILE, "bytes_per_step": {"ordinary": 28 * n_el, "lookahead": 36 * n_el},
              "max_relative_difference_of_the_parameters_after_12_steps": worst, "paths": {}}
    for name, opt in (("kernel", opt_k), ("torch_ops", opt_t)):
        single = {"ordinary": [], "lookahead": []}
        host = []
        step_no = 12
        for _ in range(args.steps):
            step_no += 1
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            opt.step()
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            single["lookahead" if step_no % 6 == 0 else "ordinary"].append((t2 - t0) * 1e3)
            host.append((t1 - t0) * 1e3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            opt.step()
        torch.cuda.synchronize()
        back_to_back = (time.perf_counter() - t0) / args.steps * 1e3
        try:
            from torch.autograd import DeviceType
            from torch.profiler import ProfilerActivity, profile

            with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
                opt.step()
                torch.cuda.synchronize()
            ev = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
            launches = {"device_events": len(ev), "copies": sum("emcpy" in e.name for e in ev)}
        except Exception as exc:      # noqa: BLE001
            launches = {"not_measured": repr(exc)[:200]}
        result["paths"][name] = {"single_step_ms_host_clock_with_synchronise": {k: med(v) for k, v in single.items()},
                                 "host_time_of_step_call_ms": med(host), "back_to_back_ms_per_step": back_to_back,
                                 "device_events_of_one_step": launches}
        print(name, json.dumps(result["paths"][name]))
    if args.kernel_stats:
        ks = kernel_stats(args.kernel_stats)
        result["kernel_stats_rocprofv3"] = ks
        if "ranger_step_kernel" in ks:      # 30 traced steps: 25 ordinary, 5 Lookahead
            mean_bytes = (25 * 28 + 5 * 36) / 30 * n_el
            t = ks["ranger_step_kernel"]["mean_us"] * 1e-6
            result["kernel_mean_bytes_per_s"] = mean_bytes / t
            result["kernel_share_of_6.3_TB_per_s"] = mean_bytes / t / HBM_STREAM_BYTES_PER_S
            result["kernel_fastest_share_of_6.3_TB_per_s"] = 28 * n_el / (ks["ranger_step_kernel"]["min_us"] * 1e-6) / HBM_STREAM_BYTES_PER_S
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps({k: v for k, v in result.items() if k != "paths"}))


if __name__ == "__main__":
    main()
