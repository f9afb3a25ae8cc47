"""Microbenchmark of ``ModelEMA.update()`` on one MI355X, on the state dicts of YOLOX-x (``build_yolox(1.33, 1.25, 21)``) and of the YCB-V
ConvNeXt-B GDRN model that bench.py builds: the multi-tensor kernel path (csrc/model_ema.hip) against ``use_kernel=False``, which is the
reference's own loop (three operator launches per floating-point state entry) on the same device.

Each path owns an EMA of the same model, and the two alternate in one process, round by round.  Per round and path:
  * one ``update()`` by the host clock, ending in a device synchronise;
  * ``--reps`` updates back to back with one synchronise at the end (what a training loop sees), per update;
  * the host time of the ``update()`` call alone (it returns before the kernel ends);
and, for the kernel path, the device time of the launch (HIP events around it, ``hip_lib.LaunchTimer``).  Reported: median, min and max
over the rounds.  Once per path: the device events of one profiled update (torch.profiler): launches and copies.
Computed from the shapes: state entries, floating-point elements, algorithmic bytes (e and m read, e written: 12 B per element), and from
them the achieved bytes/s of the kernel and its share of the 6.29 TB/s a float4 copy streams on this part and of the 8.0 TB/s on its sheet.
After the rounds both EMAs have seen the same updates: their floating-point entries are compared bit for bit.

    python tools/model_ema_microbench.py [--out profiles/model_ema_microbench.json] [--rounds 15] [--reps 10]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HBM_COPY_BYTES_PER_S = 6.29e12          # measured float4 copy
HBM_SPEC_BYTES_PER_S = 8.0e12


def med(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "n": len(v)} if v else None


def device_events(torch, fn):
    try:
        from torch.autograd import DeviceType
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        ev = [e for e in prof.events() if e.device_type == DeviceType.CUDA]
        return {"device_events": len(ev), "copies": sum("emcpy" in e.name for e in ev)}
    except Exception as exc:      # noqa: BLE001
        return {"not_measured": repr(exc)[:200]}


def measure(torch, hip_lib, E, name, model, rounds, reps):
    model = model.cuda()
    emas = {"kernel": E.ModelEMA(model, 0.9998), "torch_ops": E.ModelEMA(model, 0.9998, use_kernel=False)}
    sd = model.state_dict()
    floats = [v for v in sd.values() if v.dtype.is_floating_point]
    n_el = sum(v.numel() for v in floats)
    counted = E.torch_path_tensors()
    for _ in range(3):          # code objects, allocations, the device tables and their upload
        for ema in emas.values():
            ema.update(model)
    torch.cuda.synchronize()
    assert E.torch_path_tensors() == counted, E.last_torch_path()
    tables = emas["kernel"]._tables[torch.device("cuda", torch.cuda.current_device())]
    out = {"state_entries": len(sd), "floating_point_entries": len(floats), "integer_entries": len(sd) - len(floats), "elements": n_el,
           "largest_tensor": max(v.numel() for v in floats), "tensors_of_at_most_1280_elements": sum(v.numel() <= 1280 for v in floats),
           "tensors_whose_numel_is_no_multiple_of_4": sum(v.numel() % 4 != 0 for v in floats), "algorithmic_bytes_per_update": 12 * n_el,
           "work_items": tables.n_work, "tile": hip_lib.EMA_TILE, "paths": {}}
    single = {k: [] for k in emas}
    host = {k: [] for k in emas}
    b2b = {k: [] for k in emas}
    kernel_ms = []
    for _ in range(rounds):
        for key, ema in emas.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ema.update(model)
            t1 = time.perf_counter()
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            single[key].append((t2 - t0) * 1e3)
            host[key].append((t1 - t0) * 1e3)
            t0 = time.perf_counter()
            for _ in range(reps):
                ema.update(model)
            torch.cuda.synchronize()
            b2b[key].append((time.perf_counter() - t0) / reps * 1e3)
        timer = hip_lib.LaunchTimer()
        hip_lib.set_launch_timer(timer)
        try:
            emas["kernel"].update(model)
        finally:
            hip_lib.set_launch_timer(None)
        emas["torch_ops"].update(model)          # the two stay in step
        torch.cuda.synchronize()
        assert [r[0] for r in timer.records] == ["hbm:model_ema"], [r[0] for r in timer.records]
        kernel_ms.append(timer.records[0][2].elapsed_time(timer.records[0][3]))
    uploads = tables.uploads
    for key, ema in emas.items():
        out["paths"][key] = {"single_update_ms_host_clock_with_synchronise": med(single[key]), "back_to_back_ms_per_update": med(b2b[key]),
                             "host_time_of_update_call_ms": med(host[key]),
                             "device_events_of_one_update": device_events(torch, lambda ema=ema: ema.update(model))}
    torch.cuda.synchronize()
    assert emas["kernel"].updates == emas["torch_ops"].updates
    a, b = emas["kernel"].ema.state_dict(), emas["torch_ops"].ema.state_dict()
    out["paths_bit_equal_after_%d_updates" % emas["kernel"].updates] = all(
        torch.equal(a[k].contiguous().view(torch.int32), b[k].contiguous().view(torch.int32)) for k in a if a[k].dtype == torch.float32)
    out["table_uploads_over_all_updates"] = uploads
    k_med = statistics.median(kernel_ms) * 1e-3
    out["kernel_device_time_ms_hip_events_around_the_launch"] = med(kernel_ms)
    out["kernel_bytes_per_s_at_median"] = 12 * n_el / k_med
    out["kernel_share_of_6.29_TB_per_s_float4_copy"] = 12 * n_el / k_med / HBM_COPY_BYTES_PER_S
    out["kernel_share_of_8.0_TB_per_s_sheet"] = 12 * n_el / k_med / HBM_SPEC_BYTES_PER_S
    out["speedup_back_to_back_median"] = out["paths"]["torch_ops"]["back_to_back_ms_per_update"]["median"] / out["paths"]["kernel"]["back_to_back_ms_per_update"]["median"]
    print(name, json.dumps(out))
    emas["kernel"].close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "model_ema_microbench.json"))
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    import torch

    from gdrnpp_bop2022_amd import hip_lib
    from gdrnpp_bop2022_amd.det.yolox.models import build_yolox
    from gdrnpp_bop2022_amd.det.yolox.utils import ema as E
    from gdrnpp_bop2022_amd.gdrn_modeling.config import get_cfg
    from gdrnpp_bop2022_amd.gdrn_modeling.GDRN_double_mask import build_model_optimizer

    assert torch.cuda.is_available(), "model_ema_microbench needs the GPU"
    torch.manual_seed(0)
    result = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "reps": args.reps, "models": {}}
    result["models"]["yolox_x"] = measure(torch, hip_lib, E, "yolox_x", build_yolox(1.33, 1.25, 21), args.rounds, args.reps)
    torch.cuda.empty_cache()
    gdrn, _ = build_model_optimizer(get_cfg("ycbv_convnext_a6"), is_test=False)
    result["models"]["gdrn_convnext_b_ycbv"] = measure(torch, hip_lib, E, "gdrn_convnext_b_ycbv", gdrn, args.rounds, args.reps)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
