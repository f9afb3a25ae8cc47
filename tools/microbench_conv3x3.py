"""The geometry head's four three-product conv3x3 launches that remain at 128 ROIs (256 -> 256 channels, GroupNorm statistics in the
epilogue: 16 x 16 twice, 32 x 32, 64 x 64), the convolution launch alone: library option conv3x3_window 0 / 1 alternating in one process,
or, with --variant <libgdrnpp_hip.so>, the product library against another build of it (tools/build_variant.sh; the timing-only
-DGDRNPP2_TIMING_NO_DMA build gives the ceiling of any saving on operand traffic).  Device events, median of 7 interleaved rounds of
10 calls (profiles/conv3x3_window.md)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrnpp_bop2022_amd import hip_lib as hip
from gdrnpp_bop2022_amd.hip_lib import abi

ap = argparse.ArgumentParser()
ap.add_argument("--variant", default=None, help="another build of the library: time it against the product build instead of the option")
ap.add_argument("--rois", type=int, default=128)
ap.add_argument("--rounds", type=int, default=7)
ap.add_argument("--out", default=None, help="write the JSON result here as well")
args = ap.parse_args()

dev = "cuda"
torch.manual_seed(0)
N, C, G = args.rois, 256, 32
SHAPES = (("16x16_a", 16), ("16x16_b", 16), ("32x32", 32), ("64x64", 64))

product = hip.load()
other = abi.load(args.variant) if args.variant else None


def conv(lib, x, w_pk, y, part, h):
    rc = lib.gdrnpp_conv3x3_f32_split2(x.data_ptr(), w_pk.data_ptr(), None, y.data_ptr(), part.data_ptr(), N, h, h, C, C, G, 0, None,
                                       abi.current_stream())
    if rc:
        abi.check(rc, "gdrnpp_conv3x3_f32_split2")


def timed(fn, iters=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


out = {"rois": N, "variant": args.variant}
for name, h in SHAPES:
    x = F.gelu(torch.randn(N, C, h, h, device=dev)).contiguous(memory_format=torch.channels_last)
    w_pk = hip.pack_conv_weight_f16x2(torch.randn(C, C, 3, 3, device=dev) * (9 * C) ** -0.5)
    P = product.gdrnpp_conv3x3_gnstats_partials(h, h)
    ys = [torch.empty((N, C, h, h), device=dev).contiguous(memory_format=torch.channels_last) for _ in range(2)]
    parts = [torch.empty((N, P, G, 2), dtype=torch.float64, device=dev) for _ in range(2)]
    if other is not None:
        arms = {"product": lambda: conv(product, x, w_pk, ys[0], parts[0], h), "variant": lambda: conv(other, x, w_pk, ys[1], parts[1], h)}
    else:
        def arm(v, i):
            def run():
                hip.set_option("conv3x3_window", v)
                conv(product, x, w_pk, ys[i], parts[i], h)
            return run
        arms = {"option0": arm(0, 0), "option1": arm(1, 1)}
    for fn in arms.values():
        fn(); fn()
    torch.cuda.synchronize()
    diff = float((ys[0] - ys[1]).abs().max())
    times = {k: [] for k in arms}
    for rnd in range(args.rounds):
        for k, fn in arms.items():
            times[k].append(timed(fn))
    res = {k: {"median_ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}
    a, b = (res[k]["median_ms"] for k in arms)
    out[name] = {"max_abs_diff": diff, "times": res, "second_over_first": round(b / a, 4)}
    print(f"== {name} ({N} x {h} x {h}, {C} -> {C}): max |diff| {diff:.3e}  second/first {b / a:.4f}", flush=True)
    for k, v in res.items():
        print(f"  {k:10s} {v}", flush=True)
if other is None:
    hip.set_option("conv3x3_window", 1)
print(json.dumps(out))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
