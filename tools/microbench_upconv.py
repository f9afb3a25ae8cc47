"""[UpsamplingBilinear2d(2), conv3x3, GroupNorm + GELU] of the geometry head at its two levels (128 ROIs, 256 channels): the upsample +
convolution pair against the low-resolution form (tap GEMM + gather) at 8 .. 128 ROIs per chunk, and the tap GEMMs alone.  Device
events, median of 7 interleaved rounds of 10 calls (profiles/upconv_lowres.md)."""
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gdrnpp_bop2022_amd import hip_lib as hip

dev = "cuda"
torch.manual_seed(0)
N, C, G = 128, 256, 32


def timed(fn, iters=10):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


out = {}
for h in (16, 32):
    x = F.gelu(torch.randn(N, C, h, h, device=dev)).contiguous(memory_format=torch.channels_last)
    w = torch.randn(C, C, 3, 3, device=dev) * (9 * C) ** -0.5
    gamma, beta = torch.rand(C, device=dev) + 0.5, torch.randn(C, device=dev)
    w_old, w_new = hip.pack_conv_weight_f16x2(w), hip.pack_upconv_weight_f16x2(w)
    x2d = x.permute(0, 2, 3, 1).reshape(N * h * h, C)
    variants = {"old": lambda: hip.conv3x3_groupnorm_act(hip.upsample_bilinear2x(x), w_old, None, gamma, beta, G, gelu=True),
                "old_upsample_only": lambda: hip.upsample_bilinear2x(x)}
    for c in (8, 16, 32, 64, 128):
        variants[f"new_chunk{c}"] = (lambda c=c: hip.upsample2x_conv3x3_groupnorm_act(x, w_new, None, gamma, beta, G, gelu=True, chunk=c))
        variants[f"tapgemm_only_chunk{c}"] = (lambda c=c: [hip.linear_f32_split(x2d[i * h * h:(i + c) * h * h], w_new, None) for i in range(0, N, c)])
    a, b = variants["old"](), variants["new_chunk32"]()
    torch.cuda.synchronize()
    diff = float((a - b).abs().max())
    for fn in variants.values():
        fn(); fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for rnd in range(7):
        for k, fn in variants.items():
            times[k].append(timed(fn))
    res = {k: {"median_ms": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)} for k, v in times.items()}
    out[f"out{2*h}x{2*h}"] = {"max_abs_new_minus_old": diff, "times": res}
    print(f"== level {2*h}x{2*h}: max |new-old| {diff:.3e}", flush=True)
    for k, v in res.items():
        print(f"  {k:28s} {v}", flush=True)
out["range_words"] = {str(k): v for k, v in hip.split2_range_words().items()}
print("range words:", out["range_words"])
print(json.dumps(out))
