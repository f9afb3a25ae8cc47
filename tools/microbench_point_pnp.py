"""Microbenchmark of the point-wise PnP head on one MI355X, at 8 / 32 / 128 ROIs of 64 x 64 points:

  (a) hip      SimplePointPnPNet.forward_prepared: gdrnpp_point_pnp_pool + gdrnpp_point_pnp_fc + gdrnpp_pnp_fc_heads
      (a_pool: the pool launch alone — the number held against the f32 matrix-pipe floor)
  (b) torch    the same module on stock PyTorch-ROCm fp32 operators (HIP layers off), fed a ready contiguous [B, 69, 4096] tensor
               (its own de-normalisation / concatenation is NOT charged to it)
  (c) patch    ConvPnPNet.forward_prepared (Patch-PnP of the headline config) on the same prepared input, for scale

hipEvents around every launch sequence, warm-up first, >= 50 timed repetitions over rotating input buffers that together exceed
the 256 MB MALL (so no repetition finds its input in a cache), median reported.  Floor: 2 * B * 4096 * (69*128 + 128*128 + 128*1024)
FLOP at the 157.3 TFLOP/s of the f32 matrix pipe — derived, not measured.

    python tools/microbench_point_pnp.py [--out profiles/point_pnp_microbench.json] [--reps 60]
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from gdrnpp_bop2022_amd import hip_lib  # noqa: E402
from gdrnpp_bop2022_amd.gdrn_modeling import heads, hip_layers  # noqa: E402

F32_MATRIX_TFLOPS = 157.3
HW, PITCH, CIN = 4096, 96, 69
ROTATE_BYTES = 512 << 20


def timed(fn, bufs, reps, warmup=5):
    for i in range(warmup):
        fn(bufs[i % len(bufs)])
    torch.cuda.synchronize()
    evs = []
    for i in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(bufs[i % len(bufs)])
        e1.record()
        evs.append((e0, e1))
    torch.cuda.synchronize()
    ms = [a.elapsed_time(b) for a, b in evs]
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms), n=reps)


def prepared(b, gen):
    """[B, 96, 64, 64] channels_last with the head-tail kernel's layout: xyz in metres, coord2d, region softmax, zero pad."""
    x = torch.zeros((b, 64, 64, PITCH), device="cuda")
    x[..., :3] = (torch.rand((b, 64, 64, 3), device="cuda", generator=gen) - 0.5) * 0.2
    x[..., 3:5] = torch.rand((b, 64, 64, 2), device="cuda", generator=gen)
    x[..., 5:CIN] = torch.softmax(3 * torch.randn((b, 64, 64, 64), device="cuda", generator=gen), dim=-1)
    return x.permute(0, 3, 1, 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "point_pnp_microbench.json"))
    ap.add_argument("--reps", type=int, default=60)
    ap.add_argument("--rois", type=int, nargs="*", default=[8, 32, 128])
    args = ap.parse_args()
    hip_lib.load()
    torch.manual_seed(0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    point = heads.SimplePointPnPNet(CIN).cuda().eval()
    patch = heads.ConvPnPNet(CIN, norm="GN", act="gelu", num_gn_groups=32).cuda().eval().to(memory_format=torch.channels_last)
    p = {k: v.detach() for k, v in point.state_dict().items()}
    res = dict(device=torch.cuda.get_device_name(0), hw=HW, pitch=PITCH, cin=CIN, reps=args.reps, f32_matrix_tflops=F32_MATRIX_TFLOPS,
               rotate_bytes=ROTATE_BYTES, rois={})
    with torch.no_grad():
        for b in args.rois:
            nbuf = max(2, ROTATE_BYTES // (b * HW * PITCH * 4) + 1)
            x96 = [prepared(b, gen) for _ in range(nbuf)]
            rows = [x.permute(0, 2, 3, 1).reshape(b * HW, PITCH) for x in x96]
            nchw = [r.view(b, HW, PITCH)[:, :, :CIN].transpose(1, 2).contiguous() for r in rows]

            def pool_only(r):
                hip_lib.point_pnp_pool(r, CIN, p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"], p["conv3.weight"],
                                       p["conv3.bias"], b, HW, want_pooled=False)

            a = timed(lambda x: point.forward_prepared(x), x96, args.reps)
            a_pool = timed(pool_only, rows, args.reps)
            hip_layers.set_enabled(False)
            try:
                t = timed(lambda x: point.mlp_tail(x), nchw, args.reps)
            finally:
                hip_layers.set_enabled(True)
            c = timed(lambda x: patch.forward_prepared(x), x96, args.reps)
            flop = 2.0 * b * HW * (CIN * 128 + 128 * 128 + 128 * 1024)
            floor_ms = flop / (F32_MATRIX_TFLOPS * 1e12) * 1e3
            res["rois"][str(b)] = dict(buffers=nbuf, a_hip=a, a_pool_only=a_pool, b_torch=t, c_patch_pnp=c, gflop=flop / 1e9,
                                       f32_matrix_floor_ms=floor_ms, pool_fraction_of_floor=floor_ms / a_pool["median_ms"],
                                       pool_tflops=flop / a_pool["median_ms"] / 1e9, a_over_b=a["median_ms"] / t["median_ms"])
            print(f"{b:4d} ROIs: hip {a['median_ms']:.3f} ms (pool {a_pool['median_ms']:.3f} ms = {100 * floor_ms / a_pool['median_ms']:.0f} % of the "
                  f"f32 matrix floor {floor_ms:.3f} ms)  torch {t['median_ms']:.3f} ms  patch-pnp {c['median_ms']:.3f} ms", flush=True)
            del x96, rows, nchw
            torch.cuda.empty_cache()
    if hip_lib.x3_launch_count():
        hip_lib.split2_range_words(reset=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
