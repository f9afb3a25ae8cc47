"""dwconv7x7+LN kernel at the four ConvNeXt-B stage shapes (128 ROIs); GDRNPP_HIP_LIB selects the build.
--specialise 0 / 1 / both sets option dwconv_specialise (kernels compiled per channel count, or the run-time-width form);
--ln 1 / 0 / both times the kernel with and without its LayerNorm (the environment variable LN still gives the default).
With `both` the arms alternate inside one process, so their difference is not a difference between boxes or clocks."""
import argparse, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from gdrnpp_bop2022_amd import hip_lib

ap = argparse.ArgumentParser()
ap.add_argument("--specialise", choices=["0", "1", "both"], default=None, help="option dwconv_specialise (default: the library's)")
ap.add_argument("--ln", choices=["0", "1", "both"], default=os.environ.get("LN", "1"))
ap.add_argument("--rows", type=int, default=0, help="1: f16x2-rows output, as the network's blocks ask for")
ap.add_argument("--repeat", type=int, default=1, help="passes over all arms; every pass prints its own lines")
args = ap.parse_args()

dev = "cuda"
B = int(os.environ.get("B", "128"))
torch.manual_seed(0)
spec_arms = [None] if args.specialise is None else ([0, 1] if args.specialise == "both" else [int(args.specialise)])
ln_arms = [1, 0] if args.ln == "both" else [int(args.ln)]
default_spec = hip_lib.get_option("dwconv_specialise")
for rep in range(args.repeat):
    for ln in ln_arms:
        for spec in spec_arms:
            hip_lib.set_option("dwconv_specialise", default_spec if spec is None else spec)
            tot = 0.0
            for hw, c, nblk in [(64, 128, 3), (32, 256, 3), (16, 512, 27), (8, 1024, 3)]:
                x = torch.randn(B, c, hw, hw, device=dev).contiguous(memory_format=torch.channels_last)
                w = torch.randn(49, c, device=dev) * 0.1
                b = torch.randn(c, device=dev); g = torch.randn(c, device=dev); be = torch.randn(c, device=dev)
                fn = (lambda: hip_lib.dwconv7x7_ln(x, w, b, g, be, 1e-6, y_rows=bool(args.rows))) if ln else (lambda: hip_lib.dwconv7x7_ln(x, w, b, y_rows=bool(args.rows)))
                for _ in range(3):
                    fn()
                torch.cuda.synchronize()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(20):
                    fn()
                e1.record(); torch.cuda.synchronize()
                t = e0.elapsed_time(e1) / 20
                by = 2 * x.numel() * 4
                print(f"ln={ln} specialise={hip_lib.get_option('dwconv_specialise')} {hw}x{hw} C={c}: {t * 1e3:.1f} us  {by / t / 1e6:.0f} GB/s  {49 * 2 * x.numel() / t / 1e9:.1f} TFLOP/s")
                tot += nblk * t
            print(f"ln={ln} specialise={hip_lib.get_option('dwconv_specialise')} total per forward {tot:.3f} ms  lib={os.environ.get('GDRNPP_HIP_LIB', 'default')}")
hip_lib.set_option("dwconv_specialise", default_spec)
