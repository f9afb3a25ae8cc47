// GroupNorm's per-image group statistics from the forward's fp64 partial sums: the one statement of them, called by the forward
// (gn_apply_kernel, net_kernels.hip) and by its backward (conv_gn_bwd.hip), so that the backward's xhat has the forward's bits.
// Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include "wave_ops.hpp"

namespace gdrnpp {
namespace gn {

// mean and rstd of image n's G groups into LDS from part[N][P][G][2].  Every workgroup needs them before it can stream: 8 lanes per
// group share the P partials (8 independent loads in flight per lane instead of a chain of 64 per group thread: the serial form held
// each of the 8192 workgroups of a 64x64 launch ~6 us before its first store — a quarter of its lifetime), then a 3-step shuffle tree;
// a workgroup with fewer than 8 G threads gives each group one thread.  Every thread of the workgroup calls; the caller synchronises.
__device__ __forceinline__ void gn_group_stats(const double* __restrict__ part, int n, int P, int G, int HW, int cpg, float eps,
                                               float* s_mean, float* s_rstd) {
  if (G * 8 <= (int)blockDim.x) {
    const int g8 = threadIdx.x >> 3, sub = threadIdx.x & 7;
    double a = 0.0, c2 = 0.0;
    if (g8 < G) {
      for (int p = sub; p < P; p += 8) {
        const double* o = part + (((size_t)n * P + p) * G + g8) * 2;
        a += o[0];
        c2 += o[1];
      }
    }
#pragma unroll
    for (int off = 4; off >= 1; off >>= 1) {
      a += __shfl_xor(a, off, 64);
      c2 += __shfl_xor(c2, off, 64);
    }
    if (g8 < G && sub == 0) {
      const double cnt = (double)HW * cpg;
      const double m = a / cnt;
      double var = c2 / cnt - m * m;
      if (var < 0.0) var = 0.0;
      s_mean[g8] = (float)m;
      s_rstd[g8] = (float)(1.0 / sqrt(var + (double)eps));
    }
  } else if ((int)threadIdx.x < G) {
    double c2 = 0.0, a = 0.0;   // in this order gn_apply_kernel's instruction stream is the one it had before the function was shared
    for (int p = 0; p < P; ++p) {
      const double* o = part + (((size_t)n * P + p) * G + threadIdx.x) * 2;
      a += o[0];
      c2 += o[1];
    }
    const double cnt = (double)HW * cpg;
    const double m = a / cnt;
    double var = c2 / cnt - m * m;
    if (var < 0.0) var = 0.0;
    s_mean[threadIdx.x] = (float)m;
    s_rstd[threadIdx.x] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

}  // namespace gn
}  // namespace gdrnpp
