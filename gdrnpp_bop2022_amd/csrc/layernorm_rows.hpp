// LayerNorm over C of NHWC pixels, the body shared by layernorm_nhwc_kernel (net_kernels.hip: the result stored where the pixel lies)
// and layernorm_patch_kernel (backbone_bwd.hip: stored in 2x2 patch order) — one arithmetic, hence one set of bits.  Device code only.
// One thread holds one channel quad of LN_PIX pixels (all loads issued before the first reduction); the C/4 lanes of a pixel are
// consecutive, sums go through DPP inside the wave and, when a pixel spans several waves, through LDS.  Two passes over registers
// (mean, then centred variance), biased variance, eps inside the sqrt.  Workgroups of 256 threads, grid-stride over pixel groups.
#pragma once
#include <hip/hip_runtime.h>
#include "dpp_sum.hpp"

namespace gdrnpp {
namespace ln {

using f4 = __attribute__((ext_vector_type(4))) float;
constexpr int LN_PIX = 4;
constexpr int kThreads = 256;  // threads of the workgroup: the launch's and the kernel's __launch_bounds__

// dst(pix) -> where the C channels of pixel `pix` are stored
template <class Dst>
__device__ __forceinline__ void layernorm_rows(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                               long n_pix, int C, float eps, Dst dst) {
  __shared__ float red[LN_PIX * 4];
  const int Q = C >> 2, ppb = kThreads / Q, q = threadIdx.x % Q, pl = threadIdx.x / Q;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int width = Q < 64 ? Q : 64, wpt = Q > 64 ? Q / 64 : 1, w0 = (wave / wpt) * wpt;
  const f4 g4 = *reinterpret_cast<const f4*>(w + 4 * q), b4 = *reinterpret_cast<const f4*>(b + 4 * q);
  const long n_groups = (n_pix + (long)ppb * LN_PIX - 1) / ((long)ppb * LN_PIX);
  const float inv_c = 1.f / (float)C;
  for (long group = blockIdx.x; group < n_groups; group += gridDim.x) {
    f4 v[LN_PIX];
    long pix[LN_PIX];
#pragma unroll
    for (int u = 0; u < LN_PIX; ++u) {
      pix[u] = (group * LN_PIX + u) * ppb + pl;
      v[u] = pix[u] < n_pix ? *reinterpret_cast<const f4*>(x + pix[u] * C + 4 * q) : f4{0.f, 0.f, 0.f, 0.f};
    }
    float mean[LN_PIX], rstd[LN_PIX];
#pragma unroll
    for (int round = 0; round < 2; ++round) {
      float part[LN_PIX];
#pragma unroll
      for (int u = 0; u < LN_PIX; ++u) {
        float s;
        if (round == 0) {
          s = (v[u].x + v[u].y) + (v[u].z + v[u].w);
        } else {
          v[u] -= mean[u];
          s = (v[u].x * v[u].x + v[u].y * v[u].y) + (v[u].z * v[u].z + v[u].w * v[u].w);
        }
        if (width >= 16) {
          s = gdrnpp::dpp::group_sum_dpp(s, width, lane);
        } else {
          for (int off = width >> 1; off >= 1; off >>= 1) s += __shfl_xor(s, off, 64);
        }
        part[u] = s;
      }
      if (wpt > 1) {
        __syncthreads();
        if (lane == 0) {
#pragma unroll
          for (int u = 0; u < LN_PIX; ++u) red[u * 4 + wave] = part[u];
        }
        __syncthreads();
#pragma unroll
        for (int u = 0; u < LN_PIX; ++u) {
          float s = 0.f;
          for (int k = 0; k < wpt; ++k) s += red[u * 4 + w0 + k];
          part[u] = s;
        }
      }
#pragma unroll
      for (int u = 0; u < LN_PIX; ++u) {
        if (round == 0) mean[u] = part[u] * inv_c;
        else rstd[u] = rsqrtf(part[u] * inv_c + eps);
      }
    }
#pragma unroll
    for (int u = 0; u < LN_PIX; ++u)
      if (pix[u] < n_pix) *reinterpret_cast<f4*>(dst(pix[u]) + 4 * q) = v[u] * rstd[u] * g4 + b4;
  }
}

}  // namespace ln
}  // namespace gdrnpp
