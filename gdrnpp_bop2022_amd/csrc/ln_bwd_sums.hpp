// fp64 sums of the LayerNorm backward kernels (dwconv_ln_bwd.hip, backbone_bwd.hip): a thread owns one channel quad, the C / 4 lanes of a
// pixel are consecutive, a workgroup of 256 threads holds 256 / (C / 4) pixels at a time.  Device code only.
#pragma once
#include <hip/hip_runtime.h>
#include "dpp_sum.hpp"

namespace gdrnpp {
namespace lnbwd {

using f4 = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ f4 ld4v(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ void st4v(float* p, f4 v) { *reinterpret_cast<f4*>(p) = v; }
using d4 = __attribute__((ext_vector_type(4))) double;
__device__ __forceinline__ d4 to_d4(f4 v) { return __builtin_convertvector(v, d4); }
__device__ __forceinline__ double sum4(d4 v) { return (v.x + v.y) + (v.z + v.w); }

constexpr int kThreads = 256;  // every kernel: 4 waves; a thread owns one channel quad, consecutive lanes consecutive quads

// Sums over the Q lanes of a pixel for P values at once, in every lane of the pixel: the forward's tree in fp64 (shuffles below 16
// lanes, DPP up to a wave, per-wave partials through LDS when a pixel spans several waves).  Called by every thread of the workgroup.
// red: P x 4 doubles of LDS.
template <int P>
__device__ __forceinline__ void pixel_sums(double (&s)[P], int Q, double* red) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int width = Q < 64 ? Q : 64;
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (width >= 16) {
      s[p] = gdrnpp::dpp::group_sum_dpp_f64(s[p], width, lane);
    } else {
      for (int off = width >> 1; off >= 1; off >>= 1) s[p] += __shfl_xor(s[p], off, 64);
    }
  }
  if (Q > 64) {
    const int wpt = Q / 64, w0 = (wave / wpt) * wpt;
    __syncthreads();  // red[] of the previous call has been read by every wave
    if (lane == 0) {
#pragma unroll
      for (int p = 0; p < P; ++p) red[p * 4 + wave] = s[p];
    }
    __syncthreads();
#pragma unroll
    for (int p = 0; p < P; ++p) {
      double t = 0.0;
      for (int k = 0; k < wpt; ++k) t += red[p * 4 + w0 + k];
      s[p] = t;
    }
  }
}

// The workgroup's K / 4 per-channel sums: thread (tl, q) holds K doubles (K / 4 channel quads); the tiles-per-workgroup copies of
// a quad are added in tl order and written to out[K / 4][C].  sh: kThreads x K doubles of LDS.
template <int K>
__device__ __forceinline__ void block_partial(const double (&acc)[K], double* sh, int Q, int C, double* __restrict__ out) {
#pragma unroll
  for (int k = 0; k < K; ++k) sh[(size_t)threadIdx.x * K + k] = acc[k];
  __syncthreads();
  if ((int)threadIdx.x < Q) {
    const int q = threadIdx.x, per = kThreads / Q;
#pragma unroll
    for (int k = 0; k < K; ++k) {
      double s = 0.0;
      for (int t = 0; t < per; ++t) s += sh[(size_t)(t * Q + q) * K + k];
      out[(size_t)(k >> 2) * C + 4 * q + (k & 3)] = s;
    }
  }
}

}  // namespace lnbwd
}  // namespace gdrnpp
