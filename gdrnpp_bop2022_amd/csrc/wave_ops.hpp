// The lane-exchange and workgroup reduction trees of the library: one statement of each.  Device code only.
//
// Three trees over the 64 lanes of a wave exist, and they are not interchangeable: floating-point addition is not associative, so a
// kernel whose sums are pinned bit for bit is pinned to its tree.
//   descending  xor butterfly, offsets 32, 16, ... 1.  Every lane receives the result.  wave_sum / wave_min / wave_max: the library's
//               default (the kernels of pair_error.hpp, vsd_error / gt_visib / xyz_crop, epnp_ransac.hip, uncertainty_pnp.hip,
//               depth_refine.hip, point_pnp.hip, capi.hip).
//   ascending   xor butterfly, offsets 1, 2, ... 32.  Every lane receives the result.  wave_sum_ascending: the row mean of ranger.hip.
//   down        __shfl_down, offsets 32, 16, ... 1: lane l adds lane l + off, a lane without a source adds its own value.  Only lane 0
//               holds the sum of the 64.  wave_sum_down: pose_error.hip, sym_error.hip, gdrn_loss.hip.
// Each step is v = op(v, the other lane's v), in that operand order.  Min / Max combine with the function their callers were written
// with, because what a NaN does is part of the bits: min / max for int, fminf / fmaxf for float, fmin / fmax for double.
//
// One workgroup tree: block_sum_halving, a halving tree over one LDS slot per thread (yolox_loss.hip, ranger.hip).
// DESIGN.md "Wave and workgroup reductions" lists the kernels that still write a tree out by hand, and why.
#pragma once
#include <hip/hip_runtime.h>

namespace gdrnpp {
namespace wave {

struct Sum {
  template <class T>
  __device__ __forceinline__ T operator()(T a, T b) const { return a + b; }
};
struct Min {
  __device__ __forceinline__ int operator()(int a, int b) const { return min(a, b); }
  __device__ __forceinline__ float operator()(float a, float b) const { return fminf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b) const { return fmin(a, b); }
};
struct Max {
  __device__ __forceinline__ int operator()(int a, int b) const { return max(a, b); }
  __device__ __forceinline__ float operator()(float a, float b) const { return fmaxf(a, b); }
  __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); }
};

template <class T, class Op>
__device__ __forceinline__ T reduce_descending(T v, Op op) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_xor(v, off, 64));
  return v;
}
template <class T, class Op>
__device__ __forceinline__ T reduce_ascending(T v, Op op) {
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) v = op(v, __shfl_xor(v, off, 64));
  return v;
}
template <class T, class Op>
__device__ __forceinline__ T reduce_down(T v, Op op) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = op(v, __shfl_down(v, off, 64));
  return v;
}

template <class T>
__device__ __forceinline__ T wave_sum(T v) { return reduce_descending(v, Sum{}); }
template <class T>
__device__ __forceinline__ T wave_min(T v) { return reduce_descending(v, Min{}); }
template <class T>
__device__ __forceinline__ T wave_max(T v) { return reduce_descending(v, Max{}); }
template <class T>
__device__ __forceinline__ T wave_sum_ascending(T v) { return reduce_ascending(v, Sum{}); }
template <class T>
__device__ __forceinline__ T wave_sum_down(T v) { return reduce_down(v, Sum{}); }  // the sum of the wave in lane 0 only

// The sum of a workgroup of THREADS threads by a halving tree in LDS (THREADS slots): slot t += slot t + off for off = THREADS / 2 ... 1,
// a barrier behind each step.  No lane exchange: the order is that of the tree, whatever the wave size.  Every thread returns slot 0.
// No barrier behind that read: a caller that writes the slots again places one.
template <int THREADS, class T>
__device__ __forceinline__ T block_sum_halving(T v, T* s_slots) {
  s_slots[threadIdx.x] = v;
  __syncthreads();
  for (int off = THREADS / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) s_slots[threadIdx.x] += s_slots[threadIdx.x + off];
    __syncthreads();
  }
  return s_slots[0];
}

}  // namespace wave
}  // namespace gdrnpp
