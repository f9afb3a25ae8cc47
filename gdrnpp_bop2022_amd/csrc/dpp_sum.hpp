// Lane-group sums through DPP, shared by the NHWC network kernels (net_kernels.hip) and the backward of dwconv7x7 + LayerNorm
// (dwconv_ln_bwd.hip).  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace gdrnpp {
namespace dpp {

// Sum over each aligned group of `width` lanes (16, 32 or 64), returned in every lane of the group.  DPP row shifts
// and row broadcasts run in the VALU; the ds_bpermute tree that __shfl_xor expands to went through the LDS crossbar
// six times per value and was 36 % of the dwconv+LN kernel (tools/microbench_dwconv.py, LN on/off).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
  const int t = __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, ROW_MASK, 0xf, false);
  return v + __builtin_bit_cast(float, t);
}
__device__ __forceinline__ float group_sum_dpp(float s, int width, int lane) {
  s = dpp_add<0x111, 0xf>(s);  // row_shr:1
  s = dpp_add<0x112, 0xf>(s);  // row_shr:2
  s = dpp_add<0x114, 0xf>(s);  // row_shr:4
  s = dpp_add<0x118, 0xf>(s);  // row_shr:8   -> lane 15 of every 16-lane row holds the row total
  if (width >= 32) s = dpp_add<0x142, 0xa>(s);  // row_bcast:15 into rows 1 and 3
  if (width == 64) {
    s = dpp_add<0x143, 0xc>(s);                 // row_bcast:31 into rows 2 and 3 -> lane 63 holds the wave total
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, s), 63));
  }
  return __shfl(s, lane | (width - 1), 64);
}
// The same sums for the P pixels of a tile at a compile-time width of 32 or 64, one tree stage over all P chains at a time: a
// DPP operand may not be read in the two issue slots after its VGPR was written, and the other pixels' adds fill those slots.
// The totals are those of group_sum_dpp bit for bit (same tree, same operand order); they come back through v_readlane
// (lane 31 / 63 hold them), not through the LDS crossbar.
template <int WIDTH, int P>
__device__ __forceinline__ void group_sum_dpp_tile(float (&s)[P], int lane) {
  static_assert(WIDTH == 32 || WIDTH == 64, "group_sum_dpp_tile: one or two groups per wave");
#pragma unroll
  for (int p = 0; p < P; ++p) s[p] = dpp_add<0x111, 0xf>(s[p]);
#pragma unroll
  for (int p = 0; p < P; ++p) s[p] = dpp_add<0x112, 0xf>(s[p]);
#pragma unroll
  for (int p = 0; p < P; ++p) s[p] = dpp_add<0x114, 0xf>(s[p]);
#pragma unroll
  for (int p = 0; p < P; ++p) s[p] = dpp_add<0x118, 0xf>(s[p]);
#pragma unroll
  for (int p = 0; p < P; ++p) s[p] = dpp_add<0x142, 0xa>(s[p]);
  if (WIDTH == 64) {
#pragma unroll
    for (int p = 0; p < P; ++p) s[p] = dpp_add<0x143, 0xc>(s[p]);
  }
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int hi = __builtin_amdgcn_readlane(__builtin_bit_cast(int, s[p]), 63);
    const int lo = WIDTH == 64 ? hi : __builtin_amdgcn_readlane(__builtin_bit_cast(int, s[p]), 31);
    s[p] = __builtin_bit_cast(float, (lane & 32) ? hi : lo);
  }
}

// group_sum_dpp for doubles: the same tree, each stage moving the two halves of the value through DPP.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ double dpp_add_f64(double v) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, ROW_MASK, 0xf, false);
  const unsigned hi = (unsigned)__builtin_amdgcn_update_dpp(0, (int)(unsigned)(b >> 32), CTRL, ROW_MASK, 0xf, false);
  return v + __builtin_bit_cast(double, ((unsigned long long)hi << 32) | lo);  // a lane without a source adds +0.0
}
__device__ __forceinline__ double group_sum_dpp_f64(double s, int width, int lane) {
  s = dpp_add_f64<0x111, 0xf>(s);
  s = dpp_add_f64<0x112, 0xf>(s);
  s = dpp_add_f64<0x114, 0xf>(s);
  s = dpp_add_f64<0x118, 0xf>(s);
  if (width >= 32) s = dpp_add_f64<0x142, 0xa>(s);
  if (width == 64) s = dpp_add_f64<0x143, 0xc>(s);
  return __shfl(s, lane | (width - 1), 64);
}

}  // namespace dpp
}  // namespace gdrnpp
