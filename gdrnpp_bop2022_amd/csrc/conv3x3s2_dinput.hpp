// The data gradient of a 3x3 / stride 2 / pad 1 convolution by the parity of the input pixel, shared by its two entry points:
// gdrnpp_conv3x3s2_dinput_f32 (pnp_bwd.hip: Cout a multiple of 128, a pitched dx) and gdrnpp_conv3x3s2_dinput_any_f32
// (conv_bn_bwd.hip: any Cout % 4 == 0).  The scheme is exact_gemm_device.hpp's.
//
// grid (row tile x column tile, parity class py 2 + px).  The rows of a class are its input pixels (n, 2i + py, 2j + px), i < OH,
// j < OW; 128 of them and 128 columns (ci) per workgroup, 4 waves of 64 x 64.  The depth is the class's taps in (ky, kx) order, each
// with the Cout channels ascending, in stages of 32:
//   py = 0: ky = 1 reads dz row i;      py = 1: ky = 0 reads dz row i + 1 (none for the last input row: staged as zero, not read),
//   then ky = 2 reads dz row i;         columns alike.
//   dz      read as it lies, float4 along co, stored transposed (exact_gemm_device.hpp).
//   w       f32[9 Cout][ldw], row (ky 3 + kx) Cout + co, column ci: the k-rows of the B operand.  A float4 at or beyond ldw is not
//           read; elements at or beyond Cin are replaced by zero.
//   dx      columns [0, Cin) receive the sums, [Cin, lddx) zero; nothing beyond lddx is written.
//   kAnyCout  a tap's channels are staged in ceil(Cout / 32) stages, the channels from Cout on as zeros in both operands and not
//           read (Cout % 4 == 0: a float4 lies inside a row or outside it).  A zero term leaves an fp32 chain as it is, so a chain
//           still holds at most 128 products.  false: Cout % 32 == 0 and the tests fold away.
#pragma once
#include "exact_gemm_device.hpp"

namespace gdrnpp {
namespace exactgemm {

template <bool kAnyCout>
__device__ __forceinline__ void conv3x3s2_dinput_tile(const float* __restrict__ dz, const float* __restrict__ w, int ldw,
                                                      float* __restrict__ dx, int lddx, int N, int H, int W, int Cin, int Cout,
                                                      int tiles_n, float* sA, float* sB) {
  const int py = (int)blockIdx.y >> 1, px = (int)blockIdx.y & 1;
  const int OH = H >> 1, OW = W >> 1, OHW = OH * OW;
  const long Mc = (long)N * OHW;
  const long m0 = (long)((int)blockIdx.x / tiles_n) * 128;
  const int n0 = ((int)blockIdx.x % tiles_n) * 128;
  const int ntx = 1 + px, ntaps = (1 + py) * ntx, per_tap = kAnyCout ? (Cout + kBK - 1) / kBK : Cout / kBK, stages = ntaps * per_tap;
  // the pixels of the thread's four A rows
  int a_n[4], a_i[4], a_j[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const long m = m0 + stage_row_t() + 32 * q;
    if (m < Mc) {
      const int pix = (int)(m % OHW);
      a_n[q] = (int)(m / OHW), a_i[q] = pix / OW, a_j[q] = pix % OW;
    } else {
      a_n[q] = -1, a_i[q] = 0, a_j[q] = 0;
    }
  }
  const int bcol = n0 + stage_col();
  const bool b_in = bcol < ldw && bcol < Cin;      // ldw % 4 == 0: the float4 lies inside the row
  f4 ra[4], rb[4];
  auto fetch = [&](int s) {
    const int t = s / per_tap, c0 = (s - t * per_tap) * kBK;
    const int ty = t / ntx, tx = t - ty * ntx;
    const int ky = py ? 2 * ty : 1, kx = px ? 2 * tx : 1;
    const int oyo = py ? 1 - ty : 0, oxo = px ? 1 - tx : 0;
    const float* wrow = w + ((size_t)(ky * 3 + kx) * Cout + c0) * ldw + bcol;
    const bool a_k = !kAnyCout || c0 + stage_k_t() < Cout;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int oy = a_i[q] + oyo, ox = a_j[q] + oxo;
      const bool in = a_n[q] >= 0 && oy < OH && ox < OW && a_k;
      ra[q] = in ? ld4v(dz + (((size_t)a_n[q] * OH + oy) * OW + ox) * Cout + c0 + stage_k_t()) : f4{0.f, 0.f, 0.f, 0.f};
      const bool b_k = !kAnyCout || c0 + stage_row() + 8 * q < Cout;
      f4 b = b_in && b_k ? ld4v(wrow + (size_t)(stage_row() + 8 * q) * ldw) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = bcol + j < Cin ? b[j] : 0.f;
      rb[q] = b;
    }
  };
  Tile t;
  t.clear();
  fetch(0);
  k_loop<kPitchT, kPitch>(t, sA, sB, 0, stages, 1, fetch, [&] { store_stage<true, false>(sA, sB, ra, rb); });
  // a row of D is a pixel of the class: its address once, then both column tiles
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const long m = d_row(m0, i, e);
      if (m >= Mc) continue;
      const int n = (int)(m / OHW), pix = (int)(m % OHW);
      float* o = dx + (((size_t)n * H + 2 * (pix / OW) + py) * W + 2 * (pix % OW) + px) * lddx;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int col = d_col(n0, j);
        if (col < lddx) o[col] = col < Cin ? (float)t.carry[i][j][e] : 0.f;
      }
    }
}

}  // namespace exactgemm
}  // namespace gdrnpp
