// Backward of Patch-PnP (ConvPnPNet) on gfx950: the stride-2 3x3 convolutions, the NCHW flatten and the two pose heads.  DESIGN.md
// "Patch-PnP backward" has the scheme, the resources and the measured error against the tests' bar.
//
//   z = conv3x3 / stride 2 / pad 1 (x, W)      x f32[N,H,W,ldx] (channels [0, Cin)), z f32[N,H/2,W/2,Cout], H and W even, all NHWC
//   dW[co][ci][ky][kx] = sum_{n,oy,ox} dz[n,oy,ox,co] x[n, 2oy+ky-1, 2ox+kx-1, ci]
//   dx[n,y,x,ci]       = sum dz[n,oy,ox,co] W[co,ci,ky,kx] over the (oy, ky) with 2oy+ky-1 = y and the (ox, kx) with 2ox+kx-1 = x
//
//   wgrad     the scheme of exact_gemm_device.hpp with the rows = the N OH OW OUTPUT pixels and the x operand read at the tap's
//             pixel of the input at its pitch; channels at and beyond Cin are staged as zero whatever the memory holds.  fp32 chains of
//             128 rows, fp64 carries, slots added in index order, one rounding.  The stride-1 kernel is left as it is.
//   dinput    by the parity of the input pixel: (even, even) is reached by one tap, (even, odd) and (odd, even) by two, (odd, odd) by
//             four — nine taps per 2x2 block, none of them multiplied by an inserted zero.  Each class is a product [pixels of the
//             class][taps Cout] x [taps Cout][Cin] on the exact-f32 matrix instruction; the depth runs (ky, kx, co) ascending in fp32
//             chains of 128 carried in fp64, so the order of a sum does not depend on N.
//   flatten   f32[B,HW,C] <-> f32[B,C HW]: a tiled transpose per image, values copied.
//   heads     dfeat = g_r W_r + g_t W_t, dW = g^T feat, db = colsum(g): fp64 sums over B in index order, one rounding.
// No atomics and no scratch; every sum has a fixed order, so two calls give equal bits.
#include "conv3x3s2_dinput.hpp"
#include <algorithm>
#include <cstdint>

namespace {

using namespace gdrnpp::exactgemm;
using gdrnpp::aligned16;

constexpr int kSlotRows = 512, kSlotCap = 64, kTnGrid = 512;

inline int pad128(int c) { return (c + 127) / 128 * 128; }

// ---- wgrad ----------------------------------------------------------------------------------------------------------------------
// row_slot_plan (exact_gemm_device.hpp) with the nine taps of the padded channel count as tiles, rounded down as the stride-1 wgrad
inline SlotPlan wgrad_plan(long M, int CinP, int Cout) {
  return row_slot_plan(M, 9l * (Cout / 128) * (CinP / 128), kSlotRows, kSlotCap, kTnGrid, false);
}

// part[slot][tap][co][ci < CinP] (fp64) = sum over the slot's output pixels of dz[pix][co] x[2 pix + tap - 1][ci].  grid (co tile x ci
// tile, slot, tap); workgroup, LDS images, operand map and sums are exact_gemm_device.hpp's.  A pixel whose tap lies outside the
// image contributes nothing: both operands of that row are staged as zero.  A channel quad at or beyond the pitch is not read;
// elements at or beyond Cin are replaced by zero.
__global__ __launch_bounds__(kThreads) void conv3x3s2_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x, int ldx,
                                                                    double* __restrict__ part, int M, int H, int W, int Cin, int CinP,
                                                                    int Cout, long rows_per_slot) {
  __shared__ float sA[kBK * kPitch];
  __shared__ float sB[kBK * kPitch];
  const int tiles2 = CinP / 128;
  const int n1_0 = ((int)blockIdx.x / tiles2) * 128, n2_0 = ((int)blockIdx.x % tiles2) * 128;
  const int tap = blockIdx.z, ky = tap / 3, kx = tap % 3, OH = H >> 1, OW = W >> 1, OHW = OH * OW;
  const long r0 = (long)blockIdx.y * rows_per_slot, r1 = r0 + rows_per_slot < M ? r0 + rows_per_slot : M;
  const float* ap = dz + (size_t)n1_0 + stage_col();
  const int ci0 = n2_0 + stage_col();
  const bool b_in = ci0 < ldx && ci0 < Cin;      // ldx % 4 == 0: the float4 lies inside the row
  const float* bp = x + ci0;
  f4 ra[4], rb[4];
  auto fetch = [&](long r) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const long m = r + stage_row() + 8 * p;
      bool in = m < r1;
      long src = 0;
      if (in) {
        const int n = (int)(m / OHW), pix = (int)(m % OHW);
        const int yy = 2 * (pix / OW) + ky - 1, xx = 2 * (pix % OW) + kx - 1;
        in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        src = ((long)n * H + yy) * W + xx;
      }
      ra[p] = in ? ld4v(ap + (size_t)m * Cout) : f4{0.f, 0.f, 0.f, 0.f};
      f4 b = in && b_in ? ld4v(bp + (size_t)src * ldx) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) b[j] = ci0 + j < Cin ? b[j] : 0.f;
      rb[p] = b;
    }
  };
  Tile t;
  t.clear();
  if (r0 < r1) fetch(r0);
  k_loop<kPitch, kPitch>(t, sA, sB, r0, r1, kBK, fetch, [&] { store_stage<false, false>(sA, sB, ra, rb); });
  double* out = part + ((size_t)blockIdx.y * 9 + tap) * Cout * CinP;
  for_each_d(n1_0, n2_0, [=, &t](int i, int j, int e, int co, int ci) { out[(size_t)co * CinP + ci] = t.carry[i][j][e]; });
}

// dW[co][ci][tap] = fl(the slots in index order), ci < Cin.  Thread i = (tap, co, ci < CinP), ci fastest.
__global__ __launch_bounds__(kThreads) void conv3x3s2_wgrad_finalize_kernel(const double* __restrict__ part, int slots, int Cin, int CinP,
                                                                             int Cout, float* __restrict__ dW) {
  const size_t plane = (size_t)Cout * CinP, i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= 9 * plane) return;
  const size_t tap = i / plane, cc = i % plane, co = cc / CinP, ci = cc % CinP;
  if ((int)ci >= Cin) return;
  double s = 0.0;
#pragma unroll 4
  for (int y = 0; y < slots; ++y) s += part[(size_t)y * 9 * plane + i];
  dW[(co * Cin + ci) * 9 + tap] = (float)s;
}

// ---- dinput ---------------------------------------------------------------------------------------------------------------------
// conv3x3s2_dinput.hpp has the scheme; here Cout % 128 == 0, so every stage of 32 channels is whole.
__global__ __launch_bounds__(kThreads) void conv3x3s2_dinput_kernel(const float* __restrict__ dz, const float* __restrict__ w, int ldw,
                                                                     float* __restrict__ dx, int lddx, int N, int H, int W, int Cin,
                                                                     int Cout, int tiles_n) {
  __shared__ float sA[kBK * kPitchT];
  __shared__ float sB[kBK * kPitch];
  conv3x3s2_dinput_tile<false>(dz, w, ldw, dx, lddx, N, H, W, Cin, Cout, tiles_n, sA, sB);
}

// ---- flatten --------------------------------------------------------------------------------------------------------------------
// dst[b][c][r] = src[b][r][c] for src f32[B][R][C]: 32 x 32 tiles through LDS, 256 threads = 32 x 8.  grid (C tiles, R tiles, B).
__global__ __launch_bounds__(kThreads) void transpose_kernel(const float* __restrict__ src, float* __restrict__ dst, int R, int C) {
  __shared__ float t[32][33];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
  const float* s = src + (size_t)blockIdx.z * R * C;
  float* d = dst + (size_t)blockIdx.z * R * C;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int r = r0 + ty + 8 * k, c = c0 + tx;
    if (r < R && c < C) t[ty + 8 * k][tx] = s[(size_t)r * C + c];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + ty + 8 * k, r = r0 + tx;
    if (r < R && c < C) d[(size_t)c * R + r] = t[tx][ty + 8 * k];
  }
}

// ---- the pose heads -------------------------------------------------------------------------------------------------------------
// dfeat[b][k] = sum_j g_r[b][j] w_r[j][k] + sum_j g_t[b][j] w_t[j][k], rotation rows first, in fp64, rounded once.  A NULL source
// contributes nothing and is not read (nor is its weight).
__global__ __launch_bounds__(kThreads) void heads_dfeat_kernel(const float* __restrict__ g_r, const float* __restrict__ g_t,
                                                                const float* __restrict__ w_r, const float* __restrict__ w_t,
                                                                float* __restrict__ dfeat, int B, int K, int rot_dim) {
  const long i = (long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= (long)B * K) return;
  const int b = (int)(i / K), k = (int)(i % K);
  double s = 0.0;
  if (g_r)
    for (int j = 0; j < rot_dim; ++j) s += (double)g_r[(size_t)b * rot_dim + j] * (double)w_r[(size_t)j * K + k];
  if (g_t)
    for (int j = 0; j < 3; ++j) s += (double)g_t[(size_t)b * 3 + j] * (double)w_t[(size_t)j * K + k];
  dfeat[i] = (float)s;
}

// grid (column blocks of K + 1, rot_dim + 3 rows).  Row j < rot_dim belongs to the rotation head, the others to the translation
// head; thread k < K sums g[b][j] feat[b][k] over b in index order in fp64 (dW), thread K sums g[b][j] (db).  A head whose source is
// NULL gets zeros.
__global__ __launch_bounds__(kThreads) void heads_wgrad_kernel(const float* __restrict__ g_r, const float* __restrict__ g_t,
                                                                const float* __restrict__ feat, float* __restrict__ dW_r,
                                                                float* __restrict__ dW_t, float* __restrict__ db_r,
                                                                float* __restrict__ db_t, int B, int K, int rot_dim) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k > K) return;
  const bool rot = (int)blockIdx.y < rot_dim;
  const int j = rot ? blockIdx.y : blockIdx.y - rot_dim, n = rot ? rot_dim : 3;
  const float* g = rot ? g_r : g_t;
  float* dW = rot ? dW_r : dW_t;
  float* db = rot ? db_r : db_t;
  float* out = k < K ? (dW ? dW + (size_t)j * K + k : nullptr) : (db ? db + j : nullptr);
  if (!out) return;
  double s = 0.0;
  if (g) {
    if (k < K)
      for (int b = 0; b < B; ++b) s += (double)g[(size_t)b * n + j] * (double)feat[(size_t)b * K + k];
    else
      for (int b = 0; b < B; ++b) s += (double)g[(size_t)b * n + j];
  }
  *out = (float)s;
}

bool s2_shape_ok(int N, int H, int W, int Cin, int ld, int Cout) {
  if (!(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && ld > 0)) return false;
  const bool chan = (Cin % 128 == 0 && ld == Cin) || (Cin <= ld && ld % 32 == 0);
  return chan && H % 2 == 0 && W % 2 == 0 && Cout % 128 == 0 && (long)N * H * W < (1l << 31) - 4096 &&
         (long)N * H * W * ld < (1l << 40) && 9l * pad128(Cin) * Cout < (1l << 31);
}

}  // namespace

extern "C" {

size_t gdrnpp_conv3x3s2_wgrad_f32_workspace_bytes(int N, int H, int W, int Cin, int ldx, int Cout) {
  if (!s2_shape_ok(N, H, W, Cin, ldx, Cout)) return 0;
  const int CinP = pad128(Cin);
  return (size_t)wgrad_plan((long)N * (H / 2) * (W / 2), CinP, Cout).slots * 9 * CinP * Cout * sizeof(double);
}

int gdrnpp_conv3x3s2_wgrad_f32(const float* dz, const float* x, int ldx, float* dW, int N, int H, int W, int Cin, int Cout,
                               void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "gdrnpp_conv3x3s2_wgrad_f32";
  GDRNPP_REQUIRE(dz && x && dW && workspace, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && ldx >= Cin, GDRNPP_EINVAL, "%s: N=%d H=%d W=%d Cin=%d ldx=%d Cout=%d", what, N,
                 H, W, Cin, ldx, Cout);
  GDRNPP_REQUIRE(s2_shape_ok(N, H, W, Cin, ldx, Cout), GDRNPP_ELIMIT,
                 "%s: H=%d and W=%d must be even, Cout=%d a multiple of 128, Cin=%d a multiple of 128 with ldx=%d equal to it or ldx a multiple "
                 "of 32, N H W below 2^31", what, H, W, Cout, Cin, ldx);
  GDRNPP_REQUIRE(aligned16(dz) && aligned16(x) && aligned16(workspace), GDRNPP_EINVAL, "%s: dz, x and the workspace must be 16-byte aligned", what);
  const size_t need = gdrnpp_conv3x3s2_wgrad_f32_workspace_bytes(N, H, W, Cin, ldx, Cout);
  GDRNPP_REQUIRE(workspace_bytes >= need, GDRNPP_EINVAL, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
  const int M = N * (H / 2) * (W / 2), CinP = pad128(Cin);
  const SlotPlan p = wgrad_plan(M, CinP, Cout);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(conv3x3s2_wgrad_kernel, dim3((unsigned)((Cout / 128) * (CinP / 128)), (unsigned)p.slots, 9), dim3(kThreads), 0, st, dz, x, ldx,
                     part, M, H, W, Cin, CinP, Cout, p.rows_per_slot);
  const size_t n = (size_t)9 * CinP * Cout;
  hipLaunchKernelGGL(conv3x3s2_wgrad_finalize_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part, p.slots, Cin,
                     CinP, Cout, dW);
  return gdrnpp::check_launch(what);
}

int gdrnpp_conv3x3s2_dinput_f32(const float* dz, const float* w, int ldw, float* dx, int lddx, int N, int H, int W, int Cin, int Cout,
                                void* stream) {
  const char* what = "gdrnpp_conv3x3s2_dinput_f32";
  GDRNPP_REQUIRE(dz && w && dx, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && lddx >= Cin && ldw >= Cin && ldw % 4 == 0, GDRNPP_EINVAL,
                 "%s: N=%d H=%d W=%d Cin=%d lddx=%d ldw=%d (a multiple of 4, >= Cin) Cout=%d", what, N, H, W, Cin, lddx, ldw, Cout);
  GDRNPP_REQUIRE(s2_shape_ok(N, H, W, Cin, lddx, Cout), GDRNPP_ELIMIT,
                 "%s: H=%d and W=%d must be even, Cout=%d a multiple of 128, Cin=%d a multiple of 128 with lddx=%d equal to it or lddx a multiple "
                 "of 32, N H W below 2^31", what, H, W, Cout, Cin, lddx);
  GDRNPP_REQUIRE(aligned16(dz) && aligned16(w), GDRNPP_EINVAL, "%s: dz and w must be 16-byte aligned", what);
  const long Mc = (long)N * (H / 2) * (W / 2);
  const int tiles_n = (lddx + 127) / 128;
  const long blocks = (Mc + 127) / 128 * tiles_n;
  GDRNPP_REQUIRE(blocks < (1l << 31), GDRNPP_ELIMIT, "%s: grid too large", what);
  hipLaunchKernelGGL(conv3x3s2_dinput_kernel, dim3((unsigned)blocks, 4), dim3(kThreads), 0, (hipStream_t)stream, dz, w, ldw, dx, lddx, N, H, W, Cin,
                     Cout, tiles_n);
  return gdrnpp::check_launch(what);
}

int gdrnpp_nhwc_flatten_nchw(const float* src, float* dst, int B, int HW, int C, int inverse, void* stream) {
  const char* what = "gdrnpp_nhwc_flatten_nchw";
  GDRNPP_REQUIRE(src && dst && src != dst, GDRNPP_EINVAL, "%s: null pointer, or src == dst", what);
  GDRNPP_REQUIRE(B > 0 && HW > 0 && C > 0, GDRNPP_EINVAL, "%s: B=%d HW=%d C=%d", what, B, HW, C);
  GDRNPP_REQUIRE(B <= 65535 && (long)HW * C < (1l << 31) && (HW + 31) / 32 <= 65535 && (C + 31) / 32 <= 65535, GDRNPP_ELIMIT,
                 "%s: B=%d HW=%d C=%d outside the grid", what, B, HW, C);
  const int R = inverse ? C : HW, Cc = inverse ? HW : C;      // the source's rows and columns per image
  hipLaunchKernelGGL(transpose_kernel, dim3((unsigned)((Cc + 31) / 32), (unsigned)((R + 31) / 32), (unsigned)B), dim3(kThreads), 0,
                     (hipStream_t)stream, src, dst, R, Cc);
  return gdrnpp::check_launch(what);
}

int gdrnpp_pnp_fc_heads_backward(const float* g_r, const float* g_t, const float* feat, const float* w_r, const float* w_t, float* dfeat,
                                 float* dW_r, float* dW_t, float* db_r, float* db_t, int B, int K, int rot_dim, void* stream) {
  const char* what = "gdrnpp_pnp_fc_heads_backward";
  const bool wants_w = dW_r || dW_t || db_r || db_t;
  if (!dfeat && !wants_w) return 0;      // nothing asked for, nothing launched
  GDRNPP_REQUIRE(B > 0 && K > 0 && rot_dim > 0, GDRNPP_EINVAL, "%s: B=%d K=%d rot_dim=%d", what, B, K, rot_dim);
  GDRNPP_REQUIRE(K <= 1024 && rot_dim <= 9 && B <= (1 << 20), GDRNPP_ELIMIT, "%s: K=%d (<= 1024) rot_dim=%d (<= 9) B=%d (<= 2^20)", what, K, rot_dim, B);
  GDRNPP_REQUIRE(!dfeat || ((!g_r || w_r) && (!g_t || w_t)), GDRNPP_EINVAL, "%s: dfeat needs the weight of every head that has a gradient", what);
  GDRNPP_REQUIRE(!((dW_r && g_r) || (dW_t && g_t)) || feat, GDRNPP_EINVAL, "%s: the weight gradients need feat", what);
  hipStream_t st = (hipStream_t)stream;
  if (dfeat)
    hipLaunchKernelGGL(heads_dfeat_kernel, dim3((unsigned)(((long)B * K + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, g_r, g_t, w_r, w_t, dfeat,
                       B, K, rot_dim);
  if (wants_w)
    hipLaunchKernelGGL(heads_wgrad_kernel, dim3((unsigned)((K + 1 + kThreads - 1) / kThreads), (unsigned)(rot_dim + 3)), dim3(kThreads), 0, st, g_r,
                       g_t, feat, dW_r, dW_t, db_r, db_t, B, K, rot_dim);
  return gdrnpp::check_launch(what);
}

}  // extern "C"
