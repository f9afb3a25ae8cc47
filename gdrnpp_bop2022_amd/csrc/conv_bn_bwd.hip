// Training YOLOX's BaseConv (convolution, BatchNorm with batch statistics, SiLU) on gfx950: the batch statistics, the apply pass,
// the backward of [BatchNorm, SiLU], the weight gradient at any channel widths and the stride-2 data gradient at any widths.
// DESIGN.md "YOLOX conv + BatchNorm + SiLU backward" has the scheme, the resources and the measured error against the tests' bar.
//
//   z = conv(x, W)   ks in {1, 3}, stride in {1, 2}, pad (ks - 1) / 2, all tensors NHWC fp32, M = N OH OW rows of C channels
//   mean, var        per channel over the M rows, var biased;  invstd = 1 / sqrt(var + eps)
//   a = gamma (z - mean) invstd + beta,   y = silu(a) = a sigmoid(a)
//   dA = grad_y silu'(a),  silu'(a) = s (1 + a (1 - s)),  s = sigmoid(a)
//   dbeta = sum dA,  dgamma = sum dA xhat,  dz = gamma invstd (dA - dbeta / M - xhat dgamma / M),  xhat = (z - mean) invstd
//   dW[co][ci][ky][kx] = sum_{n,oy,ox} dz[n,oy,ox,co] x[n, stride oy + ky - pad, stride ox + kx - pad, ci]
//
//   column sums  (statistics; dbeta, dgamma) M rows cut into at most 256 slots of at least 64 rows.  A workgroup of 256 threads is
//             [row lanes][channel quads]: a thread adds its rows in fp64, the row lanes are added in lane order through LDS, the
//             slots in index order by the finalize.  The statistics are summed about the channel's first value, so that
//             var = E[(z - z0)^2] - E[z - z0]^2 cancels at the scale of the spread, not of the mean.
//   a         in fp64 from the fp32 operands, rounded once (bn_pre): the apply pass and the backward share the expression, so the
//             backward's a has the forward's bits.  sigmoid and the products around it in fp32; dz's expression in fp64, rounded once.
//   wgrad     the scheme of exact_gemm_device.hpp: rows = output pixels, the tap a grid dimension, BOTH channel tiles padded to
//             128 with zeros in the staging whatever lies beyond the tensor, only the real Cin x Cout elements stored.  fp32
//             chains of 128 rows, fp64 carries, slots (row_slot_plan) added in index order, one rounding.
//   dinput    conv3x3s2_dinput.hpp with a tap's channels padded to 32 in the staging.
// No atomics and no scratch; every sum has a fixed order, so two calls give equal bits.
#include "conv3x3s2_dinput.hpp"
#include <algorithm>
#include <cstdint>

namespace {

using namespace gdrnpp::exactgemm;
using gdrnpp::aligned16;

// ---- column sums ------------------------------------------------------------------------------------------------------------------
constexpr int kColSlots = 256;    // most slots
constexpr int kColSlotRows = 64;  // fewest rows a slot is made for
constexpr int kMaxC = 4096;

struct ColPlan { int slots; long rows; };
inline ColPlan col_plan(long M) {
  ColPlan p;
  const long want = (M + kColSlotRows - 1) / kColSlotRows;
  p.slots = (int)(want < kColSlots ? want : kColSlots);
  p.rows = (M + p.slots - 1) / p.slots;
  p.slots = (int)((M + p.rows - 1) / p.rows);
  return p;
}
// channel quads a workgroup spans: the power of two at or above C / 4, at most 64; the other 256 / quads threads are row lanes
inline int quad_lanes(int C) {
  int q = 1;
  while (q < C / 4 && q < 64) q *= 2;
  return q;
}

__device__ __forceinline__ float sigmoidf(float a) { return 1.0f / (1.0f + expf(-a)); }
// the pre-activation: fp64 from the fp32 operands, one rounding.  xhat = (z - mean) invstd is the backward's too.
__device__ __forceinline__ double bn_xhat(float z, float mean, float invstd) { return ((double)z - (double)mean) * (double)invstd; }
__device__ __forceinline__ float bn_pre(float z, float mean, float invstd, float gamma, float beta) {
  return (float)((double)gamma * bn_xhat(z, mean, invstd) + (double)beta);
}
// dA = grad_y silu'(a)
__device__ __forceinline__ float silu_bwd(float g, float a) {
  const float s = sigmoidf(a);
  return g * (s * (1.0f + a * (1.0f - s)));
}

// Two fp64 sums per channel over the rows [r0, r1) of slot blockIdx.x -> part[slot][2][C].  grid (slots, quad groups); thread =
// (row lane, quad).  STATS: sums of (z - z0) and (z - z0)^2, z0 = row 0 of the channel.  Else: of dA and dA xhat.
template <bool STATS>
__global__ __launch_bounds__(kThreads) void bn_sums_kernel(const float* __restrict__ z, const float* __restrict__ grad_y,
                                                            const float* __restrict__ mean, const float* __restrict__ invstd,
                                                            const float* __restrict__ gamma, const float* __restrict__ beta,
                                                            double* __restrict__ part, long M, int C, long rows_per_slot, int ql) {
  __shared__ double sh[kThreads * 8];
  const int tid = thread_id(), qi = tid % ql, rl = tid / ql, lanes = kThreads / ql;
  const int c = 4 * ((int)blockIdx.y * ql + qi);
  const bool live = c < C;
  const long r0 = (long)blockIdx.x * rows_per_slot, r1 = r0 + rows_per_slot < M ? r0 + rows_per_slot : M;
  double s1[4] = {0.0, 0.0, 0.0, 0.0}, s2[4] = {0.0, 0.0, 0.0, 0.0};
  if (live) {
    f4 p0, p1, p2, p3;      // STATS: z0.  Else: mean, invstd, gamma, beta.
    if (STATS) {
      p0 = ld4v(z + c);
    } else {
      p0 = ld4v(mean + c), p1 = ld4v(invstd + c), p2 = ld4v(gamma + c), p3 = ld4v(beta + c);
    }
#pragma unroll 2
    for (long r = r0 + rl; r < r1; r += lanes) {
      const f4 v = ld4v(z + (size_t)r * C + c);
      if (STATS) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double d = (double)v[j] - (double)p0[j];
          s1[j] += d, s2[j] += d * d;
        }
      } else {
        const f4 g = ld4v(grad_y + (size_t)r * C + c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const double da = (double)silu_bwd(g[j], bn_pre(v[j], p0[j], p1[j], p2[j], p3[j]));
          s1[j] += da, s2[j] += da * bn_xhat(v[j], p0[j], p1[j]);
        }
      }
    }
  }
  double* mine = sh + tid * 8;
#pragma unroll
  for (int j = 0; j < 4; ++j) mine[j] = s1[j], mine[4 + j] = s2[j];
  __syncthreads();
  if (rl == 0 && live) {
    for (int l = 1; l < lanes; ++l) {
      const double* o = sh + (l * ql + qi) * 8;
#pragma unroll
      for (int j = 0; j < 4; ++j) s1[j] += o[j], s2[j] += o[4 + j];
    }
    double* out = part + (size_t)blockIdx.x * 2 * C + c;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = s1[j], out[C + j] = s2[j];
  }
}

// channel c: the slots in index order -> mean, invstd; the running statistics where given
__global__ __launch_bounds__(kThreads) void bn_stats_finalize_kernel(const double* __restrict__ part, int slots, const float* __restrict__ z,
                                                                      long M, int C, double eps, double momentum, float* __restrict__ mean,
                                                                      float* __restrict__ invstd, float* __restrict__ running_mean,
                                                                      float* __restrict__ running_var) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
  for (int k = 0; k < slots; ++k) s1 += part[(size_t)k * 2 * C + c], s2 += part[(size_t)k * 2 * C + C + c];
  const double d = s1 / (double)M, mu = (double)z[c] + d;
  double var = s2 / (double)M - d * d;
  var = var > 0.0 ? var : 0.0;
  mean[c] = (float)mu;
  invstd[c] = (float)(1.0 / sqrt(var + eps));
  if (running_mean) running_mean[c] = (float)((1.0 - momentum) * (double)running_mean[c] + momentum * mu);
  if (running_var) running_var[c] = (float)((1.0 - momentum) * (double)running_var[c] + momentum * (var * (double)M / (double)(M - 1)));
}

// channel c: the slots in index order -> sums[2][C] (fp64, what the dz pass reads), dbeta, dgamma where asked for
__global__ __launch_bounds__(kThreads) void bn_bwd_finalize_kernel(const double* __restrict__ part, int slots, int C, double* __restrict__ sums,
                                                                    float* __restrict__ dgamma, float* __restrict__ dbeta) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  double s1 = 0.0, s2 = 0.0;
#pragma unroll 4
  for (int k = 0; k < slots; ++k) s1 += part[(size_t)k * 2 * C + c], s2 += part[(size_t)k * 2 * C + C + c];
  sums[c] = s1, sums[C + c] = s2;
  if (dbeta) dbeta[c] = (float)s1;
  if (dgamma) dgamma[c] = (float)s2;
}

// y = silu(a), a quad of channels per thread
__global__ __launch_bounds__(kThreads) void bn_silu_apply_kernel(const float* __restrict__ z, const float* __restrict__ mean,
                                                                  const float* __restrict__ invstd, const float* __restrict__ gamma,
                                                                  const float* __restrict__ beta, float* __restrict__ y, size_t n4, int qpr) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (size_t)gridDim.x * kThreads) {
    const int c = 4 * (int)(i % qpr);
    const f4 v = ld4v(z + 4 * i), mu = ld4v(mean + c), is = ld4v(invstd + c), ga = ld4v(gamma + c), be = ld4v(beta + c);
    f4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float a = bn_pre(v[j], mu[j], is[j], ga[j], be[j]);
      o[j] = a * sigmoidf(a);
    }
    st4v(y + 4 * i, o);
  }
}

// dz = gamma invstd (dA - dbeta / M - xhat dgamma / M) with the fp64 sums
__global__ __launch_bounds__(kThreads) void bn_silu_dz_kernel(const float* __restrict__ z, const float* __restrict__ grad_y,
                                                               const float* __restrict__ mean, const float* __restrict__ invstd,
                                                               const float* __restrict__ gamma, const float* __restrict__ beta,
                                                               const double* __restrict__ sums, float* __restrict__ dz, size_t n4, int qpr,
                                                               double inv_m) {
  const int C = 4 * qpr;
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (size_t)gridDim.x * kThreads) {
    const int c = 4 * (int)(i % qpr);
    const f4 v = ld4v(z + 4 * i), g = ld4v(grad_y + 4 * i);
    const f4 mu = ld4v(mean + c), is = ld4v(invstd + c), ga = ld4v(gamma + c), be = ld4v(beta + c);
    f4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double xhat = bn_xhat(v[j], mu[j], is[j]);
      const double da = (double)silu_bwd(g[j], bn_pre(v[j], mu[j], is[j], ga[j], be[j]));
      o[j] = (float)((double)ga[j] * (double)is[j] * (da - sums[c + j] * inv_m - xhat * (sums[C + c + j] * inv_m)));
    }
    st4v(dz + 4 * i, o);
  }
}

inline unsigned elementwise_blocks(size_t n4) { return (unsigned)std::min<size_t>((n4 + kThreads - 1) / kThreads, 8192); }

bool bn_shape_ok(long M, int C) { return M >= 2 && M < (1l << 31) && C > 0 && C % 4 == 0 && C <= kMaxC; }

// ---- wgrad ----------------------------------------------------------------------------------------------------------------------
constexpr int kSlotRows = 512, kSlotCap = 64, kTnGrid = 512;

__host__ __device__ inline int tiles128(int c) { return (c + 127) / 128; }
inline int out_size(int n, int ks, int stride) { return (n + 2 * ((ks - 1) / 2) - ks) / stride + 1; }

// row_slot_plan (exact_gemm_device.hpp) with the taps of the padded channel counts as tiles, rounded down as the other wgrads
inline SlotPlan wgrad_plan(long M, int Cin, int Cout, int ks) {
  return row_slot_plan(M, (long)ks * ks * tiles128(Cout) * tiles128(Cin), kSlotRows, kSlotCap, kTnGrid, false);
}

// part[slot][tap][co][ci] (fp64) = sum over the slot's output pixels of dz[pix][co] x[stride pix + tap - pad][ci].  grid (co tile x
// ci tile, slot, tap); workgroup, LDS images, operand map and sums are exact_gemm_device.hpp's.  A pixel whose tap lies outside the
// image contributes nothing: both operands of that row are staged as zero.  Cin % 4 == 0 and Cout % 4 == 0: a channel quad lies
// inside its tensor or outside it, and one outside is staged as zero and not read.
__global__ __launch_bounds__(kThreads) void conv_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                               double* __restrict__ part, int M, int H, int W, int OH, int OW, int Cin,
                                                               int Cout, int ks, int stride, long rows_per_slot) {
  __shared__ float sA[kBK * kPitch];
  __shared__ float sB[kBK * kPitch];
  const int tiles2 = tiles128(Cin);
  const int n1_0 = ((int)blockIdx.x / tiles2) * 128, n2_0 = ((int)blockIdx.x % tiles2) * 128;
  const int tap = blockIdx.z, ky = tap / ks, kx = tap % ks, pad = (ks - 1) / 2, OHW = OH * OW;
  const long r0 = (long)blockIdx.y * rows_per_slot, r1 = r0 + rows_per_slot < M ? r0 + rows_per_slot : M;
  const int co0 = n1_0 + stage_col(), ci0 = n2_0 + stage_col();
  const bool a_in = co0 < Cout, b_in = ci0 < Cin;
  const float* ap = dz + co0;
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
        const int yy = stride * (pix / OW) + ky - pad, xx = stride * (pix % OW) + kx - pad;
        in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
        src = ((long)n * H + yy) * W + xx;
      }
      ra[p] = in && a_in ? ld4v(ap + (size_t)m * Cout) : f4{0.f, 0.f, 0.f, 0.f};
      rb[p] = in && b_in ? ld4v(bp + (size_t)src * Cin) : f4{0.f, 0.f, 0.f, 0.f};
    }
  };
  Tile t;
  t.clear();
  if (r0 < r1) fetch(r0);
  k_loop<kPitch, kPitch>(t, sA, sB, r0, r1, kBK, fetch, [&] { store_stage<false, false>(sA, sB, ra, rb); });
  double* out = part + ((size_t)blockIdx.y * (ks * ks) + tap) * Cout * Cin;
  for_each_d(n1_0, n2_0, [=, &t](int i, int j, int e, int co, int ci) {
    if (co < Cout && ci < Cin) out[(size_t)co * Cin + ci] = t.carry[i][j][e];
  });
}

// dW[co][ci][tap] = fl(the slots in index order).  Thread i = (tap, co, ci), ci fastest.
__global__ __launch_bounds__(kThreads) void conv_wgrad_finalize_kernel(const double* __restrict__ part, int slots, int Cin, int Cout, int taps,
                                                                        float* __restrict__ dW) {
  const size_t plane = (size_t)Cout * Cin, i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= taps * plane) return;
  const size_t tap = i / plane, cc = i % plane;
  double s = 0.0;
#pragma unroll 4
  for (int y = 0; y < slots; ++y) s += part[(size_t)y * taps * plane + i];
  dW[cc * taps + tap] = (float)s;
}

bool conv_shape_ok(int N, int H, int W, int Cin, int Cout, int ks, int stride) {
  if (!(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0)) return false;
  if (!((ks == 1 || ks == 3) && (stride == 1 || stride == 2))) return false;
  if (stride == 2 && (H % 2 || W % 2)) return false;
  return Cin % 4 == 0 && Cout % 4 == 0 && (long)N * H * W < (1l << 31) - 4096 && (long)N * H * W * std::max(Cin, Cout) < (1l << 40) &&
         (long)ks * ks * Cin * Cout < (1l << 31) && (long)tiles128(Cin) * tiles128(Cout) < (1l << 20);
}

// ---- dinput ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void conv3x3s2_dinput_any_kernel(const float* __restrict__ dz, const float* __restrict__ w,
                                                                         float* __restrict__ dx, int N, int H, int W, int Cin, int Cout,
                                                                         int tiles_n) {
  __shared__ float sA[kBK * kPitchT];
  __shared__ float sB[kBK * kPitch];
  conv3x3s2_dinput_tile<true>(dz, w, Cin, dx, Cin, N, H, W, Cin, Cout, tiles_n, sA, sB);
}

}  // namespace

extern "C" {

size_t gdrnpp_bn_train_stats_workspace_bytes(long M, int C) {
  if (!bn_shape_ok(M, C)) return 0;
  return (size_t)col_plan(M).slots * 2 * C * sizeof(double);
}

int gdrnpp_bn_train_stats_nhwc(const float* z, float* mean, float* invstd, float* running_mean, float* running_var, long M, int C,
                               double eps, double momentum, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "gdrnpp_bn_train_stats_nhwc";
  GDRNPP_REQUIRE(z && mean && invstd && workspace, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(M >= 2 && C > 0 && C % 4 == 0 && eps >= 0.0, GDRNPP_EINVAL,
                 "%s: M=%ld (batch statistics need at least 2 values per channel) C=%d (a multiple of 4) eps=%g", what, M, C, eps);
  GDRNPP_REQUIRE(bn_shape_ok(M, C), GDRNPP_ELIMIT, "%s: M=%ld (below 2^31) C=%d (<= %d)", what, M, C, kMaxC);
  GDRNPP_REQUIRE(aligned16(z) && aligned16(workspace), GDRNPP_EINVAL, "%s: z and the workspace must be 16-byte aligned", what);
  const size_t need = gdrnpp_bn_train_stats_workspace_bytes(M, C);
  GDRNPP_REQUIRE(workspace_bytes >= need, GDRNPP_EINVAL, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
  const ColPlan p = col_plan(M);
  const int ql = quad_lanes(C);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(bn_sums_kernel<true>, dim3((unsigned)p.slots, (unsigned)((C / 4 + ql - 1) / ql)), dim3(kThreads), 0, st, z, nullptr, nullptr,
                     nullptr, nullptr, nullptr, part, M, C, p.rows, ql);
  hipLaunchKernelGGL(bn_stats_finalize_kernel, dim3((unsigned)((C + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part, p.slots, z, M, C, eps,
                     momentum, mean, invstd, running_mean, running_var);
  return gdrnpp::check_launch(what);
}

int gdrnpp_bn_silu_apply_nhwc(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta, float* y,
                              long M, int C, void* stream) {
  const char* what = "gdrnpp_bn_silu_apply_nhwc";
  GDRNPP_REQUIRE(z && mean && invstd && gamma && beta && y, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(M > 0 && C > 0 && C % 4 == 0, GDRNPP_EINVAL, "%s: M=%ld C=%d (a multiple of 4)", what, M, C);
  GDRNPP_REQUIRE(M < (1l << 31) && C <= kMaxC, GDRNPP_ELIMIT, "%s: M=%ld (below 2^31) C=%d (<= %d)", what, M, C, kMaxC);
  GDRNPP_REQUIRE(aligned16(z) && aligned16(y) && aligned16(mean) && aligned16(invstd) && aligned16(gamma) && aligned16(beta), GDRNPP_EINVAL,
                 "%s: every tensor must be 16-byte aligned", what);
  const size_t n4 = (size_t)M * (C / 4);
  hipLaunchKernelGGL(bn_silu_apply_kernel, dim3(elementwise_blocks(n4)), dim3(kThreads), 0, (hipStream_t)stream, z, mean, invstd, gamma, beta, y, n4,
                     C / 4);
  return gdrnpp::check_launch(what);
}

size_t gdrnpp_bn_silu_backward_workspace_bytes(long M, int C) {
  if (!bn_shape_ok(M, C)) return 0;
  return ((size_t)col_plan(M).slots + 1) * 2 * C * sizeof(double);
}

int gdrnpp_bn_silu_backward(const float* grad_y, const float* z, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, float* dz, float* dgamma, float* dbeta, long M, int C, void* workspace,
                            size_t workspace_bytes, void* stream) {
  const char* what = "gdrnpp_bn_silu_backward";
  GDRNPP_REQUIRE(grad_y && z && mean && invstd && gamma && beta && workspace, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(dz || dgamma || dbeta, GDRNPP_EINVAL, "%s: no output asked for", what);
  GDRNPP_REQUIRE(M >= 2 && C > 0 && C % 4 == 0, GDRNPP_EINVAL, "%s: M=%ld (at least 2) C=%d (a multiple of 4)", what, M, C);
  GDRNPP_REQUIRE(bn_shape_ok(M, C), GDRNPP_ELIMIT, "%s: M=%ld (below 2^31) C=%d (<= %d)", what, M, C, kMaxC);
  GDRNPP_REQUIRE(aligned16(grad_y) && aligned16(z) && aligned16(mean) && aligned16(invstd) && aligned16(gamma) && aligned16(beta) &&
                     aligned16(workspace) && aligned16(dz),
                 GDRNPP_EINVAL, "%s: every tensor and the workspace must be 16-byte aligned", what);
  const size_t need = gdrnpp_bn_silu_backward_workspace_bytes(M, C);
  GDRNPP_REQUIRE(workspace_bytes >= need, GDRNPP_EINVAL, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
  const ColPlan p = col_plan(M);
  const int ql = quad_lanes(C);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  double* sums = part + (size_t)p.slots * 2 * C;
  hipLaunchKernelGGL(bn_sums_kernel<false>, dim3((unsigned)p.slots, (unsigned)((C / 4 + ql - 1) / ql)), dim3(kThreads), 0, st, z, grad_y, mean,
                     invstd, gamma, beta, part, M, C, p.rows, ql);
  hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3((unsigned)((C + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part, p.slots, C, sums, dgamma,
                     dbeta);
  if (dz) {
    const size_t n4 = (size_t)M * (C / 4);
    hipLaunchKernelGGL(bn_silu_dz_kernel, dim3(elementwise_blocks(n4)), dim3(kThreads), 0, st, z, grad_y, mean, invstd, gamma, beta, sums, dz, n4,
                       C / 4, 1.0 / (double)M);
  }
  return gdrnpp::check_launch(what);
}

size_t gdrnpp_conv_wgrad_f32_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks, int stride) {
  if (!conv_shape_ok(N, H, W, Cin, Cout, ks, stride)) return 0;
  const long M = (long)N * out_size(H, ks, stride) * out_size(W, ks, stride);
  return (size_t)wgrad_plan(M, Cin, Cout, ks).slots * ks * ks * Cin * Cout * sizeof(double);
}

int gdrnpp_conv_wgrad_f32(const float* dz, const float* x, float* dW, int N, int H, int W, int Cin, int Cout, int ks, int stride,
                          void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "gdrnpp_conv_wgrad_f32";
  GDRNPP_REQUIRE(dz && x && dW && workspace, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, GDRNPP_EINVAL, "%s: N=%d H=%d W=%d Cin=%d Cout=%d", what, N, H, W, Cin, Cout);
  GDRNPP_REQUIRE(conv_shape_ok(N, H, W, Cin, Cout, ks, stride), GDRNPP_ELIMIT,
                 "%s: ks=%d must be 1 or 3, stride=%d 1 or 2 with H=%d and W=%d even at stride 2, Cin=%d and Cout=%d multiples of 4, N H W below 2^31",
                 what, ks, stride, H, W, Cin, Cout);
  GDRNPP_REQUIRE(aligned16(dz) && aligned16(x) && aligned16(workspace), GDRNPP_EINVAL, "%s: dz, x and the workspace must be 16-byte aligned", what);
  const size_t need = gdrnpp_conv_wgrad_f32_workspace_bytes(N, H, W, Cin, Cout, ks, stride);
  GDRNPP_REQUIRE(workspace_bytes >= need, GDRNPP_EINVAL, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
  const int OH = out_size(H, ks, stride), OW = out_size(W, ks, stride), M = N * OH * OW, taps = ks * ks;
  const SlotPlan p = wgrad_plan(M, Cin, Cout, ks);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(conv_wgrad_kernel, dim3((unsigned)(tiles128(Cout) * tiles128(Cin)), (unsigned)p.slots, (unsigned)taps), dim3(kThreads), 0, st,
                     dz, x, part, M, H, W, OH, OW, Cin, Cout, ks, stride, p.rows_per_slot);
  const size_t n = (size_t)taps * Cin * Cout;
  hipLaunchKernelGGL(conv_wgrad_finalize_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part, p.slots, Cin, Cout,
                     taps, dW);
  return gdrnpp::check_launch(what);
}

int gdrnpp_conv3x3s2_dinput_any_f32(const float* dz, const float* w, float* dx, int N, int H, int W, int Cin, int Cout, void* stream) {
  const char* what = "gdrnpp_conv3x3s2_dinput_any_f32";
  GDRNPP_REQUIRE(dz && w && dx, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, GDRNPP_EINVAL, "%s: N=%d H=%d W=%d Cin=%d Cout=%d", what, N, H, W, Cin, Cout);
  GDRNPP_REQUIRE(conv_shape_ok(N, H, W, Cin, Cout, 3, 2), GDRNPP_ELIMIT,
                 "%s: H=%d and W=%d must be even, Cin=%d and Cout=%d multiples of 4, N H W below 2^31", what, H, W, Cin, Cout);
  GDRNPP_REQUIRE(aligned16(dz) && aligned16(w), GDRNPP_EINVAL, "%s: dz and w must be 16-byte aligned", what);
  const long Mc = (long)N * (H / 2) * (W / 2);
  const int tiles_n = tiles128(Cin);
  const long blocks = (Mc + 127) / 128 * tiles_n;
  GDRNPP_REQUIRE(blocks < (1l << 31), GDRNPP_ELIMIT, "%s: grid too large", what);
  hipLaunchKernelGGL(conv3x3s2_dinput_any_kernel, dim3((unsigned)blocks, 4), dim3(kThreads), 0, (hipStream_t)stream, dz, w, dx, N, H, W, Cin, Cout,
                     tiles_n);
  return gdrnpp::check_launch(what);
}

}  // extern "C"
