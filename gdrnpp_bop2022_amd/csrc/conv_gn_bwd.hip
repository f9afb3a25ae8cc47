// Backward of the geometry head's layers  y = act(GroupNorm(conv3x3(x)))  and  bilinear x2  on gfx950.  DESIGN.md "Geometry head
// backward" has the scheme, the measured error against the tests' bar and the times.
//
//   z = conv3x3(x, W) (+ b)    xhat = (z - mean) rstd    a = gamma xhat + beta    y = gelu(a) or a    g = dL/dy      all NHWC fp32
//   dA = g gelu'(a)    dbeta = sum dA    dgamma = sum dA xhat    s1 = sum_group gamma dA    s2 = sum_group gamma dA xhat
//   dz = rstd (gamma dA - (s1 + xhat s2) / m)    dW[co][ci][ky][kx] = sum_pix dz[pix][co] x[pix + (ky-1, kx-1)][ci]    dx = conv3x3(dz, W')
// The two forward-shaped convolutions (z and dx) run on gdrnpp_conv_bias_act_f32 (yolox_net.hip) as it is; hip_lib/gemm.py has the
// measurement behind that.
//
//   gn_bwd      pass 1: fp64 partial sums of dA and dA xhat per (image, slot, channel); finalize: slots in index order -> per-image
//               channel sums, the group sums s1 / s2, and dgamma / dbeta over the images in index order; pass 2: dz.  y and a are
//               recomputed from z with the forward's own expression; mean and rstd from the forward's partials by gn_apply_kernel's.
//   wgrad       the exact-f32 scheme of exact_gemm_device.hpp with the tap as a grid dimension: rows are the N H W pixels, the x
//               operand is read at the tap's shifted pixel, zero outside the image.  fp32 chains of 128 rows, fp64 carries, slots
//               added in index order.
//   up_bwd      the adjoint of upsample2x_kernel (net_kernels.hip) in gather form.
//   im2col      the adjoint of deconv_col2im_kernel (net_kernels.hip): the operand of the transposed convolution's two gradient GEMMs.
// No atomics and no scratch; every sum has a fixed order, so two calls give equal bits.
#include "exact_gemm_device.hpp"
#include "gn_stats.hpp"
#include <algorithm>
#include <cstdint>

namespace {

using namespace gdrnpp::exactgemm;
using gdrnpp::aligned16;
using gdrnpp::gelu_erf;
using gdrnpp::gelu_grad;
using gdrnpp::gn::gn_group_stats;

// ---- GroupNorm (+ GELU) backward ------------------------------------------------------------------------------------------------
// mean and rstd of image n's groups come from gn_group_stats (gn_stats.hpp), the forward's own function: xhat has the forward's bits.
// The pixels of an image are dealt to at most 64 slots of at least 32 pixels; the count depends on HW alone.
struct GnPlan { int slots, pixels; };
inline GnPlan gn_plan(int HW) {
  const int want = std::min(64, (HW + 31) / 32);
  GnPlan p;
  p.pixels = (HW + want - 1) / want;
  p.slots = (HW + p.pixels - 1) / p.pixels;
  return p;
}
// workspace, in doubles: slot[N][S][2][C]  chan[N][2][C]  grp[N][G][2]
struct GnWs { size_t slot, chan, grp, total; };
inline GnWs gn_ws(int N, int HW, int C, int G) {
  const GnPlan p = gn_plan(HW);
  GnWs w;
  w.slot = 0;
  w.chan = (size_t)N * p.slots * 2 * C;
  w.grp = w.chan + (size_t)N * 2 * C;
  w.total = w.grp + (size_t)N * G * 2;
  return w;
}

__device__ __forceinline__ float gn_dA(float z, float m, float r, float ga, float be, float g, bool gelu, float* xhat) {
  const float xh = (z - m) * r;
  *xhat = xh;
  if (!gelu) return g;
  return g * gelu_grad(xh * ga + be);      // a: the forward's expression, (z - m) * r * gamma + beta without contraction
}

// pass 1: grid (slots, N); thread -> channel quad tid % Q, pixels p0 + tid / Q, + 256 / Q, ...; the rows of a workgroup are added in
// row order through LDS.
template <bool GELU>
__global__ __launch_bounds__(kThreads) void gn_bwd_sums_kernel(const float* __restrict__ z, const float* __restrict__ gy,
                                                                const double* __restrict__ part, const float* __restrict__ gamma,
                                                                const float* __restrict__ beta, double* __restrict__ slot, int HW, int C,
                                                                int G, int P, float eps, int pixels) {
  __shared__ float s_mean[64], s_rstd[64];
  __shared__ double sred[kThreads * 8];
  const int Q = C >> 2, cpg = C / G, n = blockIdx.y;
  gn_group_stats(part, n, P, G, HW, cpg, eps, s_mean, s_rstd);
  __syncthreads();
  const int q = threadIdx.x % Q, row = threadIdx.x / Q, rows = kThreads / Q;
  const int g = (4 * q) / cpg;
  const float m = s_mean[g], r = s_rstd[g];
  const f4 ga = ld4v(gamma + 4 * q), be = ld4v(beta + 4 * q);
  const int p0 = blockIdx.x * pixels, p1 = min(HW, p0 + pixels);
  const size_t base = (size_t)n * HW * C + 4 * q;
  double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
  for (int p = p0 + row; p < p1; p += rows) {
    const f4 zv = ld4v(z + base + (size_t)p * C), gv = ld4v(gy + base + (size_t)p * C);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float xh;
      const float dA = gn_dA(zv[j], m, r, ga[j], be[j], gv[j], GELU, &xh);
      a[j] += (double)dA;
      b[j] += (double)dA * (double)xh;
    }
  }
  double* o = sred + threadIdx.x * 8;
#pragma unroll
  for (int j = 0; j < 4; ++j) o[j] = a[j], o[4 + j] = b[j];
  __syncthreads();
  if (row == 0) {
    for (int rr = 1; rr < rows; ++rr) {
      const double* s = sred + (rr * Q + q) * 8;
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] += s[j], b[j] += s[4 + j];
    }
    double* out = slot + ((size_t)n * gridDim.x + blockIdx.x) * 2 * C + 4 * q;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = a[j], out[C + j] = b[j];
  }
}

// finalize 1: grid N.  chan[n][0 / 1][c] = the slots in index order; grp[n][g] = (s1, s2) = the group's channels in index order times gamma.
__global__ __launch_bounds__(kThreads) void gn_bwd_image_kernel(const double* __restrict__ slot, const float* __restrict__ gamma,
                                                                 double* __restrict__ chan, double* __restrict__ grp, int slots, int C, int G) {
  __shared__ double sc[2048];      // 2 C <= 2048 (C / 4 <= 256)
  const int n = blockIdx.x, cpg = C / G;
  for (int c = threadIdx.x; c < 2 * C; c += kThreads) {
    double s = 0.0;
    for (int k = 0; k < slots; ++k) s += slot[((size_t)n * slots + k) * 2 * C + c];
    sc[c] = s;
    chan[(size_t)n * 2 * C + c] = s;
  }
  __syncthreads();
  if ((int)threadIdx.x < G) {
    const int g = threadIdx.x;
    double s1 = 0.0, s2 = 0.0;
    for (int k = 0; k < cpg; ++k) {
      const int c = g * cpg + k;
      s1 += (double)gamma[c] * sc[c];
      s2 += (double)gamma[c] * sc[C + c];
    }
    grp[((size_t)n * G + g) * 2] = s1;
    grp[((size_t)n * G + g) * 2 + 1] = s2;
  }
}

// finalize 2: dbeta[c], dgamma[c] = the images in index order
__global__ __launch_bounds__(kThreads) void gn_bwd_params_kernel(const double* __restrict__ chan, float* __restrict__ dgamma,
                                                                  float* __restrict__ dbeta, int N, int C) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= C) return;
  double sa = 0.0, sb = 0.0;
  for (int n = 0; n < N; ++n) sa += chan[(size_t)n * 2 * C + c], sb += chan[(size_t)n * 2 * C + C + c];
  if (dbeta) dbeta[c] = (float)sa;
  if (dgamma) dgamma[c] = (float)sb;
}

// pass 2: grid (bx, N), the grid stride a multiple of Q (host) so that a thread keeps its channel quad.  The combination runs in
// fp64 and is rounded once: at a handful of elements per group gamma dA and (s1 + xhat s2) / m cancel.
template <bool GELU>
__global__ __launch_bounds__(kThreads) void gn_bwd_dz_kernel(const float* __restrict__ z, const float* __restrict__ gy,
                                                              const double* __restrict__ part, const float* __restrict__ gamma,
                                                              const float* __restrict__ beta, const double* __restrict__ grp,
                                                              float* __restrict__ dz, int HW, int C, int G, int P, float eps) {
  __shared__ float s_mean[64], s_rstd[64];
  const int Q = C >> 2, cpg = C / G, n = blockIdx.y;
  gn_group_stats(part, n, P, G, HW, cpg, eps, s_mean, s_rstd);
  __syncthreads();
  const long total = (long)HW * Q, stride = (long)gridDim.x * kThreads;
  const long i0 = (long)blockIdx.x * kThreads + threadIdx.x;
  const int q = (int)(i0 % Q), g = (4 * q) / cpg;
  const float m = s_mean[g], r = s_rstd[g];
  const f4 ga = ld4v(gamma + 4 * q), be = ld4v(beta + 4 * q);
  const double inv_m = 1.0 / ((double)HW * cpg), rd = (double)r;
  const double s1 = grp[((size_t)n * G + g) * 2], s2 = grp[((size_t)n * G + g) * 2 + 1];
  const size_t base = (size_t)n * HW * C;
  for (long i = i0; i < total; i += stride) {
    const f4 zv = ld4v(z + base + 4 * i), gv = ld4v(gy + base + 4 * i);
    f4 o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float xh;
      const float dA = gn_dA(zv[j], m, r, ga[j], be[j], gv[j], GELU, &xh);
      o[j] = (float)(rd * ((double)ga[j] * (double)dA - (s1 + (double)xh * s2) * inv_m));
    }
    st4v(dz + base + 4 * i, o);
  }
}

// ---- slot plan of the weight gradient: row_slot_plan (exact_gemm_device.hpp) with the nine taps counted as tiles -----------------
// At most min(64, 512 / tiles) slots, rounded down: the grid stays within two workgroups per CU (a workgroup holds a CU's registers),
// and every slot costs 9 Cin Cout doubles written and read once.
constexpr int kSlotRows = 512, kSlotCap = 64, kTnGrid = 512;
inline SlotPlan wgrad_plan(long M, int Cin, int Cout) {
  return row_slot_plan(M, 9l * (Cout / 128) * (Cin / 128), kSlotRows, kSlotCap, kTnGrid, false);
}

// ---- wgrad ----------------------------------------------------------------------------------------------------------------------
// part[slot][tap][co][ci] (fp64) = sum over the slot's pixels of dz[pix][co] x[pix + tap][ci].  grid (co tile x ci tile, slot, tap);
// the workgroup, the LDS images, the operand map and the sums are exact_gemm_device.hpp's.  A pixel whose shifted neighbour is
// outside its image contributes nothing: both operands of that row are staged as zero (so a NaN in dz there stays out of the sum,
// as in the definition).  Rows are pixels of the whole batch: a chunk may end mid image row or span images.
__global__ __launch_bounds__(kThreads) void conv3x3_wgrad_kernel(const float* __restrict__ dz, const float* __restrict__ x,
                                                                  double* __restrict__ part, int M, int H, int W, int Cin, int Cout,
                                                                  long rows_per_slot) {
  __shared__ float sA[kBK * kPitch];
  __shared__ float sB[kBK * kPitch];
  const int tiles2 = Cin / 128;
  const int n1_0 = ((int)blockIdx.x / tiles2) * 128, n2_0 = ((int)blockIdx.x % tiles2) * 128;
  const int tap = blockIdx.z, dy = tap / 3 - 1, dx = tap % 3 - 1, HW = H * W;
  const long r0 = (long)blockIdx.y * rows_per_slot, r1 = r0 + rows_per_slot < M ? r0 + rows_per_slot : M;
  const float* ap = dz + (size_t)n1_0 + stage_col();
  const float* bp = x + (size_t)n2_0 + stage_col();
  f4 ra[4], rb[4];
  auto fetch = [&](long r) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const long m = r + stage_row() + 8 * p;
      bool in = m < r1;
      if (in) {
        const int pix = (int)(m % HW), yy = pix / W + dy, xx = pix % W + dx;
        in = (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
      }
      ra[p] = in ? ld4v(ap + (size_t)m * Cout) : f4{0.f, 0.f, 0.f, 0.f};
      rb[p] = in ? ld4v(bp + (size_t)(m + dy * W + dx) * Cin) : f4{0.f, 0.f, 0.f, 0.f};
    }
  };
  Tile t;
  t.clear();
  if (r0 < r1) fetch(r0);
  k_loop<kPitch, kPitch>(t, sA, sB, r0, r1, kBK, fetch, [&] { store_stage<false, false>(sA, sB, ra, rb); });
  double* out = part + ((size_t)blockIdx.y * 9 + tap) * Cout * Cin;
  for_each_d(n1_0, n2_0, [=, &t](int i, int j, int e, int co, int ci) { out[(size_t)co * Cin + ci] = t.carry[i][j][e]; });
}

// dW[co][ci][tap] = fl(the slots in index order).  Thread i = (tap, co, ci), ci fastest: coalesced reads of every slot's plane.
__global__ __launch_bounds__(kThreads) void conv3x3_wgrad_finalize_kernel(const double* __restrict__ part, int slots, int Cin, int Cout,
                                                                           float* __restrict__ dW) {
  const size_t plane = (size_t)Cout * Cin, i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= 9 * plane) return;
  const size_t tap = i / plane, cc = i % plane;
  double s = 0.0;
#pragma unroll 4
  for (int y = 0; y < slots; ++y) s += part[(size_t)y * 9 * plane + i];
  dW[cc * 9 + tap] = (float)s;
}

// ---- bilinear x2 backward -------------------------------------------------------------------------------------------------------
// One thread per channel quad of an INPUT pixel (i, j).  Output row oy reads input rows y0 and y0 + yp with the weights 1 - l and l
// of upsample2x_kernel (fy = sh oy in fp32, y0 = (int) fy, yp = y0 < H - 1, l = fy - y0); with sh = (H - 1) / (2H - 1) the rows that
// read row i lie in [2i - 2, 2i + 4].  The row weights of those seven candidates (-1 for a row that does not read i) and the seven
// column weights are formed first; the sum then runs over the candidates in (oy, ox) order in fp64 and is rounded once.
__device__ __forceinline__ double up_weight(int o, int i, int in_size, float scale) {
  const float f = scale * (float)o;
  const int i0 = (int)f, ip = i0 < in_size - 1 ? 1 : 0;
  const float l1 = f - (float)i0, l0 = 1.f - l1;
  if (i0 != i && i0 + ip != i) return -1.0;
  return (i0 == i ? (double)l0 : 0.0) + (i0 + ip == i ? (double)l1 : 0.0);
}

__global__ __launch_bounds__(kThreads) void upsample2x_bwd_kernel(const float* __restrict__ gy, float* __restrict__ dx, int N, int H,
                                                                   int W, int C) {
  const int Q = C >> 2, OH = 2 * H, OW = 2 * W;
  const long total = (long)N * H * W * Q;
  const float sh = (OH > 1) ? (float)(H - 1) / (float)(OH - 1) : 0.f;
  const float sw = (OW > 1) ? (float)(W - 1) / (float)(OW - 1) : 0.f;
  for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < total; t += (long)gridDim.x * kThreads) {
    const int q = (int)(t % Q);
    long p = t / Q;
    const int j = (int)(p % W);
    p /= W;
    const int i = (int)(p % H), n = (int)(p / H);
    double wy[7], wx[7];
#pragma unroll
    for (int a = 0; a < 7; ++a) {
      const int oy = 2 * i - 2 + a, ox = 2 * j - 2 + a;
      wy[a] = (oy >= 0 && oy < OH) ? up_weight(oy, i, H, sh) : -1.0;
      wx[a] = (ox >= 0 && ox < OW) ? up_weight(ox, j, W, sw) : -1.0;
    }
    const float* g = gy + ((size_t)n * OH * OW) * C + 4 * q;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int a = 0; a < 7; ++a) {
      if (wy[a] < 0.0) continue;
#pragma unroll
      for (int b = 0; b < 7; ++b) {
        if (wx[b] < 0.0) continue;
        const f4 v = ld4v(g + ((size_t)(2 * i - 2 + a) * OW + (2 * j - 2 + b)) * C);
        const double w = wy[a] * wx[b];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] += w * (double)v[k];
      }
    }
    st4v(dx + (((size_t)n * H + i) * W + j) * C + 4 * q, f4{(float)s[0], (float)s[1], (float)s[2], (float)s[3]});
  }
}

// ---- transposed convolution: im2col ---------------------------------------------------------------------------------------------
// dcols[n][h][w][ky][kx][c] = dy[n][h stride - pad + ky][w stride - pad + kx][c], 0 where that pixel is outside OH x OW.  One thread
// per channel quad of a (pixel, tap): values are copied, nothing is summed.
__global__ __launch_bounds__(kThreads) void deconv_im2col_kernel(const float* __restrict__ dy, float* __restrict__ dcols, int H, int W, int C,
                                                                  int KS, int stride, int pad, int OH, int OW, long total) {
  const int Q = C >> 2;
  for (long t = (long)blockIdx.x * kThreads + threadIdx.x; t < total; t += (long)gridDim.x * kThreads) {
    const int q = (int)(t % Q);
    long p = t / Q;
    const int kx = (int)(p % KS);
    p /= KS;
    const int ky = (int)(p % KS);
    p /= KS;
    const int w = (int)(p % W);
    p /= W;
    const int h = (int)(p % H), n = (int)(p / H);
    const int oy = h * stride - pad + ky, ox = w * stride - pad + kx;
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if ((unsigned)oy < (unsigned)OH && (unsigned)ox < (unsigned)OW) v = ld4v(dy + (((size_t)n * OH + oy) * OW + ox) * C + 4 * q);
    st4v(dcols + 4 * (size_t)t, v);
  }
}

bool gn_shape_ok(int N, int HW, int C, int G) {
  if (N <= 0 || HW <= 0 || C <= 0 || G <= 0 || C % G) return false;
  const int cpg = C / G, Q = C / 4;
  return C % 4 == 0 && cpg % 4 == 0 && Q <= 256 && 256 % Q == 0 && G <= 64 && N <= 65535;
}

bool conv_shape_ok(int N, int H, int W, int Cin, int Cout) {
  return N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0 && Cin % 128 == 0 && Cout % 128 == 0 && (long)N * H * W < (1l << 31) - 4096
         && (long)Cin * Cout * 9 < (1l << 31);
}

}  // namespace

extern "C" {

size_t gdrnpp_groupnorm_act_backward_workspace_bytes(int N, int HW, int C, int G) {
  if (!gn_shape_ok(N, HW, C, G)) return 0;
  return gn_ws(N, HW, C, G).total * sizeof(double);
}

int gdrnpp_groupnorm_act_backward(const float* z, const double* gn_partials, int P, const float* gamma, const float* beta,
                                  const float* grad_y, float* dz, float* dgamma, float* dbeta, int N, int HW, int C, int G, float eps,
                                  int act_gelu, void* workspace, size_t workspace_bytes, void* stream) {
  const char* what = "gdrnpp_groupnorm_act_backward";
  GDRNPP_REQUIRE(z && gn_partials && gamma && beta && grad_y && workspace && (dz || dgamma || dbeta), GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(N > 0 && HW > 0 && C > 0 && G > 0 && P > 0 && C % G == 0, GDRNPP_EINVAL, "%s: N=%d HW=%d C=%d G=%d P=%d", what, N, HW, C, G, P);
  GDRNPP_REQUIRE(gn_shape_ok(N, HW, C, G), GDRNPP_ELIMIT, "%s: unsupported shape C=%d G=%d N=%d", what, C, G, N);
  GDRNPP_REQUIRE(aligned16(z) && aligned16(grad_y) && aligned16(dz) && aligned16(gamma) && aligned16(beta) && aligned16(workspace), GDRNPP_EINVAL,
                 "%s: the tensors and the workspace must be 16-byte aligned", what);
  const GnWs ws = gn_ws(N, HW, C, G);
  GDRNPP_REQUIRE(workspace_bytes >= ws.total * sizeof(double), GDRNPP_EINVAL, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes,
                 ws.total * sizeof(double));
  const GnPlan p = gn_plan(HW);
  double* w = (double*)workspace;
  hipStream_t st = (hipStream_t)stream;
  const dim3 g1((unsigned)p.slots, (unsigned)N);
  if (act_gelu)
    hipLaunchKernelGGL(gn_bwd_sums_kernel<true>, g1, dim3(kThreads), 0, st, z, grad_y, gn_partials, gamma, beta, w + ws.slot, HW, C, G, P, eps, p.pixels);
  else
    hipLaunchKernelGGL(gn_bwd_sums_kernel<false>, g1, dim3(kThreads), 0, st, z, grad_y, gn_partials, gamma, beta, w + ws.slot, HW, C, G, P, eps, p.pixels);
  hipLaunchKernelGGL(gn_bwd_image_kernel, dim3((unsigned)N), dim3(kThreads), 0, st, w + ws.slot, gamma, w + ws.chan, w + ws.grp, p.slots, C, G);
  if (dgamma || dbeta)
    hipLaunchKernelGGL(gn_bwd_params_kernel, dim3((unsigned)((C + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, w + ws.chan, dgamma, dbeta, N, C);
  if (dz) {
    const long total = (long)HW * (C / 4);
    long bx = (total + kThreads * 8 - 1) / (kThreads * 8);      // 256 threads = a whole number of pixels: the stride keeps the quad
    bx = std::max<long>(1, std::min<long>(bx, 256));
    const dim3 g2((unsigned)bx, (unsigned)N);
    if (act_gelu)
      hipLaunchKernelGGL(gn_bwd_dz_kernel<true>, g2, dim3(kThreads), 0, st, z, grad_y, gn_partials, gamma, beta, w + ws.grp, dz, HW, C, G, P, eps);
    else
      hipLaunchKernelGGL(gn_bwd_dz_kernel<false>, g2, dim3(kThreads), 0, st, z, grad_y, gn_partials, gamma, beta, w + ws.grp, dz, HW, C, G, P, eps);
  }
  return gdrnpp::check_launch(what);
}

size_t gdrnpp_conv3x3_wgrad_f32_workspace_bytes(int N, int H, int W, int Cin, int Cout) {
  if (!conv_shape_ok(N, H, W, Cin, Cout)) return 0;
  return (size_t)wgrad_plan((long)N * H * W, Cin, Cout).slots * 9 * Cin * Cout * sizeof(double);
}

int gdrnpp_conv3x3_wgrad_f32(const float* dz, const float* x, float* dW, int N, int H, int W, int Cin, int Cout, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const char* what = "gdrnpp_conv3x3_wgrad_f32";
  GDRNPP_REQUIRE(dz && x && dW && workspace, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, GDRNPP_EINVAL, "%s: N=%d H=%d W=%d Cin=%d Cout=%d", what, N, H, W, Cin, Cout);
  GDRNPP_REQUIRE(conv_shape_ok(N, H, W, Cin, Cout), GDRNPP_ELIMIT, "%s: Cin=%d and Cout=%d must be multiples of 128, N H W below 2^31", what, Cin, Cout);
  GDRNPP_REQUIRE(aligned16(dz) && aligned16(x) && aligned16(workspace), GDRNPP_EINVAL, "%s: dz, x and the workspace must be 16-byte aligned", what);
  const size_t need = gdrnpp_conv3x3_wgrad_f32_workspace_bytes(N, H, W, Cin, Cout);
  GDRNPP_REQUIRE(workspace_bytes >= need, GDRNPP_EINVAL, "%s: workspace of %zu bytes, %zu needed", what, workspace_bytes, need);
  const int M = N * H * W;
  const SlotPlan p = wgrad_plan(M, Cin, Cout);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(conv3x3_wgrad_kernel, dim3((unsigned)((Cout / 128) * (Cin / 128)), (unsigned)p.slots, 9), dim3(kThreads), 0, st, dz, x, part, M,
                     H, W, Cin, Cout, p.rows_per_slot);
  const size_t n = (size_t)9 * Cin * Cout;
  hipLaunchKernelGGL(conv3x3_wgrad_finalize_kernel, dim3((unsigned)((n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part, p.slots, Cin, Cout, dW);
  return gdrnpp::check_launch(what);
}

int gdrnpp_upsample_bilinear2x_backward_nhwc(const float* grad_y, float* dx, int N, int H, int W, int C, void* stream) {
  const char* what = "gdrnpp_upsample_bilinear2x_backward_nhwc";
  GDRNPP_REQUIRE(grad_y && dx, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && aligned16(grad_y) && aligned16(dx), GDRNPP_EINVAL,
                 "%s: N=%d H=%d W=%d C=%d (C %% 4 == 0, 16-byte aligned tensors)", what, N, H, W, C);
  GDRNPP_REQUIRE(H < (1 << 29) && W < (1 << 29), GDRNPP_ELIMIT, "%s: H=%d W=%d", what, H, W);
  const long total = (long)N * H * W * (C / 4);
  const long blocks = (total + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3((unsigned)std::min<long>(blocks, 65536 * 8)), dim3(kThreads), 0, (hipStream_t)stream, grad_y, dx, N, H,
                     W, C);
  return gdrnpp::check_launch(what);
}

int gdrnpp_deconv_im2col_nhwc(const float* dy, float* dcols, int N, int H, int W, int C, int KS, int stride, int pad, int out_pad,
                              void* stream) {
  const char* what = "gdrnpp_deconv_im2col_nhwc";
  GDRNPP_REQUIRE(dy && dcols, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && KS > 0 && stride > 0 && pad >= 0 && out_pad >= 0 && out_pad < stride &&
                     aligned16(dy) && aligned16(dcols),
                 GDRNPP_EINVAL, "%s: bad shape N=%d H=%d W=%d C=%d KS=%d stride=%d pad=%d out_pad=%d (C %% 4 == 0, 16-byte aligned tensors)", what, N, H,
                 W, C, KS, stride, pad, out_pad);
  const long OH = (long)(H - 1) * stride - 2 * pad + KS + out_pad, OW = (long)(W - 1) * stride - 2 * pad + KS + out_pad;
  GDRNPP_REQUIRE(OH > 0 && OW > 0, GDRNPP_EINVAL, "%s: empty output", what);
  GDRNPP_REQUIRE(OH < (1 << 30) && OW < (1 << 30) && KS <= 64, GDRNPP_ELIMIT, "%s: OH=%ld OW=%ld KS=%d", what, OH, OW, KS);
  const long total = (long)N * H * W * KS * KS * (C / 4);
  const long blocks = (total + kThreads - 1) / kThreads;
  hipLaunchKernelGGL(deconv_im2col_kernel, dim3((unsigned)std::min<long>(blocks, 65536 * 8)), dim3(kThreads), 0, (hipStream_t)stream, dy, dcols, H, W, C,
                     KS, stride, pad, (int)OH, (int)OW, total);
  return gdrnpp::check_launch(what);
}

}  // extern "C"
