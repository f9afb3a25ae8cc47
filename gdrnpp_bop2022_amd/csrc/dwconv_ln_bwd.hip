// Backward of depthwise 7x7 (pad 3) + bias + LayerNorm over C, NHWC fp32, on gfx950: the training counterpart of
// dwconv7_ln_kernel (net_kernels.hip), which stays the forward.  DESIGN.md "dwconv7x7 + LayerNorm backward" has the traffic,
// the FMA counts and the measured resources.
//
//   forward   u = b + sum_tap w x(shifted)      mu, var over c      r = 1 / sqrt(var + eps)      xh = (u - mu) r      y = gamma xh + beta
//   backward  dbeta = sum_pix g    dgamma = sum_pix g xh    gh = g gamma    du = r (gh - mean_c(gh) - xh mean_c(gh xh))    db = sum_pix du
//             dw[c,ky,kx] = sum_pix du[p] x[p + (ky-3, kx-3)]              dx[p] = sum_tap w[c,ky,kx] du[p - (ky-3, kx-3)]
//
// Four kernels, no floating-point atomics, every sum in a fixed order:
//   du   (pass A)  recomputes u from x and forms the LayerNorm statistics and du in fp64 (conv_tile_f64 says why), with the
//                  forward's lane layout and its DPP group sums (dpp_sum.hpp, the fp64 form); writes du as fp32 to the workspace.
//                  Persistent workgroups keep dbeta / dgamma / db of the pixels they walk in fp64 registers and write ONE
//                  partial [3][C] each.
//   dx   (pass B1) the forward's convolution over du with the taps mirrored.
//   dw   (pass B2) grid (slots, 7): workgroup (s, ky) owns kernel row ky — 7 taps x a channel quad = 28 accumulators per thread instead
//                  of 196 — sums du x over a row segment in fp32 and carries the running total in fp64; one partial [7][C] each.
//   finalize       sums the partials over the slots in fp64, writes dw in the [C,1,7,7] layout of conv.weight.
// The slot counts depend on the shape alone (tile_groups / kSlots*), tiles are dealt to workgroups with a fixed stride.
// dx and dw are separate passes because fusing them needs the 196 dw accumulators beside the dx tile (no scratch: the
// budget is 256 VGPRs at this workgroup size); separate, each is skipped when its output is not wanted.
#include "common.hpp"
#include "dpp_sum.hpp"
#include "ln_bwd_sums.hpp"
#include <algorithm>
#include <cstdint>

namespace {

using namespace gdrnpp::lnbwd;  // f4 / d4 helpers, kThreads, pixel_sums, block_partial

constexpr int kTW = 4;         // pixels of one image row per thread, passes A and B1
constexpr int kTWB = 8;        // ... pass B2
constexpr int kSlotsA = 512;   // most workgroups (= partials [3][C]) of pass A
constexpr int kSlotsB = 64;    // most workgroups per kernel row (= partials [7][C]) of pass B2

// a tile = `tw` pixels of one image row; a tile group = the kThreads / Q tiles one workgroup holds at a time
__host__ __device__ inline long n_tiles_of(int N, int H, int W, int tw) { return (long)N * H * ((W + tw - 1) / tw); }
__host__ __device__ inline long tile_groups(int N, int H, int W, int Q, int tw) {
  const int per = kThreads / Q;
  return (n_tiles_of(N, H, W, tw) + per - 1) / per;
}
inline int slots_a(int N, int H, int W, int Q) { return (int)std::min<long>(tile_groups(N, H, W, Q, kTW), kSlotsA); }
inline int slots_b(int N, int H, int W, int Q) { return (int)std::min<long>(tile_groups(N, H, W, Q, kTWB), kSlotsB); }

struct Tile {
  bool active;
  int n, oy, ox0;
};
__device__ __forceinline__ Tile tile_at(long tile, long n_tiles, int H, int tiles_x, int tw) {
  Tile t{tile < n_tiles, 0, 0, 0};
  if (t.active) {
    const long row = tile / tiles_x;  // n * H + oy
    t.n = (int)(row / H);
    t.oy = (int)(row - (long)t.n * H);
    t.ox0 = (int)(tile - row * tiles_x) * tw;
  }
  return t;
}

// Pass B1's convolution, the forward's with the taps mirrored: acc[j] += sum_tap w[48 - tap] src[oy + ky - 3][ox0 + j + kx - 3], zero
// outside the image.  img = the image's base + 4 q, wq = the tap-major weights + 4 q.  fp32 fma chain in (ky, kx) order, rows outside
// the image skipped, columns outside add an exact zero.
template <int TW>
__device__ __forceinline__ void conv_tile_mirrored(const float* __restrict__ img, const float* __restrict__ wq, int H, int W, int C, int oy,
                                                   int ox0, f4 (&acc)[TW]) {
#pragma unroll 1
  for (int ky = 0; ky < 7; ++ky) {
    const int iy = oy + ky - 3;
    if (iy < 0 || iy >= H) continue;
    f4 row[TW + 6];
#pragma unroll
    for (int c = 0; c < TW + 6; ++c) {
      const int ix = ox0 + c - 3;
      row[c] = (ix >= 0 && ix < W) ? ld4v(img + ((size_t)iy * W + ix) * C) : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) {
      const f4 wv = ld4v(wq + (size_t)(48 - (ky * 7 + kx)) * C);
#pragma unroll
      for (int j = 0; j < TW; ++j) acc[j] = __builtin_elementwise_fma(row[j + kx], wv, acc[j]);
    }
  }
}

// Pass A's convolution: the forward's taps, unmirrored, on top of the bias in acc, in fp64.  du = r (gh - mean(gh) - xh mean(gh xh)) cancels (sum_c du = 0 = sum_c du xh), and r
// grows as a pixel's channels agree, so an fp32 u — half an ulp off at best — already costs du about an ulp of its largest entry:
// measured at 1 x 1 x C = 4, 1.4 times the tests' bar in fp32, below it in fp64.  Cost: two v_fma_f64 where the fp32 chain has one
// v_pk_fma_f32.  Rows are converted once, when they are loaded.
template <int TW>
__device__ __forceinline__ void conv_tile_f64(const float* __restrict__ img, const float* __restrict__ wq, int H, int W, int C, int oy, int ox0,
                                              d4 (&acc)[TW]) {
#pragma unroll 1
  for (int ky = 0; ky < 7; ++ky) {
    const int iy = oy + ky - 3;
    if (iy < 0 || iy >= H) continue;
    d4 row[TW + 6];
#pragma unroll
    for (int c = 0; c < TW + 6; ++c) {
      const int ix = ox0 + c - 3;
      row[c] = (ix >= 0 && ix < W) ? to_d4(ld4v(img + ((size_t)iy * W + ix) * C)) : d4{0.0, 0.0, 0.0, 0.0};
    }
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) {
      const d4 wv = to_d4(ld4v(wq + (size_t)(ky * 7 + kx) * C));
#pragma unroll
      for (int j = 0; j < TW; ++j) acc[j] = __builtin_elementwise_fma(row[j + kx], wv, acc[j]);
    }
  }
}

// ---- pass A -------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dwln_bwd_du_kernel(const float* __restrict__ x, const float* __restrict__ w49c,
                                                                const float* __restrict__ bias, const float* __restrict__ ln_w,
                                                                const float* __restrict__ g, float* __restrict__ du,
                                                                double* __restrict__ part, int N, int H, int W, int C, float eps) {
  __shared__ double red[2 * kTW * 4];
  __shared__ double sh[kThreads * 12];
  const int Q = C >> 2, q = threadIdx.x % Q, tl = threadIdx.x / Q, per = kThreads / Q;
  const int tiles_x = (W + kTW - 1) / kTW;
  const long n_tiles = n_tiles_of(N, H, W, kTW), n_groups = (n_tiles + per - 1) / per;
  const d4 b4 = to_d4(ld4v(bias + 4 * q)), gam = to_d4(ld4v(ln_w + 4 * q));
  const double inv_c = 1.0 / (double)C;
  double acc[12];  // dbeta, dgamma, db of this thread's quad
#pragma unroll
  for (int k = 0; k < 12; ++k) acc[k] = 0.0;
  for (long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const Tile t = tile_at(grp * per + tl, n_tiles, H, tiles_x, kTW);
    const size_t img = (size_t)t.n * H * W * C + 4 * q;
    d4 u[kTW];
#pragma unroll
    for (int j = 0; j < kTW; ++j) u[j] = b4;
    if (t.active) conv_tile_f64<kTW>(x + img, w49c + 4 * q, H, W, C, t.oy, t.ox0, u);
    double s[kTW], rstd[kTW];
#pragma unroll
    for (int j = 0; j < kTW; ++j) s[j] = sum4(u[j]);
    pixel_sums(s, Q, red);
#pragma unroll
    for (int j = 0; j < kTW; ++j) {
      u[j] = u[j] - s[j] * inv_c;
      s[j] = sum4(u[j] * u[j]);
    }
    pixel_sums(s, Q, red);
    d4 gv[kTW], gh[kTW];
    double m[2 * kTW];
#pragma unroll
    for (int j = 0; j < kTW; ++j) {
      rstd[j] = 1.0 / sqrt(s[j] * inv_c + (double)eps);
      u[j] = u[j] * rstd[j];  // xh
      const bool in = t.active && t.ox0 + j < W;
      gv[j] = in ? to_d4(ld4v(g + img + ((size_t)t.oy * W + t.ox0 + j) * C)) : d4{0.0, 0.0, 0.0, 0.0};
      gh[j] = gv[j] * gam;
      m[j] = sum4(gh[j]);
      m[kTW + j] = sum4(gh[j] * u[j]);
    }
    pixel_sums(m, Q, red);
#pragma unroll
    for (int j = 0; j < kTW; ++j) {
      if (!(t.active && t.ox0 + j < W)) continue;
      const d4 d = (gh[j] - m[j] * inv_c - u[j] * (m[kTW + j] * inv_c)) * rstd[j];
      st4v(du + img + ((size_t)t.oy * W + t.ox0 + j) * C, __builtin_convertvector(d, f4));
      const d4 gx = gv[j] * u[j];
      acc[0] += gv[j].x, acc[1] += gv[j].y, acc[2] += gv[j].z, acc[3] += gv[j].w;
      acc[4] += gx.x, acc[5] += gx.y, acc[6] += gx.z, acc[7] += gx.w;
      acc[8] += d.x, acc[9] += d.y, acc[10] += d.z, acc[11] += d.w;
    }
  }
  block_partial(acc, sh, Q, C, part + (size_t)blockIdx.x * 3 * C);
}

// ---- pass B1 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dwln_bwd_dx_kernel(const float* __restrict__ du, const float* __restrict__ w49c,
                                                                float* __restrict__ dx, int N, int H, int W, int C) {
  const int Q = C >> 2, q = threadIdx.x % Q, tl = threadIdx.x / Q, per = kThreads / Q;
  const int tiles_x = (W + kTW - 1) / kTW;
  const long n_tiles = n_tiles_of(N, H, W, kTW), n_groups = (n_tiles + per - 1) / per;
  for (long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const Tile t = tile_at(grp * per + tl, n_tiles, H, tiles_x, kTW);
    if (!t.active) continue;
    const size_t img = (size_t)t.n * H * W * C + 4 * q;
    f4 acc[kTW];
#pragma unroll
    for (int j = 0; j < kTW; ++j) acc[j] = f4{0.f, 0.f, 0.f, 0.f};
    conv_tile_mirrored<kTW>(du + img, w49c + 4 * q, H, W, C, t.oy, t.ox0, acc);
#pragma unroll
    for (int j = 0; j < kTW; ++j)
      if (t.ox0 + j < W) st4v(dx + img + ((size_t)t.oy * W + t.ox0 + j) * C, acc[j]);
  }
}

// ---- pass B2 ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void dwln_bwd_dw_kernel(const float* __restrict__ du, const float* __restrict__ x,
                                                                double* __restrict__ part, int N, int H, int W, int C) {
  __shared__ double sh[kThreads * 28];
  const int Q = C >> 2, q = threadIdx.x % Q, tl = threadIdx.x / Q, per = kThreads / Q;
  const int ky = blockIdx.y;
  const int tiles_x = (W + kTWB - 1) / kTWB;
  const long n_tiles = n_tiles_of(N, H, W, kTWB), n_groups = (n_tiles + per - 1) / per;
  double acc[28];  // [kx][4]
#pragma unroll
  for (int k = 0; k < 28; ++k) acc[k] = 0.0;
  for (long grp = blockIdx.x; grp < n_groups; grp += gridDim.x) {
    const Tile t = tile_at(grp * per + tl, n_tiles, H, tiles_x, kTWB);
    const int iy = t.oy + ky - 3;
    if (!t.active || iy < 0 || iy >= H) continue;
    const size_t img = (size_t)t.n * H * W * C + 4 * q;
    f4 d[kTWB], row[kTWB + 6];
#pragma unroll
    for (int j = 0; j < kTWB; ++j)
      d[j] = t.ox0 + j < W ? ld4v(du + img + ((size_t)t.oy * W + t.ox0 + j) * C) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int c = 0; c < kTWB + 6; ++c) {
      const int ix = t.ox0 + c - 3;
      row[c] = (ix >= 0 && ix < W) ? ld4v(x + img + ((size_t)iy * W + ix) * C) : f4{0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int kx = 0; kx < 7; ++kx) {
      f4 a = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < kTWB; ++j) a = __builtin_elementwise_fma(d[j], row[j + kx], a);
      acc[4 * kx + 0] += (double)a.x, acc[4 * kx + 1] += (double)a.y, acc[4 * kx + 2] += (double)a.z, acc[4 * kx + 3] += (double)a.w;
    }
  }
  block_partial(acc, sh, Q, C, part + ((size_t)blockIdx.x * 7 + ky) * 7 * C);
}

// ---- finalize -----------------------------------------------------------------------------------------------------------------
// Output e < 49 C: dw of (tap, c) = (e / C, e % C) over the sb slots of pass B2; then dbeta / dgamma / db of channel c over the sa
// slots of pass A.  A workgroup sums kFinOut outputs: 16 threads per output take the slots k = ty, ty + 16, ... in index order, and
// their 16 sums are added in ty order — fp64, the same order in every call.  (One thread per output would walk up to 512 slots one
// load behind the other: 0.2 ms.)
constexpr int kFinOut = 16;
__global__ __launch_bounds__(kThreads) void dwln_bwd_finalize_kernel(const double* __restrict__ part_a, int sa,
                                                                      const double* __restrict__ part_b, int sb, float* __restrict__ dw,
                                                                      float* __restrict__ db, float* __restrict__ dln_w,
                                                                      float* __restrict__ dln_b, int C) {
  __shared__ double sh[kThreads];
  const int ex = threadIdx.x % kFinOut, ty = threadIdx.x / kFinOut;
  const int e = blockIdx.x * kFinOut + ex;
  const double* src = nullptr;
  float* dst = nullptr;
  size_t stride = 0;
  int n = 0;
  if (e < 49 * C) {
    const int tap = e / C, c = e - tap * C;
    if (dw) src = part_b + e, stride = (size_t)49 * C, n = sb, dst = dw + (size_t)c * 49 + tap;
  } else if (e < 52 * C) {
    const int v = (e - 49 * C) / C, c = e - (49 + v) * C;
    float* out = v == 0 ? dln_b : v == 1 ? dln_w : db;
    if (out) src = part_a + (size_t)v * C + c, stride = (size_t)3 * C, n = sa, dst = out + c;
  }
  double s = 0.0;
#pragma unroll 4
  for (int k = ty; k < n; k += kThreads / kFinOut) s += src[(size_t)k * stride];
  sh[threadIdx.x] = s;
  __syncthreads();
  if (ty == 0 && dst) {
    double t = 0.0;
    for (int j = 0; j < kThreads / kFinOut; ++j) t += sh[j * kFinOut + ex];
    *dst = (float)t;
  }
}

struct Layout {
  size_t du_bytes, a_bytes, b_bytes;
  int sa, sb;
  size_t total() const { return du_bytes + a_bytes + b_bytes; }
};
Layout layout_of(int N, int H, int W, int C) {
  const int Q = C / 4;
  Layout l;
  l.sa = slots_a(N, H, W, Q);
  l.sb = slots_b(N, H, W, Q);
  l.du_bytes = (size_t)N * H * W * C * sizeof(float);
  l.a_bytes = (size_t)l.sa * 3 * C * sizeof(double);
  l.b_bytes = (size_t)l.sb * 49 * C * sizeof(double);
  return l;
}
bool shape_ok(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 4) return false;
  const int Q = C / 4;
  return Q <= 256 && (Q & (Q - 1)) == 0;
}

}  // namespace

extern "C" {

size_t gdrnpp_dwconv7x7_ln_backward_workspace_bytes(int N, int H, int W, int C) {
  return shape_ok(N, H, W, C) ? layout_of(N, H, W, C).total() : 0;
}

int gdrnpp_dwconv7x7_ln_backward(const float* x, const float* w49c, const float* bias, const float* ln_w, const float* grad_y, float* dx,
                                 float* dw, float* db, float* dln_w, float* dln_b, int N, int H, int W, int C, float eps, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  GDRNPP_REQUIRE(x && w49c && bias && ln_w && grad_y && workspace, GDRNPP_EINVAL, "gdrnpp_dwconv7x7_ln_backward: null pointer");
  GDRNPP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0, GDRNPP_EINVAL, "gdrnpp_dwconv7x7_ln_backward: N=%d H=%d W=%d C=%d", N, H, W, C);
  GDRNPP_REQUIRE(shape_ok(N, H, W, C), GDRNPP_ELIMIT,
                 "gdrnpp_dwconv7x7_ln_backward: C=%d must be a multiple of 4 with a power-of-two quad count <= 256", C);
  GDRNPP_REQUIRE(eps >= 0.f, GDRNPP_EINVAL, "gdrnpp_dwconv7x7_ln_backward: eps=%g", (double)eps);
  GDRNPP_REQUIRE(dx || dw || db || dln_w || dln_b, GDRNPP_EINVAL, "gdrnpp_dwconv7x7_ln_backward: no gradient asked for");
  const int Q = C / 4;
  const long groups_x = tile_groups(N, H, W, Q, kTW);
  GDRNPP_REQUIRE(groups_x < (1l << 31), GDRNPP_ELIMIT, "gdrnpp_dwconv7x7_ln_backward: grid too large");
  const Layout l = layout_of(N, H, W, C);
  GDRNPP_REQUIRE(workspace_bytes >= l.total(), GDRNPP_EINVAL, "gdrnpp_dwconv7x7_ln_backward: workspace of %zu bytes, %zu needed", workspace_bytes,
                 l.total());
  GDRNPP_REQUIRE(((uintptr_t)workspace & 15) == 0, GDRNPP_EINVAL, "gdrnpp_dwconv7x7_ln_backward: workspace must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  float* du = (float*)workspace;
  double* part_a = (double*)((char*)workspace + l.du_bytes);
  double* part_b = (double*)((char*)workspace + l.du_bytes + l.a_bytes);
  hipLaunchKernelGGL(dwln_bwd_du_kernel, dim3((unsigned)l.sa), dim3(kThreads), 0, st, x, w49c, bias, ln_w, grad_y, du, part_a, N, H, W, C, eps);
  if (dx) hipLaunchKernelGGL(dwln_bwd_dx_kernel, dim3((unsigned)groups_x), dim3(kThreads), 0, st, du, w49c, dx, N, H, W, C);
  if (dw) hipLaunchKernelGGL(dwln_bwd_dw_kernel, dim3((unsigned)l.sb, 7), dim3(kThreads), 0, st, du, x, part_b, N, H, W, C);
  if (dw || db || dln_w || dln_b)
    hipLaunchKernelGGL(dwln_bwd_finalize_kernel, dim3((unsigned)((52 * C + kFinOut - 1) / kFinOut)), dim3(kThreads), 0, st, part_a, l.sa, part_b,
                       l.sb, dw, db, dln_w, dln_b, C);
  return gdrnpp::check_launch("gdrnpp_dwconv7x7_ln_backward");
}

}  // extern "C"
