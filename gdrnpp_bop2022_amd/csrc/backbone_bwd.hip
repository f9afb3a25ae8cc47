// Training kernels of the ConvNeXt stem and downsample layers on gfx950: what the existing products (gdrnpp_linear_f32_exact,
// gdrnpp_gemm_tn_f32, gdrnpp_colsum_f32) leave over.  DESIGN.md "stem and downsample backward" has the traffic and the measured error.
//
//   stem        y = LN(u), u = b + conv4x4/4(x) (stem_conv_ln_kernel, net_kernels.hip, stays the forward).  One kernel recomputes u of a
//               pixel from x with the forward's fma chain in (ci, ky, kx) order, in fp64, forms the LayerNorm statistics and
//               du = r (gh - mean_c(gh) - xh mean_c(gh xh)) in fp64 and keeps du in LDS: 32 pixels of du [32][128] and of patches [32][48]
//               are one k-stage of dW = du^T patches on v_mfma_f32_32x32x2_f32 (wave w owns rows 32 w .. 32 w + 31 of dW, two 32-column
//               accumulators, the second half used).  gemm_tn's sums with a shorter chain: after every stage of 32 pixels the fp32 accumulators
//               go into fp64 carries (32 v_add_f64 per lane against 32 MFMAs; chains of 128 measured up to 0.80 of the tests' bar); a
//               workgroup is one slot of rows (stem_plan: the count from the shape alone), its fp64 tile and its db / dln_w / dln_b
//               partials go to the workspace, the finalize adds the slots in fp64 and rounds once.  x and grad_y are read once, du never
//               reaches HBM.  ln_w == NULL: du = grad_y (no LayerNorm, nothing recomputed).
//   downsample  LayerNorm2d + conv2x2/2 as a product over patch rows: layernorm_patch2x2 is layernorm_nhwc_kernel's body
//               (layernorm_rows.hpp) with the store address of the patch layout A [N H/2 W/2, 4 C], columns (ky, kx, ci); its backward
//               reads dA through the same map, recomputes the statistics from x in fp64 and writes dx NHWC and one [2][C] partial of
//               dln_b / dln_w per workgroup.
// No atomics, no scratch; two calls give equal bits.
#include "common.hpp"
#include "dpp_sum.hpp"
#include "layernorm_rows.hpp"
#include "ln_bwd_sums.hpp"
#include <algorithm>
#include <cstdint>

namespace {

using namespace gdrnpp::lnbwd;  // f4 / d4 helpers, kThreads, pixel_sums, block_partial
using gdrnpp::dpp::group_sum_dpp_f64;
using f32x16 = __attribute__((ext_vector_type(16))) float;

// ---- slot sums ------------------------------------------------------------------------------------------------------------------
// out[e] = fl(sum over the slots k of part[k stride + e]) for the outputs e of up to four segments (a segment whose dst is NULL is
// skipped).  16 threads per output take the slots k = ty, ty + 16, ... in index order, their 16 sums are added in ty order: fp64, the
// same order in every call (dwln_bwd_finalize_kernel's scheme).
constexpr int kFinOut = 16;
struct Seg {
  float* dst;
  int off, n;
};
struct Segs {
  Seg s[4];
};
__global__ __launch_bounds__(kThreads) void slot_sum_kernel(const double* __restrict__ part, int slots, size_t stride, Segs segs) {
  __shared__ double sh[kThreads];
  const int ex = threadIdx.x % kFinOut, ty = threadIdx.x / kFinOut;
  const int e = blockIdx.x * kFinOut + ex;
  float* dst = nullptr;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const Seg sg = segs.s[i];
    if (sg.dst && e >= sg.off && e < sg.off + sg.n) dst = sg.dst + (e - sg.off);
  }
  double s = 0.0;
  if (dst) {
#pragma unroll 4
    for (int k = ty; k < slots; k += kThreads / kFinOut) s += part[(size_t)k * stride + e];
  }
  sh[threadIdx.x] = s;
  __syncthreads();
  if (ty == 0 && dst) {
    double t = 0.0;
    for (int j = 0; j < kThreads / kFinOut; ++j) t += sh[j * kFinOut + ex];
    *dst = (float)t;
  }
}
void launch_slot_sum(const double* part, int slots, size_t stride, int total, const Segs& segs, hipStream_t st) {
  hipLaunchKernelGGL(slot_sum_kernel, dim3((unsigned)((total + kFinOut - 1) / kFinOut)), dim3(kThreads), 0, st, part, slots, stride, segs);
}

// ---- stem backward --------------------------------------------------------------------------------------------------------------
constexpr int kStemC = 128, kStemK = 48;
constexpr int kStemStage = 32;        // pixels of one k-stage = one fp32 chain: the accumulators go into the fp64 carries after every stage
constexpr int kStemSlotRows = 256;    // a slot's rows are a multiple of this
constexpr int kStemSlotCap = 256;     // most slots (= workgroups)
constexpr int kDuPitch = 132, kPatchPitch = 52;
constexpr int kStemPart = kStemC * kStemK + 3 * kStemC;  // doubles of one slot: dW [128][48], db, dln_w, dln_b

struct StemPlan {
  int slots;
  long rows;
};
inline StemPlan stem_plan(long M) {
  const long chunks = (M + kStemSlotRows - 1) / kStemSlotRows;
  const long per = (chunks + kStemSlotCap - 1) / kStemSlotCap;
  return StemPlan{(int)((chunks + per - 1) / per), per * kStemSlotRows};
}

template <bool LN, bool DW>
__global__ __launch_bounds__(kThreads) void stem_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, const float* __restrict__ ln_w,
                                                             const float* __restrict__ g, double* __restrict__ part, int N, int H, int W,
                                                             float eps, long rows_per_slot) {
  __shared__ float sDu[kStemStage * kDuPitch];
  __shared__ float sP[kStemStage * kPatchPitch];
  __shared__ double sRed[3 * 64 * 6];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int OH = H >> 2, OW = W >> 2;
  const long M = (long)N * OH * OW;
  const long r0 = (long)blockIdx.x * rows_per_slot, r1 = r0 + rows_per_slot < M ? r0 + rows_per_slot : M;
  float wr[2][kStemK];  // the lane's two output channels, as in the forward (unused, and removed, without LayerNorm)
  float b0 = 0.f, b1 = 0.f;
  double gam0 = 1.0, gam1 = 1.0;
  if (LN) {
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int k4 = 0; k4 < kStemK / 4; ++k4) {
        const f4 v = ld4v(w + (size_t)(2 * lane + c) * kStemK + 4 * k4);
        wr[c][4 * k4] = v.x, wr[c][4 * k4 + 1] = v.y, wr[c][4 * k4 + 2] = v.z, wr[c][4 * k4 + 3] = v.w;
      }
    if (bias) b0 = bias[2 * lane], b1 = bias[2 * lane + 1];
    gam0 = (double)ln_w[2 * lane], gam1 = (double)ln_w[2 * lane + 1];
  }
  f32x16 acc[2];
  double carry[2][16];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[j][e] = 0.f, carry[j][e] = 0.0;
  auto fold = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) carry[j][e] += (double)acc[j][e], acc[j][e] = 0.f;
  };
  double sums[6];  // db, dln_w, dln_b of the lane's two channels
#pragma unroll
  for (int k = 0; k < 6; ++k) sums[k] = 0.0;
  const double inv_c = 1.0 / (double)kStemC;
  for (long r = r0; r < r1; r += kStemStage) {
    __syncthreads();  // every wave has read the previous stage
    if (LN || DW) {
      // the 32 patches [ci][ky][kx]: 12 float4 each, consecutive threads consecutive pixels (consecutive 16 bytes of an image row)
      for (int i = tid; i < kStemStage * 12; i += kThreads) {
        const int pix = i & (kStemStage - 1), rr = i >> 5, ci = rr >> 2, ky = rr & 3;
        const long p = r + pix;
        f4 v = f4{0.f, 0.f, 0.f, 0.f};
        if (p < r1) {
          const long row = p / OW;  // n * OH + oy
          const int ox = (int)(p - row * OW), n = (int)(row / OH), oy = (int)(row - (long)n * OH);
          v = ld4v(x + (((size_t)n * 3 + ci) * H + 4 * oy + ky) * W + 4 * ox);
        }
        st4v(sP + pix * kPatchPitch + 4 * rr, v);
      }
      __syncthreads();
    }
#pragma unroll 2
    for (int j = 0; j < kStemStage / 4; ++j) {
      const int pix = wave * (kStemStage / 4) + j;
      const long p = r + pix;
      const bool in = p < r1;
      float2 gv = float2{0.f, 0.f};
      if (in) gv = *reinterpret_cast<const float2*>(g + (size_t)p * kStemC + 2 * lane);
      float du0 = gv.x, du1 = gv.y;
      if (LN) {
        // the forward's fma chain, (ci, ky, kx) order, in fp64 as the statistics and du are: du cancels (conv_tile_f64 of
        // dwconv_ln_bwd.hip says the same of its layer); measured, dln_w at 0.20 - 0.61 of the tests' bar with an fp32 u, 0.05 - 0.10 so
        double u0 = (double)b0, u1 = (double)b1;
#pragma unroll
        for (int rr = 0; rr < 12; ++rr) {
          const d4 v = to_d4(ld4v(sP + pix * kPatchPitch + 4 * rr));  // same address in every lane: LDS broadcast
          u0 = fma(v.x, (double)wr[0][4 * rr], u0), u1 = fma(v.x, (double)wr[1][4 * rr], u1);
          u0 = fma(v.y, (double)wr[0][4 * rr + 1], u0), u1 = fma(v.y, (double)wr[1][4 * rr + 1], u1);
          u0 = fma(v.z, (double)wr[0][4 * rr + 2], u0), u1 = fma(v.z, (double)wr[1][4 * rr + 2], u1);
          u0 = fma(v.w, (double)wr[0][4 * rr + 3], u0), u1 = fma(v.w, (double)wr[1][4 * rr + 3], u1);
        }
        const double mean = group_sum_dpp_f64(u0 + u1, 64, lane) * inv_c;
        u0 -= mean, u1 -= mean;
        const double rstd = 1.0 / sqrt(group_sum_dpp_f64(u0 * u0 + u1 * u1, 64, lane) * inv_c + (double)eps);
        u0 *= rstd, u1 *= rstd;  // xh
        const double g0 = (double)gv.x, g1 = (double)gv.y;
        const double gh0 = g0 * gam0, gh1 = g1 * gam1;
        const double m1 = group_sum_dpp_f64(gh0 + gh1, 64, lane) * inv_c;
        const double m2 = group_sum_dpp_f64(gh0 * u0 + gh1 * u1, 64, lane) * inv_c;
        const double d0 = in ? (gh0 - m1 - u0 * m2) * rstd : 0.0, d1 = in ? (gh1 - m1 - u1 * m2) * rstd : 0.0;
        du0 = (float)d0, du1 = (float)d1;
        if (in) {
          sums[0] += d0, sums[1] += d1;
          sums[2] += g0 * u0, sums[3] += g1 * u1;
          sums[4] += g0, sums[5] += g1;
        }
      } else {
        sums[0] += (double)du0, sums[1] += (double)du1;
      }
      if (DW) *reinterpret_cast<float2*>(sDu + pix * kDuPitch + 2 * lane) = float2{du0, du1};
    }
    if (DW) {
      __syncthreads();
      const float* la = sDu + (lane >> 5) * kDuPitch + wave * 32 + (lane & 31);
      const float* lb = sP + (lane >> 5) * kPatchPitch + (lane & 31);
      const bool hi = (lane & 31) < kStemK - 32;
#pragma unroll 4
      for (int s = 0; s < kStemStage / 2; ++s) {
        const float a = la[2 * s * kDuPitch];
        const float bl = lb[2 * s * kPatchPitch];
        const float bh = hi ? lb[2 * s * kPatchPitch + 32] : 0.f;
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bl, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bh, acc[1], 0, 0, 0);
      }
      fold();
    }
  }
  double* out = part + (size_t)blockIdx.x * kStemPart;
  if (DW) {
    // D: column = lane & 31 (patch column), row = (e & 3) + 8 (e >> 2) + 4 (lane >> 5) (output channel within the wave's 32)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int co = wave * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
        const int k = j * 32 + (lane & 31);
        if (k < kStemK) out[(size_t)co * kStemK + k] = carry[j][e];
      }
  }
  // the four waves' sums of a channel in wave order
  if (wave > 0) {
#pragma unroll
    for (int k = 0; k < 6; ++k) sRed[((wave - 1) * 64 + lane) * 6 + k] = sums[k];
  }
  __syncthreads();
  if (wave == 0) {
    for (int w2 = 0; w2 < 3; ++w2)
#pragma unroll
      for (int k = 0; k < 6; ++k) sums[k] += sRed[(w2 * 64 + lane) * 6 + k];
#pragma unroll
    for (int k = 0; k < 6; ++k) out[kStemC * kStemK + (k >> 1) * kStemC + 2 * lane + (k & 1)] = sums[k];
  }
}

bool stem_shape_ok(int N, int H, int W, int Cout) {
  return N > 0 && H > 0 && W > 0 && H % 4 == 0 && W % 16 == 0 && W <= 1024 && Cout == kStemC && (long)N * (H / 4) * (W / 4) < (1l << 31) - kStemStage;
}

// ---- LayerNorm in patch order ---------------------------------------------------------------------------------------------------
// pixel (n, y, x) of an NHWC tensor -> its place in A [N H/2 W/2, 4 C]: row = output pixel, column block (y & 1, x & 1)
__device__ __forceinline__ size_t patch_at(long pix, int H, int W, int C) {
  const long row = pix / W;  // n * H + y
  const int xx = (int)(pix - row * W);
  const long n = row / H;
  const int y = (int)(row - n * H);
  const long orow = (n * (H >> 1) + (y >> 1)) * (W >> 1) + (xx >> 1);
  return (size_t)orow * 4 * C + (size_t)(((y & 1) << 1) | (xx & 1)) * C;
}

// layernorm_nhwc_kernel's arithmetic (the shared body of layernorm_rows.hpp) with the store going to the patch layout; w == NULL: the
// copy alone
using gdrnpp::ln::LN_PIX;
// groups of (256 / Q pixels) x LN_PIX that the LayerNorm kernels walk
__host__ __device__ inline long ln_groups(long n_pix, int Q) {
  const long per = (long)(kThreads / Q) * LN_PIX;
  return (n_pix + per - 1) / per;
}
__global__ __launch_bounds__(256) void layernorm_patch_kernel(const float* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ b, float* __restrict__ A, long n_pix, int H, int W,
                                                              int C, float eps) {
  if (w) {
    gdrnpp::ln::layernorm_rows(x, w, b, n_pix, C, eps, [=](long pix) { return A + patch_at(pix, H, W, C); });
    return;
  }
  const int Q = C >> 2, ppb = kThreads / Q, q = threadIdx.x % Q, pl = threadIdx.x / Q;
  const long n_groups = ln_groups(n_pix, Q);
  for (long group = blockIdx.x; group < n_groups; group += gridDim.x) {
#pragma unroll
    for (int u = 0; u < LN_PIX; ++u) {
      const long pix = (group * LN_PIX + u) * ppb + pl;
      if (pix < n_pix) st4v(A + patch_at(pix, H, W, C) + 4 * q, ld4v(x + pix * C + 4 * q));
    }
  }
}

// Its adjoint: persistent workgroups, dln_b / dln_w of the pixels a workgroup walks in fp64 registers, ONE partial [2][C] each.
constexpr int kLnSlots = 512;
inline int ln_slots(long n_pix, int Q) { return (int)std::min<long>(ln_groups(n_pix, Q), kLnSlots); }

template <bool LN>
__global__ __launch_bounds__(kThreads) void layernorm_patch_bwd_kernel(const float* __restrict__ x, const float* __restrict__ ln_w,
                                                                        const float* __restrict__ dA, float* __restrict__ dx,
                                                                        double* __restrict__ part, long n_pix, int H, int W, int C, float eps) {
  __shared__ double red[2 * LN_PIX * 4];
  __shared__ double sh[LN ? kThreads * 8 : 1];
  const int Q = C >> 2, ppb = kThreads / Q, q = threadIdx.x % Q, pl = threadIdx.x / Q;
  const long n_groups = ln_groups(n_pix, Q);
  if (!LN) {
    for (long group = blockIdx.x; group < n_groups; group += gridDim.x) {
#pragma unroll
      for (int u = 0; u < LN_PIX; ++u) {
        const long pix = (group * LN_PIX + u) * ppb + pl;
        if (pix < n_pix) st4v(dx + pix * C + 4 * q, ld4v(dA + patch_at(pix, H, W, C) + 4 * q));
      }
    }
    return;
  }
  const d4 gam = to_d4(ld4v(ln_w + 4 * q));
  const double inv_c = 1.0 / (double)C;
  double acc[8];  // dln_b, dln_w of this thread's quad
#pragma unroll
  for (int k = 0; k < 8; ++k) acc[k] = 0.0;
  for (long group = blockIdx.x; group < n_groups; group += gridDim.x) {
    d4 v[LN_PIX], gv[LN_PIX], gh[LN_PIX];
    long pix[LN_PIX];
    double s[LN_PIX], rstd[LN_PIX], m[2 * LN_PIX];
#pragma unroll
    for (int u = 0; u < LN_PIX; ++u) {
      pix[u] = (group * LN_PIX + u) * ppb + pl;
      const bool in = pix[u] < n_pix;
      v[u] = in ? to_d4(ld4v(x + pix[u] * C + 4 * q)) : d4{0.0, 0.0, 0.0, 0.0};
      gv[u] = in ? to_d4(ld4v(dA + patch_at(pix[u], H, W, C) + 4 * q)) : d4{0.0, 0.0, 0.0, 0.0};
      s[u] = sum4(v[u]);
    }
    pixel_sums(s, Q, red);
#pragma unroll
    for (int u = 0; u < LN_PIX; ++u) {
      v[u] = v[u] - s[u] * inv_c;
      s[u] = sum4(v[u] * v[u]);
    }
    pixel_sums(s, Q, red);
#pragma unroll
    for (int u = 0; u < LN_PIX; ++u) {
      rstd[u] = 1.0 / sqrt(s[u] * inv_c + (double)eps);
      v[u] = v[u] * rstd[u];  // xh
      gh[u] = gv[u] * gam;
      m[u] = sum4(gh[u]);
      m[LN_PIX + u] = sum4(gh[u] * v[u]);
    }
    pixel_sums(m, Q, red);
#pragma unroll
    for (int u = 0; u < LN_PIX; ++u) {
      if (pix[u] >= n_pix) continue;
      if (dx) {
        const d4 d = (gh[u] - m[u] * inv_c - v[u] * (m[LN_PIX + u] * inv_c)) * rstd[u];
        st4v(dx + pix[u] * C + 4 * q, __builtin_convertvector(d, f4));
      }
      const d4 gx = gv[u] * v[u];
      acc[0] += gv[u].x, acc[1] += gv[u].y, acc[2] += gv[u].z, acc[3] += gv[u].w;
      acc[4] += gx.x, acc[5] += gx.y, acc[6] += gx.z, acc[7] += gx.w;
    }
  }
  block_partial(acc, sh, Q, C, part + (size_t)blockIdx.x * 2 * C);
}

// every pointer given (NULL = not given) on a 16-byte boundary: the kernels move float4s
template <class... P>
bool aligned16(const P*... p) {
  return ((... | (uintptr_t)p) & 15) == 0;
}

bool patch_shape_ok(int N, int H, int W, int C) {
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 128 || H % 2 || W % 2) return false;
  const int Q = C / 4;
  return Q <= 256 && (Q & (Q - 1)) == 0 && (long)N * H * W < (1l << 31) - 4096;
}

}  // namespace

extern "C" {

size_t gdrnpp_stem_conv4x4_ln_backward_workspace_bytes(int N, int H, int W, int Cout) {
  if (!stem_shape_ok(N, H, W, Cout)) return 0;
  return (size_t)stem_plan((long)N * (H / 4) * (W / 4)).slots * kStemPart * sizeof(double);
}

int gdrnpp_stem_conv4x4_ln_backward(const float* x_nchw, const float* weight, const float* bias, const float* ln_w, const float* grad_y,
                                    float* dw, float* db, float* dln_w, float* dln_b, int N, int H, int W, int Cout, float eps,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  const char* me = "gdrnpp_stem_conv4x4_ln_backward";
  GDRNPP_REQUIRE(x_nchw && grad_y && workspace && (weight || !ln_w), GDRNPP_EINVAL, "%s: null pointer", me);
  GDRNPP_REQUIRE(stem_shape_ok(N, H, W, Cout), GDRNPP_ELIMIT, "%s: N=%d H=%d W=%d Cout=%d (H %% 4, W %% 16, W <= 1024, Cout = %d)", me, N, H, W,
                 Cout, kStemC);
  GDRNPP_REQUIRE(eps >= 0.f, GDRNPP_EINVAL, "%s: eps=%g", me, (double)eps);
  GDRNPP_REQUIRE(dw || db || dln_w || dln_b, GDRNPP_EINVAL, "%s: no gradient asked for", me);
  GDRNPP_REQUIRE(ln_w || !(dln_w || dln_b), GDRNPP_EINVAL, "%s: dln_w / dln_b without a LayerNorm (ln_w is NULL)", me);
  const size_t need = gdrnpp_stem_conv4x4_ln_backward_workspace_bytes(N, H, W, Cout);
  GDRNPP_REQUIRE(workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0, GDRNPP_EINVAL, "%s: workspace of %zu bytes, %zu needed, 16-byte aligned",
                 me, workspace_bytes, need);
  GDRNPP_REQUIRE((((uintptr_t)x_nchw | (uintptr_t)grad_y | (uintptr_t)weight) & 15) == 0, GDRNPP_EINVAL, "%s: x, weight and grad_y must be 16-byte aligned", me);
  const StemPlan p = stem_plan((long)N * (H / 4) * (W / 4));
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  const dim3 grid((unsigned)p.slots), block(kThreads);
#define GDRNPP_STEM_BWD(LN, DW) \
  hipLaunchKernelGGL((stem_bwd_kernel<LN, DW>), grid, block, 0, st, x_nchw, weight, bias, ln_w, grad_y, part, N, H, W, eps, p.rows)
  if (ln_w) {
    if (dw) GDRNPP_STEM_BWD(true, true);
    else GDRNPP_STEM_BWD(true, false);
  } else {
    if (dw) GDRNPP_STEM_BWD(false, true);
    else GDRNPP_STEM_BWD(false, false);
  }
#undef GDRNPP_STEM_BWD
  Segs segs{};
  segs.s[0] = Seg{dw, 0, kStemC * kStemK};
  segs.s[1] = Seg{db, kStemC * kStemK, kStemC};
  segs.s[2] = Seg{dln_w, kStemC * kStemK + kStemC, kStemC};
  segs.s[3] = Seg{dln_b, kStemC * kStemK + 2 * kStemC, kStemC};
  launch_slot_sum(part, p.slots, kStemPart, kStemPart, segs, st);
  return gdrnpp::check_launch(me);
}

int gdrnpp_layernorm_patch2x2_nhwc(const float* x, const float* ln_w, const float* ln_b, float* A, int N, int H, int W, int C, float eps,
                                   void* stream) {
  const char* me = "gdrnpp_layernorm_patch2x2_nhwc";
  GDRNPP_REQUIRE(x && A && (!ln_w == !ln_b), GDRNPP_EINVAL, "%s: null pointer (ln_w and ln_b come together)", me);
  GDRNPP_REQUIRE(patch_shape_ok(N, H, W, C), GDRNPP_ELIMIT, "%s: N=%d H=%d W=%d C=%d (H, W even; C = 128, 256, 512 or 1024)", me, N, H, W, C);
  GDRNPP_REQUIRE(aligned16(x, ln_w, ln_b, A), GDRNPP_EINVAL, "%s: x, ln_w, ln_b and A must be 16-byte aligned", me);
  const long n_pix = (long)N * H * W;
  const long n_groups = ln_groups(n_pix, C / 4);
  const long blocks = n_groups < 256 * 16 ? n_groups : 256 * 16;
  hipLaunchKernelGGL(layernorm_patch_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, x, ln_w, ln_b, A, n_pix, H, W, C, eps);
  return gdrnpp::check_launch(me);
}

size_t gdrnpp_layernorm_patch2x2_backward_workspace_bytes(int N, int H, int W, int C) {
  if (!patch_shape_ok(N, H, W, C)) return 0;
  return (size_t)ln_slots((long)N * H * W, C / 4) * 2 * C * sizeof(double);
}

int gdrnpp_layernorm_patch2x2_backward(const float* x, const float* ln_w, const float* dA, float* dx, float* dln_w, float* dln_b, int N, int H,
                                       int W, int C, float eps, void* workspace, size_t workspace_bytes, void* stream) {
  const char* me = "gdrnpp_layernorm_patch2x2_backward";
  GDRNPP_REQUIRE(dA && (x || !ln_w), GDRNPP_EINVAL, "%s: null pointer", me);
  GDRNPP_REQUIRE(patch_shape_ok(N, H, W, C), GDRNPP_ELIMIT, "%s: N=%d H=%d W=%d C=%d (H, W even; C = 128, 256, 512 or 1024)", me, N, H, W, C);
  GDRNPP_REQUIRE(eps >= 0.f, GDRNPP_EINVAL, "%s: eps=%g", me, (double)eps);
  GDRNPP_REQUIRE(dx || dln_w || dln_b, GDRNPP_EINVAL, "%s: no gradient asked for", me);
  GDRNPP_REQUIRE(ln_w || (dx && !dln_w && !dln_b), GDRNPP_EINVAL, "%s: without a LayerNorm (ln_w is NULL) dx alone is formed", me);
  GDRNPP_REQUIRE(aligned16(x, ln_w, dA, dx), GDRNPP_EINVAL, "%s: x, ln_w, dA and dx must be 16-byte aligned", me);
  const long n_pix = (long)N * H * W;
  const int Q = C / 4;
  hipStream_t st = (hipStream_t)stream;
  if (!ln_w) {
    const long n_groups = ln_groups(n_pix, Q);
    const long blocks = n_groups < 256 * 16 ? n_groups : 256 * 16;
    hipLaunchKernelGGL(layernorm_patch_bwd_kernel<false>, dim3((unsigned)blocks), dim3(kThreads), 0, st, x, ln_w, dA, dx, (double*)nullptr, n_pix, H,
                       W, C, eps);
    return gdrnpp::check_launch(me);
  }
  const size_t need = gdrnpp_layernorm_patch2x2_backward_workspace_bytes(N, H, W, C);
  GDRNPP_REQUIRE(workspace && workspace_bytes >= need && ((uintptr_t)workspace & 15) == 0, GDRNPP_EINVAL,
                 "%s: workspace of %zu bytes, %zu needed, 16-byte aligned", me, workspace_bytes, need);
  const int slots = ln_slots(n_pix, Q);
  double* part = (double*)workspace;
  hipLaunchKernelGGL(layernorm_patch_bwd_kernel<true>, dim3((unsigned)slots), dim3(kThreads), 0, st, x, ln_w, dA, dx, part, n_pix, H, W, C, eps);
  if (dln_w || dln_b) {
    Segs segs{};
    segs.s[0] = Seg{dln_b, 0, C};
    segs.s[1] = Seg{dln_w, C, C};
    launch_slot_sum(part, slots, (size_t)2 * C, 2 * C, segs, st);
  }
  return gdrnpp::check_launch(me);
}

}  // extern "C"
