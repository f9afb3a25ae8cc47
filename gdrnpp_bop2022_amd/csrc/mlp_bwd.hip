// Backward of the ConvNeXt MLP tail  y = s + gamma (.) (gelu(x W1^T + b1) W2^T + b2)  on gfx950: the kernels the split GEMMs do not
// have.  DESIGN.md "ConvNeXt MLP backward" has the scheme, the measured resources and the times.
//
//   x [M,C]   pre = x W1^T + b1 [M,H]   h = gelu(pre)   z = h W2^T + b2   y = s + gamma (.) z   g = dL/dy          (H = 4C)
//   ds = g    dh = g (diag(gamma) W2)    dpre = dh (.) gelu'(pre)    db1 = colsum(dpre)    dx = dpre W1    dW1 = dpre^T x
//   G = g^T h    dW2 = diag(gamma) G    sg = colsum(g)    db2 = gamma (.) sg    dgamma = rowsum(W2 (.) G) + b2 (.) sg
//
// The forward-shaped products (fc1, fc2, dh, dx) run on gdrnpp_linear_f32_split as it is up to a depth of 256 and on gemm_rows beyond
// (hip_lib/gemm.py has the rule and the measurement behind it); this file holds
//   gemm_rows  out = epilogue(A Bop) on the exact-f32 matrix instruction with gemm_tn's sums, for the deep products;
//   pack_t     pack_weight_bf16x3 of (diag(row_scale) W)^T read straight from W: the operand of those two products;
//   gelu       h = gelu(pre) with the epilogue's own function (common.hpp), for the forward under autograd;
//   act        one pass over [M,H]: dpre = dh gelu'(pre) in place, h recomputed for G, fp64 column partials of dpre;
//   colsum     fp64 column sums of a matrix through fixed partial slots (sg, and the partials of act);
//   gemm_tn    G[N1,N2] = sum_m A[m,N1] B[m,N2] on the exact-f32 matrix instruction, the weight-gradient product.
// No floating-point atomics: every sum over rows goes to workspace slots whose count depends on the shape alone and is added in
// slot order in fp64, so two calls give equal bits.
#include "exact_gemm_device.hpp"
#include "gemm_split.hpp"
#include <algorithm>
#include <cstdint>

namespace {

using namespace gdrnpp::exactgemm;
using gdrnpp::aligned16;
using gdrnpp::gelu_erf;
using gdrnpp::gelu_grad;

// ---- pack_t ---------------------------------------------------------------------------------------------------------------------
// W f32[R][K] -> the packed image [K/128][R/16][3][2][128][8] of T = (diag(s) W)^T, T[n][r] = s[r] W[r][n] (one fp32 product, as
// the ATen multiply it replaces).  One thread per (8 consecutive r, n), n fastest: a wave reads 64 consecutive floats of a row of W
// eight times and writes 64 consecutive 16-byte slots three times.
__global__ __launch_bounds__(kThreads) void pack_weight_t_kernel(const float* __restrict__ W, const float* __restrict__ s,
                                                                  uint4* __restrict__ packed, int R, int K) {
  using namespace gdrnpp::splitgemm;
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)K * (R / 8)) return;
  const int n = (int)(i % K), kb_g = (int)(i / K);
  float v[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int r = kb_g * 8 + j;
    const float w = W[(size_t)r * K + n];
    v[j] = s ? w * s[r] : w;
  }
  const Split3 p0 = split_pair(v[0], v[1]), p1 = split_pair(v[2], v[3]), p2 = split_pair(v[4], v[5]), p3 = split_pair(v[6], v[7]);
  const int tn = n / BN, row = n % BN, tk = kb_g / KB, kb = kb_g % KB;
  uint4* img = packed + ((size_t)tn * (R / BK) + tk) * W_TILE_SLOTS;
  img[(0 * KB + kb) * BN + row] = make_uint4(p0.h, p1.h, p2.h, p3.h);
  img[(1 * KB + kb) * BN + row] = make_uint4(p0.m, p1.m, p2.m, p3.m);
  img[(2 * KB + kb) * BN + row] = make_uint4(p0.l, p1.l, p2.l, p3.l);
}

// ---- gelu -----------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kThreads) void gelu_kernel(const float* __restrict__ pre, float* __restrict__ h, size_t n4) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < n4; i += (size_t)gridDim.x * kThreads) {
    const f4 p = ld4v(pre + 4 * i);
    st4v(h + 4 * i, f4{gelu_erf(p.x), gelu_erf(p.y), gelu_erf(p.z), gelu_erf(p.w)});
  }
}

// ---- act / colsum ---------------------------------------------------------------------------------------------------------------
// gelu_grad (common.hpp) runs on ocml's erff / expf: the pass moves 16 or 20 bytes per element, the ~60 instructions hide behind
// them.
// A workgroup = 4 waves; lane l of every wave owns column quad 64 blockIdx.y + l, wave w the rows r0 + w, r0 + w + 4, ... of slot
// blockIdx.x; a wave reads 1 KB of a row at a time.  Sums in fp64 per thread, the four waves added in wave order, one partial
// [cols] per slot.
constexpr int kColSlots = 256;    // most slots (= partial rows)
constexpr int kColSlotRows = 64;  // fewest rows a slot is made for
struct ColPlan { int slots; long rows; };
__host__ __device__ inline ColPlan col_plan(long M) {
  ColPlan p;
  const long want = (M + kColSlotRows - 1) / kColSlotRows;
  p.slots = (int)(want < kColSlots ? want : kColSlots);
  p.rows = (M + p.slots - 1) / p.slots;
  p.slots = (int)((M + p.rows - 1) / p.rows);
  return p;
}

// ACT: x = pre, io = dh in / dpre out, h (optional) = gelu(pre) out; the column sums are those of dpre as stored.  Else: of x.
template <bool ACT>
__global__ __launch_bounds__(kThreads) void colsum_kernel(const float* __restrict__ x, float* __restrict__ io, float* __restrict__ h,
                                                           double* __restrict__ part, long M, int cols, long rows_per_slot) {
  __shared__ double sh[3 * 64 * 4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q = blockIdx.y * 64 + lane;
  const bool live = 4 * q < cols;
  const long r0 = (long)blockIdx.x * rows_per_slot, r1 = r0 + rows_per_slot < M ? r0 + rows_per_slot : M;
  double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
  if (live) {
#pragma unroll 2
    for (long r = r0 + wave; r < r1; r += 4) {
      const size_t at = (size_t)r * cols + 4 * q;
      f4 v = ld4v(x + at);
      if (ACT) {
        const f4 d = ld4v(io + at);
        if (h) st4v(h + at, f4{gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w)});
        v = f4{d.x * gelu_grad(v.x), d.y * gelu_grad(v.y), d.z * gelu_grad(v.z), d.w * gelu_grad(v.w)};
        st4v(io + at, v);
      }
      a0 += (double)v.x, a1 += (double)v.y, a2 += (double)v.z, a3 += (double)v.w;
    }
  }
  if (wave > 0) {
    double* o = sh + ((wave - 1) * 64 + lane) * 4;
    o[0] = a0, o[1] = a1, o[2] = a2, o[3] = a3;
  }
  __syncthreads();
  if (wave == 0 && live) {
    for (int w = 0; w < 3; ++w) {
      const double* o = sh + (w * 64 + lane) * 4;
      a0 += o[0], a1 += o[1], a2 += o[2], a3 += o[3];
    }
    double* out = part + (size_t)blockIdx.x * cols + 4 * q;
    out[0] = a0, out[1] = a1, out[2] = a2, out[3] = a3;
  }
}

// column c: the slots in index order -> sum64[c] (optional), sum32[c] = fl(scale[c] sum) (optional, scale optional)
__global__ __launch_bounds__(kThreads) void colsum_finalize_kernel(const double* __restrict__ part, int slots, int cols,
                                                                    const float* __restrict__ scale, double* __restrict__ sum64,
                                                                    float* __restrict__ sum32) {
  const int c = blockIdx.x * kThreads + threadIdx.x;
  if (c >= cols) return;
  double s = 0.0;
#pragma unroll 4
  for (int k = 0; k < slots; ++k) s += part[(size_t)k * cols + c];
  if (sum64) sum64[c] = s;
  if (sum32) sum32[c] = (float)(scale ? (double)scale[c] * s : s);
}

int launch_colsum(bool act, const float* x, float* io, float* h, const float* scale, double* sum64, float* sum32, long M, int cols,
                  void* workspace, hipStream_t st) {
  const ColPlan p = col_plan(M);
  double* part = (double*)workspace;
  const dim3 grid((unsigned)p.slots, (unsigned)((cols / 4 + 63) / 64));
  if (act)
    hipLaunchKernelGGL(colsum_kernel<true>, grid, dim3(kThreads), 0, st, x, io, h, part, M, cols, p.rows);
  else
    hipLaunchKernelGGL(colsum_kernel<false>, grid, dim3(kThreads), 0, st, x, io, h, part, M, cols, p.rows);
  if (sum64 || sum32)
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3((unsigned)((cols + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, part, p.slots, cols,
                       scale, sum64, sum32);
  return 0;
}

// ---- gemm_tn --------------------------------------------------------------------------------------------------------------------
// G[n1][n2] = sum_m A[m][n1] B[m][n2]: the scheme of exact_gemm_device.hpp as it stands, both operands staged as they lie.  Slot y of
// the grid owns rows [y R, (y + 1) R), R a multiple of 512 and the slot count at most min(64, what brings the grid to 512
// workgroups), rounded up; each slot's fp64 tile goes to the workspace.
constexpr int kTnSlotRows = 512, kTnSlotCap = 64, kTnGrid = 512;
inline SlotPlan tn_plan(long M, int N1, int N2) {
  return row_slot_plan(M, (long)(N1 / 128) * (N2 / 128), kTnSlotRows, kTnSlotCap, kTnGrid, true);
}

__global__ __launch_bounds__(kThreads) void gemm_tn_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                            double* __restrict__ part, int M, int N1, int N2, long rows_per_slot) {
  __shared__ float sA[kBK * kPitch];
  __shared__ float sB[kBK * kPitch];
  const int tiles2 = N2 / 128;
  const int n1_0 = ((int)blockIdx.x / tiles2) * 128, n2_0 = ((int)blockIdx.x % tiles2) * 128;
  const long r0 = (long)blockIdx.y * rows_per_slot, r1 = r0 + rows_per_slot < M ? r0 + rows_per_slot : M;
  const float* ap = A + (size_t)n1_0 + stage_col();
  const float* bp = B + (size_t)n2_0 + stage_col();
  f4 ra[4], rb[4];
  auto fetch = [&](long r) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const long m = r + stage_row() + 8 * p;
      const bool in = m < r1;
      ra[p] = in ? ld4v(ap + (size_t)m * N1) : f4{0.f, 0.f, 0.f, 0.f};
      rb[p] = in ? ld4v(bp + (size_t)m * N2) : f4{0.f, 0.f, 0.f, 0.f};
    }
  };
  Tile t;
  t.clear();
  if (r0 < r1) fetch(r0);
  k_loop<kPitch, kPitch>(t, sA, sB, r0, r1, kBK, fetch, [&] { store_stage<false, false>(sA, sB, ra, rb); });
  double* out = part + (size_t)blockIdx.y * N1 * N2;
  for_each_d(n1_0, n2_0, [=, &t](int i, int j, int e, int n1, int n2) { out[(size_t)n1 * N2 + n2] = t.carry[i][j][e]; });
}

// One workgroup per row c of G; thread t takes the columns t, t + 256, ...: the slots in index order in fp64, then
//   G[c][k] = fl(row_scale[c] sum)  (row_scale optional, G optional)      and, with W:
//   drow[c] = fl(sum_k W[c][k] sum[c][k] + b[c] sg[c])  from the fp64 sums, before G is rounded — per thread in column order, the
//   256 threads by a fixed tree.
__global__ __launch_bounds__(kThreads) void gemm_tn_finalize_kernel(const double* __restrict__ part, int slots, int N1, int N2,
                                                                     const float* __restrict__ row_scale, float* __restrict__ G,
                                                                     const float* __restrict__ W, const float* __restrict__ b,
                                                                     const double* __restrict__ sg, float* __restrict__ drow) {
  __shared__ double sh[kThreads];
  const int c = blockIdx.x;
  const size_t plane = (size_t)N1 * N2;
  const double scale = row_scale ? (double)row_scale[c] : 1.0;
  double dot = 0.0;
  for (int k = threadIdx.x; k < N2; k += kThreads) {
    const double* src = part + (size_t)c * N2 + k;
    double s = 0.0;
#pragma unroll 8
    for (int y = 0; y < slots; ++y) s += src[(size_t)y * plane];
    if (W) dot += (double)W[(size_t)c * N2 + k] * s;
    if (G) G[(size_t)c * N2 + k] = (float)(row_scale ? scale * s : s);
  }
  if (!drow) return;
  sh[threadIdx.x] = dot;
  __syncthreads();
  for (int off = kThreads / 2; off >= 1; off >>= 1) {
    if ((int)threadIdx.x < off) sh[threadIdx.x] += sh[threadIdx.x + off];
    __syncthreads();
  }
  if (threadIdx.x == 0) drow[c] = (float)(sh[0] + (double)b[c] * sg[c]);
}

// ---- gemm_rows ------------------------------------------------------------------------------------------------------------------
// Out[m][n] = epilogue(sum_k A[m][k] Bop[k][n]) for the DEEP forward-shaped products of the tail (fc2, dx; from K = 512 on), on the same
// instruction with the same fp64 carries as gemm_tn: measured, gdrnpp_linear_f32_split's fp32 accumulation of six partial products
// per k-tile is 1.4x the error of a CPU sgemm at K = 256 and 2.5 - 3.4x at K = 1024, beyond the factor 2 the tests' bar allows.
//   A     [M,K] row-major: k is contiguous, so a stage [128 rows][32 k] is stored transposed (exact_gemm_device.hpp); rows at and
//         beyond M are zero-filled, never read, and their results not stored.
//   B     B_NK: the weight as nn.Linear holds it, [N,K], staged transposed the same way;  else [K,N] row-major, staged as it lies,
//         times row_scale[k] (optional; one fp32 product, as pack_weight_t_kernel does).
//   sums  fp32 chains of 128, fp64 carries, then in fp64  v = sum + bias[n];  out = fl(v)  or, with gamma,  out = fl(resid[m][n] +
//         gamma[n] v) — one rounding.  With one depth slot the workgroup does that itself and there is no workspace.
//   depth a launch with fewer than 256 output tiles (small batches in the deep stages) cuts K into slots of a multiple of 128 until the
//         grid reaches 256 workgroups (rows_plan: from the shape alone); slot y writes its fp64 tile to part[y][M][N] and
//         gemm_rows_finalize_kernel adds the slots in index order and applies the epilogue.
constexpr int kRowsGrid = 256;
struct RowsPlan { int slots, depth; };
inline RowsPlan rows_plan(int M, int N, int K) {
  const long tiles = (long)((M + 127) / 128) * (N / 128);
  const int chunks = (K + 127) / 128;
  const int want = (int)std::min<long>(chunks, std::max<long>(1, (kRowsGrid + tiles - 1) / tiles));
  const int per = (chunks + want - 1) / want;
  return RowsPlan{(chunks + per - 1) / per, per * 128};
}

__device__ __forceinline__ float rows_epilogue(double sum, size_t at, int n, const float* __restrict__ bias, const float* __restrict__ gamma,
                                               const float* __restrict__ resid) {
  const double v = sum + (bias ? (double)bias[n] : 0.0);
  return (float)(gamma ? (double)resid[at] + (double)gamma[n] * v : v);
}

__global__ __launch_bounds__(kThreads) void gemm_rows_finalize_kernel(const double* __restrict__ part, int slots, const float* __restrict__ bias,
                                                                       const float* __restrict__ gamma, const float* __restrict__ resid,
                                                                       float* __restrict__ out, size_t mn, int N) {
  for (size_t i = (size_t)blockIdx.x * kThreads + threadIdx.x; i < mn; i += (size_t)gridDim.x * kThreads) {
    double s = 0.0;
    for (int y = 0; y < slots; ++y) s += part[(size_t)y * mn + i];
    out[i] = rows_epilogue(s, i, (int)(i % N), bias, gamma, resid);
  }
}

template <bool B_NK>
__global__ __launch_bounds__(kThreads) void gemm_rows_kernel(const float* __restrict__ A, const float* __restrict__ B,
                                                              const float* __restrict__ row_scale, const float* __restrict__ bias,
                                                              const float* __restrict__ gamma, const float* __restrict__ resid,
                                                              float* __restrict__ out, double* __restrict__ part, int M, int N, int K,
                                                              int slot_depth) {
  constexpr int PB = B_NK ? kPitchT : kPitch;
  __shared__ float sA[kBK * kPitchT];
  __shared__ float sB[kBK * PB];
  const int tiles_n = N / 128;
  const int m0 = ((int)blockIdx.x / tiles_n) * 128, n0 = ((int)blockIdx.x % tiles_n) * 128;
  f4 ra[4], rb[4];
  auto fetch = [&](int k) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const int m = m0 + stage_row_t() + 32 * p;
      ra[p] = m < M ? ld4v(A + (size_t)m * K + k + stage_k_t()) : f4{0.f, 0.f, 0.f, 0.f};
      if (B_NK) {
        rb[p] = ld4v(B + (size_t)(n0 + stage_row_t() + 32 * p) * K + k + stage_k_t());
      } else {
        const int kk = k + stage_row() + 8 * p;
        rb[p] = ld4v(B + (size_t)kk * N + n0 + stage_col());
        if (row_scale) rb[p] = rb[p] * row_scale[kk];
      }
    }
  };
  Tile t;
  t.clear();
  const int k0 = (int)blockIdx.y * slot_depth, k1 = k0 + slot_depth < K ? k0 + slot_depth : K;  // k0 < K: rows_plan leaves no empty slot
  fetch(k0);
  k_loop<kPitchT, PB>(t, sA, sB, k0, k1, kBK, fetch, [&] { store_stage<true, B_NK>(sA, sB, ra, rb); });
  double* slot = part + (size_t)blockIdx.y * M * N;
  for_each_d(m0, n0, [=, &t](int i, int j, int e, int m, int n) {
    if (m >= M) return;
    const size_t at = (size_t)m * N + n;
    if (part)
      slot[at] = t.carry[i][j][e];
    else
      out[at] = rows_epilogue(t.carry[i][j][e], at, n, bias, gamma, resid);
  });
}
}  // namespace

extern "C" {

int gdrnpp_pack_weight_bf16x3_t(const float* W, const float* row_scale, void* packed, int R, int K, void* stream) {
  GDRNPP_REQUIRE(W && packed, GDRNPP_EINVAL, "gdrnpp_pack_weight_bf16x3_t: null pointer");
  GDRNPP_REQUIRE(R > 0 && K > 0 && K % gdrnpp::splitgemm::BN == 0 && R % 32 == 0, GDRNPP_ELIMIT,
                 "gdrnpp_pack_weight_bf16x3_t: W is [R=%d, K=%d]; K and R must be multiples of %d/32", R, K, gdrnpp::splitgemm::BN);
  const long threads = (long)K * (R / 8);
  hipLaunchKernelGGL(pack_weight_t_kernel, dim3((unsigned)((threads + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, W,
                     row_scale, (uint4*)packed, R, K);
  return gdrnpp::check_launch("gdrnpp_pack_weight_bf16x3_t");
}

int gdrnpp_gelu_f32(const float* pre, float* h, size_t n, void* stream) {
  GDRNPP_REQUIRE(pre && h, GDRNPP_EINVAL, "gdrnpp_gelu_f32: null pointer");
  GDRNPP_REQUIRE(n > 0 && n % 4 == 0 && aligned16(pre) && aligned16(h), GDRNPP_EINVAL,
                 "gdrnpp_gelu_f32: n=%zu must be a positive multiple of 4, the tensors 16-byte aligned", n);
  const size_t n4 = n / 4;
  const unsigned blocks = (unsigned)std::min<size_t>((n4 + kThreads - 1) / kThreads, 1u << 16);
  hipLaunchKernelGGL(gelu_kernel, dim3(blocks), dim3(kThreads), 0, (hipStream_t)stream, pre, h, n4);
  return gdrnpp::check_launch("gdrnpp_gelu_f32");
}

size_t gdrnpp_colsum_workspace_bytes(long M, int cols) {
  if (M <= 0 || cols <= 0 || cols % 4) return 0;
  return (size_t)col_plan(M).slots * cols * sizeof(double);
}

int gdrnpp_colsum_f32(const float* x, const float* scale, double* sum64, float* sum32, long M, int cols, void* workspace,
                      size_t workspace_bytes, void* stream) {
  GDRNPP_REQUIRE(x && workspace && (sum64 || sum32), GDRNPP_EINVAL, "gdrnpp_colsum_f32: null pointer");
  GDRNPP_REQUIRE(M > 0 && cols > 0 && cols % 4 == 0 && aligned16(x), GDRNPP_EINVAL,
                 "gdrnpp_colsum_f32: M=%ld cols=%d (a multiple of 4), x 16-byte aligned", M, cols);
  GDRNPP_REQUIRE(workspace_bytes >= gdrnpp_colsum_workspace_bytes(M, cols) && aligned16(workspace), GDRNPP_EINVAL,
                 "gdrnpp_colsum_f32: workspace of %zu bytes, %zu needed, 16-byte aligned", workspace_bytes, gdrnpp_colsum_workspace_bytes(M, cols));
  launch_colsum(false, x, nullptr, nullptr, scale, sum64, sum32, M, cols, workspace, (hipStream_t)stream);
  return gdrnpp::check_launch("gdrnpp_colsum_f32");
}

int gdrnpp_mlp_bwd_act(const float* pre, float* dh_dpre, float* h, float* db1, long M, int cols, void* workspace, size_t workspace_bytes,
                       void* stream) {
  GDRNPP_REQUIRE(pre && dh_dpre && workspace, GDRNPP_EINVAL, "gdrnpp_mlp_bwd_act: null pointer");
  GDRNPP_REQUIRE(M > 0 && cols > 0 && cols % 4 == 0 && aligned16(pre) && aligned16(dh_dpre) && aligned16(h), GDRNPP_EINVAL,
                 "gdrnpp_mlp_bwd_act: M=%ld cols=%d (a multiple of 4), the tensors 16-byte aligned", M, cols);
  GDRNPP_REQUIRE(workspace_bytes >= gdrnpp_colsum_workspace_bytes(M, cols) && aligned16(workspace), GDRNPP_EINVAL,
                 "gdrnpp_mlp_bwd_act: workspace of %zu bytes, %zu needed, 16-byte aligned", workspace_bytes, gdrnpp_colsum_workspace_bytes(M, cols));
  launch_colsum(true, pre, dh_dpre, h, nullptr, nullptr, db1, M, cols, workspace, (hipStream_t)stream);
  return gdrnpp::check_launch("gdrnpp_mlp_bwd_act");
}

size_t gdrnpp_linear_f32_exact_workspace_bytes(int M, int N, int K) {
  if (M <= 0 || N <= 0 || K <= 0 || N % 128 || K % 32) return 0;
  const RowsPlan p = rows_plan(M, N, K);
  return p.slots > 1 ? (size_t)p.slots * M * N * sizeof(double) : 0;
}

int gdrnpp_linear_f32_exact(const float* A, const float* B, int b_is_nk, const float* row_scale, const float* bias, const float* gamma,
                            const float* resid, float* out, int M, int N, int K, void* workspace, size_t workspace_bytes, void* stream) {
  GDRNPP_REQUIRE(A && B && out, GDRNPP_EINVAL, "gdrnpp_linear_f32_exact: null pointer");
  GDRNPP_REQUIRE(M > 0 && N > 0 && K > 0, GDRNPP_EINVAL, "gdrnpp_linear_f32_exact: M=%d N=%d K=%d", M, N, K);
  GDRNPP_REQUIRE(N % 128 == 0 && K % 32 == 0 && ((long)(M + 127) / 128) * (N / 128) < (1l << 31), GDRNPP_ELIMIT,
                 "gdrnpp_linear_f32_exact: N=%d K=%d must be multiples of 128/32 (M=%d is free)", N, K, M);
  GDRNPP_REQUIRE(!gamma == !resid, GDRNPP_EINVAL, "gdrnpp_linear_f32_exact: gamma and resid come together");
  GDRNPP_REQUIRE(!(b_is_nk && row_scale), GDRNPP_EINVAL, "gdrnpp_linear_f32_exact: row_scale goes with a [K,N] operand");
  GDRNPP_REQUIRE(aligned16(A) && aligned16(B), GDRNPP_EINVAL, "gdrnpp_linear_f32_exact: A and B must be 16-byte aligned");
  const RowsPlan p = rows_plan(M, N, K);
  const size_t need = gdrnpp_linear_f32_exact_workspace_bytes(M, N, K);
  GDRNPP_REQUIRE(need == 0 || (workspace && workspace_bytes >= need && aligned16(workspace)), GDRNPP_EINVAL,
                 "gdrnpp_linear_f32_exact: workspace of %zu bytes, %zu needed, 16-byte aligned", workspace_bytes, need);
  double* part = p.slots > 1 ? (double*)workspace : nullptr;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(((M + 127) / 128) * (N / 128)), (unsigned)p.slots);
  if (b_is_nk)
    hipLaunchKernelGGL(gemm_rows_kernel<true>, grid, dim3(kThreads), 0, st, A, B, row_scale, bias, gamma, resid, out, part, M, N, K, p.depth);
  else
    hipLaunchKernelGGL(gemm_rows_kernel<false>, grid, dim3(kThreads), 0, st, A, B, row_scale, bias, gamma, resid, out, part, M, N, K, p.depth);
  if (part) {
    const size_t mn = (size_t)M * N;
    const unsigned blocks = (unsigned)std::min<size_t>((mn + kThreads - 1) / kThreads, 1u << 16);
    hipLaunchKernelGGL(gemm_rows_finalize_kernel, dim3(blocks), dim3(kThreads), 0, st, part, p.slots, bias, gamma, resid, out, mn, N);
  }
  return gdrnpp::check_launch("gdrnpp_linear_f32_exact");
}

size_t gdrnpp_gemm_tn_f32_workspace_bytes(int M, int N1, int N2) {
  if (M <= 0 || N1 <= 0 || N2 <= 0 || N1 % 128 || N2 % 128) return 0;
  return (size_t)tn_plan(M, N1, N2).slots * N1 * N2 * sizeof(double);
}

int gdrnpp_gemm_tn_f32(const float* A, const float* B, float* G, int M, int N1, int N2, const float* row_scale, const float* W,
                       const float* b, const double* sg, float* drow, void* workspace, size_t workspace_bytes, void* stream) {
  GDRNPP_REQUIRE(A && B && workspace && (G || drow), GDRNPP_EINVAL, "gdrnpp_gemm_tn_f32: null pointer");
  GDRNPP_REQUIRE(M > 0 && N1 > 0 && N2 > 0, GDRNPP_EINVAL, "gdrnpp_gemm_tn_f32: M=%d N1=%d N2=%d", M, N1, N2);
  GDRNPP_REQUIRE(N1 % 128 == 0 && N2 % 128 == 0 && (long)(N1 / 128) * (N2 / 128) < (1l << 31) && N1 <= 65535 * 128, GDRNPP_ELIMIT,
                 "gdrnpp_gemm_tn_f32: N1=%d N2=%d must be multiples of 128", N1, N2);
  GDRNPP_REQUIRE(!drow || (W && b && sg), GDRNPP_EINVAL, "gdrnpp_gemm_tn_f32: drow needs W, b and sg");
  GDRNPP_REQUIRE(aligned16(A) && aligned16(B) && aligned16(workspace), GDRNPP_EINVAL, "gdrnpp_gemm_tn_f32: A, B and the workspace must be 16-byte aligned");
  const size_t need = gdrnpp_gemm_tn_f32_workspace_bytes(M, N1, N2);
  GDRNPP_REQUIRE(workspace_bytes >= need, GDRNPP_EINVAL, "gdrnpp_gemm_tn_f32: workspace of %zu bytes, %zu needed", workspace_bytes, need);
  const SlotPlan p = tn_plan(M, N1, N2);
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(gemm_tn_kernel, dim3((unsigned)((N1 / 128) * (N2 / 128)), (unsigned)p.slots), dim3(kThreads), 0, st, A, B, part, M, N1, N2,
                     p.rows_per_slot);
  hipLaunchKernelGGL(gemm_tn_finalize_kernel, dim3((unsigned)N1), dim3(kThreads), 0, st, part, p.slots, N1, N2, row_scale, G, drow ? W : nullptr,
                     b, sg, drow);
  return gdrnpp::check_launch("gdrnpp_gemm_tn_f32");
}

}  // extern "C"
