// Backward of the geometry head's tail on gfx950: the class-sliced 1x1 output layer (gdrnpp_linear_f32_split_grouped) and the
// kernel behind it (head_tail_kernel, net_kernels.hip).  DESIGN.md "Head tail backward" has the scheme, the resources and the times.
//
//   out [B hw][pitch] = feat [B hw][K] W[sel[b]]^T + bias[sel[b]]       channels [vis | full (double mask) | x | y | z | region 0..64]
//   pnp_in = [(xyz - 0.5) extent | coord2d | softmax(region[1..64]) | 0]      planes = vis, (full,) x, y, z
//
//   tail     d_out  = the adjoint of head_tail_kernel from (g_pnp_in, g_planes) + g_out, one pass;
//   dinput   dfeat[m] = d_out[m][0..n_out) W[sel[m / hw]]  on the exact-f32 matrix instruction, one fp32 chain in column order;
//   wgrad    per ROI r the fp64 tile d_out[r]^T feat[r] and the fp64 column sums of d_out[r] through fixed row slots (the staging
//            and sums of exact_gemm_device.hpp), then per class the ROIs in index order, the slots in index order, one rounding,
//            written through the row table into gradients shaped like the output layer's parameters.
// No floating-point atomics; slot counts depend on the shape alone: two calls give equal bits, and the rows of a class do not depend
// on which other classes the batch holds.
#include "exact_gemm_device.hpp"
#include <algorithm>
#include <cstdint>

namespace {

using namespace gdrnpp::exactgemm;
using gdrnpp::aligned16;

constexpr int kMaxOut = 72;      // deepest sliced layer: 2 masks + xyz + 65 regions = 70, stored in 72 columns

// ---- tail -----------------------------------------------------------------------------------------------------------------------
// One workgroup of 256 threads = 64 pixels, 4 lanes per pixel with 16 region logits each: head_tail_kernel's split, so that the
// softmax is rebuilt with its expression, its order and therefore its bits.  With p = softmax(region[1..64]) and g = g_pnp_in[5..68]:
//   d_region[j] = p_j (g_j - sum_i p_i g_i)   the sum per lane in channel order, the four lanes in lane order, all in fp64;
//   d_xyz[c]    = g_planes[kx + c] + g_pnp_in[c] extent[b][c];   d_vis, d_full = their planes;   d_region[0] = 0 (the background
//   logit is dropped by the forward);   coord2d has no gradient.
// g_out (what autograd delivers for the region view of out) is added in fp64 before the one rounding.  Columns n_out..pitch-1 of
// d_out are written 0 and never read from any input; a NULL input is not read.
constexpr int kTailPix = 64, kTailIn = 72, kTailPnp = 96;
__global__ __launch_bounds__(kThreads) void head_tail_bwd_kernel(const float* __restrict__ out, int pitch, const float* __restrict__ extents,
                                                                  const float* __restrict__ g_pnp, const float* __restrict__ g_planes,
                                                                  const float* __restrict__ g_out, float* __restrict__ d_out, int hw,
                                                                  long n_pix, int double_mask) {
  __shared__ float T[kTailPix][kTailIn + 1];      // the logits, then g_out's tile, then the result
  __shared__ float G[kTailPix][kTailPnp + 1];
  const int tid = threadIdx.x;
  const long p0 = (long)blockIdx.x * kTailPix;
  const int kx = double_mask ? 2 : 1, kr = kx + 3, n_out = kr + 65;
  auto stage_T = [&](const float* __restrict__ src) {
    for (int idx = tid; idx < kTailPix * (kTailIn / 4); idx += kThreads) {
      const int row = idx / (kTailIn / 4), c4 = idx - row * (kTailIn / 4);
      const f4 v = ld4v(src + (size_t)(p0 + row) * pitch + 4 * c4);
      T[row][4 * c4] = v.x; T[row][4 * c4 + 1] = v.y; T[row][4 * c4 + 2] = v.z; T[row][4 * c4 + 3] = v.w;
    }
  };
  const int p = tid >> 2, part = tid & 3;
  const long pix = p0 + p;
  const int b = (int)(pix / hw);
  double dr[16];
  double dxyz[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int i = 0; i < 16; ++i) dr[i] = 0.0;
  if (g_pnp) {
    stage_T(out);
    for (int idx = tid; idx < kTailPix * (kTailPnp / 4); idx += kThreads) {
      const int row = idx / (kTailPnp / 4), c4 = idx - row * (kTailPnp / 4);
      const f4 v = ld4v(g_pnp + (size_t)(p0 + row) * kTailPnp + 4 * c4);
      G[row][4 * c4] = v.x; G[row][4 * c4 + 1] = v.y; G[row][4 * c4 + 2] = v.z; G[row][4 * c4 + 3] = v.w;
    }
    __syncthreads();
    // head_tail_kernel's softmax, statement for statement
    float e[16];
    float m = -3.402823466e38f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { e[i] = T[p][kr + 1 + part * 16 + i]; m = fmaxf(m, e[i]); }
    m = fmaxf(m, __shfl_xor(m, 1, 64));
    m = fmaxf(m, __shfl_xor(m, 2, 64));
    float ssum = 0.f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { e[i] = expf(e[i] - m); ssum += e[i]; }
    ssum += __shfl_xor(ssum, 1, 64);
    ssum += __shfl_xor(ssum, 2, 64);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      e[i] = e[i] / ssum;
      s += (double)e[i] * (double)G[p][5 + part * 16 + i];
    }
    const int base = (tid & 63) & ~3;
    const double s0 = __shfl(s, base, 64), s1 = __shfl(s, base + 1, 64), s2 = __shfl(s, base + 2, 64), s3 = __shfl(s, base + 3, 64);
    const double dot = ((s0 + s1) + s2) + s3;
#pragma unroll
    for (int i = 0; i < 16; ++i) dr[i] = (double)e[i] * ((double)G[p][5 + part * 16 + i] - dot);
    if (part == 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) dxyz[c] = (double)G[p][c] * (double)extents[3 * (size_t)b + c];
    }
    __syncthreads();      // every lane holds what it needs of T and G
  }
  if (g_out) {
    stage_T(g_out);
    __syncthreads();
  }
  // every cell below is read (g_out's value) and written by one thread
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    float* cell = &T[p][kr + 1 + part * 16 + i];
    *cell = (float)(g_out ? dr[i] + (double)*cell : dr[i]);
  }
  if (part == 0) {
    for (int k = 0; k <= kr; ++k) {
      double v = g_planes && k < kr ? (double)g_planes[(size_t)k * n_pix + pix] : 0.0;
      if (k >= kx && k < kr) v += dxyz[k - kx];
      if (g_out) v += (double)T[p][k];
      T[p][k] = (float)v;
    }
  }
  __syncthreads();
  const int q4 = pitch / 4;
  for (int idx = tid; idx < kTailPix * q4; idx += kThreads) {
    const int row = idx / q4, c4 = idx - row * q4, c = 4 * c4;
    f4 v = {0.f, 0.f, 0.f, 0.f};
    if (c < kTailIn) {
      v.x = c < n_out ? T[row][c] : 0.f;
      v.y = c + 1 < n_out ? T[row][c + 1] : 0.f;
      v.z = c + 2 < n_out ? T[row][c + 2] : 0.f;
      v.w = c + 3 < n_out ? T[row][c + 3] : 0.f;
    }
    st4v(d_out + (size_t)(p0 + row) * pitch + c, v);
  }
}

// ---- dinput ---------------------------------------------------------------------------------------------------------------------
// dfeat[m][k] = sum_c d_out[m][c] W[s][c][k], c < n_out <= 72, on v_mfma_f32_32x32x2_f32: bit for bit one fmaf chain in column order
// (72 terms with the zero-filled tail; the project's rule is chains of at most 128, so there are no fp64 carries here).
//   workgroup   exact_gemm_device.hpp's 128 rows x 128 columns of dfeat, the depth in three stages of 24, each loaded and stored in
//               one step.  hw % 256 == 0: the 128 rows lie in one ROI, the selector is uniform.  A selector outside [0, n_slices)
//               writes NaN rows and reads no weight.
//   d_out       read at its pitch, float4; elements at and beyond column n_out are replaced by 0 before they reach the LDS; stored
//               transposed into the [c][row] image (pitch 133).
//   W           read as it lies: row c of slice s is the B operand's k-row, 128 consecutive floats; rows at and beyond n_out are
//               zero-filled and not read.
constexpr int kDiBK = 24, kDiStages = kMaxOut / kDiBK;
__global__ __launch_bounds__(kThreads) void grouped_dinput_kernel(const float* __restrict__ d_out, int pitch, int n_out,
                                                                   const float* __restrict__ W, const int* __restrict__ sel, int n_slices,
                                                                   int hw, float* __restrict__ dfeat, int K) {
  __shared__ float sA[kDiBK * kPitchT];
  __shared__ float sB[kDiBK * kPitch];
  const int tid = threadIdx.x;
  const int tiles_n = K / 128;
  const long m0 = (long)(blockIdx.x / tiles_n) * 128;
  const int n0 = ((int)blockIdx.x % tiles_n) * 128;
  const int s = sel[m0 / hw];
  if (s < 0 || s >= n_slices) {
    const float nan = __uint_as_float(0x7fc00000u);
    for (int idx = tid; idx < 128 * 32; idx += kThreads)
      st4v(dfeat + (size_t)(m0 + idx / 32) * K + n0 + 4 * (idx % 32), f4{nan, nan, nan, nan});
    return;
  }
  const float* Ws = W + (size_t)s * n_out * K + n0;
  Acc t;      // one fp32 chain: no carries
  t.clear();
  const float* la = lane_a<kPitchT>(sA);
  const float* lb = lane_b<kPitch>(sB);
  for (int st = 0; st < kDiStages; ++st) {
    const int k0 = st * kDiBK;
    __syncthreads();      // every wave has read the previous stage
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      const int idx = tid + kThreads * q;
      {   // A: 128 rows x 6 float4
        const int row = idx / 6, c4 = idx - row * 6, c = k0 + 4 * c4;
        f4 v = ld4v(d_out + (size_t)(m0 + row) * pitch + c);      // c + 3 < 72 <= pitch
#pragma unroll
        for (int j = 0; j < 4; ++j) sA[(4 * c4 + j) * kPitchT + row] = c + j < n_out ? v[j] : 0.f;
      }
      {   // B: 24 k-rows x 32 float4
        const int kr = idx >> 5, c4 = idx & 31;
        const f4 v = k0 + kr < n_out ? ld4v(Ws + (size_t)(k0 + kr) * K + 4 * c4) : f4{0.f, 0.f, 0.f, 0.f};
        st4v(sB + kr * kPitch + 4 * c4, v);
      }
    }
    __syncthreads();
    t.mma<kPitchT, kPitch, kDiBK>(la, lb);
  }
  for_each_d(m0, n0, [=, &t](int i, int j, int e, long m, int n) { dfeat[(size_t)m * K + n] = t.acc[i][j][e]; });
}

// ---- wgrad ----------------------------------------------------------------------------------------------------------------------
// Workgroup (column tile kt of K, row slot y, ROI r): the fp64 tile  d_out[r]^T feat[r]  [n_out padded to 128][128] over the slot's
// rows of the ROI, by the scheme of exact_gemm_device.hpp with both operands staged as they lie.  The loop is written out here: the
// column sums read the A image between the MFMAs and the fold, and a launch that wants no dW runs no MFMAs.
//   d_out   read at its pitch; elements at and beyond column n_out (and whole float4s at and beyond the pitch) are zero-filled in the
//           staging and never reach a sum.  Rows at and beyond the slot's end — the next slot's, or the next ROI's — are zero-filled and
//           not read.
//   db      the workgroups of column tile 0 also add the staged d_out rows column by column in fp64, in row order.
//   slots   wgrad_plan: chunks of 512 rows dealt to at most 16 slots per ROI, and no more than bring the grid to 1024 workgroups
//           (rounded up); from (B, hw, K) alone.
//   out     workspace  tiles f64[B][slots][n_out][K]  then  sums f64[B][slots][128].  A ROI whose selector is outside [0, n_slices)
//           does nothing; the finalize never reads its part.
constexpr int kWgSlotRows = 512, kWgSlotCap = 16, kWgGrid = 1024;
inline SlotPlan wgrad_plan(int B, int hw, int K) {
  return row_slot_plan(hw, (long)B * (K / 128), kWgSlotRows, kWgSlotCap, kWgGrid, true);
}

template <bool WANT_W, bool WANT_B>
__global__ __launch_bounds__(kThreads) void grouped_wgrad_kernel(const float* __restrict__ d_out, int pitch, int n_out,
                                                                  const float* __restrict__ feat, int K, const int* __restrict__ sel,
                                                                  int n_slices, int hw, long rows_per_slot, double* __restrict__ ws_w,
                                                                  double* __restrict__ ws_b) {
  __shared__ float sA[kBK * kPitch];
  __shared__ float sB[kBK * kPitch];
  const int r = blockIdx.z, slot = blockIdx.y, slots = gridDim.y, kt = blockIdx.x;
  const int cls = sel[r];
  if (cls < 0 || cls >= n_slices) return;
  const int tid = threadIdx.x, scol = stage_col();
  const long r0 = (long)slot * rows_per_slot, r1 = r0 + rows_per_slot < hw ? r0 + rows_per_slot : hw;
  const float* ap = d_out + (size_t)r * hw * pitch + scol;
  const float* bp = feat + (size_t)r * hw * K + (size_t)kt * 128 + scol;
  const bool a_in = scol < pitch && scol < n_out;      // pitch % 4 == 0: the float4 lies inside the row
  f4 ra[4], rb[4];
  auto fetch = [&](long row) {
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      const long m = row + stage_row() + 8 * p;
      const bool in = m < r1;
      f4 a = in && a_in ? ld4v(ap + (size_t)m * pitch) : f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = scol + j < n_out ? a[j] : 0.f;
      ra[p] = a;
      if (WANT_W) rb[p] = in ? ld4v(bp + (size_t)m * K) : f4{0.f, 0.f, 0.f, 0.f};
    }
  };
  Tile t;
  t.clear();
  const float* la = lane_a<kPitch>(sA);
  const float* lb = lane_b<kPitch>(sB);
  const bool sums = WANT_B && kt == 0 && tid < 128;
  double colsum = 0.0;
  if (r0 < r1) fetch(r0);
  int stage = 0;
  for (long row = r0; row < r1; row += kBK) {
    __syncthreads();      // every wave has read the previous stage
#pragma unroll
    for (int p = 0; p < 4; ++p) {
      store_natural(sA, p, ra[p]);
      if (WANT_W) store_natural(sB, p, rb[p]);
    }
    __syncthreads();
    if (row + kBK < r1) fetch(row + kBK);
    if (WANT_W) {
      t.mma<kPitch, kPitch, kBK>(la, lb);
      if (++stage == kChainStages) {
        t.fold();
        stage = 0;
      }
    }
    if (sums) {
#pragma unroll 8
      for (int k = 0; k < kBK; ++k) colsum += (double)sA[k * kPitch + tid];
    }
  }
  const size_t part = (size_t)r * slots + slot;
  if (sums) ws_b[part * 128 + tid] = colsum;
  if (WANT_W) {
    t.fold();
    double* o = ws_w + part * n_out * K;
    for_each_d(0, kt * 128, [=, &t](int i, int j, int e, int n1, int n2) {
      if (n1 < n_out) o[(size_t)n1 * K + n2] = t.carry[i][j][e];
    });
  }
}

// Workgroup (channel j of the slice, slice c): over the ROIs with sel[r] == c in index order, each ROI's slots in index order, in
// fp64, one rounding; written to row cls_rows[c][j] of gradients shaped like the layer's weight [out_rows][K] and bias.  A slice no
// ROI selects sums nothing and writes 0.  Thread t takes the columns t, t + 256, ...
__global__ __launch_bounds__(kThreads) void grouped_wgrad_finalize_kernel(const double* __restrict__ ws_w, const double* __restrict__ ws_b,
                                                                           const int* __restrict__ sel, int B, int slots, int n_out, int K,
                                                                           const long long* __restrict__ cls_rows, int out_rows,
                                                                           float* __restrict__ dW, float* __restrict__ db) {
  const int j = blockIdx.x, c = blockIdx.y;
  const long long row = cls_rows[(size_t)c * n_out + j];
  if (row < 0 || row >= out_rows) return;
  if (dW) {
    for (int k = threadIdx.x; k < K; k += kThreads) {
      double s = 0.0;
      for (int r = 0; r < B; ++r) {
        if (sel[r] != c) continue;
        const double* src = ws_w + (((size_t)r * slots) * n_out + j) * K + k;
        for (int y = 0; y < slots; ++y) s += src[(size_t)y * n_out * K];
      }
      dW[(size_t)row * K + k] = (float)s;
    }
  }
  if (db && threadIdx.x == 0) {
    double s = 0.0;
    for (int r = 0; r < B; ++r) {
      if (sel[r] != c) continue;
      for (int y = 0; y < slots; ++y) s += ws_b[((size_t)r * slots + y) * 128 + j];
    }
    db[row] = (float)s;
  }
}

bool grouped_shape_ok(int B, int hw, int K, int n_out, int pitch) {
  return B > 0 && B <= 65535 && hw > 0 && hw % 256 == 0 && K > 0 && K % 128 == 0 && n_out > 0 && n_out <= kMaxOut && pitch >= kMaxOut &&
         pitch % 4 == 0 && (long)B * hw < (1l << 31) - 128 && (long)B * hw / 128 * (K / 128) < (1l << 31);
}

}  // namespace

extern "C" {

int gdrnpp_head_tail_backward_nhwc(const float* out_nhwc, int pitch, const float* extents, const float* g_pnp_in, const float* g_planes,
                                   const float* g_out, float* d_out, int b, int hw, int double_mask, void* stream) {
  GDRNPP_REQUIRE(d_out && (!g_pnp_in || (out_nhwc && extents)), GDRNPP_EINVAL,
                 "gdrnpp_head_tail_backward_nhwc: null pointer (d_out; out_nhwc and extents with g_pnp_in)");
  GDRNPP_REQUIRE(b > 0 && hw > 0 && hw % kTailPix == 0 && pitch >= kTailIn && pitch % 4 == 0, GDRNPP_EINVAL,
                 "gdrnpp_head_tail_backward_nhwc: b=%d hw=%d (multiple of %d) pitch=%d (>= %d, multiple of 4)", b, hw, kTailPix, pitch, kTailIn);
  GDRNPP_REQUIRE(aligned16(out_nhwc) && aligned16(g_pnp_in) && aligned16(g_out) && aligned16(d_out), GDRNPP_EINVAL,
                 "gdrnpp_head_tail_backward_nhwc: the tensors must be 16-byte aligned");
  const long n_pix = (long)b * hw;
  GDRNPP_REQUIRE(n_pix / kTailPix < (1l << 31), GDRNPP_ELIMIT, "gdrnpp_head_tail_backward_nhwc: grid too large");
  hipLaunchKernelGGL(head_tail_bwd_kernel, dim3((unsigned)(n_pix / kTailPix)), dim3(kThreads), 0, (hipStream_t)stream, out_nhwc, pitch,
                     extents, g_pnp_in, g_planes, g_out, d_out, hw, n_pix, double_mask);
  return gdrnpp::check_launch("gdrnpp_head_tail_backward_nhwc");
}

int gdrnpp_grouped_linear_dinput_f32(const float* d_out, int pitch, int n_out, const float* W, const int* group_sel, int n_slices,
                                     int rows_per_group, float* dfeat, int M, int K, void* stream) {
  GDRNPP_REQUIRE(d_out && W && group_sel && dfeat, GDRNPP_EINVAL, "gdrnpp_grouped_linear_dinput_f32: null pointer");
  GDRNPP_REQUIRE(M > 0 && rows_per_group > 0 && M % rows_per_group == 0 && n_slices > 0, GDRNPP_EINVAL,
                 "gdrnpp_grouped_linear_dinput_f32: M=%d rows_per_group=%d n_slices=%d", M, rows_per_group, n_slices);
  GDRNPP_REQUIRE(grouped_shape_ok(M / rows_per_group, rows_per_group, K, n_out, pitch), GDRNPP_ELIMIT,
                 "gdrnpp_grouped_linear_dinput_f32: rows_per_group=%d (multiple of 256) K=%d (multiple of 128) n_out=%d (<= %d) pitch=%d (>= %d, "
                 "multiple of 4)", rows_per_group, K, n_out, kMaxOut, pitch, kMaxOut);
  GDRNPP_REQUIRE(aligned16(d_out) && aligned16(W) && aligned16(dfeat), GDRNPP_EINVAL,
                 "gdrnpp_grouped_linear_dinput_f32: the tensors must be 16-byte aligned");
  hipLaunchKernelGGL(grouped_dinput_kernel, dim3((unsigned)((M / 128) * (K / 128))), dim3(kThreads), 0, (hipStream_t)stream, d_out, pitch,
                     n_out, W, group_sel, n_slices, rows_per_group, dfeat, K);
  return gdrnpp::check_launch("gdrnpp_grouped_linear_dinput_f32");
}

size_t gdrnpp_grouped_linear_wgrad_f32_workspace_bytes(int B, int hw, int K, int n_out) {
  if (!grouped_shape_ok(B, hw, K, n_out, kMaxOut)) return 0;
  return (size_t)B * wgrad_plan(B, hw, K).slots * ((size_t)n_out * K + 128) * sizeof(double);
}

int gdrnpp_grouped_linear_wgrad_f32(const float* d_out, int pitch, int n_out, const float* feat, const int* group_sel, int n_slices,
                                    const long long* cls_rows, int out_rows, float* dW, float* db, int B, int hw, int K, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  if (!dW && !db) return 0;      // nothing asked for, nothing launched
  GDRNPP_REQUIRE(d_out && group_sel && cls_rows && workspace && (!dW || feat), GDRNPP_EINVAL, "gdrnpp_grouped_linear_wgrad_f32: null pointer");
  GDRNPP_REQUIRE(n_slices > 0 && n_slices <= 65535 && out_rows > 0, GDRNPP_EINVAL, "gdrnpp_grouped_linear_wgrad_f32: n_slices=%d out_rows=%d",
                 n_slices, out_rows);
  GDRNPP_REQUIRE(grouped_shape_ok(B, hw, K, n_out, pitch), GDRNPP_ELIMIT,
                 "gdrnpp_grouped_linear_wgrad_f32: B=%d hw=%d (multiple of 256) K=%d (multiple of 128) n_out=%d (<= %d) pitch=%d (>= %d, multiple of 4)",
                 B, hw, K, n_out, kMaxOut, pitch, kMaxOut);
  const size_t need = gdrnpp_grouped_linear_wgrad_f32_workspace_bytes(B, hw, K, n_out);
  GDRNPP_REQUIRE(workspace_bytes >= need && aligned16(workspace) && aligned16(d_out) && aligned16(feat), GDRNPP_EINVAL,
                 "gdrnpp_grouped_linear_wgrad_f32: workspace of %zu bytes, %zu needed; d_out, feat and the workspace 16-byte aligned",
                 workspace_bytes, need);
  const SlotPlan p = wgrad_plan(B, hw, K);
  hipStream_t st = (hipStream_t)stream;
  double* ws_w = (double*)workspace;
  double* ws_b = ws_w + (size_t)B * p.slots * n_out * K;
  const dim3 grid((unsigned)(dW ? K / 128 : 1), (unsigned)p.slots, (unsigned)B);
  if (dW && db)
    hipLaunchKernelGGL((grouped_wgrad_kernel<true, true>), grid, dim3(kThreads), 0, st, d_out, pitch, n_out, feat, K, group_sel, n_slices, hw,
                       p.rows_per_slot, ws_w, ws_b);
  else if (dW)
    hipLaunchKernelGGL((grouped_wgrad_kernel<true, false>), grid, dim3(kThreads), 0, st, d_out, pitch, n_out, feat, K, group_sel, n_slices, hw,
                       p.rows_per_slot, ws_w, ws_b);
  else
    hipLaunchKernelGGL((grouped_wgrad_kernel<false, true>), grid, dim3(kThreads), 0, st, d_out, pitch, n_out, feat, K, group_sel, n_slices, hw,
                       p.rows_per_slot, ws_w, ws_b);
  hipLaunchKernelGGL(grouped_wgrad_finalize_kernel, dim3((unsigned)n_out, (unsigned)n_slices), dim3(kThreads), 0, st, ws_w, ws_b, group_sel, B,
                     p.slots, n_out, K, cls_rows, out_rows, dW, db);
  return gdrnpp::check_launch("gdrnpp_grouped_linear_wgrad_f32");
}

}  // extern "C"
