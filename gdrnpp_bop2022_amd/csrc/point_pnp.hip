// SimplePointPnPNet (models/heads/point_pnp_net.py:208-293) on the GPU: the point-wise MLP cin -> 128 -> 128 -> 1024 with the
// global max over the points taken in the last GEMM's epilogue, then fc1 -> fc2 on the pooled vector.
//
// gdrnpp_point_pnp_pool: one workgroup (4 waves) per (ROI, tile of 128 points).  All three layers run on the exact-f32 matrix
// instruction v_mfma_f32_32x32x2_f32 with the POINTS as the M dimension: D[point][channel] = sum_k H[point][k] * W[channel][k],
// a k-ordered fmaf chain per output that starts from the bias (layers 1, 2) or from zero (layer 3: the bias is added after the
// max, which is the same number because rounding is monotonic).  Wave w owns points 32w .. 32w + 31 and all 128 output channels
// of a layer (four 32x32 accumulators), so
//   * the activation image [channel][point] in LDS is wave-private by columns: a layer's result overwrites its input in place
//     and no barrier guards it;
//   * the weight image [k][channel] (one 128 x 128 block: W1, W2 or a 128-channel chunk of W3) is shared; the next block is
//     fetched into registers before the current block's k-loop and written to LDS behind it, between two barriers;
//   * in the accumulator a lane holds ONE channel and 16 points: the column max is 15 v_max in registers, one cross-lane step
//     (lane ^ 32) and one [chunk][wave][128] LDS slab that the workgroup folds once at the end.
// LDS: 128 x 132 (activations) + 128 x 129 (weights) + 8 x 4 x 128 (max slab) floats = 150,016 bytes of the CU's 160 KB, one
// workgroup and one wave per SIMD (512 VGPRs each: 64 accumulator + 64 prefetch registers).
// Per-tile maxima go to the workspace f32[b][hw / 128][1024]; fp32 max is exact and order-independent, so the result is
// bit-reproducible without atomics on any stream.
#include "common.hpp"
#include "wave_ops.hpp"

#include <cmath>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kPT = 128;               // points per workgroup
constexpr int kHid = 128;              // channels of the two hidden layers
constexpr int kOut = 1024;             // channels of conv3 = length of the pooled vector
constexpr int kChunks = kOut / 128;
constexpr int kHP = kPT + 4;           // pitch of the activation image [channel][point]: 16-byte aligned rows for the b128 writes
constexpr int kWP = 129;               // pitch of the weight image [k][channel]: odd, the transposing writes spread over all banks
constexpr int kMaxCin = 128;           // rows of the activation image
constexpr int kPoolLdsBytes = (128 * kHP + 128 * kWP + kChunks * 4 * 128) * (int)sizeof(float);
constexpr int kFcRois = 4;             // ROIs per workgroup of the fc kernel: fc1 / fc2 weights are read once per group
constexpr int kFc1 = 512, kFc2 = 256;

__device__ __forceinline__ float lrelu(float v) { return v > 0.f ? v : 0.1f * v; }

// a [128 channels][128 k] row-major weight block -> 16 float4 per thread; 16 lanes cover 256 contiguous bytes of a row
__device__ __forceinline__ void fetch_block(const float* __restrict__ w, float4 (&pre)[16], int t) {
  const int q = t & 15, rr = t >> 4;
#pragma unroll
  for (int i = 0; i < 16; ++i)
    pre[i] = *reinterpret_cast<const float4*>(w + (size_t)((i >> 1) * 16 + rr) * 128 + 4 * ((i & 1) * 16 + q));
}

// ... -> the weight image [k][channel]; the 64 lanes of a wave hit 64 different banks (4q + r with pitch 129)
__device__ __forceinline__ void store_block(float* __restrict__ Wb, const float4 (&pre)[16], int t) {
  const int q = t & 15, rr = t >> 4;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int row = (i >> 1) * 16 + rr, k = 4 * ((i & 1) * 16 + q);
    Wb[(k + 0) * kWP + row] = pre[i].x;
    Wb[(k + 1) * kWP + row] = pre[i].y;
    Wb[(k + 2) * kWP + row] = pre[i].z;
    Wb[(k + 3) * kWP + row] = pre[i].w;
  }
}

// acc[nt][.] += H[k][32 wave + .] x W[k][32 nt + .] over 2 * ksteps values of k (one 32x32x2 instruction per nt and step)
// (KSTEPS > 0: a compile-time trip count for the two 128-deep layers, unrolled by four)
template <int KSTEPS>
__device__ __forceinline__ void mfma_layer(const float* __restrict__ Hb, const float* __restrict__ Wb, int ksteps, f32x16 (&acc)[4],
                                           int lane, int wave) {
  const float* ap = Hb + (lane >> 5) * kHP + 32 * wave + (lane & 31);
  const float* bp = Wb + (lane >> 5) * kWP + (lane & 31);
  const int n = KSTEPS > 0 ? KSTEPS : ksteps;
  constexpr int kUnroll = KSTEPS > 0 ? 4 : 1;
#pragma unroll kUnroll
  for (int s = 0; s < n; ++s) {
    const float a = ap[2 * s * kHP];
    const float b0 = bp[2 * s * kWP], b1 = bp[2 * s * kWP + 32], b2 = bp[2 * s * kWP + 64], b3 = bp[2 * s * kWP + 96];
    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b0, acc[0], 0, 0, 0);
    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b1, acc[1], 0, 0, 0);
    acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b2, acc[2], 0, 0, 0);
    acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b3, acc[3], 0, 0, 0);
  }
}

__device__ __forceinline__ void init_acc(f32x16 (&acc)[4], const float* __restrict__ bias, int lane) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt) {
    const float b = bias ? bias[32 * nt + (lane & 31)] : 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = b;
  }
}

// LeakyReLU(0.1) and back into the wave's own columns of the activation image: accumulator register r of lane l is
// channel 32 nt + (l & 31), point (r & 3) + 8 (r >> 2) + 4 (l >> 5) -> four consecutive points per 16-byte write
__device__ __forceinline__ void store_hidden(float* __restrict__ Hb, const f32x16 (&acc)[4], int lane, int wave) {
#pragma unroll
  for (int nt = 0; nt < 4; ++nt)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      float4 v;
      v.x = lrelu(acc[nt][4 * g + 0]);
      v.y = lrelu(acc[nt][4 * g + 1]);
      v.z = lrelu(acc[nt][4 * g + 2]);
      v.w = lrelu(acc[nt][4 * g + 3]);
      *reinterpret_cast<float4*>(Hb + (32 * nt + (lane & 31)) * kHP + 32 * wave + 8 * g + 4 * (lane >> 5)) = v;
    }
}

__global__ __launch_bounds__(256) void point_pnp_pool_kernel(const float* __restrict__ x, int pitch, int cin,
                                                             const float* __restrict__ w1, const float* __restrict__ b1,
                                                             const float* __restrict__ w2, const float* __restrict__ b2,
                                                             const float* __restrict__ w3, const float* __restrict__ b3,
                                                             float* __restrict__ partial) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* Hb = lds;                       // [128][kHP]   x tile, then hidden 1, then hidden 2: [channel][point]
  float* Wb = Hb + 128 * kHP;            // [128][kWP]   current weight block: [k][channel]
  float* red = Wb + 128 * kWP;           // [kChunks][4 waves][128]
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const size_t row0 = (size_t)blockIdx.x * kPT;      // first point of the tile in [b * hw]: tiles never straddle ROIs (hw % 128 == 0)
  const int k1p = (cin + 1) & ~1;                    // K of layer 1, padded to the instruction's two

  // W1 f32[128][cin] -> Wb[k][channel], zero rows up to k1p
  for (int idx = t; idx < 128 * k1p; idx += 256) {
    const int ch = idx / k1p, k = idx - ch * k1p;
    Wb[k * kWP + ch] = k < cin ? w1[(size_t)ch * cin + k] : 0.f;
  }
  // the wave's 32 points of x -> Hb[k][point], channels >= cin as zeros (pitch % 4 == 0 and cin <= pitch: the float4 stays in the row)
  {
    const int p = 32 * wave + (lane & 31);
    const float* xr = x + (row0 + p) * (size_t)pitch;
    const int nk4 = (cin + 3) >> 2;
    for (int k4 = lane >> 5; k4 < nk4; k4 += 2) {
      const float4 v = *reinterpret_cast<const float4*>(xr + 4 * k4);
      const int k = 4 * k4;
      Hb[(k + 0) * kHP + p] = v.x;
      Hb[(k + 1) * kHP + p] = k + 1 < cin ? v.y : 0.f;
      Hb[(k + 2) * kHP + p] = k + 2 < cin ? v.z : 0.f;
      Hb[(k + 3) * kHP + p] = k + 3 < cin ? v.w : 0.f;
    }
  }
  float4 pre[16];
  fetch_block(w2, pre, t);
  __syncthreads();

  f32x16 acc[4];
  init_acc(acc, b1, lane);
  mfma_layer<0>(Hb, Wb, k1p >> 1, acc, lane, wave);
  store_hidden(Hb, acc, lane, wave);
  __syncthreads();                       // every wave is done with W1
  store_block(Wb, pre, t);
  fetch_block(w3, pre, t);
  __syncthreads();

  init_acc(acc, b2, lane);
  mfma_layer<kHid / 2>(Hb, Wb, 0, acc, lane, wave);
  store_hidden(Hb, acc, lane, wave);

  for (int c = 0; c < kChunks; ++c) {
    __syncthreads();                     // every wave is done with the previous block
    store_block(Wb, pre, t);
    if (c + 1 < kChunks) fetch_block(w3 + (size_t)(c + 1) * 128 * 128, pre, t);
    __syncthreads();
    init_acc(acc, nullptr, lane);
    mfma_layer<kHid / 2>(Hb, Wb, 0, acc, lane, wave);
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      float m = acc[nt][0];
#pragma unroll
      for (int r = 1; r < 16; ++r) m = fmaxf(m, acc[nt][r]);
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      if (lane < 32) red[(c * 4 + wave) * 128 + 32 * nt + lane] = m;
    }
  }
  __syncthreads();
  float* out = partial + (size_t)blockIdx.x * kOut;
  for (int ch = t; ch < kOut; ch += 256) {
    const float* r = red + (ch >> 7) * 4 * 128 + (ch & 127);
    const float m = fmaxf(fmaxf(r[0], r[128]), fmaxf(r[256], r[384]));
    out[ch] = m + (b3 ? b3[ch] : 0.f);
  }
}

// partial f32[b][tiles][1024] -> pooled f32[b][1024]
__global__ __launch_bounds__(256) void point_pnp_fold_kernel(const float* __restrict__ partial, float* __restrict__ pooled, int tiles) {
  const int roi = blockIdx.x >> 2, ch = (blockIdx.x & 3) * 256 + threadIdx.x;
  const float* p = partial + (size_t)roi * tiles * kOut + ch;
  float m = p[0];
  for (int i = 1; i < tiles; ++i) m = fmaxf(m, p[(size_t)i * kOut]);
  pooled[(size_t)roi * kOut + ch] = m;
}

// one output row of a Linear layer for the group's ROIs: lane l takes k = 4 l + 256 j, the partial sums meet in a fixed-order butterfly
template <int K>
__device__ __forceinline__ void fc_row(const float* __restrict__ wrow, const float (*xs)[K], float (&s)[kFcRois], int lane) {
#pragma unroll
  for (int r = 0; r < kFcRois; ++r) s[r] = 0.f;
#pragma unroll
  for (int j = 0; j < K / 256; ++j) {
    const int k = 4 * lane + 256 * j;
    const float4 w = *reinterpret_cast<const float4*>(wrow + k);
#pragma unroll
    for (int r = 0; r < kFcRois; ++r) {
      const float4 v = *reinterpret_cast<const float4*>(&xs[r][k]);
      s[r] = fmaf(w.x, v.x, s[r]);
      s[r] = fmaf(w.y, v.y, s[r]);
      s[r] = fmaf(w.z, v.z, s[r]);
      s[r] = fmaf(w.w, v.w, s[r]);
    }
  }
#pragma unroll
  for (int r = 0; r < kFcRois; ++r) s[r] = gdrnpp::wave::wave_sum(s[r]);
}

// feat = lrelu(fc2(lrelu(fc1(max over tiles)))) for kFcRois ROIs per workgroup of 16 waves
__global__ __launch_bounds__(1024) void point_pnp_fc_kernel(const float* __restrict__ partial, int tiles, const float* __restrict__ w_fc1,
                                                            const float* __restrict__ b_fc1, const float* __restrict__ w_fc2,
                                                            const float* __restrict__ b_fc2, float* __restrict__ feat, int b) {
  __shared__ __attribute__((aligned(16))) float pooled[kFcRois][kOut];
  __shared__ __attribute__((aligned(16))) float h1[kFcRois][kFc1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int roi0 = blockIdx.x * kFcRois;
#pragma unroll
  for (int r = 0; r < kFcRois; ++r) {
    float m = 0.f;
    if (roi0 + r < b) {
      const float* p = partial + (size_t)(roi0 + r) * tiles * kOut + t;
      m = p[0];
      for (int i = 1; i < tiles; ++i) m = fmaxf(m, p[(size_t)i * kOut]);
    }
    pooled[r][t] = m;
  }
  __syncthreads();
  float s[kFcRois];
  for (int o = wave; o < kFc1; o += 16) {
    fc_row<kOut>(w_fc1 + (size_t)o * kOut, pooled, s, lane);
    if (lane == 0) {
      const float bias = b_fc1 ? b_fc1[o] : 0.f;
#pragma unroll
      for (int r = 0; r < kFcRois; ++r) h1[r][o] = lrelu(s[r] + bias);
    }
  }
  __syncthreads();
  for (int o = wave; o < kFc2; o += 16) {
    fc_row<kFc1>(w_fc2 + (size_t)o * kFc1, h1, s, lane);
    if (lane == 0) {
      const float bias = b_fc2 ? b_fc2[o] : 0.f;
#pragma unroll
      for (int r = 0; r < kFcRois; ++r)
        if (roi0 + r < b) feat[(size_t)(roi0 + r) * kFc2 + o] = lrelu(s[r] + bias);
    }
  }
}

}  // namespace

extern "C" {

size_t gdrnpp_point_pnp_workspace_bytes(int b, int hw) {
  if (b <= 0 || hw <= 0 || hw % kPT != 0) return 0;
  return (size_t)b * (size_t)(hw / kPT) * kOut * sizeof(float);
}

int gdrnpp_point_pnp_pool(const float* x, int pitch, int cin, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* w3, const float* b3, float* pooled, int b, int hw, void* workspace, size_t workspace_bytes,
                          void* stream) {
  GDRNPP_REQUIRE(x && w1 && b1 && w2 && b2 && w3 && b3 && workspace, GDRNPP_EINVAL, "gdrnpp_point_pnp_pool: null pointer");
  GDRNPP_REQUIRE(b > 0 && hw > 0 && hw % kPT == 0, GDRNPP_EINVAL,
                 "gdrnpp_point_pnp_pool: b=%d (> 0) hw=%d (a positive multiple of the %d-point tile)", b, hw, kPT);
  GDRNPP_REQUIRE(pitch > 0 && pitch % 32 == 0 && cin > 0 && cin <= pitch, GDRNPP_EINVAL,
                 "gdrnpp_point_pnp_pool: cin=%d (1 .. pitch) pitch=%d (a multiple of 32)", cin, pitch);
  GDRNPP_REQUIRE(cin <= kMaxCin, GDRNPP_ELIMIT, "gdrnpp_point_pnp_pool: cin=%d (<= %d)", cin, kMaxCin);
  const long blocks = (long)b * (hw / kPT);
  GDRNPP_REQUIRE(blocks < (1l << 30), GDRNPP_ELIMIT, "gdrnpp_point_pnp_pool: grid too large (b=%d hw=%d)", b, hw);
  GDRNPP_REQUIRE(workspace_bytes >= gdrnpp_point_pnp_workspace_bytes(b, hw), GDRNPP_EINVAL,
                 "gdrnpp_point_pnp_pool: workspace of %zu bytes, %zu needed", workspace_bytes, gdrnpp_point_pnp_workspace_bytes(b, hw));
  if (int rc = gdrnpp::ensure_dynamic_lds((const void*)point_pnp_pool_kernel, kPoolLdsBytes)) return rc;
  hipLaunchKernelGGL(point_pnp_pool_kernel, dim3((unsigned)blocks), dim3(256), kPoolLdsBytes, (hipStream_t)stream, x, pitch, cin, w1,
                     b1, w2, b2, w3, b3, (float*)workspace);
  if (int rc = gdrnpp::check_launch("gdrnpp_point_pnp_pool")) return rc;
  if (pooled) {
    hipLaunchKernelGGL(point_pnp_fold_kernel, dim3((unsigned)b * 4), dim3(256), 0, (hipStream_t)stream, (const float*)workspace, pooled,
                       hw / kPT);
    return gdrnpp::check_launch("gdrnpp_point_pnp_pool (fold)");
  }
  return 0;
}

int gdrnpp_point_pnp_fc(const void* workspace, size_t workspace_bytes, const float* w_fc1, const float* b_fc1, const float* w_fc2,
                        const float* b_fc2, float* feat, int b, int hw, void* stream) {
  GDRNPP_REQUIRE(workspace && w_fc1 && b_fc1 && w_fc2 && b_fc2 && feat, GDRNPP_EINVAL, "gdrnpp_point_pnp_fc: null pointer");
  GDRNPP_REQUIRE(b > 0 && hw > 0 && hw % kPT == 0, GDRNPP_EINVAL,
                 "gdrnpp_point_pnp_fc: b=%d (> 0) hw=%d (a positive multiple of the %d-point tile)", b, hw, kPT);
  GDRNPP_REQUIRE(workspace_bytes >= gdrnpp_point_pnp_workspace_bytes(b, hw), GDRNPP_EINVAL,
                 "gdrnpp_point_pnp_fc: workspace of %zu bytes, %zu needed", workspace_bytes, gdrnpp_point_pnp_workspace_bytes(b, hw));
  hipLaunchKernelGGL(point_pnp_fc_kernel, dim3((unsigned)((b + kFcRois - 1) / kFcRois)), dim3(1024), 0, (hipStream_t)stream,
                     (const float*)workspace, hw / kPT, w_fc1, b_fc1, w_fc2, b_fc2, feat, b);
  return gdrnpp::check_launch("gdrnpp_point_pnp_fc");
}

}  // extern "C"
