// conv3x3 (stride 1, zero pad 1) of a bilinear x2 upsampled tensor, second half (geometry head: UpsamplingBilinear2d(2) in front of
// a ConvModule, top_down_doublemask_xyz_region_head.py:80-107).
//
// Channel mixing and per-channel spatial interpolation commute, W_t U(x) = U(W_t x), so
//   conv3x3(U(x))[p] = bias + sum_t [p + d_t inside 2H x 2W] U(y_t)[p + d_t],      y_t = W_t x at the LOW resolution:
// one GEMM of the low-res NHWC activation [N*H*W, Cin] with the weight reordered to rows (ky, kx, co) — a quarter of the
// matrix flops of the convolution at 2H x 2W — then this gather over y f32[N*H*W, 9*C] (the deconv layer of the same head runs
// in this shape: GEMM + deconv_col2im_gn_kernel).
//
// Interpolation is align_corners=True with upsample2x_kernel's float expressions: src = s * dst, s = (H-1)/(2H-1) in fp32,
// weight of the upper neighbour = src - floor(src).  In real arithmetic floor(s * q) = floor((q-1)/2) for every 0 < q < 2H
// (s q = i - i/(2H-1) for q = 2i, i + (H-1-i)/(2H-1) for q = 2i+1), which is what makes every register index below static: a
// thread's 4 x 4 output block and its 3 x 3 taps touch the 6 x 6 high-res positions around it, and those read the 4 x 4 low-res
// window that starts at (2bi-1, 2bj-1) in a fixed pattern — position u = 0..5 of the six reads window rows u/2 and u/2 + 1.
// The float product leaves the pattern in two places only, and both carry weight 0 / 1: q = 0 (src 0: the pattern's row -1 is
// clamped to row 0, weight 1 on row 0 either way) and q = 2H-1 (src = H-1 up to an ulp: the weight is clamped to [0, 1], the
// real-arithmetic value).  Window rows / columns outside the image are clamped addresses that only ever meet weight 0 or a
// position outside 2H x 2W, which contributes nothing (zero padding at the HIGH resolution).
//
// Summation order per output: bias, then taps 0..8, within a tap bilerp4's expression ly0*(lx0*v00 + lx1*v01) + ly1*(lx0*v10 +
// lx1*v11) (the horizontal pair sums are shared between the outputs of a block: same operations, same bits).  GroupNorm
// statistics: fp64 per thread in block / pixel order, then the fixed-order LDS gather of gn_stats_kernel -> part[N, P, G, 2],
// the layout gn_apply_kernel consumes.  The pixel partition depends on (H, W, C) only, so an image's result and partials do not
// depend on which images share its launch.
//
// Loads: a tap (ky, kx) needs window rows ky/2 .. (ky+3)/2 + 1, i.e. 3 / 4 / 3 of them, and columns alike: (3+4+3)^2 = 100
// 16-byte loads per 16 outputs = 6.25 per output (the one-output form would take 36).
#include "common.hpp"

namespace {

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ void st4(float* p, float4 v) { *reinterpret_cast<float4*>(p) = v; }

constexpr int kB = 4;   // a thread owns kB x kB output pixels of one channel quad

// the six high-res positions o0-1 .. o0+4 of one axis: inside the image?  weights of window entries u/2 and u/2 + 1
struct Axis {
  bool in[kB + 2];
  float w0[kB + 2], w1[kB + 2];
};
__device__ __forceinline__ Axis axis_of(int o0, int O, float s) {
  Axis a;
  const int base = (o0 >> 1) - 1;               // first low-res index of the window (may be -1)
#pragma unroll
  for (int u = 0; u < kB + 2; ++u) {
    const int q = o0 - 1 + u;
    a.in[u] = q >= 0 && q < O;
    const float f = s * (float)q;
    const float l1 = fminf(fmaxf(f - (float)(base + (u >> 1)), 0.f), 1.f);
    a.w1[u] = l1;
    a.w0[u] = 1.f - l1;
  }
  return a;
}

__global__ __launch_bounds__(256) void upconv_gather_gn_kernel(const float* __restrict__ y, const float* __restrict__ bias,
                                                               float* __restrict__ out, double* __restrict__ part, int H, int W,
                                                               int C, int G, int P) {
  extern __shared__ double sred[];  // [2][256]
  const int Q = C >> 2, cpg = C / G;
  const int OH = 2 * H, OW = 2 * W;
  const int BW = (OW + kB - 1) / kB, nblk = ((OH + kB - 1) / kB) * BW;
  const int n = blockIdx.y, pc = blockIdx.x;
  const int q = threadIdx.x % Q, row = threadIdx.x / Q, rows = blockDim.x / Q;
  const int per = (nblk + P - 1) / P;
  const int b0 = pc * per, b1 = min(nblk, b0 + per);
  const float sh = (OH > 1) ? (float)(H - 1) / (float)(OH - 1) : 0.f;
  const float sw = (OW > 1) ? (float)(W - 1) / (float)(OW - 1) : 0.f;
  const size_t pitch = (size_t)9 * C;
  const float* yn = y + (size_t)n * H * W * pitch + 4 * q;
  float* on = out + (size_t)n * OH * OW * C + 4 * q;
  const float4 b4 = bias ? ld4(bias + 4 * q) : make_float4(0.f, 0.f, 0.f, 0.f);
  double s = 0.0, ss = 0.0;
  for (int b = b0 + row; b < b1; b += rows) {
    const int bi = b / BW, bj = b - bi * BW;
    const int oy0 = kB * bi, ox0 = kB * bj;
    const Axis ay = axis_of(oy0, OH, sh), ax = axis_of(ox0, OW, sw);
    size_t roff[4], coff[4];        // the window's rows / columns, clamped into the image
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      roff[k] = (size_t)min(max(2 * bi - 1 + k, 0), H - 1) * W * pitch;
      coff[k] = (size_t)min(max(2 * bj - 1 + k, 0), W - 1) * pitch;
    }
    float4 acc[kB][kB];
#pragma unroll
    for (int r = 0; r < kB; ++r)
#pragma unroll
      for (int c = 0; c < kB; ++c) acc[r][c] = b4;
#pragma unroll
    for (int ky = 0; ky < 3; ++ky)
#pragma unroll
      for (int kx = 0; kx < 3; ++kx) {
        const float* yt = yn + (size_t)(ky * 3 + kx) * C;
        float4 v[4][4], h[4][kB];
#pragma unroll
        for (int wr = ky / 2; wr <= (ky + 3) / 2 + 1; ++wr)
#pragma unroll
          for (int wc = kx / 2; wc <= (kx + 3) / 2 + 1; ++wc) v[wr][wc] = ld4(yt + roff[wr] + coff[wc]);
#pragma unroll
        for (int wr = ky / 2; wr <= (ky + 3) / 2 + 1; ++wr)
#pragma unroll
          for (int c = 0; c < kB; ++c) {
            const int u = kx + c;
            const float l0 = ax.w0[u], l1 = ax.w1[u];
            const float4 a = v[wr][u / 2], d = v[wr][u / 2 + 1];
            h[wr][c] = make_float4(l0 * a.x + l1 * d.x, l0 * a.y + l1 * d.y, l0 * a.z + l1 * d.z, l0 * a.w + l1 * d.w);
          }
#pragma unroll
        for (int r = 0; r < kB; ++r) {
          const int u = ky + r;
          const float l0 = ay.w0[u], l1 = ay.w1[u];
#pragma unroll
          for (int c = 0; c < kB; ++c) {
            if (!(ay.in[u] && ax.in[kx + c])) continue;      // zero padding of the 2H x 2W image
            const float4 a = h[u / 2][c], d = h[u / 2 + 1][c];
            acc[r][c].x += l0 * a.x + l1 * d.x;
            acc[r][c].y += l0 * a.y + l1 * d.y;
            acc[r][c].z += l0 * a.z + l1 * d.z;
            acc[r][c].w += l0 * a.w + l1 * d.w;
          }
        }
      }
#pragma unroll
    for (int r = 0; r < kB; ++r)
#pragma unroll
      for (int c = 0; c < kB; ++c) {
        if (oy0 + r >= OH || ox0 + c >= OW) continue;
        const float4 a = acc[r][c];
        st4(on + ((size_t)(oy0 + r) * OW + ox0 + c) * C, a);
        s += ((double)a.x + (double)a.y) + ((double)a.z + (double)a.w);
        ss += ((double)a.x * a.x + (double)a.y * a.y) + ((double)a.z * a.z + (double)a.w * a.w);
      }
  }
  sred[threadIdx.x] = s;
  sred[256 + threadIdx.x] = ss;
  __syncthreads();
  // one thread per group sums the (rows x quads-per-group) partials in a fixed order
  if ((int)threadIdx.x < G) {
    const int g = threadIdx.x, qpg = cpg >> 2;
    double a = 0.0, c2 = 0.0;
    for (int r = 0; r < rows; ++r)
      for (int k = 0; k < qpg; ++k) {
        const int t = r * Q + g * qpg + k;
        a += sred[t];
        c2 += sred[256 + t];
      }
    double* o = part + (((size_t)n * P + pc) * G + g) * 2;
    o[0] = a;
    o[1] = c2;
  }
}

}  // namespace

extern "C" {

int gdrnpp_upconv_gather_partials(int H, int W, int C) {
  if (H <= 0 || W <= 0 || H > 16384 || W > 16384 || C <= 0 || C % 4 || C / 4 > 256 || 256 % (C / 4)) return 0;
  const long nblk = (long)((2 * H + kB - 1) / kB) * ((2 * W + kB - 1) / kB);
  const int rows = 256 / (C / 4);
  const long p = (nblk + rows - 1) / rows;       // one block per thread where that leaves at most 64 partials
  return (int)(p < 64 ? p : 64);
}

int gdrnpp_upconv_gather_gn_nhwc(const float* y_taps, const float* bias, float* out, double* gn_partials, int N, int H, int W,
                                 int C, int G, void* stream) {
  GDRNPP_REQUIRE(y_taps && out && gn_partials, GDRNPP_EINVAL, "gdrnpp_upconv_gather_gn_nhwc: null pointer");
  GDRNPP_REQUIRE(N > 0 && H > 0 && W > 0 && C > 0 && C % 4 == 0 && G > 0 && C % G == 0, GDRNPP_EINVAL,
                 "gdrnpp_upconv_gather_gn_nhwc: N=%d H=%d W=%d C=%d G=%d", N, H, W, C, G);
  const int cpg = C / G;
  const int P = gdrnpp_upconv_gather_partials(H, W, C);
  GDRNPP_REQUIRE(P > 0 && cpg % 4 == 0 && G <= 64 && N <= 65535, GDRNPP_ELIMIT,
                 "gdrnpp_upconv_gather_gn_nhwc: unsupported shape H=%d W=%d C=%d G=%d N=%d", H, W, C, G, N);
  hipLaunchKernelGGL(upconv_gather_gn_kernel, dim3(P, N), dim3(256), sizeof(double) * 512, (hipStream_t)stream, y_taps, bias, out,
                     gn_partials, H, W, C, G, P);
  return gdrnpp::check_launch("gdrnpp_upconv_gather_gn_nhwc");
}

}  // extern "C"
