// The YOLOX detector forward (CSPDarknet + PAFPN + decoupled head) on NHWC fp32 tensors.
//
// gdrnpp_conv_bias_act_f32: implicit-GEMM convolution (1x1 or 3x3, stride 1 or 2, padding (k-1)/2) on the exact-f32 matrix
// instruction v_mfma_f32_32x32x2_f32 (the engine of point_pnp.hip), pixels as M, output channels as N, K = taps x Cin walked
// tap by tap in chunks of 16 input channels.  One workgroup (4 waves) owns 128 pixels x 32 NT channels (NT = 1, 2, 4); wave w owns
// pixels 32 w .. 32 w + 31 and all 32 NT channels (NT accumulators of 32x32).  Per chunk the A tile [16 k][128 pixels] and the
// B tile [16 k][32 NT channels] pass through LDS (16.7 KB at NT = 4: several workgroups per CU hide each other's barriers); the
// next chunk is fetched into registers before the current chunk's eight MFMA steps and stored behind them.  Every output is
// summed in a fixed order by one lane: no split over K between workgroups, no atomics, bit-reproducible on any stream.  The sum
// has two levels: the matrix instruction chains `flush` chunks (about sqrt(K) values of k) into a partial accumulator, which is
// then added to the total and cleared — a chain of K fp32 additions loses ~sqrt(K / 2) ulp, two balanced levels ~sqrt(sqrt K):
// at 640 -> 640, 3x3 (K = 5760) 2.3e-6 -> of the order of the six-product split GEMM's 2.9e-7 of the largest output.
//   * A, C and the residual are channel slices of wider buffers (row stride in channels, pointer pre-offset by the slice's first
//     channel), so a layer reads and writes its slot of a concatenation in place;
//   * partial tiles: pixels beyond M and channels beyond Cout are computed on zeros and never stored;
//   * epilogue: + bias, activation (none, SiLU, sigmoid, YOLOX box decode), + residual, in this order;
//   * the C row of pixel (img, oy, ox) is img * c_img_rows + c_row0 + oy * OW + ox: a prediction layer writes at its level's anchor
//     offset of det_preds[B, A, 5 + C] directly.
// LDS banking (ds_write_b32 / ds_read_b32: 32 banks per 32-lane half): the A image has pitch 130 (the four 4-channel groups of a
// half-wave's 8 pixels land 8 banks apart), operand reads are 32 consecutive floats per half.
//
// gdrnpp_yolox_focus, gdrnpp_spp_maxpool_5_9_13, gdrnpp_upsample_nearest2x_slice: the three data-movement layers, exact.
#include "common.hpp"

#include <cmath>

namespace {

using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int kBM = 128;     // pixels per workgroup
constexpr int kBK = 16;      // input channels per chunk
constexpr int kAP = 130;     // pitch of the A image [k][pixel]

struct ConvArgs {
  const float* a;            // + a_off
  const float* w;            // f32[ks * ks * cin][ldw]
  const float* bias;         // f32[cout] or null
  const float* res;          // + r_off, or null (may alias c)
  float* c;                  // + c_off
  int B, H, W, OH, OW, cin, cout, ldw, ks, stride, lda, ldc, ldr, act, flush;
  long c_img_rows, c_row0;
  float dec_stride;
};

template <int NT>
__global__ __launch_bounds__(256) void conv_bias_act_kernel(const ConvArgs p) {
  constexpr int BN = 32 * NT, BP = BN + 4, NB = (128 * NT + 255) / 256;
  __shared__ float As[kBK * kAP];
  __shared__ __attribute__((aligned(16))) float Bs[kBK * BP];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const long M = (long)p.B * p.OH * p.OW;
  const long m0 = (long)blockIdx.x * kBM;
  const int n0 = blockIdx.y * BN;
  const int pad = (p.ks - 1) >> 1;
  const int ohw = p.OH * p.OW;

  // the two pixels whose 4-channel group kq this thread fetches
  const int kq = t & 3;
  const float* abase[2];
  int iy0[2], ix0[2];
  bool pv[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const long m = m0 + (t >> 2) + 64 * j;
    pv[j] = m < M;
    const long mm = pv[j] ? m : 0;
    const int img = (int)(mm / ohw), rem = (int)(mm - (long)img * ohw);
    const int oy = rem / p.OW, ox = rem - oy * p.OW;
    iy0[j] = oy * p.stride - pad;
    ix0[j] = ox * p.stride - pad;
    abase[j] = p.a + (size_t)img * p.H * p.W * p.lda + 4 * kq;
  }
  const int cchunks = (p.cin + kBK - 1) / kBK;
  const int nchunks = p.ks * p.ks * cchunks;

  float4 ra[2], rb[NB];
  auto fetch = [&](int chunk) {
    const int tap = chunk / cchunks, c0 = (chunk - tap * cchunks) * kBK;
    const int ky = tap / p.ks, kx = tap - ky * p.ks;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int iy = iy0[j] + ky, ix = ix0[j] + kx;
      const bool ok = pv[j] && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W && c0 + 4 * kq < p.cin;
      ra[j] = ok ? *reinterpret_cast<const float4*>(abase[j] + ((size_t)iy * p.W + ix) * p.lda + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = t + 256 * i;
      const int kk = idx / (8 * NT), nq = idx - kk * (8 * NT);
      const int n = n0 + 4 * nq;
      const bool ok = idx < 128 * NT && c0 + kk < p.cin && n < p.ldw;
      rb[i] = ok ? *reinterpret_cast<const float4*>(p.w + ((size_t)tap * p.cin + c0 + kk) * p.ldw + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      float* d = As + (4 * kq) * kAP + (t >> 2) + 64 * j;
      d[0] = ra[j].x;
      d[kAP] = ra[j].y;
      d[2 * kAP] = ra[j].z;
      d[3 * kAP] = ra[j].w;
    }
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      const int idx = t + 256 * i;
      const int kk = idx / (8 * NT), nq = idx - kk * (8 * NT);
      if (idx < 128 * NT) *reinterpret_cast<float4*>(Bs + kk * BP + 4 * nq) = rb[i];
    }
  };

  f32x16 acc[NT], part[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f, part[nt][r] = 0.f;
  int since = 0;

  fetch(0);
  const float* ap = As + (lane >> 5) * kAP + 32 * wave + (lane & 31);
  const float* bp = Bs + (lane >> 5) * BP + (lane & 31);
  for (int chunk = 0; chunk < nchunks; ++chunk) {
    __syncthreads();                     // every wave is done with the previous chunk
    stash();
    __syncthreads();
    if (chunk + 1 < nchunks) fetch(chunk + 1);
#pragma unroll
    for (int s = 0; s < kBK / 2; ++s) {
      const float a = ap[2 * s * kAP];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) part[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(a, bp[2 * s * BP + 32 * nt], part[nt], 0, 0, 0);
    }
    if (++since == p.flush || chunk + 1 == nchunks) {
      since = 0;
#pragma unroll
      for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] += part[nt][r], part[nt][r] = 0.f;
    }
  }

  // accumulator register r of lane l: pixel 32 wave + (r & 3) + 8 (r >> 2) + 4 (l >> 5), channel 32 nt + (l & 31)
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const long m = m0 + 32 * wave + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
    if (m >= M) continue;
    const int img = (int)(m / ohw), rem = (int)(m - (long)img * ohw);
    const int oy = rem / p.OW, ox = rem - oy * p.OW;
    float* crow = p.c + (size_t)((long)img * p.c_img_rows + p.c_row0 + rem) * p.ldc;
    const float* rrow = p.res ? p.res + (size_t)m * p.ldr : nullptr;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
      const int n = n0 + 32 * nt + (lane & 31);
      if (n >= p.cout) continue;
      float v = acc[nt][r] + (p.bias ? p.bias[n] : 0.f);
      if (p.act == GDRNPP_ACT_SILU) {
        v = v / (1.f + expf(-v));
      } else if (p.act == GDRNPP_ACT_SIGMOID) {
        v = 1.f / (1.f + expf(-v));
      } else if (p.act == GDRNPP_ACT_YOLOX_BOX) {
        v = n < 2 ? (v + (float)(n == 0 ? ox : oy)) * p.dec_stride : expf(v) * p.dec_stride;
      }
      if (rrow) v += rrow[n];
      crow[n] = v;
    }
  }
}

// x f32[B,3,H,W] -> y[B,H/2,W/2, slice of 12]: channel 3 q + c with q = top-left, bottom-left, top-right, bottom-right
__global__ __launch_bounds__(256) void focus_kernel(const float* __restrict__ x, float* __restrict__ y, int ldy, int B, int H, int W) {
  const int oh = H >> 1, ow = W >> 1;
  const long total = (long)B * oh * ow * 12;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int ch = (int)(i % 12);
  const long pix = i / 12;
  const int ox = (int)(pix % ow), oy = (int)((pix / ow) % oh), b = (int)(pix / ((long)ow * oh));
  const int q = ch / 3, c = ch - 3 * q;
  const int dy = q & 1, dx = q >> 1;
  y[(size_t)pix * ldy + ch] = x[(((size_t)b * 3 + c) * H + 2 * oy + dy) * W + 2 * ox + dx];
}

// buf[B,H,W,ld]: channels [0, C) of the (pre-offset) slice -> max over the 5x5, 9x9, 13x13 windows into [C, 2C), [2C, 3C), [3C, 4C).
// One pass over the 13x13 window; the two inner windows are its sub-windows (max is exact and order-free); taps outside the
// image do not take part (nn.MaxPool2d pads with -inf).
__global__ __launch_bounds__(256) void spp_kernel(float* buf, int ld, int C, int B, int H, int W) {
  const long total = (long)B * H * W * C;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C);
  const long pix = i / C;
  const int x = (int)(pix % W), y = (int)((pix / W) % H), b = (int)(pix / ((long)W * H));
  const float* src = buf + (size_t)b * H * W * ld + c;
  float m5 = -INFINITY, m9 = -INFINITY, m13 = -INFINITY;
  for (int dy = -6; dy <= 6; ++dy) {
    const int yy = y + dy;
    if (yy < 0 || yy >= H) continue;
    const int ady = dy < 0 ? -dy : dy;
    for (int dx = -6; dx <= 6; ++dx) {
      const int xx = x + dx;
      if (xx < 0 || xx >= W) continue;
      const int adx = dx < 0 ? -dx : dx;
      const float v = src[((size_t)yy * W + xx) * ld];
      m13 = fmaxf(m13, v);
      if (ady <= 4 && adx <= 4) m9 = fmaxf(m9, v);
      if (ady <= 2 && adx <= 2) m5 = fmaxf(m5, v);
    }
  }
  float* dst = buf + (size_t)pix * ld + c;
  dst[C] = m5;
  dst[2 * C] = m9;
  dst[3 * C] = m13;
}

// x[B,h,w, slice of C] -> y[B,2h,2w, slice of C], nearest; four channels per thread
__global__ __launch_bounds__(256) void upsample2x_kernel(const float* __restrict__ x, int ldx, float* __restrict__ y, int ldy, int B,
                                                         int h, int w, int C4) {
  const long total = (long)B * 4 * h * w * C4;
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int c4 = (int)(i % C4);
  const long pix = i / C4;
  const int ox = (int)(pix % (2 * w)), oy = (int)((pix / (2 * w)) % (2 * h)), b = (int)(pix / ((long)4 * w * h));
  const float4 v = *reinterpret_cast<const float4*>(x + (((size_t)b * h + (oy >> 1)) * w + (ox >> 1)) * ldx + 4 * c4);
  *reinterpret_cast<float4*>(y + (size_t)pix * ldy + 4 * c4) = v;
}

}  // namespace

extern "C" {

int gdrnpp_conv_bias_act_f32(const float* a, int lda, int a_off, const float* w, int ldw, const float* bias, const float* res, int ldr,
                             int r_off, float* c, int ldc, int c_off, long c_img_rows, long c_row0, int B, int H, int W, int cin,
                             int cout, int ks, int stride, int act, float dec_stride, void* stream) {
  GDRNPP_REQUIRE(a && w && c, GDRNPP_EINVAL, "gdrnpp_conv_bias_act_f32: null pointer");
  GDRNPP_REQUIRE(B > 0 && H > 0 && W > 0 && cin > 0 && cout > 0, GDRNPP_EINVAL,
                 "gdrnpp_conv_bias_act_f32: B=%d H=%d W=%d cin=%d cout=%d must be positive", B, H, W, cin, cout);
  GDRNPP_REQUIRE((ks == 1 || ks == 3) && (stride == 1 || stride == 2), GDRNPP_EINVAL,
                 "gdrnpp_conv_bias_act_f32: kernel size %d (1 or 3) stride %d (1 or 2)", ks, stride);
  GDRNPP_REQUIRE(cin % 4 == 0 && lda % 4 == 0 && a_off % 4 == 0 && a_off >= 0 && a_off + cin <= lda, GDRNPP_EINVAL,
                 "gdrnpp_conv_bias_act_f32: cin=%d, lda=%d and a_off=%d must be multiples of 4 with a_off + cin <= lda", cin, lda, a_off);
  GDRNPP_REQUIRE(ldw % 4 == 0 && ldw >= cout, GDRNPP_EINVAL, "gdrnpp_conv_bias_act_f32: ldw=%d (a multiple of 4, >= cout=%d)", ldw, cout);
  GDRNPP_REQUIRE(c_off >= 0 && c_off + cout <= ldc, GDRNPP_EINVAL,
                 "gdrnpp_conv_bias_act_f32: the output slice overruns its buffer (c_off=%d + cout=%d > ldc=%d)", c_off, cout, ldc);
  GDRNPP_REQUIRE(!res || (r_off >= 0 && r_off + cout <= ldr), GDRNPP_EINVAL,
                 "gdrnpp_conv_bias_act_f32: the residual slice overruns its buffer (r_off=%d + cout=%d > ldr=%d)", r_off, cout, ldr);
  GDRNPP_REQUIRE(act >= GDRNPP_ACT_NONE && act <= GDRNPP_ACT_YOLOX_BOX, GDRNPP_EINVAL, "gdrnpp_conv_bias_act_f32: activation %d (0 .. 3)", act);
  GDRNPP_REQUIRE(act != GDRNPP_ACT_YOLOX_BOX || (cout == 4 && !res), GDRNPP_EINVAL,
                 "gdrnpp_conv_bias_act_f32: the box decode takes cout=4 and no residual (cout=%d)", cout);
  const int pad = (ks - 1) / 2;
  const int OH = (H + 2 * pad - ks) / stride + 1, OW = (W + 2 * pad - ks) / stride + 1;
  const long ohw = (long)OH * OW;
  if (c_img_rows == 0) {
    GDRNPP_REQUIRE(c_row0 == 0, GDRNPP_EINVAL, "gdrnpp_conv_bias_act_f32: c_row0=%ld without c_img_rows", c_row0);
    c_img_rows = ohw;
  }
  GDRNPP_REQUIRE(c_row0 >= 0 && c_row0 + ohw <= c_img_rows, GDRNPP_EINVAL,
                 "gdrnpp_conv_bias_act_f32: rows %ld .. %ld of an image of %ld output rows", c_row0, c_row0 + ohw, c_img_rows);
  const long M = (long)B * ohw;
  const long mtiles = (M + kBM - 1) / kBM;
  GDRNPP_REQUIRE(mtiles < (1l << 30) && (long)B * H * W < (1l << 31), GDRNPP_ELIMIT, "gdrnpp_conv_bias_act_f32: problem too large (B=%d H=%d W=%d)", B, H, W);
  // N tile: the width that pads cout least (ties: the wider, which reads A fewer times), halved while the grid leaves CUs empty
  int nt = 4;
  {
    long best = -1;
    for (int cand = 4; cand >= 1; cand >>= 1) {
      const long padded = (long)((cout + 32 * cand - 1) / (32 * cand)) * 32 * cand;
      if (best < 0 || padded < best) best = padded, nt = cand;
    }
    while (nt > 1 && mtiles * ((cout + 32 * nt - 1) / (32 * nt)) < 256) nt >>= 1;
  }
  ConvArgs p;
  p.a = a + a_off;
  p.w = w;
  p.bias = bias;
  p.res = res ? res + r_off : nullptr;
  p.c = c + c_off;
  p.B = B, p.H = H, p.W = W, p.OH = OH, p.OW = OW, p.cin = cin, p.cout = cout, p.ldw = ldw, p.ks = ks, p.stride = stride;
  p.lda = lda, p.ldc = ldc, p.ldr = ldr, p.act = act;
  p.c_img_rows = c_img_rows, p.c_row0 = c_row0, p.dec_stride = dec_stride;
  p.flush = (int)lround(sqrt((double)ks * ks * cin) / kBK);      // chunks per partial sum: both levels about sqrt(K) long
  if (p.flush < 1) p.flush = 1;
  const dim3 grid((unsigned)mtiles, (unsigned)((cout + 32 * nt - 1) / (32 * nt)));
  if (nt == 4)
    hipLaunchKernelGGL(conv_bias_act_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else if (nt == 2)
    hipLaunchKernelGGL(conv_bias_act_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, p);
  else
    hipLaunchKernelGGL(conv_bias_act_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p);
  return gdrnpp::check_launch("gdrnpp_conv_bias_act_f32");
}

int gdrnpp_yolox_focus(const float* x_nchw, float* y, int ldy, int y_off, int B, int H, int W, void* stream) {
  GDRNPP_REQUIRE(x_nchw && y, GDRNPP_EINVAL, "gdrnpp_yolox_focus: null pointer");
  GDRNPP_REQUIRE(B > 0 && H > 0 && W > 0 && H % 2 == 0 && W % 2 == 0, GDRNPP_EINVAL, "gdrnpp_yolox_focus: B=%d H=%d W=%d (positive, H and W even)", B, H, W);
  GDRNPP_REQUIRE(y_off >= 0 && y_off + 12 <= ldy, GDRNPP_EINVAL, "gdrnpp_yolox_focus: the output slice overruns its buffer (y_off=%d + 12 > ldy=%d)", y_off, ldy);
  const long total = (long)B * (H / 2) * (W / 2) * 12;
  GDRNPP_REQUIRE(total < (1l << 38), GDRNPP_ELIMIT, "gdrnpp_yolox_focus: problem too large");
  hipLaunchKernelGGL(focus_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x_nchw, y + y_off, ldy, B, H, W);
  return gdrnpp::check_launch("gdrnpp_yolox_focus");
}

int gdrnpp_spp_maxpool_5_9_13(float* buf, int ld, int off, int C, int B, int H, int W, void* stream) {
  GDRNPP_REQUIRE(buf, GDRNPP_EINVAL, "gdrnpp_spp_maxpool_5_9_13: null pointer");
  GDRNPP_REQUIRE(B > 0 && H > 0 && W > 0 && C > 0, GDRNPP_EINVAL, "gdrnpp_spp_maxpool_5_9_13: B=%d H=%d W=%d C=%d must be positive", B, H, W, C);
  GDRNPP_REQUIRE(off >= 0 && (long)off + 4l * C <= ld, GDRNPP_EINVAL,
                 "gdrnpp_spp_maxpool_5_9_13: the four slices overrun the buffer (off=%d + 4 * C=%d > ld=%d)", off, C, ld);
  const long total = (long)B * H * W * C;
  GDRNPP_REQUIRE(total < (1l << 38), GDRNPP_ELIMIT, "gdrnpp_spp_maxpool_5_9_13: problem too large");
  hipLaunchKernelGGL(spp_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, buf + off, ld, C, B, H, W);
  return gdrnpp::check_launch("gdrnpp_spp_maxpool_5_9_13");
}

int gdrnpp_upsample_nearest2x_slice(const float* x, int ldx, int x_off, float* y, int ldy, int y_off, int B, int h, int w, int C,
                                    void* stream) {
  GDRNPP_REQUIRE(x && y, GDRNPP_EINVAL, "gdrnpp_upsample_nearest2x_slice: null pointer");
  GDRNPP_REQUIRE(B > 0 && h > 0 && w > 0 && C > 0, GDRNPP_EINVAL, "gdrnpp_upsample_nearest2x_slice: B=%d h=%d w=%d C=%d must be positive", B, h, w, C);
  GDRNPP_REQUIRE(C % 4 == 0 && ldx % 4 == 0 && x_off % 4 == 0 && ldy % 4 == 0 && y_off % 4 == 0, GDRNPP_EINVAL,
                 "gdrnpp_upsample_nearest2x_slice: C=%d, ldx=%d, x_off=%d, ldy=%d, y_off=%d must be multiples of 4", C, ldx, x_off, ldy, y_off);
  GDRNPP_REQUIRE(x_off >= 0 && x_off + C <= ldx && y_off >= 0 && y_off + C <= ldy, GDRNPP_EINVAL,
                 "gdrnpp_upsample_nearest2x_slice: a slice overruns its buffer (x_off=%d, y_off=%d, C=%d, ldx=%d, ldy=%d)", x_off, y_off, C, ldx, ldy);
  const long total = (long)B * 4 * h * w * (C / 4);
  GDRNPP_REQUIRE(total < (1l << 38), GDRNPP_ELIMIT, "gdrnpp_upsample_nearest2x_slice: problem too large");
  hipLaunchKernelGGL(upsample2x_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x + x_off, ldx, y + y_off, ldy,
                     B, h, w, C / 4);
  return gdrnpp::check_launch("gdrnpp_upsample_nearest2x_slice");
}

}  // extern "C"
