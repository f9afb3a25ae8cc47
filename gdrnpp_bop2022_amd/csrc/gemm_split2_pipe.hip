// Three-product form of the split GEMM ("fp16x2"): the default of the ConvNeXt MLPs, the convolutions of the head / downsample
// layers / Patch-PnP and the transposed-convolution GEMM where a launch has at least 256 tiles of 256x128
// (hip_layers.set_gemm_products; entry points gdrnpp_linear_f32_split2 / gdrnpp_conv3x3_f32_split2 / gdrnpp_conv2d_f32_split2)
// — SURVEY.md §8 row a3.
//
// Numerical scheme.  Every fp32 operand is written as x = h + l + e with h = rn_f16(x), l = rn_f16(x - h) (the subtraction is
// exact) and |e| <= 2^-22 |x| as long as l stays in the normal fp16 range (else |e| <= 2^-25 absolute): 22 significant bits in
// two fp16 values.  Three of the four partial products go through v_mfma_f32_32x32x16_f16 with fp32 accumulation
// (h*l, l*h, h*h, small terms first); l*l (2^-22 relative) is dropped.  fp16 products are exact in fp32, so what is lost
// against the six-product bf16x3 form (gemm_split.hip: exact to 2^-26) is the operand representation: 1.3e-7 .. 2.2e-7 of the
// output scale (the same three products evaluated in fp64).  On operands with outlier channels (ConvNeXt activations) that sits
// below the error every fp32-accumulating GEMM makes in its accumulation chain: measured against fp64 at K = 128 .. 4096 the
// three-product result carries 3.9e-7 .. 3.0e-6, the six-product form 4.8e-7 .. 3.0e-6, hipBLASLt's fp32 GEMM 6.2e-7 .. 3.9e-6
// (tools/split2_error_probe.py, profiles/r03y_split2_accuracy.txt; tests/test_gpu_split2.py pins the three against each other), and
// the network outputs sit at the same 4e-6 .. 8e-6 from the reference's recorded forward with any of the three engines.
// Half the matrix-pipe work of the six-product form for the accuracy of the arithmetic the reference itself runs in.
//
// Range.  fp16 has 5 exponent bits, so the operands are brought into range by exact power-of-two scaling:
//   * weights: gdrnpp_pack_weight_f16x2 scales the tensor by 2^e with max|w| * 2^e in [2^13, 2^14) before splitting and stores
//     2^-e behind the packed tiles; the epilogue multiplies the accumulator by it (exact);
//   * activations are split as they are: |x| up to 65504 is representable, elements below 2^-2 lose l's low bits to the fp16
//     subnormal spacing (absolute error 2^-25, i.e. still 2^-22 of any tensor whose scale is 2^-3 or more — LayerNorm /
//     GroupNorm / GELU outputs).  An activation beyond 65504 becomes inf and the output non-finite: the epilogue checks every
//     value it stores and raises bit 0 of the launch's range word (the range_flag argument: one word per layer and stream on
//     the Python side);
//   * the small side is checked on every launch as well, per A row: the k-loop accumulates the sum of squares of the row's h
//     halves (v_dot2c_f32_f16, 8 per k-tile and wave), and a row that is not all zero with rms below 2^-4 raises bit 1 — below
//     that scale the 2^-25 absolute operand error of the subnormal l would exceed 2^-21 of the row's own output scale (zero-padded
//     taps of a convolution count as zeros; so does a row whose every element is below half the fp16 subnormal spacing, 3e-8:
//     its h and l are all zero, what it would have contributed — less than 3e-8 * sum|w| — is dropped, which is the 2^-25 absolute
//     operand error again).  A non-finite A element makes the sum non-finite and raises bit 0.
//   On either bit the host side re-runs the step in the six-product form and keeps the flagged layer there
//   (engine.run_with_range_check) — never silently wrong, on either side of the range, on every launch;
//   * weights: gdrnpp_pack_weight_f16x2 applies the same per-row test to the scaled weight rows (trailer word 3); such a layer
//     is not eligible for this form (x3_policy.six_product_weight).
//
// Kernel: the software-pipelined LDS-DMA kernel of gemm_split_pipe.hip with 24 instead of 48 MFMA slots per k-tile: block tile
// 256x128x16, 4 waves stacked along M (2 x 4 MFMA tiles each), fp32 A by LDS-DMA into three 16 KB stages private to the waves,
// pre-packed fp16 weight tiles (8 KB: [split][k-block][128][8]) by LDS-DMA into four slots (k-tile kt in slot kt & 3, the DMA two
// k-tiles ahead), the split of k-tile t+1 (cvt_pk, v_fma_mix_f32 residual, cvt_pk: 32 VALU operations) spread over the MFMA
// slots of k-tile t, both weight fragment sets read just in time (l behind slot 19 of the previous k-tile, h in slots 1 and 3),
// one barrier per two k-tiles behind slot 19 of the odd one.  80 KB of dynamic LDS (three A stages, four weight slots), two
// workgroups per CU.  Linear form, the 3x3 / stride 1 / pad 1 convolution and the general K x K / stride / pad convolution
// (implicit im2col, k-tile order of gemm_split.hpp), optional GroupNorm statistics in the epilogue (GnStats,
// split_gemm_device.hpp).  -DGDRNPP2_TIMING_NO_{BREAD,SPLIT,SYNC,DMA}, -DGDRNPP2_NO_RANGE_CHECK: timing-only builds (results
// invalid) that take one component out of the k-loop (profiles/r03y_split2_kloop_dissection.txt).  At W = 16 / 32 / 64 the 3x3
// convolution runs conv3x3_window_kernel below, which stages the input once per 16-channel chunk instead of once per tap (library
// option "conv3x3_window", profiles/conv3x3_window.md).  The alternatives this kernel
// was measured against are retired (docs/DESIGN_HISTORY.md, "Retired variants").
#include "split2_common.hpp"

namespace {

using namespace gdrnpp::split2;

constexpr int NA = 3;                          // A stages: the A DMA runs two k-tiles ahead
constexpr int A_STAGE_B = 256 * BK * 4;        // fp32 A image of one k-tile: 16 KB
constexpr int W2_TILE_SLOTS = 2 * KB * BN;     // uint4 slots of one packed 128x16 fp16x2 weight tile
constexpr int W2_TILE_B = W2_TILE_SLOTS * 16;  // 8 KB
constexpr int NB = 4;                          // weight slots: k-tile kt in slot kt & 3, the weight DMA runs two k-tiles ahead
constexpr int NJ = 4;                          // 32-column MFMA tiles per wave: the block tile is 256 x 128
constexpr int LDS_BYTES = NA * A_STAGE_B + NB * W2_TILE_B;   // 80 KB: two workgroups fill the CU's 160 KB

__device__ int g_split2_range_word;  // sticky range word (GDRNPP_SPLIT2_NONFINITE | GDRNPP_SPLIT2_SMALL_ROWS) of launches that pass no word of their own

// One half of a wave's A tile for one k-tile: 32 rows x 16 k, 8 consecutive k of one row per lane.  x ~ h + l in 8 steps of two
// VALU operations (the residual overwrites x).  APRE: A is an "f16x2 rows" tensor (split2_common.hpp) — the two 16-byte chunks the
// lane reads ARE its h and l fragments, there is nothing to split.
template <bool APRE>
struct HalfSplit2T {
  float x[APRE ? 1 : 8];
  unsigned h[4], l[4];

  template <int S>
  __device__ __forceinline__ void step() {
    if constexpr (APRE) {
    } else if constexpr (S < 2) {
      h[2 * S] = cvt_pk_f16(x[4 * S], x[4 * S + 1]);
      h[2 * S + 1] = cvt_pk_f16(x[4 * S + 2], x[4 * S + 3]);
    } else if constexpr (S < 6) {
      constexpr int p = S - 2;
      x[2 * p] = residual<0>(x[2 * p], h[p]);
      x[2 * p + 1] = residual<1>(x[2 * p + 1], h[p]);
    } else {
      constexpr int q = S - 6;
      l[2 * q] = cvt_pk_f16(x[4 * q], x[4 * q + 1]);
      l[2 * q + 1] = cvt_pk_f16(x[4 * q + 2], x[4 * q + 3]);
    }
  }
  __device__ __forceinline__ void load(const uint4* lds, int slot0, int slot1) {
    if constexpr (APRE) {
      const uint4 a = lds[slot0], b = lds[slot1];
      h[0] = a.x; h[1] = a.y; h[2] = a.z; h[3] = a.w;
      l[0] = b.x; l[1] = b.y; l[2] = b.z; l[3] = b.w;
    } else {
      const float4 a = __builtin_bit_cast(float4, lds[slot0]), b = __builtin_bit_cast(float4, lds[slot1]);
      x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
      x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
    }
  }
  template <int SPLIT>
  __device__ __forceinline__ f16x8 frag() const {
    const unsigned* s = SPLIT == 0 ? h : l;
    return __builtin_bit_cast(f16x8, make_uint4(s[0], s[1], s[2], s[3]));
  }
};

// W f32[N][K] -> packed fp16 [N/128][K/16][2][2][128][8]; one thread per (row, k-block) = 8 consecutive k.
// trailer (16 B behind the tiles): {amax bits, 2^-e, 2^e, rows-below-range bit (weight_rows_range_kernel)}
__global__ void pack_weight2_kernel(const float* __restrict__ W, uint4* __restrict__ packed, int N, int K) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int kbs = K / 8;
  unsigned* trailer = reinterpret_cast<unsigned*>(packed + (size_t)(N / BN) * (K / BK) * W2_TILE_SLOTS);
  const int e = weight_exp(trailer[0]);
  const float sc = __builtin_ldexpf(1.f, e);
  if (i == 0) {
    trailer[1] = __float_as_uint(__builtin_ldexpf(1.f, -e));
    trailer[2] = __float_as_uint(sc);
    trailer[3] = 0u;
  }
  if (i >= (long)N * kbs) return;
  const int n = (int)(i / kbs), kb_g = (int)(i % kbs);
  const float4 v0 = *reinterpret_cast<const float4*>(W + (size_t)n * K + kb_g * 8);
  const float4 v1 = *reinterpret_cast<const float4*>(W + (size_t)n * K + kb_g * 8 + 4);
  const float x[8] = {v0.x * sc, v0.y * sc, v0.z * sc, v0.w * sc, v1.x * sc, v1.y * sc, v1.z * sc, v1.w * sc};
  unsigned h[4], l[4];
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    h[p] = cvt_pk_f16(x[2 * p], x[2 * p + 1]);
    const f16x2 hv = __builtin_bit_cast(f16x2, h[p]);
    l[p] = cvt_pk_f16(x[2 * p] - (float)hv[0], x[2 * p + 1] - (float)hv[1]);
  }
  const int tn = n / BN, row = n % BN, tk = kb_g / KB, kb = kb_g % KB;
  uint4* img = packed + ((size_t)tn * (K / BK) + tk) * W2_TILE_SLOTS;
  img[(0 * KB + kb) * BN + row] = make_uint4(h[0], h[1], h[2], h[3]);
  img[(1 * KB + kb) * BN + row] = make_uint4(l[0], l[1], l[2], l[3]);
}

// CONV: 0 = linear (A row-major [M,K]), 1 = 3x3 / stride 1 / pad 1 convolution over an NHWC image (geometry folded at compile
//       time), 2 = any KH x KW / stride / zero padding with at most 32 taps (ConvNeXt's 2x2/2 downsamples, Patch-PnP's 3x3/2)
// GNS: GroupNorm (sum, sum of squares) partials of the stored result per wave (64 rows x 8-channel groups), CONV only
// APRE: A is an "f16x2 rows" tensor (linear form only).  c_rows (run time): C is written as one (bias / GELU epilogues).
template <int EPI, int CONV, bool GNS, bool APRE = false>
__global__ __launch_bounds__(256, 2) void gemm_split2_pipe_kernel(const float* __restrict__ A, const uint4* __restrict__ Wp,
                                                                  const float* __restrict__ bias,
                                                                  const float* __restrict__ gamma,
                                                                  const float* __restrict__ resid, float* __restrict__ C,
                                                                  int M, int N, int K, ConvGeom cg, int panel, GnStats gn, int* range_flag, int c_rows) {
  static_assert(!APRE || CONV == 0, "f16x2-rows A: linear form only");
  using HalfSplit2 = HalfSplit2T<APRE>;
  constexpr int NS = 6 * NJ;   // MFMA slots per k-tile: 24
  constexpr int SB = 19;       // slot of the wait (and, in odd k-tiles, the barrier): behind it two slots of weight fragment
                               // reads and one raw A read
  extern __shared__ uint4 smem[];  // the only LDS object: [NA][1024] A slots | [NB][512] weight slots
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntn = N / BN;
  const TileMN tile = tile_coords(xcd_tile_id(), ntn, panel, M);   // panel order for wide layers, see launch_split_pipe (gemm_split_pipe.hip)
  const int tile_n = tile.n, m0 = tile.m * 256, n0 = tile_n * BN;
  const int nk = K / BK;
  const unsigned lds0 = lds_addr(smem);
  const float wsc = reinterpret_cast<const float*>(Wp + (size_t)(N / BN) * nk * W2_TILE_SLOTS)[1];   // 2^-e of the weight scale (trailer)

  // ---- DMA lanes: piece c (0..3) of this wave fills A slots (wave*4 + c)*64 + lane = rows wave*64 + c*16 + lane/4, chunk
  // q = (lane & 3) ^ ((row >> 2) & 3) of the row's 64-byte k segment (the swizzle is on the source address)
  const int prow = lane >> 2, pq = lane & 3;
  unsigned aoff[4];        // linear: byte offset of the lane's chunk from A + kt*64
  const float* ap[4];      // conv: anchor pixel of the lane's row (+ chunk)
  unsigned okmask[4];      // conv: bit tap = the tap lies inside the image
  int cpt = 1;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int lrow = wave * 64 + c * 16 + prow;
    const int q = pq ^ ((lrow >> 2) & 3);
    const int arow = min(m0 + lrow, M - 1);
    if constexpr (CONV == 1) {
      const int img = arow / (cg.H * cg.W), pp = arow - img * (cg.H * cg.W);
      const int iy = pp / cg.W, ix = pp - iy * cg.W;
      ap[c] = A + ((size_t)arow) * cg.C + q * 4;
      unsigned mk = 0;
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int dy = t / 3 - 1, dx = t % 3 - 1;
        if ((unsigned)(iy + dy) < (unsigned)cg.H && (unsigned)(ix + dx) < (unsigned)cg.W) mk |= 1u << t;
      }
      okmask[c] = mk;
      aoff[c] = 0;
    } else if constexpr (CONV == 2) {   // general KH x KW / stride / pad: row = output pixel, anchor = its input pixel (oy*s, ox*s)
      const int img = arow / (cg.OH * cg.OW), pp = arow - img * (cg.OH * cg.OW);
      const int iy = (pp / cg.OW) * cg.stride, ix = (pp % cg.OW) * cg.stride;
      ap[c] = A + (((size_t)img * cg.H + iy) * cg.W + ix) * cg.C + q * 4;
      const int ntaps = K / cg.C;     // <= 32 (checked by the entry point)
      unsigned mk = 0;
      for (int t = 0; t < ntaps; ++t) {
        const int ky = t / cg.KW, dy = ky - cg.pad, dx = t - ky * cg.KW - cg.pad;
        if ((unsigned)(iy + dy) < (unsigned)cg.H && (unsigned)(ix + dx) < (unsigned)cg.W) mk |= 1u << t;
      }
      okmask[c] = mk;
      aoff[c] = 0;
    } else {
      aoff[c] = (unsigned)arow * (unsigned)(K * 4) + (unsigned)(q * 16);
      ap[c] = nullptr;
      okmask[c] = 0;
    }
  }
  if constexpr (CONV) cpt = cg.C / BK;
  const int ntaps = CONV == 1 ? 9 : (CONV == 2 ? K / cg.C : 1), ckw = CONV == 1 ? 3 : cg.KW, cpad = CONV == 1 ? 1 : cg.pad;
  const unsigned boff = (unsigned)((wave * 2) * 64 + lane) * 16u;
  const char* const wbase = reinterpret_cast<const char*>(Wp + (size_t)tile_n * nk * W2_TILE_SLOTS);
  const unsigned ldsA = lds0 + (unsigned)(wave * 4) * 1024u;
  const unsigned ldsB = lds0 + (unsigned)(NA * A_STAGE_B) + (unsigned)(wave * 2) * 1024u;

  // piece c of the A image of k-tile kt -> stage byte offset sb
  auto dma_a = [&](int kt, unsigned sb, auto cc) {
    constexpr int c = decltype(cc)::value;
    if constexpr (CONV) {
      GDRNPP_CONV_KTILE(kt, cpt, ntaps);
      const int c0 = chunk * BK;
      const int ky = tap / ckw, dy = ky - cpad, dx = tap - ky * ckw - cpad;
      const long off = ((long)dy * cg.W + dx) * cg.C + c0;
      const bool ok = (okmask[c] >> tap) & 1u;
      dma_v(ok ? (const void*)(ap[c] + off) : (const void*)g_zero_page, ldsA + sb + c * 1024u);
    } else {
      dma_s(aoff[c], reinterpret_cast<const char*>(A) + (size_t)kt * (BK * 4), ldsA + sb + c * 1024u);
    }
  };
  auto dma_b = [&](int kt, unsigned sb, auto cc) {
    constexpr int c = decltype(cc)::value;
    int wkt = kt;
    if constexpr (CONV) {
      GDRNPP_CONV_KTILE(kt, cpt, ntaps);
      wkt = tap * cpt + chunk;
    }
    // piece c = half c of this wave's 2 KB share of the packed weight tile
    dma_s(boff, wbase + ((size_t)wkt * W2_TILE_B + c * 1024), ldsB + sb + (unsigned)(c * 1024));
  };

  f32x16 acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // ---- fragment lanes: MFMA operand lane = row/column (lane & 31), k-block fk = lane >> 5
  const int frow = lane & 31, fk = lane >> 5;
  const int lrow0 = wave * 64 + frow, g0 = (lrow0 >> 2) & 3;  // rows +32 (second half) have the same swizzle
  const int aslot0 = 4 * lrow0 + ((2 * fk) ^ g0), aslot1 = 4 * lrow0 + ((2 * fk + 1) ^ g0);
  const uint4* const sA = smem;
  const uint4* const sBf = smem + NA * (A_STAGE_B / 16) + fk * BN + frow;

  auto load_half = [&](HalfSplit2& hs, int stage, int half) {
    hs.load(sA + stage * (A_STAGE_B / 16) + half * 128, aslot0, aslot1);
  };

  // fragment slot of column tile J, split plane P, relative to sBf (+ weight slot)
  auto bslot = [](int P, int J) { return P * KB * BN + J * 32; };

  // range check: per lane the sum of squares of the h halves it has multiplied (row frow / frow + 32 of the wave, k-blocks fk),
  // two accumulators per row half; -DGDRNPP2_NO_RANGE_CHECK: timing-only build without it
  [[maybe_unused]] float ssq[4] = {0.f, 0.f, 0.f, 0.f};

  // One k-tile, NS = 24 slots (slot S: product group G = S / 8 in the order h*l, l*h, h*h; row half I, column tile J).
  // cur: split A fragments of k-tile kt; nxt: receives the split of k-tile kt+1 (its raw first half is already in nxt[0].x).
  // fbL holds the weight split l of kt on entry (dead after slot 7, refilled with the split l of kt+1 behind slot SB); fbH is
  // read in slots 1 and 3 and used from slot 8.  ODD: parity of kt (compile time).  The workgroup meets at ONE barrier per TWO
  // k-tiles, behind slot SB of the odd one: the weight slots a pair of k-tiles reads were complete at the previous barrier, the
  // slots its DMA fills were last read before it.  Waves of a workgroup may then drift by a whole k-tile.
  // sa1 / sa2 / sa_wr: A stages of kt+1, of kt+2, and the one receiving kt+NA (= the stage kt has left).
  auto ktile = [&](int kt, HalfSplit2 (&cur)[2], HalfSplit2 (&nxt)[2], f16x8 (&fbL)[NJ], f16x8 (&fbH)[NJ], auto odd_, int sa1, int sa2,
                   int sa_wr) {
    constexpr int ODD = decltype(odd_)::value;
    const uint4* const b = sBf + (kt & 3) * (W2_TILE_B / 16);
    const uint4* const bn = sBf + ((kt + 1) & 3) * (W2_TILE_B / 16);
    const int kt_b = min(kt + 2, nk - 1), kt_a = min(kt + NA, nk - 1);
    const unsigned sb_wr = (unsigned)(((kt + 2) & 3) * W2_TILE_B), sa_wr_b = (unsigned)(sa_wr * A_STAGE_B);
    static_for<0, NS>([&](auto s_) {
      constexpr int S = decltype(s_)::value;
      constexpr int G = S / (2 * NJ), I = (S % (2 * NJ)) / NJ, J = S % NJ;
      const f16x8 fa = (G == 1) ? cur[I].template frag<1>() : cur[I].template frag<0>();
      const f16x8 fb = (G == 0) ? fbL[J] : fbH[J];
      acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc[I][J], 0, 0, 0);
      // weight DMA of k-tile kt+2 (slots 0, 2), then A DMA of k-tile kt+NA (slots 4 .. 10; the A pieces are the newest four
      // loads at the wait)
#ifndef GDRNPP2_TIMING_NO_DMA
      if constexpr (S % 2 == 0 && S < 4) dma_b(kt_b, sb_wr, std::integral_constant<int, S / 2>{});
      if constexpr (S % 2 == 0 && S >= 4 && S < 12) dma_a(kt_a, sa_wr_b, std::integral_constant<int, (S - 4) / 2>{});
#endif
#ifndef GDRNPP2_TIMING_NO_BREAD   // timing-only builds (results invalid)
      if constexpr (S % 2 == 1 && S < NJ) {   // weight split h of kt
        constexpr int j0 = S - 1;
        fbH[j0] = __builtin_bit_cast(f16x8, b[bslot(0, j0)]);
        fbH[j0 + 1] = __builtin_bit_cast(f16x8, b[bslot(0, j0 + 1)]);
      }
#endif
#ifndef GDRNPP2_NO_RANGE_CHECK
      // sums of squares of cur's h halves in the four slots without split arithmetic (cur[..].h stays live through group
      // h*h); the fastest of the placements measured in profiles/r04c_range_check_slots.txt
      {
        constexpr int rc[4] = {0, 2, 11, 12};
        if constexpr (S == rc[0]) { ssq[2] = sumsq2(cur[1].h[0], ssq[2]); ssq[3] = sumsq2(cur[1].h[1], ssq[3]); }
        if constexpr (S == rc[1]) { ssq[2] = sumsq2(cur[1].h[2], ssq[2]); ssq[3] = sumsq2(cur[1].h[3], ssq[3]); }
        if constexpr (S == rc[2]) { ssq[0] = sumsq2(cur[0].h[0], ssq[0]); ssq[1] = sumsq2(cur[0].h[1], ssq[1]); }
        if constexpr (S == rc[3]) { ssq[0] = sumsq2(cur[0].h[2], ssq[0]); ssq[1] = sumsq2(cur[0].h[3], ssq[1]); }
      }
#endif
      constexpr int S1 = 13;   // first split slot of the second row half (its raw read four slots earlier).  Declared here and
                               // not beside SB: from there the f16x2-rows kernels come out with other register numbers
      if constexpr (S == S1 - 4) load_half(nxt[1], sa1, 1);   // APRE: nxt[1].h / .l directly (dead since the previous k-tile)
      // split of the next k-tile: first half in slots 3..10, second half in slots S1..S1+7
#ifndef GDRNPP2_TIMING_NO_SPLIT
      if constexpr (S >= 3 && S < 11) nxt[0].template step<S - 3>();
      if constexpr (S >= S1 && S < S1 + 8) nxt[1].template step<S - S1>();
#else
      if constexpr (S == 3) { nxt[0].h[0] = __float_as_uint(nxt[0].x[0]); nxt[0].h[1] = __float_as_uint(nxt[0].x[1]); nxt[0].h[2] = __float_as_uint(nxt[0].x[2]); nxt[0].h[3] = __float_as_uint(nxt[0].x[3]);
                              nxt[0].l[0] = __float_as_uint(nxt[0].x[4]); nxt[0].l[1] = __float_as_uint(nxt[0].x[5]); nxt[0].l[2] = __float_as_uint(nxt[0].x[6]); nxt[0].l[3] = __float_as_uint(nxt[0].x[7]); }
      if constexpr (S == S1) { nxt[1].h[0] = __float_as_uint(nxt[1].x[0]); nxt[1].h[1] = __float_as_uint(nxt[1].x[1]); nxt[1].h[2] = __float_as_uint(nxt[1].x[2]); nxt[1].h[3] = __float_as_uint(nxt[1].x[3]);
                               nxt[1].l[0] = __float_as_uint(nxt[1].x[4]); nxt[1].l[1] = __float_as_uint(nxt[1].x[5]); nxt[1].l[2] = __float_as_uint(nxt[1].x[6]); nxt[1].l[3] = __float_as_uint(nxt[1].x[7]); }
#endif
      if constexpr (S == SB) {
#ifndef GDRNPP2_TIMING_NO_SYNC
        wait_vmcnt<4>();
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): every LDS read of the stages about to be refilled has returned
        if constexpr (ODD) __builtin_amdgcn_s_barrier();
#endif
      }
      // behind slot SB: weight split l of k-tile kt+1 (fbL is dead since slot 7) and the raw first half of k-tile kt+2
      // (cur[0] is nxt[0] of the next k-tile; only cur[0].h / .l are still in use)
      // (APRE: the A read goes first — it IS the operand of slot 0 of the next k-tile, cur[0].h / .l are dead since slots 19 / 11)
      constexpr int SL = APRE ? SB + 1 : SB;         // slot before the first weight read
#ifndef GDRNPP2_TIMING_NO_BREAD
      if constexpr (S > SL && S <= SL + NJ / 2) {
        constexpr int j0 = 2 * (S - SL - 1);
        fbL[j0] = __builtin_bit_cast(f16x8, bn[bslot(1, j0)]);
        fbL[j0 + 1] = __builtin_bit_cast(f16x8, bn[bslot(1, j0 + 1)]);
      }
#endif
      if constexpr (S == (APRE ? SB + 1 : SB + NJ / 2 + 1)) load_half(cur[0], sa2, 0);
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  // ---- prologue: k-tiles 0 .. 2 of A and k-tiles 0, 1 of the weights; split k-tile 0; first fragments of the loop
  HalfSplit2 f0[2], f1[2];
  f16x8 fbL[NJ], fbH[NJ];
  static_for<0, 4>([&](auto c) { dma_a(0, 0u, c); });
  static_for<0, 2>([&](auto c) { dma_b(0, 0u, c); });
  static_for<0, 2>([&](auto c) { dma_b(min(1, nk - 1), (unsigned)W2_TILE_B, c); });
  static_for<0, 4>([&](auto c) { dma_a(min(1, nk - 1), (unsigned)A_STAGE_B, c); });
  static_for<0, 4>([&](auto c) { dma_a(min(2, nk - 1), 2u * A_STAGE_B, c); });
  wait_vmcnt<4>();
  __builtin_amdgcn_s_barrier();
  load_half(f0[0], 0, 0);
  load_half(f0[1], 0, 1);
  static_for<0, 8>([&](auto s) { f0[0].template step<decltype(s)::value>(); f0[1].template step<decltype(s)::value>(); });
#pragma unroll
  for (int j = 0; j < NJ; ++j) fbL[j] = __builtin_bit_cast(f16x8, sBf[bslot(1, j)]);
  load_half(f1[0], 1, 0);

  // ---- main loop, two k-tiles per trip (nk is even: K % 32 == 0)
  int sa = 0;  // kt % NA
  for (int kt = 0; kt < nk; kt += 2) {
    const int sa1 = sa + 1 == NA ? 0 : sa + 1, sa2 = sa1 + 1 == NA ? 0 : sa1 + 1, sa3 = sa2 + 1 == NA ? 0 : sa2 + 1;
    ktile(kt, f0, f1, fbL, fbH, std::integral_constant<int, 0>{}, sa1, sa2, sa);
    ktile(kt + 1, f1, f0, fbL, fbH, std::integral_constant<int, 1>{}, sa2, sa3, sa1);
    sa = sa2;
  }
  wait_vmcnt<0>();               // the clamped A pieces of the last trip are still in flight
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_s_barrier();  // every wave's stages are dead: the epilogue reuses them

  bool bad = false;
#define EPI_TILES_M 2
#define EPI_HALVES (NJ / 2)
#define EPI_ACC(i, j) acc[i][j]
#define EPI_ROW0 m0 + wave * 64
#define EPI_COL0 n0
#define EPI_BIAS bias
#define EPI_STAGE smem
#define EPI_STAGE_BYTES (NA * A_STAGE_B)
#define EPI_SCALE wsc
#define EPI_GN gn
#define EPI_RANGE_BAD bad
#include "split_epilogue_body.hpp"
  // range verdict of the wave's 64 A rows: lanes l and l ^ 32 hold the two k-block halves of rows frow and frow + 32
  bool small = false;
#ifndef GDRNPP2_NO_RANGE_CHECK
  {
    float s0 = ssq[0] + ssq[1], s1 = ssq[2] + ssq[3];
    s0 += __shfl_xor(s0, 32, 64);
    s1 += __shfl_xor(s1, 32, 64);
    const float thr = (float)K * 0x1p-8f;                         // rms 2^-4 over the K elements of the row
    small = (s0 > 0.f && s0 < thr) || (s1 > 0.f && s1 < thr);
    bad |= !(s0 < __builtin_inff()) || !(s1 < __builtin_inff());  // an inf / NaN element of A
  }
#endif
  const int word = (__builtin_amdgcn_ballot_w64(bad) != 0 ? GDRNPP_SPLIT2_NONFINITE : 0) |
                   (__builtin_amdgcn_ballot_w64(small) != 0 ? GDRNPP_SPLIT2_SMALL_ROWS : 0);
  if (word && lane == 0) atomicOr(range_flag ? range_flag : &g_split2_range_word, word);
}

template <int EPI, int CONV, bool GNS, bool APRE = false>
int launch_kernel(const float* A, const uint4* Wp, const float* bias, const float* gamma, const float* resid, float* C, int M, int N,
                  int K, ConvGeom cg, int panel, GnStats gn, int* range_flag, hipStream_t st, const char* what, int c_rows = 0) {
  const int rc = gdrnpp::ensure_dynamic_lds((const void*)gemm_split2_pipe_kernel<EPI, CONV, GNS, APRE>, LDS_BYTES);
  if (rc) return rc;
  const long tiles = (long)((M + 255) / 256) * (N / BN);
  GDRNPP_REQUIRE(tiles < (1l << 30), GDRNPP_ELIMIT, "%s: grid too large", what);
  hipLaunchKernelGGL((gemm_split2_pipe_kernel<EPI, CONV, GNS, APRE>), dim3((unsigned)tiles), dim3(256), LDS_BYTES, st, A, Wp, bias, gamma,
                     resid, C, M, N, K, cg, panel, gn, range_flag, c_rows);
  return gdrnpp::check_launch(what);
}

// a_rows: A is an f16x2-rows tensor; those forms exist for the two MLP layers (GELU / scale + residual)
template <int EPI, int CONV, bool GNS>
int launch_one(const float* A, const uint4* Wp, const float* bias, const float* gamma, const float* resid, float* C, int M, int N,
               int K, ConvGeom cg, int panel, GnStats gn, int* range_flag, hipStream_t st, const char* what, int a_rows = 0, int c_rows = 0) {
  if constexpr (CONV == 0 && EPI != EPI_BIAS) {
    if (a_rows) return launch_kernel<EPI, CONV, GNS, true>(A, Wp, bias, gamma, resid, C, M, N, K, cg, panel, gn, range_flag, st, what, c_rows);
  }
  return launch_kernel<EPI, CONV, GNS>(A, Wp, bias, gamma, resid, C, M, N, K, cg, panel, gn, range_flag, st, what, c_rows);
}

// ---- window-staged form of the 3x3 / stride 1 / pad 1 convolution (library option "conv3x3_window") ---------------------------
// The CONV == 1 form above brings every input pixel of a tile from L2 into LDS nine times, once per tap.  Here the image width W
// (16 / 32 / 64) is a compile-time constant, a tile is 256 / W whole image rows, and all nine taps of a 16-channel chunk read one
// window of the tile's rows plus the row above and the row below: (256 + 2 W) pixels x 64 bytes, staged once per chunk by LDS-DMA
// (24 / 20 / 18 pieces of 1 KB against 9 x 16) and double-buffered.  The window is the run of pixels m0 - W .. m0 + 255 + W of the
// NHWC tensor, so the A fragment of tap (dy, dx) of tile row r is window pixel r + W (1 + dy) + dx: one wave-uniform offset per tap,
// and the swizzle key (pixel >> 2) & 3 — that of the A stages above, applied on the source side of the DMA — is recomputed from that
// pixel.  Halo ROWS outside the image come from g_zero_page (decided per piece: a piece is 16 pixels of one row; no address outside
// the tensor is formed).  There are no halo COLUMNS: left and right of the image the run holds the neighbouring row's pixel, and the
// lanes whose row sits in column 0 / W - 1 replace what they read for a dx = -1 / +1 tap by zeros ahead of the split (8 v_cndmask
// per row half).  Two windows of 24 KB and the four weight slots are the 80 KB of the form above, so the weight protocol (slot
// kt & 3, DMA two k-tiles ahead, one barrier per two k-tiles) is that form's, unchanged.  k order: chunk outer, tap inner
// (kt = 9 chunk + tap; the packed weights are tap-major and are visited as wkt = tap * cpt + chunk).
//
// Window protocol.  Wave w moves pieces j * 4 + w; piece j of the window of chunk c + 1 is issued in slot 4 of k-tile (c, tap j),
// j < 6.  A k-tile that issued one waits with vmcnt(1) behind slot SB (the weights are older), one that did not with vmcnt(0); so
// behind slot SB of (c, 6) every piece of a wave has landed, and the barrier of (c, 6) or (c, 7) — whichever k-tile is odd —
// publishes them ahead of the first read, the one behind slot SB of (c, 7).  The buffer the pieces go to held chunk c - 1, last
// read in slot 9 of (c - 1, 7), ahead of the barrier of (c - 1, 7) or (c - 1, 8).
constexpr int WIN_B = (256 + 2 * 64) * 64;      // bytes of a window buffer (that of W = 64, whatever W): 24 KB
constexpr int WIN_LDS_BYTES = 2 * WIN_B + NB * W2_TILE_B;
static_assert(WIN_LDS_BYTES <= LDS_BYTES, "two workgroups per CU");

// z: the lane's pixel lies outside the image for the tap of this raw fragment (left / right border): it multiplies zeros
__device__ __forceinline__ void zero_raw(HalfSplit2T<false>& hs, bool z) {
#pragma unroll
  for (int i = 0; i < 8; ++i) hs.x[i] = z ? 0.f : hs.x[i];
}

// IW: image width (16 / 32 / 64).  Requires H % (256 / IW) == 0 (a tile is whole rows of one image; M % 256 == 0 follows) and
// Cin % 32 == 0.  Waves, accumulators, row -> lane map, weight slots, epilogue and GnStats partials are those of
// gemm_split2_pipe_kernel<EPI, 1, GNS>.
template <int EPI, int IW, bool GNS>
__global__ __launch_bounds__(256, 2) void conv3x3_window_kernel(const float* __restrict__ A, const uint4* __restrict__ Wp,
                                                                const float* __restrict__ bias, float* __restrict__ C, int M, int N,
                                                                ConvGeom cg, GnStats gn, int* range_flag) {
  using HalfSplit2 = HalfSplit2T<false>;
  constexpr int NS = 6 * NJ, SB = 19, S1 = 13;        // slots of a k-tile as in gemm_split2_pipe_kernel
  constexpr int NPIECES = (256 + 2 * IW) / 16;        // 1 KB pieces (16 pixels) of a window
  constexpr int NPW = (NPIECES + 3) / 4;              // pieces per wave: 6 / 5 / 5
  constexpr int WPMAX = 255 + 2 * IW;                 // last window pixel
  static_assert(NPW <= 6, "the pieces of a window go out in k-tiles 0 .. 5 of the chunk before");
  extern __shared__ uint4 smem[];  // [2][WIN_B / 16] windows | [NB][512] weight slots
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntn = N / BN;
  const TileMN tile = tile_coords(xcd_tile_id(), ntn, 0, M);
  const int tile_n = tile.n, m0 = tile.m * 256, n0 = tile_n * BN;
  const int cpt = cg.C / BK, nk = 9 * cpt, K = 9 * cg.C;
  const unsigned lds0 = lds_addr(smem);
  const float wsc = reinterpret_cast<const float*>(Wp + (size_t)(N / BN) * nk * W2_TILE_SLOTS)[1];
  const float* const gamma = nullptr;   // (names the shared epilogue refers to under epilogues this kernel does not have)
  const float* const resid = nullptr;
  constexpr int c_rows = 0;

  // ---- window DMA: a lane of piece p fills chunk position (lane & 3) of window pixel 16 p + lane / 4 with source chunk
  // (lane & 3) ^ key, key = (pixel >> 2) & 3 = (lane >> 4) & 3
  const int y0 = (m0 % (cg.H * IW)) / IW;             // image row of the tile's first pixel
  const unsigned woff = (unsigned)(lane >> 2) * (unsigned)(cg.C * 4) + (unsigned)(((lane & 3) ^ ((lane >> 4) & 3)) * 16);
  const unsigned zoff = (unsigned)(lane & 3) * 16u;
  // piece j of this wave of the window of chunk `chunk` -> window buffer at LDS byte offset wb
  auto dma_win = [&](int chunk, unsigned wb, int j) {
    const int p = j * 4 + wave;
    if (p < NPIECES) {
      const int y = y0 - 1 + (16 * p) / IW;           // image row of the piece's 16 pixels
      const unsigned dst = lds0 + wb + (unsigned)p * 1024u;
      if ((unsigned)y < (unsigned)cg.H)
        dma_s(woff, A + ((long)m0 - IW + 16 * p) * cg.C + chunk * BK, dst);
      else
        dma_s(zoff, g_zero_page, dst);
    }
  };
  const unsigned boff = (unsigned)((wave * 2) * 64 + lane) * 16u;
  const char* const wbase = reinterpret_cast<const char*>(Wp + (size_t)tile_n * nk * W2_TILE_SLOTS);
  const unsigned ldsB = lds0 + (unsigned)(2 * WIN_B) + (unsigned)(wave * 2) * 1024u;
  auto dma_b = [&](int kt, unsigned sb, auto cc) {
    constexpr int c = decltype(cc)::value;
    const int chunk = kt / 9, tap = kt - 9 * chunk;
    dma_s(boff, wbase + ((size_t)(tap * cpt + chunk) * W2_TILE_B + c * 1024), ldsB + sb + (unsigned)(c * 1024));
  };

  f32x16 acc[2][NJ];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // ---- fragment lanes: MFMA operand lane = tile row (lane & 31) (+ 32 in the second half), k-block fk = lane >> 5
  const int frow = lane & 31, fk = lane >> 5;
  const int lrow0 = wave * 64 + frow;
  const bool edgeL0 = lrow0 % IW == 0, edgeL1 = (lrow0 + 32) % IW == 0;                 // column 0 (row halves 0 / 1)
  const bool edgeR0 = lrow0 % IW == IW - 1, edgeR1 = (lrow0 + 32) % IW == IW - 1;       // column W - 1
  const uint4* const sBf = smem + 2 * (WIN_B / 16) + fk * BN + frow;

  // raw A fragment of row half `half` for k-tile kt (clamped to the last): window pixel = tile row + tap offset
  auto load_half = [&](HalfSplit2& hs, int kt, int half) {
    const int ktc = min(kt, nk - 1), chunk = ktc / 9, tap = ktc - 9 * chunk, ty = tap / 3;
    const int toff = IW * ty + (tap - 3 * ty) - 1;
    // pixels -1 and WPMAX + 1 belong to lanes that are zeroed (tile row 0 / 255, column 0 / W - 1): keep their reads inside the window
    const int wp = min(max(lrow0 + half * 32 + toff, 0), WPMAX);
    const int s0 = 4 * wp + ((2 * fk) ^ ((wp >> 2) & 3));
    hs.load(smem + (chunk & 1) * (WIN_B / 16), s0, s0 ^ 1);
  };
  // dx of k-tile kt (clamped to the last): -1 / +1 = the lanes in column 0 / W - 1 multiply zeros
  auto tap_dx = [&](int kt) {
    const int ktc = min(kt, nk - 1), tap = ktc % 9;
    return tap % 3 - 1;
  };

  auto bslot = [](int P, int J) { return P * KB * BN + J * 32; };
  [[maybe_unused]] float ssq[4] = {0.f, 0.f, 0.f, 0.f};

  // One k-tile: the slot plan of gemm_split2_pipe_kernel's ktile with the window in place of the A stages
  auto ktile = [&](int kt, HalfSplit2 (&cur)[2], HalfSplit2 (&nxt)[2], f16x8 (&fbL)[NJ], f16x8 (&fbH)[NJ], auto odd_) {
    constexpr int ODD = decltype(odd_)::value;
    const uint4* const b = sBf + (kt & 3) * (W2_TILE_B / 16);
    const uint4* const bn = sBf + ((kt + 1) & 3) * (W2_TILE_B / 16);
    const int kt_b = min(kt + 2, nk - 1);
    const unsigned sb_wr = (unsigned)(((kt + 2) & 3) * W2_TILE_B);
    const int chunk = kt / 9, tap = kt - 9 * chunk;
    const bool piece = tap < NPW && tap * 4 + wave < NPIECES && chunk + 1 < cpt;   // wave-uniform
    const int dxn = tap_dx(kt + 1);
    const bool z0 = (dxn < 0 && edgeL0) || (dxn > 0 && edgeR0), z1 = (dxn < 0 && edgeL1) || (dxn > 0 && edgeR1);
    static_for<0, NS>([&](auto s_) {
      constexpr int S = decltype(s_)::value;
      constexpr int G = S / (2 * NJ), I = (S % (2 * NJ)) / NJ, J = S % NJ;
      const f16x8 fa = (G == 1) ? cur[I].template frag<1>() : cur[I].template frag<0>();
      const f16x8 fb = (G == 0) ? fbL[J] : fbH[J];
      acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa, fb, acc[I][J], 0, 0, 0);
      if constexpr (S % 2 == 0 && S < 4) dma_b(kt_b, sb_wr, std::integral_constant<int, S / 2>{});
      if constexpr (S == 4) {
        if (piece) dma_win(chunk + 1, (unsigned)(((chunk + 1) & 1) * WIN_B), tap);
      }
      if constexpr (S % 2 == 1 && S < NJ) {   // weight split h of kt
        constexpr int j0 = S - 1;
        fbH[j0] = __builtin_bit_cast(f16x8, b[bslot(0, j0)]);
        fbH[j0 + 1] = __builtin_bit_cast(f16x8, b[bslot(0, j0 + 1)]);
      }
#ifndef GDRNPP2_NO_RANGE_CHECK
      {
        constexpr int rc[4] = {0, 2, 11, 12};
        if constexpr (S == rc[0]) { ssq[2] = sumsq2(cur[1].h[0], ssq[2]); ssq[3] = sumsq2(cur[1].h[1], ssq[3]); }
        if constexpr (S == rc[1]) { ssq[2] = sumsq2(cur[1].h[2], ssq[2]); ssq[3] = sumsq2(cur[1].h[3], ssq[3]); }
        if constexpr (S == rc[2]) { ssq[0] = sumsq2(cur[0].h[0], ssq[0]); ssq[1] = sumsq2(cur[0].h[1], ssq[1]); }
        if constexpr (S == rc[3]) { ssq[0] = sumsq2(cur[0].h[2], ssq[0]); ssq[1] = sumsq2(cur[0].h[3], ssq[1]); }
      }
#endif
      if constexpr (S == S1 - 4) load_half(nxt[1], kt + 1, 1);
      if constexpr (S == 3) zero_raw(nxt[0], z0);
      if constexpr (S == S1) zero_raw(nxt[1], z1);
      if constexpr (S >= 3 && S < 11) nxt[0].template step<S - 3>();
      if constexpr (S >= S1 && S < S1 + 8) nxt[1].template step<S - S1>();
      if constexpr (S == SB) {
        if (piece) wait_vmcnt<1>(); else wait_vmcnt<0>();
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): every LDS read of what is about to be refilled has returned
        if constexpr (ODD) __builtin_amdgcn_s_barrier();
      }
      if constexpr (S > SB && S <= SB + NJ / 2) {   // weight split l of k-tile kt+1
        constexpr int j0 = 2 * (S - SB - 1);
        fbL[j0] = __builtin_bit_cast(f16x8, bn[bslot(1, j0)]);
        fbL[j0 + 1] = __builtin_bit_cast(f16x8, bn[bslot(1, j0 + 1)]);
      }
      if constexpr (S == SB + NJ / 2 + 1) load_half(cur[0], kt + 2, 0);
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  // ---- prologue: the window of chunk 0, k-tiles 0 and 1 of the weights; split k-tile 0; first fragments of the loop
  HalfSplit2 f0[2], f1[2];
  f16x8 fbL[NJ], fbH[NJ];
  for (int j = 0; j < NPW; ++j) dma_win(0, 0u, j);
  static_for<0, 2>([&](auto c) { dma_b(0, 0u, c); });
  static_for<0, 2>([&](auto c) { dma_b(1, (unsigned)W2_TILE_B, c); });
  wait_vmcnt<0>();
  __builtin_amdgcn_s_barrier();
  load_half(f0[0], 0, 0);
  load_half(f0[1], 0, 1);
  zero_raw(f0[0], edgeL0);   // tap 0: dx = -1
  zero_raw(f0[1], edgeL1);
  static_for<0, 8>([&](auto s) { f0[0].template step<decltype(s)::value>(); f0[1].template step<decltype(s)::value>(); });
#pragma unroll
  for (int j = 0; j < NJ; ++j) fbL[j] = __builtin_bit_cast(f16x8, sBf[bslot(1, j)]);
  load_half(f1[0], 1, 0);

  // ---- main loop, two k-tiles per trip (nk = 9 cpt is even: Cin % 32 == 0)
  for (int kt = 0; kt < nk; kt += 2) {
    ktile(kt, f0, f1, fbL, fbH, std::integral_constant<int, 0>{});
    ktile(kt + 1, f1, f0, fbL, fbH, std::integral_constant<int, 1>{});
  }
  wait_vmcnt<0>();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_s_barrier();  // both windows are dead: the epilogue reuses them

  bool bad = false;
#define EPI_TILES_M 2
#define EPI_HALVES (NJ / 2)
#define EPI_ACC(i, j) acc[i][j]
#define EPI_ROW0 m0 + wave * 64
#define EPI_COL0 n0
#define EPI_BIAS bias
#define EPI_STAGE smem
#define EPI_STAGE_BYTES (2 * WIN_B)
#define EPI_SCALE wsc
#define EPI_GN gn
#define EPI_RANGE_BAD bad
#include "split_epilogue_body.hpp"
  // range verdict of the wave's 64 A rows, as in gemm_split2_pipe_kernel
  bool small = false;
#ifndef GDRNPP2_NO_RANGE_CHECK
  {
    float s0 = ssq[0] + ssq[1], s1 = ssq[2] + ssq[3];
    s0 += __shfl_xor(s0, 32, 64);
    s1 += __shfl_xor(s1, 32, 64);
    const float thr = (float)K * 0x1p-8f;
    small = (s0 > 0.f && s0 < thr) || (s1 > 0.f && s1 < thr);
    bad |= !(s0 < __builtin_inff()) || !(s1 < __builtin_inff());
  }
#endif
  const int word = (__builtin_amdgcn_ballot_w64(bad) != 0 ? GDRNPP_SPLIT2_NONFINITE : 0) |
                   (__builtin_amdgcn_ballot_w64(small) != 0 ? GDRNPP_SPLIT2_SMALL_ROWS : 0);
  if (word && lane == 0) atomicOr(range_flag ? range_flag : &g_split2_range_word, word);
}

template <int EPI, int IW, bool GNS>
int launch_window_w(const float* A, const uint4* Wp, const float* bias, float* C, int M, int N, ConvGeom cg, GnStats gn, int* range_flag,
                    hipStream_t st, const char* what) {
  const int rc = gdrnpp::ensure_dynamic_lds((const void*)conv3x3_window_kernel<EPI, IW, GNS>, WIN_LDS_BYTES);
  if (rc) return rc;
  const long tiles = (long)(M / 256) * (N / BN);
  GDRNPP_REQUIRE(tiles < (1l << 30), GDRNPP_ELIMIT, "%s: grid too large", what);
  hipLaunchKernelGGL((conv3x3_window_kernel<EPI, IW, GNS>), dim3((unsigned)tiles), dim3(256), WIN_LDS_BYTES, st, A, Wp, bias, C, M, N, cg, gn,
                     range_flag);
  return gdrnpp::check_launch(what);
}

// the window-staged form serves W = 16 / 32 / 64 with tiles of whole rows of one image
bool window_form(int H, int W) {
  return gdrnpp::option_conv3x3_window() && (W == 16 || W == 32 || W == 64) && H % (256 / W) == 0;
}

template <int EPI, bool GNS>
int launch_window(const float* A, const uint4* Wp, const float* bias, float* C, int M, int N, ConvGeom cg, GnStats gn, int* range_flag,
                  hipStream_t st, const char* what) {
  if (cg.W == 16) return launch_window_w<EPI, 16, GNS>(A, Wp, bias, C, M, N, cg, gn, range_flag, st, what);
  if (cg.W == 32) return launch_window_w<EPI, 32, GNS>(A, Wp, bias, C, M, N, cg, gn, range_flag, st, what);
  return launch_window_w<EPI, 64, GNS>(A, Wp, bias, C, M, N, cg, gn, range_flag, st, what);
}

}  // namespace

extern "C" size_t gdrnpp_pack_weight_f16x2_bytes(int N, int K) {
  return (N > 0 && K > 0) ? (size_t)N * (size_t)K * 4 + 16 : 0;
}

extern "C" int gdrnpp_pack_weight_f16x2(const float* W, void* packed, int N, int K, void* stream) {
  GDRNPP_REQUIRE(W && packed, GDRNPP_EINVAL, "gdrnpp_pack_weight_f16x2: null pointer");
  GDRNPP_REQUIRE(N > 0 && K > 0 && N % BN == 0 && K % 32 == 0, GDRNPP_ELIMIT,
                 "gdrnpp_pack_weight_f16x2: N=%d K=%d must be multiples of %d/32", N, K, BN);
  hipStream_t st = (hipStream_t)stream;
  unsigned* trailer = reinterpret_cast<unsigned*>(reinterpret_cast<uint4*>(packed) + (size_t)(N / BN) * (K / BK) * W2_TILE_SLOTS);
  GDRNPP_HIP_TRY(hipMemsetAsync(trailer, 0, 16, st));
  const long n = (long)N * K;
  hipLaunchKernelGGL(amax_kernel, dim3((unsigned)min((n + 1023) / 1024, 1024l)), dim3(256), 0, st, W, n, trailer);
  const long threads = (long)N * (K / 8);
  hipLaunchKernelGGL(pack_weight2_kernel, dim3((unsigned)((threads + 255) / 256)), dim3(256), 0, st, W, (uint4*)packed, N, K);
  hipLaunchKernelGGL(weight_rows_range_kernel, dim3((unsigned)N), dim3(256), 0, st, W, trailer, trailer + 3, K);   // behind the pack: it writes trailer[3] = 0
  return gdrnpp::check_launch("gdrnpp_pack_weight_f16x2");
}

extern "C" int gdrnpp_linear_f32_split2_rows(const float* A, const void* W_packed, const float* bias, const float* gamma,
                                             const float* resid, float* C, int M, int N, int K, int epilogue, int rows,
                                             int* range_flag, void* stream) {
  GDRNPP_REQUIRE(A && W_packed && C, GDRNPP_EINVAL, "gdrnpp_linear_f32_split2: null pointer");
  GDRNPP_REQUIRE(M > 0 && N > 0 && K > 0 && N % BN == 0 && K % 32 == 0, GDRNPP_ELIMIT,
                 "gdrnpp_linear_f32_split2: N=%d K=%d must be multiples of %d/32 (M=%d is free)", N, K, BN, M);
  GDRNPP_REQUIRE((unsigned long long)M * (unsigned long long)K * 4ull < (1ull << 32), GDRNPP_ELIMIT,
                 "gdrnpp_linear_f32_split2: M*K*4 must stay below 4 GiB (32-bit lane offsets)");
  GDRNPP_REQUIRE(epilogue >= 0 && epilogue <= 2, GDRNPP_EINVAL, "gdrnpp_linear_f32_split2: epilogue=%d", epilogue);
  GDRNPP_REQUIRE(epilogue != EPI_SCALE_RES || (gamma && resid), GDRNPP_EINVAL,
                 "gdrnpp_linear_f32_split2: scale+residual epilogue needs gamma and resid");
  GDRNPP_REQUIRE((rows & ~(GDRNPP_A_F16X2_ROWS | GDRNPP_C_F16X2_ROWS)) == 0, GDRNPP_EINVAL, "gdrnpp_linear_f32_split2_rows: rows=%d", rows);
  GDRNPP_REQUIRE(!(rows & GDRNPP_C_F16X2_ROWS) || epilogue != EPI_SCALE_RES, GDRNPP_EINVAL,
                 "gdrnpp_linear_f32_split2_rows: the scale+residual epilogue writes fp32");
  GDRNPP_REQUIRE(!(rows & GDRNPP_A_F16X2_ROWS) || epilogue != EPI_BIAS, GDRNPP_ELIMIT,
                 "gdrnpp_linear_f32_split2_rows: an f16x2-rows A needs the GELU or the scale+residual epilogue (the two MLP layers)");
  // wide layers walk the tiles in panels (gemm_split_pipe.hip: launch_split_pipe); the fp16x2 image is 4 bytes per weight
  const int panel = (N / BN >= 8 && (long)N * K * 4 > (2l << 20)) ? gdrnpp::option_split_gemm_panel() : 0;
  const ConvGeom cg{0, 0, 0, 0, 0, 0, 0, 0, 0};
  const GnStats gn{nullptr, 0, 0};
  hipStream_t st = (hipStream_t)stream;
  const uint4* Wp = (const uint4*)W_packed;
  const char* what = "gdrnpp_linear_f32_split2";
  const int ar = rows & GDRNPP_A_F16X2_ROWS, cr = (rows & GDRNPP_C_F16X2_ROWS) ? 1 : 0;
  return with_epilogue(epilogue, [&](auto epi) {   // (the checks above leave ar = 0 with EPI_BIAS and cr = 0 with EPI_SCALE_RES)
    return launch_one<decltype(epi)::value, 0, false>(A, Wp, bias, gamma, resid, C, M, N, K, cg, panel, gn, range_flag, st, what, ar, cr);
  });
}

extern "C" int gdrnpp_linear_f32_split2(const float* A, const void* W_packed, const float* bias, const float* gamma,
                                        const float* resid, float* C, int M, int N, int K, int epilogue, int* range_flag,
                                        void* stream) {
  return gdrnpp_linear_f32_split2_rows(A, W_packed, bias, gamma, resid, C, M, N, K, epilogue, 0, range_flag, stream);
}

extern "C" int gdrnpp_conv3x3_f32_split2(const float* x_nhwc, const void* W_packed, const float* bias, float* y_nhwc,
                                         double* gn_partials, int n_img, int H, int W, int Cin, int Cout, int groups, int epilogue,
                                         int* range_flag, void* stream) {
  GDRNPP_REQUIRE(x_nhwc && W_packed && y_nhwc, GDRNPP_EINVAL, "gdrnpp_conv3x3_f32_split2: null pointer");
  GDRNPP_REQUIRE(n_img > 0 && H > 0 && W > 0 && H < 32768 && W < 32768 && Cin > 0 && Cout > 0, GDRNPP_EINVAL,
                 "gdrnpp_conv3x3_f32_split2: bad shape");
  const long M = (long)n_img * H * W;
  GDRNPP_REQUIRE(M < (1l << 31) && Cout % BN == 0 && Cin % 32 == 0, GDRNPP_ELIMIT,
                 "gdrnpp_conv3x3_f32_split2: Cout=%d Cin=%d must be multiples of %d/32", Cout, Cin, BN);
  GDRNPP_REQUIRE(epilogue == EPI_BIAS || epilogue == EPI_GELU, GDRNPP_EINVAL, "gdrnpp_conv3x3_f32_split2: epilogue=%d", epilogue);
  const ConvGeom cg{H, W, Cin, H, W, 3, 1, 1, 0};
  hipStream_t st = (hipStream_t)stream;
  const uint4* Wp = (const uint4*)W_packed;
  const char* what = "gdrnpp_conv3x3_f32_split2";
  if (gn_partials) {
    GDRNPP_REQUIRE(epilogue == EPI_BIAS && (H * W) % 256 == 0 && groups > 0 && Cout == 8 * groups, GDRNPP_ELIMIT,
                   "gdrnpp_conv3x3_f32_split2: GroupNorm statistics need the plain epilogue, H*W %% 256 == 0 and 8 channels per group "
                   "(H*W=%d Cout=%d groups=%d)", H * W, Cout, groups);
    if (window_form(H, W))
      return launch_window<EPI_BIAS, true>(x_nhwc, Wp, bias, y_nhwc, (int)M, Cout, cg, GnStats{gn_partials, groups, (H * W) / 256}, range_flag, st, what);
    return launch_one<EPI_BIAS, 1, true>(x_nhwc, Wp, bias, nullptr, nullptr, y_nhwc, (int)M, Cout, 9 * Cin, cg, 0,
                                         GnStats{gn_partials, groups, (H * W) / 256}, range_flag, st, what);
  }
  const GnStats gn{nullptr, 0, 0};
  if (window_form(H, W)) {
    if (epilogue == EPI_GELU) return launch_window<EPI_GELU, false>(x_nhwc, Wp, bias, y_nhwc, (int)M, Cout, cg, gn, range_flag, st, what);
    return launch_window<EPI_BIAS, false>(x_nhwc, Wp, bias, y_nhwc, (int)M, Cout, cg, gn, range_flag, st, what);
  }
  if (epilogue == EPI_GELU)
    return launch_one<EPI_GELU, 1, false>(x_nhwc, Wp, bias, nullptr, nullptr, y_nhwc, (int)M, Cout, 9 * Cin, cg, 0, gn, range_flag, st, what);
  return launch_one<EPI_BIAS, 1, false>(x_nhwc, Wp, bias, nullptr, nullptr, y_nhwc, (int)M, Cout, 9 * Cin, cg, 0, gn, range_flag, st, what);
}

extern "C" int gdrnpp_conv2d_f32_split2(const float* x_nhwc, const void* W_packed, const float* bias, float* y_nhwc, int n_img,
                                        int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad, int epilogue,
                                        int* range_flag, void* stream) {
  GDRNPP_REQUIRE(x_nhwc && W_packed && y_nhwc, GDRNPP_EINVAL, "gdrnpp_conv2d_f32_split2: null pointer");
  ConvShape sh;
  if (const int rc = check_conv_shape("gdrnpp_conv2d_f32_split2", n_img, H, W, Cin, Cout, KH, KW, stride, pad, 32, &sh)) return rc;
  if (KH == 3 && KW == 3 && stride == 1 && pad == 1)
    return gdrnpp_conv3x3_f32_split2(x_nhwc, W_packed, bias, y_nhwc, nullptr, n_img, H, W, Cin, Cout, 0, epilogue, range_flag, stream);
  const int OH = sh.OH, OW = sh.OW;
  const long M = sh.M;
  GDRNPP_REQUIRE(epilogue == EPI_BIAS || epilogue == EPI_GELU, GDRNPP_EINVAL, "gdrnpp_conv2d_f32_split2: epilogue=%d", epilogue);
  const ConvGeom cg{H, W, Cin, OH, OW, KW, stride, pad, 0};
  const GnStats gn{nullptr, 0, 0};
  hipStream_t st = (hipStream_t)stream;
  const uint4* Wp = (const uint4*)W_packed;
  const char* what = "gdrnpp_conv2d_f32_split2";
  if (epilogue == EPI_GELU)
    return launch_one<EPI_GELU, 2, false>(x_nhwc, Wp, bias, nullptr, nullptr, y_nhwc, (int)M, Cout, KH * KW * Cin, cg, 0, gn, range_flag, st, what);
  return launch_one<EPI_BIAS, 2, false>(x_nhwc, Wp, bias, nullptr, nullptr, y_nhwc, (int)M, Cout, KH * KW * Cin, cg, 0, gn, range_flag, st, what);
}

// The library's own sticky range word (launches with range_flag == NULL): *word = the bits raised since the last reset
// (synchronises the stream).  Callers running several streams / host threads / layers pass words of their own per launch.
extern "C" int gdrnpp_split2_range_word(int* flag, int reset, void* stream) {
  GDRNPP_REQUIRE(flag, GDRNPP_EINVAL, "gdrnpp_split2_range_word: null pointer");
  hipStream_t st = (hipStream_t)stream;
  int v = 0;
  GDRNPP_HIP_TRY(hipMemcpyFromSymbolAsync(&v, HIP_SYMBOL(g_split2_range_word), sizeof(int), 0, hipMemcpyDeviceToHost, st));
  GDRNPP_HIP_TRY(hipStreamSynchronize(st));
  if (reset && v) {
    const int zero = 0;
    GDRNPP_HIP_TRY(hipMemcpyToSymbolAsync(HIP_SYMBOL(g_split2_range_word), &zero, sizeof(int), 0, hipMemcpyHostToDevice, st));
    GDRNPP_HIP_TRY(hipStreamSynchronize(st));
  }
  *flag = v;
  return 0;
}
