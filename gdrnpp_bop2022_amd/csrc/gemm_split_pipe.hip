// Software-pipelined LDS-DMA form of the split GEMM (gemm_split.hip explains the numerical scheme) — SURVEY.md §8 row a3.
//
// Same tile as gemm_split_glds_kernel: 256x128x16 block tile, 4 waves stacked along M (each 64 rows x 128 columns = 2 x 4
// MFMA 32x32x16 tiles, 48 MFMAs per k-tile), fp32 A by LDS-DMA with the swizzled lane-linear image, pre-packed weights by
// LDS-DMA, exact 3-way bf16 split of A at fragment-read time.  What changes is the instruction stream of one wave:
//
//   * register-level software pipeline: while the matrix pipe works on k-tile t (A fragments already split, in registers),
//     the same wave reads the raw fp32 A of k-tile t+1 from LDS and splits it, two VALU operations per MFMA slot; the glds
//     kernel splits a whole k-tile (72 VALU operations, v_pk_add_f32 among them) in front of its first MFMA;
//   * the split subtracts with v_sub_f32 (this file is built with -fno-slp-vectorize): packed fp32 VALU beside MFMAs costs
//     more than the two scalar operations it replaces (MI355X_MICROARCH.md, per-instruction constants);
//   * weight fragments are read just in time, one split set (4 x ds_read_b128) ahead of the product group that uses it; the
//     product order groups by weight split (gemm_split.hpp) so two sets (32 VGPRs) are live instead of three;
//   * A stages are private to a wave (a wave stages exactly the rows it consumes), so with NA = 3 stages the A DMA runs two
//     k-tiles ahead: the wait in front of the barrier is a counted vmcnt(4) that leaves the newest four A pieces in flight;
//     weights (L2-resident) stay one k-tile ahead in two stages;
//   * A is addressed as SGPR base + 32-bit lane offset (linear form): no per-lane pointer arithmetic in the loop;
//   * the schedule is pinned slot by slot with sched_barrier(0): slot = one MFMA + its share of the other work.
//
// LDS: NA x 16 KB (A, fp32) + 2 x 12 KB (weights) = 56 / 72 KB dynamic, two workgroups per CU.
// Results are bitwise equal to the other split-GEMM kernels (same products, same order per accumulator).
#include "split_gemm_device.hpp"

namespace {

using namespace gdrnpp::splitgemm;

constexpr int A_STAGE_B = 256 * BK * 4;       // fp32 A image of one k-tile: 16 KB
constexpr int B_STAGE_B = W_TILE_SLOTS * 16;  // packed weight tile image: 12 KB

__device__ __forceinline__ unsigned cvt_pk_bf16(float a, float b) {
  const f32x2 v = {a, b};
  return __builtin_bit_cast(unsigned, __builtin_convertvector(v, bf16x2));
}

// One half of a wave's A tile for one k-tile: 32 rows x 16 k, 8 consecutive k of one row per lane (two 16-byte chunks).
// x = h + m + l exactly (h = rn(x), m = rn(x - h), l = x - h - m), produced in 22 steps of two VALU operations so that the
// work can be spread over the MFMA slots of the previous k-tile.
struct HalfSplit {
  float x[8], r[8];
  unsigned h[4], m[4], l[4];

  template <int S>
  __device__ __forceinline__ void step() {
#ifdef GDRNPP_TIMING_NO_SPLIT  // timing-only build (results invalid): the k-loop without the split arithmetic, m = l = h
    if constexpr (S < 2) {
      h[2 * S] = cvt_pk_bf16(x[4 * S], x[4 * S + 1]);
      h[2 * S + 1] = cvt_pk_bf16(x[4 * S + 2], x[4 * S + 3]);
    } else if constexpr (S == 10 || S == 11) {
      m[2 * (S - 10)] = h[2 * (S - 10)]; m[2 * (S - 10) + 1] = h[2 * (S - 10) + 1];
    } else if constexpr (S == 20 || S == 21) {
      l[2 * (S - 20)] = h[2 * (S - 20)]; l[2 * (S - 20) + 1] = h[2 * (S - 20) + 1];
    }
    return;
#endif
    if constexpr (S < 2) {
      h[2 * S] = cvt_pk_bf16(x[4 * S], x[4 * S + 1]);
      h[2 * S + 1] = cvt_pk_bf16(x[4 * S + 2], x[4 * S + 3]);
    } else if constexpr (S < 10) {
      constexpr int e = S - 2, p = e >> 1;
      r[e] = x[e] - __uint_as_float((e & 1) ? (h[p] & 0xffff0000u) : (h[p] << 16));
    } else if constexpr (S < 12) {
      constexpr int q = S - 10;
      m[2 * q] = cvt_pk_bf16(r[4 * q], r[4 * q + 1]);
      m[2 * q + 1] = cvt_pk_bf16(r[4 * q + 2], r[4 * q + 3]);
    } else if constexpr (S < 20) {
      constexpr int e = S - 12, p = e >> 1;
      r[e] = r[e] - __uint_as_float((e & 1) ? (m[p] & 0xffff0000u) : (m[p] << 16));
    } else {
      constexpr int q = S - 20;
      l[2 * q] = cvt_pk_bf16(r[4 * q], r[4 * q + 1]);
      l[2 * q + 1] = cvt_pk_bf16(r[4 * q + 2], r[4 * q + 3]);
    }
  }
  __device__ __forceinline__ void load(const uint4* lds, int slot0, int slot1) {
    const float4 a = __builtin_bit_cast(float4, lds[slot0]), b = __builtin_bit_cast(float4, lds[slot1]);
    x[0] = a.x; x[1] = a.y; x[2] = a.z; x[3] = a.w;
    x[4] = b.x; x[5] = b.y; x[6] = b.z; x[7] = b.w;
  }
  template <int SPLIT>
  __device__ __forceinline__ bf16x8 frag() const {
    const unsigned* s = SPLIT == 0 ? h : SPLIT == 1 ? m : l;
    return __builtin_bit_cast(bf16x8, make_uint4(s[0], s[1], s[2], s[3]));
  }
};

// Grouped launch (linear form): rows [g*rows_per_group, (g+1)*rows_per_group) use weight / bias slice sel[g] of a stack of
// equally shaped packed weights — the class-sliced 1x1 output layer of the geometry head (every ROI = 4096 rows selects the
// 70 output channels of its class).  rows_per_group is a multiple of the 256-row tile.  Columns >= n_store are not written.
struct Grouped {
  const int* sel;          // null = plain launch
  int rows_per_group;
  long w_stride;           // uint4 slots between consecutive weight slices
  int bias_stride;         // floats between consecutive bias slices
  int n_store;
  int panel;               // > 1: tiles are walked in panels of that many row blocks, column tile outer (launch_split_pipe)
  int n_groups;            // slices in the stack: a selector outside [0, n_groups) poisons its tiles with NaN instead of reading
                           // out of bounds (a detector label >= NUM_CLASSES must not come out as finite garbage maps)
};

// Linear form only (A row-major [M,K]); convolutions run on the kernels of gemm_split.hip.
// NA: A stages (2: one k-tile ahead, 3: two k-tiles ahead)
template <int EPI, int NA>
__global__ __launch_bounds__(256, 2) void gemm_split_pipe_kernel(const float* __restrict__ A, const uint4* __restrict__ Wp,
                                                                 const float* __restrict__ bias,
                                                                 const float* __restrict__ gamma,
                                                                 const float* __restrict__ resid, float* __restrict__ C,
                                                                 int M, int N, int K, ConvGeom cg, Grouped grp) {
  extern __shared__ uint4 smem[];  // the only LDS object: [NA][1024] A slots | [2][768] weight slots
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntn = N / BN;
  const TileMN tile = tile_coords(xcd_tile_id(), ntn, grp.panel, M);   // panel order for wide layers, see launch_split_pipe
  const int tile_n = tile.n, m0 = tile.m * 256, n0 = tile_n * BN;
  // split-K (cg.nk_split > 0, the only field of cg in use): workgroup (x, y) multiplies k-tiles [y * nk_split, (y + 1) * nk_split) and writes
  // the partial result C + y*M*N; gdrnpp_linear_f32_splitk sums the partials in fixed order and applies bias / epilogue
  const int kt0 = cg.nk_split > 0 ? (int)blockIdx.y * cg.nk_split : 0;
  const int nk = cg.nk_split > 0 ? cg.nk_split : K / BK;
  if (cg.nk_split > 0) C += (size_t)blockIdx.y * (size_t)M * (size_t)N;
  const unsigned lds0 = lds_addr(smem);

  // ---- DMA lanes: piece c (0..3) of this wave fills A slots (wave*4 + c)*64 + lane = rows wave*64 + c*16 + lane/4, chunk
  // q = (lane & 3) ^ ((row >> 2) & 3) of the row's 64-byte k segment (the swizzle is on the source address)
  const int prow = lane >> 2, pq = lane & 3;
  unsigned aoff[4];        // byte offset of the lane's chunk from A + kt*64
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int lrow = wave * 64 + c * 16 + prow;
    const int q = pq ^ ((lrow >> 2) & 3);
    const int arow = min(m0 + lrow, M - 1);
    aoff[c] = (unsigned)arow * (unsigned)(K * 4) + (unsigned)(q * 16);
  }
  const unsigned boff = (unsigned)((wave * 3) * 64 + lane) * 16u;
  const int grp_i = grp.sel ? grp.sel[m0 / grp.rows_per_group] : 0;   // weight / bias slice of this tile's rows
  if (grp.sel && (unsigned)grp_i >= (unsigned)grp.n_groups) {          // workgroup-uniform: nothing was issued yet
    const float qnan = __builtin_nanf("");
    const int c4n = BN / 4;
    for (int idx = tid; idx < 256 * c4n; idx += 256) {
      const int row = m0 + idx / c4n, col = n0 + (idx % c4n) * 4;
      if (row < M && col < grp.n_store) *reinterpret_cast<float4*>(C + (size_t)row * N + col) = make_float4(qnan, qnan, qnan, qnan);
    }
    return;
  }
  const char* const wbase = reinterpret_cast<const char*>(Wp + (size_t)grp_i * grp.w_stride + (size_t)tile_n * (K / BK) * W_TILE_SLOTS);
  const float* const bias_t = bias ? bias + (size_t)grp_i * grp.bias_stride : nullptr;
  const unsigned ldsA = lds0 + (unsigned)(wave * 4) * 1024u;
  const unsigned ldsB = lds0 + (unsigned)(NA * A_STAGE_B) + (unsigned)(wave * 3) * 1024u;

  // piece c of the A image of k-tile kt -> stage byte offset sb
  auto dma_a = [&](int kt, unsigned sb, auto cc) {
    constexpr int c = decltype(cc)::value;
    dma_s(aoff[c], reinterpret_cast<const char*>(A) + (size_t)(kt0 + kt) * (BK * 4), ldsA + sb + c * 1024u);
  };
  auto dma_b = [&](int kt, unsigned sb, auto cc) {
    constexpr int c = decltype(cc)::value;
    dma_s(boff, wbase + ((size_t)(kt0 + kt) * B_STAGE_B + c * 1024), ldsB + sb + c * 1024u);
  };

  f32x16 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.f;

  // ---- fragment lanes: MFMA operand lane = row/column (lane & 31), k-block fk = lane >> 5
  const int frow = lane & 31, fk = lane >> 5;
  const int lrow0 = wave * 64 + frow, g0 = (lrow0 >> 2) & 3;  // rows +32 (second half) have the same swizzle
  const int aslot0 = 4 * lrow0 + ((2 * fk) ^ g0), aslot1 = 4 * lrow0 + ((2 * fk + 1) ^ g0);
  const uint4* const sA = smem;
  const uint4* const sBf = smem + NA * (A_STAGE_B / 16) + fk * BN + frow;

  auto load_half = [&](HalfSplit& hs, int stage, int half) {
    hs.load(sA + stage * (A_STAGE_B / 16) + half * 128, aslot0, aslot1);
  };

  // One k-tile.  cur: split A fragments of k-tile kt (registers); nxt: receives the split of k-tile kt+1 (the raw first half
  // is already in nxt[0].x).  fbX holds the weight split l of kt on entry, then its split h; fbY its split m, then the
  // split l of kt+1 (the two sets swap roles from one k-tile to the next).  BS: weight stage of kt (compile-time parity).
  // sa1 / sa2 / sa_wr: A stages of kt+1, of kt+2, and the one receiving kt+NA (= the stage kt has left).
  // The wait + barrier that publishes k-tile kt+1 sits behind slot 39: the last eight MFMAs need no new data and run while
  // the first fragments of kt+1 (weight split l, raw A of kt+2's first half) come out of LDS.
  auto ktile = [&](int kt, HalfSplit (&cur)[2], HalfSplit (&nxt)[2], bf16x8 (&fbX)[4], bf16x8 (&fbY)[4], auto bs_, int sa1,
                   int sa2, int sa_wr) {
    constexpr int BS = decltype(bs_)::value;
    const uint4* const b = sBf + BS * (B_STAGE_B / 16);
    const uint4* const bn = sBf + (BS ^ 1) * (B_STAGE_B / 16);
    const int kt_b = min(kt + 1, nk - 1), kt_a = min(kt + NA, nk - 1);
    const unsigned sb_wr = (unsigned)((BS ^ 1) * B_STAGE_B), sa_wr_b = (unsigned)(sa_wr * A_STAGE_B);
    static_for<0, 48>([&](auto s_) {
      constexpr int S = decltype(s_)::value;
      constexpr int G = S / 8, I = (S % 8) >> 2, J = S & 3;
      GDRNPP_SPLIT_PRODUCT_ORDER
      constexpr int SA_ = TA[G], SB_ = TB[G];
      const bf16x8 fa = cur[I].template frag<SA_>();
      const bf16x8 fb = (SB_ == 1) ? fbY[J] : fbX[J];
      acc[I][J] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[I][J], 0, 0, 0);
      // weight DMA of k-tile kt+1, then A DMA of k-tile kt+NA (the A pieces are the newest four loads at the wait)
      if constexpr (S == 0) dma_b(kt_b, sb_wr, std::integral_constant<int, 0>{});
      if constexpr (S == 2) dma_b(kt_b, sb_wr, std::integral_constant<int, 1>{});
      if constexpr (S == 4) dma_b(kt_b, sb_wr, std::integral_constant<int, 2>{});
      if constexpr (S == 6) dma_a(kt_a, sa_wr_b, std::integral_constant<int, 0>{});
      if constexpr (S == 8) dma_a(kt_a, sa_wr_b, std::integral_constant<int, 1>{});
      if constexpr (S == 10) dma_a(kt_a, sa_wr_b, std::integral_constant<int, 2>{});
      if constexpr (S == 12) dma_a(kt_a, sa_wr_b, std::integral_constant<int, 3>{});
      // weight split m for groups 1-2 (slots 8..23), weight split h for groups 3-5 (slots 24..47; reuses the l registers)
      if constexpr (S == 1 || S == 3) {
        constexpr int j0 = S - 1;
        fbY[j0] = __builtin_bit_cast(bf16x8, b[1 * KB * BN + j0 * 32]);
        fbY[j0 + 1] = __builtin_bit_cast(bf16x8, b[1 * KB * BN + (j0 + 1) * 32]);
      }
      if constexpr (S == 9 || S == 11) {
        constexpr int j0 = S - 9;
        fbX[j0] = __builtin_bit_cast(bf16x8, b[j0 * 32]);
        fbX[j0 + 1] = __builtin_bit_cast(bf16x8, b[(j0 + 1) * 32]);
      }
      if constexpr (S == 19) load_half(nxt[1], sa1, 1);
      // split of the next k-tile: first half in slots 4..25, second half in slots 26..47
      if constexpr (S >= 4 && S < 26) nxt[0].template step<S - 4>();
      if constexpr (S >= 26) nxt[1].template step<S - 26>();
      if constexpr (S == 39) {
#ifndef GDRNPP_TIMING_NO_VMWAIT   // timing-only builds (results invalid): the k-loop without the DMA wait / without the barrier
        wait_vmcnt<NA == 3 ? 4 : 0>();
#endif
        __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): every LDS read of the stages about to be refilled has returned
#ifndef GDRNPP_TIMING_NO_BARRIER
        __builtin_amdgcn_s_barrier();
#endif
      }
      // behind the barrier: first fragments of k-tile kt+1 (its weight split l; fbY's split m is dead since slot 23) and the
      // raw first half of k-tile kt+2 (cur[0] is nxt[0] of the next k-tile; only cur[0].h is still in use)
      if constexpr (S == 40 || S == 41) {
        constexpr int j0 = 2 * (S - 40);
        fbY[j0] = __builtin_bit_cast(bf16x8, bn[2 * KB * BN + j0 * 32]);
        fbY[j0 + 1] = __builtin_bit_cast(bf16x8, bn[2 * KB * BN + (j0 + 1) * 32]);
      }
      if constexpr (S == 42) load_half(cur[0], sa2, 0);
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  // ---- prologue: k-tiles 0 .. NA-1 of A and k-tile 0 of the weights; split k-tile 0; first fragments of the loop
  static_for<0, 4>([&](auto c) { dma_a(0, 0u, c); });
  static_for<0, 3>([&](auto c) { dma_b(0, 0u, c); });
  static_for<0, 4>([&](auto c) { dma_a(min(1, nk - 1), (unsigned)A_STAGE_B, c); });
  if constexpr (NA == 3) static_for<0, 4>([&](auto c) { dma_a(min(2, nk - 1), 2u * A_STAGE_B, c); });
  wait_vmcnt<NA == 3 ? 4 : 0>();
  __builtin_amdgcn_s_barrier();
  HalfSplit f0[2], f1[2];
  bf16x8 fbA[4], fbB[4];
  load_half(f0[0], 0, 0);
  load_half(f0[1], 0, 1);
  static_for<0, 22>([&](auto s) { f0[0].template step<decltype(s)::value>(); f0[1].template step<decltype(s)::value>(); });
#pragma unroll
  for (int j = 0; j < 4; ++j) fbA[j] = __builtin_bit_cast(bf16x8, sBf[2 * KB * BN + j * 32]);
  load_half(f1[0], 1, 0);

  // ---- main loop, two k-tiles per trip (nk is even: K % 32 == 0)
  int sa = 0;  // kt % NA
  for (int kt = 0; kt < nk; kt += 2) {
    const int sa1 = sa + 1 == NA ? 0 : sa + 1, sa2 = sa1 + 1 == NA ? 0 : sa1 + 1, sa3 = sa2 + 1 == NA ? 0 : sa2 + 1;
    ktile(kt, f0, f1, fbA, fbB, std::integral_constant<int, 0>{}, sa1, sa2, sa);
    ktile(kt + 1, f1, f0, fbB, fbA, std::integral_constant<int, 1>{}, sa2, sa3, sa1);
    sa = sa2;
  }
  wait_vmcnt<0>();               // NA = 3: the clamped A pieces of the last trip are still in flight
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_s_barrier();  // every wave's stages are dead: the epilogue reuses them

#define EPI_TILES_M 2
#define EPI_HALVES 2
#define EPI_ACC(i, j) acc[i][j]
#define EPI_ROW0 m0 + wave * 64
#define EPI_COL0 n0
#define EPI_BIAS bias_t
#define EPI_STAGE smem
#define EPI_STAGE_BYTES (NA * A_STAGE_B)
#define EPI_N_STORE grp.n_store
#include "split_epilogue_body.hpp"
}

// --------------------------------------------------------------------------------------------------------------------
// 128-row form of the pipelined kernel (linear only) for launches with fewer than 256 tiles of 256 x 128 — the deep ConvNeXt
// stages at the reference's own batch sizes (one image = a few to ~30 ROIs per forward, data_loader.py:901): twice the
// workgroups for the same problem, and the same k-loop per workgroup as above at half the size.  Block tile 128 x 128 x 16, 4
// waves stacked along M (32 rows x 128 columns = 1 x 4 MFMA tiles, 24 MFMAs per k-tile), four 8 KB A stages private to the
// wave (its 32 rows: two LDS-DMA pieces) and three 12 KB weight stages — the A DMA runs four k-tiles ahead, the weight DMA two:
// with the 3 + 2 stages of the 256-row kernel a k-tile took 0.83 us at one workgroup per CU, the memory latency of the operand
// issued one 24-MFMA k-tile earlier; one barrier per k-tile behind slot 19 of 24; the register
// pipeline is the one of gemm_split_pipe_kernel with one half instead of two (split of k-tile t+1 in slots 1..22 of k-tile t,
// weight fragments one split set ahead, raw A of k-tile t+2 read behind the barrier).  68 KB of LDS.  Split-K through
// cg.nk_split like the 256-row kernel.  Same products in the same order per accumulator: bitwise equal to the other kernels.
// --------------------------------------------------------------------------------------------------------------------
constexpr int A128_STAGE_B = 128 * BK * 4;   // 8 KB
constexpr int P128_NA = 4, P128_NB = 3;      // A and weight stages of the 128-row kernel

template <int EPI>
__global__ __launch_bounds__(256, 2) void gemm_split_pipe128_kernel(const float* __restrict__ A, const uint4* __restrict__ Wp,
                                                                    const float* __restrict__ bias,
                                                                    const float* __restrict__ gamma,
                                                                    const float* __restrict__ resid, float* __restrict__ C,
                                                                    int M, int N, int K, int nk_split) {
  constexpr int NA = P128_NA, NB = P128_NB;
  extern __shared__ uint4 smem[];  // [NA][512] A slots | [NB][768] weight slots
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int ntn = N / BN;
  const TileMN tile = tile_coords(xcd_tile_id(), ntn);
  const int tile_n = tile.n, m0 = tile.m * 128, n0 = tile_n * BN;
  const int kt0 = nk_split > 0 ? (int)blockIdx.y * nk_split : 0;
  const int nk = nk_split > 0 ? nk_split : K / BK;
  if (nk_split > 0) C += (size_t)blockIdx.y * (size_t)M * (size_t)N;
  const unsigned lds0 = lds_addr(smem);

  const int prow = lane >> 2, pq = lane & 3;
  unsigned aoff[2];
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int lrow = wave * 32 + c * 16 + prow;
    const int q = pq ^ ((lrow >> 2) & 3);
    const int arow = min(m0 + lrow, M - 1);
    aoff[c] = (unsigned)arow * (unsigned)(K * 4) + (unsigned)(q * 16);
  }
  const unsigned boff = (unsigned)((wave * 3) * 64 + lane) * 16u;
  const char* const wbase = reinterpret_cast<const char*>(Wp + (size_t)tile_n * (K / BK) * W_TILE_SLOTS);
  const unsigned ldsA = lds0 + (unsigned)(wave * 2) * 1024u;
  const unsigned ldsB = lds0 + (unsigned)(NA * A128_STAGE_B) + (unsigned)(wave * 3) * 1024u;
  auto dma_a = [&](int kt, unsigned sb, auto cc) {
    constexpr int c = decltype(cc)::value;
    dma_s(aoff[c], reinterpret_cast<const char*>(A) + (size_t)(kt0 + kt) * (BK * 4), ldsA + sb + c * 1024u);
  };
  auto dma_b = [&](int kt, unsigned sb, auto cc) {
    constexpr int c = decltype(cc)::value;
    dma_s(boff, wbase + ((size_t)(kt0 + kt) * B_STAGE_B + c * 1024), ldsB + sb + c * 1024u);
  };

  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;

  const int frow = lane & 31, fk = lane >> 5;
  const int lrow0 = wave * 32 + frow, g0 = (lrow0 >> 2) & 3;
  const int aslot0 = 4 * lrow0 + ((2 * fk) ^ g0), aslot1 = 4 * lrow0 + ((2 * fk + 1) ^ g0);
  const uint4* const sA = smem;
  const uint4* const sBf = smem + NA * (A128_STAGE_B / 16) + fk * BN + frow;
  auto load_raw = [&](HalfSplit& hs, int stage) { hs.load(sA + stage * (A128_STAGE_B / 16), aslot0, aslot1); };

  // One k-tile.  cur: split A fragments of k-tile kt; nxt.x: raw A of k-tile kt+1 on entry, its split on exit.  fbX: weight
  // split l of kt on entry, then its split h; fbY: its split m, then the split l of kt+1.  BS: weight stage of kt.
  // sa2 / sa_wr: A stage of kt+2, and the one receiving kt+NA (= the stage kt has left).
  auto ktile = [&](int kt, HalfSplit& cur, HalfSplit& nxt, bf16x8 (&fbX)[4], bf16x8 (&fbY)[4], int bs, int sa2, int sa_wr) {
    const int bs1 = bs + 1 == NB ? 0 : bs + 1, bs2 = bs1 + 1 == NB ? 0 : bs1 + 1;   // weight stages of kt+1, and of kt+2 (written now)
    const uint4* const b = sBf + bs * (B_STAGE_B / 16);
    const uint4* const bn = sBf + bs1 * (B_STAGE_B / 16);
    const int kt_b = min(kt + 2, nk - 1), kt_a = min(kt + NA, nk - 1);
    const unsigned sb_wr = (unsigned)(bs2 * B_STAGE_B), sa_wr_b = (unsigned)(sa_wr * A128_STAGE_B);
    static_for<0, 24>([&](auto s_) {
      constexpr int S = decltype(s_)::value;
      constexpr int G = S / 4, J = S & 3;
      GDRNPP_SPLIT_PRODUCT_ORDER
      constexpr int SA_ = TA[G], SB_ = TB[G];
      const bf16x8 fa = cur.template frag<SA_>();
      const bf16x8 fb = (SB_ == 1) ? fbY[J] : fbX[J];
      acc[J] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa, fb, acc[J], 0, 0, 0);
      // weight DMA of k-tile kt+2, then A DMA of k-tile kt+NA: both operands run two or more k-tiles ahead — at one workgroup
      // per CU (what this kernel is for) nothing else hides the memory latency, and a k-tile is only 24 MFMAs long
      if constexpr (S == 0) dma_b(kt_b, sb_wr, std::integral_constant<int, 0>{});
      if constexpr (S == 1) dma_b(kt_b, sb_wr, std::integral_constant<int, 1>{});
      if constexpr (S == 2) dma_b(kt_b, sb_wr, std::integral_constant<int, 2>{});
      if constexpr (S == 3) dma_a(kt_a, sa_wr_b, std::integral_constant<int, 0>{});
      if constexpr (S == 5) dma_a(kt_a, sa_wr_b, std::integral_constant<int, 1>{});
      // weight split m for groups 1-2 (slots 4..11); weight split h for groups 3-5 (slots 12..23; reuses the l registers,
      // free after group 0)
      if constexpr (S == 0 || S == 1) {
        constexpr int j0 = 2 * S;
        fbY[j0] = __builtin_bit_cast(bf16x8, b[1 * KB * BN + j0 * 32]);
        fbY[j0 + 1] = __builtin_bit_cast(bf16x8, b[1 * KB * BN + (j0 + 1) * 32]);
      }
      if constexpr (S == 4 || S == 6) {
        constexpr int j0 = S - 4;
        fbX[j0] = __builtin_bit_cast(bf16x8, b[j0 * 32]);
        fbX[j0 + 1] = __builtin_bit_cast(bf16x8, b[(j0 + 1) * 32]);
      }
      // split of the next k-tile in slots 1..22
      if constexpr (S >= 1 && S < 23) nxt.template step<S - 1>();
      if constexpr (S == 19) {
        wait_vmcnt<7>();                      // all but the newest A(kt-1+NA), W(kt+2), A(kt+NA) pieces: weights of kt+1, A of kt+2 are in
        __builtin_amdgcn_s_waitcnt(0xc07f);   // lgkmcnt(0): every LDS read of the stages about to be refilled has returned
        __builtin_amdgcn_s_barrier();
      }
      // behind the barrier (the last four MFMAs use only cur's h fragments): weight split l of k-tile kt+1 (fbY's split m is
      // dead since slot 11) and the raw A of k-tile kt+2 (cur is nxt of the next k-tile)
      if constexpr (S == 20 || S == 21) {
        constexpr int j0 = 2 * (S - 20);
        fbY[j0] = __builtin_bit_cast(bf16x8, bn[2 * KB * BN + j0 * 32]);
        fbY[j0 + 1] = __builtin_bit_cast(bf16x8, bn[2 * KB * BN + (j0 + 1) * 32]);
      }
      if constexpr (S == 22) load_raw(cur, sa2);
      __builtin_amdgcn_sched_barrier(0);
    });
  };

  // ---- prologue: A of k-tiles 0..2, weights of k-tile 0; split k-tile 0; first fragments of the loop
  static_for<0, 2>([&](auto c) { dma_a(0, 0u, c); });
  static_for<0, 3>([&](auto c) { dma_b(0, 0u, c); });
  static_for<0, 2>([&](auto c) { dma_a(min(1, nk - 1), (unsigned)A128_STAGE_B, c); });
  static_for<0, 3>([&](auto c) { dma_b(min(1, nk - 1), (unsigned)B_STAGE_B, c); });
  static_for<0, 2>([&](auto c) { dma_a(min(2, nk - 1), 2u * A128_STAGE_B, c); });
  static_for<0, 2>([&](auto c) { dma_a(min(3, nk - 1), 3u * A128_STAGE_B, c); });
  wait_vmcnt<7>();               // A(0), W(0), A(1) are in
  __builtin_amdgcn_s_barrier();
  HalfSplit f0, f1;
  bf16x8 fbA[4], fbB[4];
  load_raw(f0, 0);
  static_for<0, 22>([&](auto s) { f0.template step<decltype(s)::value>(); });
#pragma unroll
  for (int j = 0; j < 4; ++j) fbA[j] = __builtin_bit_cast(bf16x8, sBf[2 * KB * BN + j * 32]);
  load_raw(f1, 1);

  static_assert(NA == 4 && NB == 3, "the wait counts and the prologue above are written for four A and three weight stages");
  int sa = 0, bs = 0;  // kt % NA, kt % NB
  for (int kt = 0; kt < nk; kt += 2) {
    const int sa1 = (sa + 1) & 3, sa2 = (sa + 2) & 3, sa3 = (sa + 3) & 3;
    const int bsn = bs + 1 == NB ? 0 : bs + 1;
    ktile(kt, f0, f1, fbA, fbB, bs, sa2, sa);
    ktile(kt + 1, f1, f0, fbB, fbA, bsn, sa3, sa1);
    sa = sa2;
    bs = bsn + 1 == NB ? 0 : bsn + 1;
  }
  wait_vmcnt<0>();
  __builtin_amdgcn_s_waitcnt(0xc07f);
  __builtin_amdgcn_s_barrier();  // every wave's stages are dead: the epilogue reuses them

#define EPI_TILES_M 1
#define EPI_HALVES 2
#define EPI_ACC(i, j) acc[j]
#define EPI_ROW0 m0 + wave * 32
#define EPI_COL0 n0
#define EPI_BIAS bias
#define EPI_STAGE smem
#define EPI_STAGE_BYTES (NA * A128_STAGE_B)
#include "split_epilogue_body.hpp"
}

template <int EPI>
int launch_pipe128(const float* A, const uint4* Wp, const float* bias, const float* gamma, const float* resid, float* C, int M,
                   int N, int K, int nk_split, hipStream_t st, const char* what) {
  constexpr int lds_bytes = P128_NA * A128_STAGE_B + P128_NB * B_STAGE_B;   // 68 KB
  static bool raised[64] = {};
  int dev = 0;
  GDRNPP_HIP_TRY(hipGetDevice(&dev));
  if (dev >= 0 && dev < 64 && !raised[dev]) {
    GDRNPP_HIP_TRY(hipFuncSetAttribute((const void*)gemm_split_pipe128_kernel<EPI>, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    raised[dev] = true;
  }
  const long tiles = (long)((M + 127) / 128) * (N / BN);
  const unsigned splits = nk_split > 0 ? (unsigned)((K / BK) / nk_split) : 1u;
  hipLaunchKernelGGL((gemm_split_pipe128_kernel<EPI>), dim3((unsigned)tiles, splits), dim3(256), lds_bytes, st, A, Wp, bias, gamma,
                     resid, C, M, N, K, nk_split);
  return gdrnpp::check_launch(what);
}

// hipFuncSetAttribute is a per-device setting: done once per (kernel, device), not per launch
template <int EPI, int NA>
int launch_one(const float* A, const uint4* Wp, const float* bias, const float* gamma, const float* resid, float* C, int M,
               int N, int K, ConvGeom cg, Grouped grp, hipStream_t st, const char* what) {
  constexpr int lds_bytes = NA * A_STAGE_B + 2 * B_STAGE_B;
  static bool raised[64] = {};
  int dev = 0;
  GDRNPP_HIP_TRY(hipGetDevice(&dev));
  if (dev >= 0 && dev < 64 && !raised[dev]) {
    GDRNPP_HIP_TRY(hipFuncSetAttribute((const void*)gemm_split_pipe_kernel<EPI, NA>,
                                       hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
    raised[dev] = true;
  }
  const long tiles = (long)((M + 255) / 256) * (N / BN);
  const unsigned splits = cg.nk_split > 0 ? (unsigned)((K / BK) / cg.nk_split) : 1u;
  hipLaunchKernelGGL((gemm_split_pipe_kernel<EPI, NA>), dim3((unsigned)tiles, splits), dim3(256), lds_bytes, st, A, Wp, bias,
                     gamma, resid, C, M, N, K, cg, grp);
  return gdrnpp::check_launch(what);
}

template <int EPI>
int launch_na(int a_stages, const float* A, const uint4* Wp, const float* bias, const float* gamma, const float* resid,
              float* C, int M, int N, int K, ConvGeom cg, Grouped grp, hipStream_t st, const char* what) {
  if (a_stages == 3) return launch_one<EPI, 3>(A, Wp, bias, gamma, resid, C, M, N, K, cg, grp, st, what);
  return launch_one<EPI, 2>(A, Wp, bias, gamma, resid, C, M, N, K, cg, grp, st, what);
}

int launch_epi(int epilogue, int a_stages, const float* A, const uint4* Wp, const float* bias, const float* gamma,
               const float* resid, float* C, int M, int N, int K, ConvGeom cg, Grouped grp, hipStream_t st, const char* what) {
  return with_epilogue(epilogue, [&](auto epi) {
    return launch_na<decltype(epi)::value>(a_stages, A, Wp, bias, gamma, resid, C, M, N, K, cg, grp, st, what);
  });
}

}  // namespace

namespace gdrnpp {
namespace splitgemm {

int launch_split_pipe(const float* A, const uint4* Wp, const float* bias, const float* gamma, const float* resid, float* C,
                      int M, int N, int K, int epilogue, ConvGeom cg, int a_stages, hipStream_t st, const char* what) {
  if (K % 32 || N % BN || M <= 0) return -1;
  // Wide layers (packed weight beyond an XCD's L2: N*K*6 bytes > 2 MB, at least 8 column tiles) walk the tiles in panels of
  // option split_gemm_panel (4) row blocks, column tile outer: workgroups that start back to back then share the weight tile
  // and meet the same row blocks again `panel` starts later, so both operands are re-read while still in the XCD's L2.
  // Row-major order (narrow layers) shares the row block between neighbours and the weight tile only N/128 starts apart.
  // Measured fetch of the 32768x512 -> 2048 layer per launch: row-major 464 MB, panels of 2/3/4/5/6/8/16: 464/415/317/376/
  // 348/357/575 MB (profiles/r02l_gemm_traffic_by_shape.md); launch time unchanged (the operands come from the memory-side
  // cache either way).
  const int panel = (N / BN >= 8 && (long)N * K * 6 > (2l << 20)) ? gdrnpp::option_split_gemm_panel() : 0;
  const Grouped grp{nullptr, 1, 0, 0, N, panel, 1};
  if ((unsigned long long)M * (unsigned long long)K * 4ull >= (1ull << 32)) return -1;  // 32-bit lane offsets
  return launch_epi(epilogue, a_stages, A, Wp, bias, gamma, resid, C, M, N, K, cg, grp, st, what);
}

// 128-row form: plain launch with the fused epilogue (nk_split == 0) or split-K partials (nk_split > 0, bias-less raw sums)
int launch_split_pipe128(const float* A, const uint4* Wp, const float* bias, const float* gamma, const float* resid, float* C,
                         int M, int N, int K, int epilogue, int nk_split, hipStream_t st, const char* what) {
  if (K % 32 || N % BN || M <= 0 || (nk_split > 0 && (nk_split < 2 || nk_split % 2 || (K / BK) % nk_split))) return -1;
  if ((unsigned long long)M * (unsigned long long)K * 4ull >= (1ull << 32)) return -1;  // 32-bit lane offsets
  if ((long)((M + 127) / 128) * (N / BN) >= (1l << 30)) return -1;
  if (nk_split > 0) return launch_pipe128<EPI_BIAS>(A, Wp, nullptr, nullptr, nullptr, C, M, N, K, nk_split, st, what);
  return with_epilogue(epilogue, [&](auto epi) { return launch_pipe128<decltype(epi)::value>(A, Wp, bias, gamma, resid, C, M, N, K, 0, st, what); });
}

// Split-K launch of the pipelined kernel: partials[y][M][N] for the (K/16) / nk_split chunks of nk_split (even) k-tiles.
int launch_split_pipe_splitk(const float* A, const uint4* Wp, float* partials, int M, int N, int K, int nk_split, int a_stages,
                             hipStream_t st, const char* what) {
  if (K % 32 || N % BN || M <= 0 || nk_split < 2 || nk_split % 2 || (K / BK) % nk_split) return -1;
  if ((unsigned long long)M * (unsigned long long)K * 4ull >= (1ull << 32)) return -1;  // 32-bit lane offsets
  const Grouped grp{nullptr, 1, 0, 0, N, 0, 1};
  return launch_epi(EPI_BIAS, a_stages, A, Wp, nullptr, nullptr, nullptr, partials, M, N, K,
                       ConvGeom{0, 0, 0, 0, 0, 0, 0, 0, nk_split}, grp, st, what);
}

}  // namespace splitgemm
}  // namespace gdrnpp

extern "C" int gdrnpp_linear_f32_split_grouped(const float* A, const void* W_packed_stack, const float* bias_stack,
                                               const int* group_sel, int n_groups, int rows_per_group, float* C, int M, int N,
                                               int K, int n_store, void* stream) {
  using namespace gdrnpp::splitgemm;
  GDRNPP_REQUIRE(A && W_packed_stack && group_sel && C, GDRNPP_EINVAL, "gdrnpp_linear_f32_split_grouped: null pointer");
  GDRNPP_REQUIRE(M > 0 && N > 0 && K > 0 && N % BN == 0 && K % 32 == 0, GDRNPP_ELIMIT,
                 "gdrnpp_linear_f32_split_grouped: N=%d K=%d must be multiples of %d/32", N, K, BN);
  GDRNPP_REQUIRE(n_groups > 0, GDRNPP_EINVAL, "gdrnpp_linear_f32_split_grouped: n_groups=%d", n_groups);
  GDRNPP_REQUIRE(rows_per_group > 0 && rows_per_group % 256 == 0 && M % rows_per_group == 0, GDRNPP_EINVAL,
                 "gdrnpp_linear_f32_split_grouped: rows_per_group=%d must be a multiple of 256 that divides M=%d", rows_per_group, M);
  GDRNPP_REQUIRE(n_store > 0 && n_store <= N && n_store % 4 == 0, GDRNPP_EINVAL, "gdrnpp_linear_f32_split_grouped: n_store=%d", n_store);
  GDRNPP_REQUIRE((unsigned long long)M * (unsigned long long)K * 4ull < (1ull << 32), GDRNPP_ELIMIT,
                 "gdrnpp_linear_f32_split_grouped: M*K*4 must stay below 4 GiB");
  GDRNPP_REQUIRE((long)(M / 256) * (N / BN) < (1l << 30), GDRNPP_ELIMIT, "gdrnpp_linear_f32_split_grouped: grid too large");
  const Grouped grp{group_sel, rows_per_group, (long)(N / BN) * (K / BK) * W_TILE_SLOTS, N, n_store, 0, n_groups};
  return launch_epi(EPI_BIAS, gdrnpp::option_split_gemm_pipe() == 2 ? 2 : 3, A, (const uint4*)W_packed_stack, bias_stack, nullptr,
                       nullptr, C, M, N, K, ConvGeom{0, 0, 0, 0, 0, 0, 0, 0, 0}, grp, (hipStream_t)stream, "gdrnpp_linear_f32_split_grouped");
}
