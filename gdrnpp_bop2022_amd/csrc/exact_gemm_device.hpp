// Device code shared by the exact-f32 MFMA kernels of the backward pass (mlp_bwd.hip: gemm_tn, gemm_rows; conv_gn_bwd.hip:
// conv3x3_wgrad; pnp_bwd.hip: conv3x3s2_wgrad, conv3x3s2_dinput; head_tail_bwd.hip: grouped_wgrad, grouped_dinput; conv_bn_bwd.hip:
// conv_wgrad, conv3x3s2_dinput_any): the workgroup scheme, its LDS images, the accumulators with their fp64 carries, the k-loop and
// the D map.  A kernel keeps what is its own: where a stage's rows come from (its fetch), what a row slot or a depth slot is, and
// where the 128 x 128 tile goes (its store).
// DESIGN.md "exact_gemm_device.hpp" has the scheme and the measured resources.
//
// D[i][j] = sum_k A[k][i] B[k][j] on v_mfma_f32_32x32x2_f32, both operands as [k][128] images in LDS.  With the sum running over
// the ROWS of two row-major operands the instruction's operand map is the natural one: at k-step s lanes 0..31 hold 32 consecutive
// columns of row 2s, lanes 32..63 of row 2s + 1, for A (the i index of D) and for B (the j index) alike — contiguous row reads,
// nothing transposed.
//   workgroup   128 x 128 of D, 4 waves of 64 x 64 (2 x 2 accumulators of 32 x 32), the depth staged kBK = 32 at a time: global ->
//               registers (the next stage's loads fly under this stage's MFMAs) -> LDS [32][132] per operand -> one ds_read_b32 per
//               operand tile and k-step.  ds_read_b32 banks by 32-lane halves, each half reads 32 consecutive floats: conflict-free;
//               the pitch of 132 floats (not 128) keeps the two halves, a whole row apart, off one another's banks as well.
//   transposed  an operand whose depth is contiguous in memory (a row-major [rows][k]) is read float4 along k, 8 lanes per 128-byte
//               row segment, and stored TRANSPOSED into the same [k][row] image with four ds_write_b32; the image pitch of 133 makes
//               those 2-way conflicts at worst.
//   sums        the MFMA is bit for bit a k-ordered fmaf chain.  After kChainStages = 4 stages = 128 terms the fp32 accumulators
//               are added into fp64 carries (registers) and cleared: the fp32 chain never exceeds 128 terms whatever the depth, which
//               is at or below the in-register chain of a blocked CPU sgemm (the yardstick of the tests' bar, K blocks of 256 and
//               more) — and costs 64 v_add_f64 per wave against 256 MFMAs.
//   slots       a sum over many rows is cut into row slots whose count depends on the shape alone (row_slot_plan); rows at and
//               beyond a slot's end are zero-filled in the staging and never read.  Each slot's fp64 tile goes to a workspace; the
//               kernel's finalize adds the slots in index order in fp64 and rounds once, so two calls give equal bits.
#pragma once
#include <algorithm>
#include "common.hpp"

namespace gdrnpp {
namespace exactgemm {

using f32x16 = __attribute__((ext_vector_type(16))) float;
using f4 = __attribute__((ext_vector_type(4))) float;
__device__ __forceinline__ f4 ld4v(const float* p) { return *reinterpret_cast<const f4*>(p); }
__device__ __forceinline__ void st4v(float* p, f4 v) { *reinterpret_cast<f4*>(p) = v; }

constexpr int kThreads = 256;      // 4 waves
constexpr int kBK = 32;            // depth of a stage
constexpr int kPitch = 132;        // floats per k-row of an image stored as it lies
constexpr int kPitchT = 133;       // ... of an image stored transposed
constexpr int kChainStages = 4;    // stages per fp32 chain (128 terms)

// ---- wave and lane map ------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int thread_id() { return threadIdx.x; }      // signed: it enters row and column sums with ints and longs
__device__ __forceinline__ int lane_id() { return thread_id() & 63; }
__device__ __forceinline__ int wave_m() { return (thread_id() >> 6) >> 1; }      // the wave's 64 rows of D
__device__ __forceinline__ int wave_n() { return (thread_id() >> 6) & 1; }       // ... and its 64 columns
// what a lane reads at k-step 0 from an image of pitch P: its k-row (lane >> 5) and its column of the wave's first 32 x 32 tile
template <int P>
__device__ __forceinline__ const float* lane_a(const float* sA) {
  return sA + (lane_id() >> 5) * P + wave_m() * 64 + (lane_id() & 31);
}
template <int P>
__device__ __forceinline__ const float* lane_b(const float* sB) {
  return sB + (lane_id() >> 5) * P + wave_n() * 64 + (lane_id() & 31);
}

// ---- accumulators -----------------------------------------------------------------------------------------------------------------
// the wave's 64 x 64 of D in fp32: all a kernel of one short chain (grouped_dinput) holds
struct Acc {
  f32x16 acc[2][2];

  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
  }
  // one stage of depth BK from images of pitch PA / PB: four MFMAs per k-step
  template <int PA, int PB, int BK>
  __device__ __forceinline__ void mma(const float* la, const float* lb) {
#pragma unroll 4
    for (int s = 0; s < BK / 2; ++s) {
      const float a0 = la[2 * s * PA], a1 = la[2 * s * PA + 32];
      const float b0 = lb[2 * s * PB], b1 = lb[2 * s * PB + 32];
      acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
  }
};
// ... with the fp64 carries of a sum deeper than one chain
struct Tile : Acc {
  double carry[2][2][16];

  __device__ __forceinline__ void clear() {
    Acc::clear();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) carry[i][j][e] = 0.0;
  }
  __device__ __forceinline__ void fold() {
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) carry[i][j][e] += (double)acc[i][j][e], acc[i][j][e] = 0.f;
  }
};

// ---- stage stores -----------------------------------------------------------------------------------------------------------------
// natural: thread -> k-rows stage_row() + 8 p, p < 4, columns stage_col() .. + 3 of the 128
__device__ __forceinline__ int stage_row() { return thread_id() >> 5; }
__device__ __forceinline__ int stage_col() { return (thread_id() & 31) * 4; }
__device__ __forceinline__ void store_natural(float* s, int p, f4 v) { st4v(s + (stage_row() + 8 * p) * kPitch + stage_col(), v); }
// transposed: thread -> rows stage_row_t() + 32 p, p < 4, of the 128, k stage_k_t() .. + 3
__device__ __forceinline__ int stage_row_t() { return thread_id() >> 3; }
__device__ __forceinline__ int stage_k_t() { return (thread_id() & 7) * 4; }
__device__ __forceinline__ void store_transposed(float* s, int p, f4 v) {
#pragma unroll
  for (int j = 0; j < 4; ++j) s[(stage_k_t() + j) * kPitchT + stage_row_t() + 32 * p] = v[j];
}
// a thread's four float4 of each operand, A and B stored transposed (TA, TB) or as they lie
template <bool TA, bool TB>
__device__ __forceinline__ void store_stage(float* sA, float* sB, const f4 (&ra)[4], const f4 (&rb)[4]) {
#pragma unroll
  for (int p = 0; p < 4; ++p) {
    if (TA) store_transposed(sA, p, ra[p]); else store_natural(sA, p, ra[p]);
    if (TB) store_transposed(sB, p, rb[p]); else store_natural(sB, p, rb[p]);
  }
}

// ---- the k-loop -------------------------------------------------------------------------------------------------------------------
// One stage per position pos, pos + step, ... below end, whatever the positions count (rows, k, stages).  fetch(position) loads a
// stage into the caller's registers, store() writes those registers to the LDS images sA / sB of pitch PA / PB.  The caller has
// fetched the first stage; the tile's carries hold the whole sum on return.
template <int PA, int PB, class Pos, class Fetch, class Store>
__device__ __forceinline__ void k_loop(Tile& t, const float* sA, const float* sB, Pos pos, Pos end, int step, Fetch&& fetch,
                                       Store&& store) {
  const float* la = lane_a<PA>(sA);
  const float* lb = lane_b<PB>(sB);
  int stage = 0;
  for (; pos < end; pos += step) {
    __syncthreads();      // every wave has read the previous stage
    store();
    __syncthreads();
    if (pos + step < end) fetch(pos + step);
    t.mma<PA, PB, kBK>(la, lb);
    if (++stage == kChainStages) {
      t.fold();
      stage = 0;
    }
  }
  t.fold();
}

// ---- D map ------------------------------------------------------------------------------------------------------------------------
// Element e of accumulator (i, j) is row d_row(row0, i, e), column d_col(col0, j) of the tile whose corner is (row0, col0); the
// corner leads the sum so that the compiler sees one base and a small offset
template <class R>
__device__ __forceinline__ R d_row(R row0, int i, int e) {
  return row0 + wave_m() * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane_id() >> 5);
}
__device__ __forceinline__ int d_col(int col0, int j) { return col0 + wave_n() * 64 + j * 32 + (lane_id() & 31); }
// f(i, j, e, row, col) over the wave's 64 x 64.  f captures its pointers and sizes by value ([=, &t]): reached through a
// reference capture they are tested and added again for every element (gemm_rows: 4 131 against 4 386 instructions)
template <class R, class F>
__device__ __forceinline__ void for_each_d(R row0, int col0, F&& f) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) f(i, j, e, d_row(row0, i, e), d_col(col0, j));
}

// ---- row slots (host) -------------------------------------------------------------------------------------------------------------
// M rows in chunks of chunk_rows, dealt to at most min(slot_cap, grid_target / tiles) slots, that quotient rounded up or down as the
// caller says: a problem with many tiles of D fills the chip without cutting M, and every slot costs a tile of doubles written and
// read once.  The slot count decides the order of the fp64 additions and so the bits: it comes from the shape alone.
struct SlotPlan { int slots; long rows_per_slot; };
inline SlotPlan row_slot_plan(long M, long tiles, int chunk_rows, int slot_cap, int grid_target, bool round_up) {
  const long want = round_up ? (grid_target + tiles - 1) / tiles : grid_target / tiles;
  const long cap = std::max<long>(1, std::min<long>(slot_cap, want));
  const long chunks = (M + chunk_rows - 1) / chunk_rows;
  const long per = (chunks + cap - 1) / cap;
  return SlotPlan{(int)((chunks + per - 1) / per), per * chunk_rows};
}

}  // namespace exactgemm
}  // namespace gdrnpp
