// Device code shared by every split-GEMM kernel (gemm_split.hip, gemm_split_pipe.hip, gemm_split2_pipe.hip, gemm_mlp_fused.hip):
// the LDS-DMA layer, the workgroup -> tile map and the GroupNorm statistics of the epilogue.  gemm_split.hpp holds the
// host-visible declarations.
#pragma once
#include "gemm_split.hpp"

namespace gdrnpp {
namespace splitgemm {

// ---- LDS-DMA layer ---------------------------------------------------------------------------------------------------------
// LDS-DMA pieces (1 KiB per wave): M0 = LDS destination, written in the statement that uses it (cdna_hip_programming.md
// §5.7).  hipcc does not count these loads: the kernel waits for them itself with counted vmcnt.
// (No instruction offset: on an LDS-DMA load the immediate moves the LDS destination as well as the source address.)
__device__ __forceinline__ void dma_s(unsigned voff, const void* sbase, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %1" ::"v"(voff), "s"(sbase), "s"(lds_dst)
               : "memory");
}
__device__ __forceinline__ void dma_v(const void* gsrc, unsigned lds_dst) {
  asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off" ::"v"(gsrc), "s"(lds_dst) : "memory");
}
// dma_v for a kernel whose other LDS traffic is the compiler's: M0 is restored inside the statement
__device__ __forceinline__ void glds16(const void* gsrc, unsigned lds_dst) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_dst)
               : "memory");
}
template <int N>
__device__ __forceinline__ void wait_vmcnt() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}
template <int I, int E, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < E) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, E>(f);
  }
}
__device__ __forceinline__ unsigned lds_addr(const void* p) {
  return (unsigned)(size_t)(__attribute__((address_space(3))) const char*)p;
}
// source of the convolution taps that lie outside the image (one copy per translation unit: no relocatable device code)
[[maybe_unused]] static __device__ __attribute__((aligned(64))) float g_zero_page[16];

// ---- tile coordinates ------------------------------------------------------------------------------------------------------
// XCD-aware map: hardware deals consecutive workgroup ids round-robin to the 8 XCDs; give each XCD a contiguous range of tile
// ids (bijective for any grid size), so the n-tiles that share A rows hit the same L2
__device__ __forceinline__ int xcd_tile_id() {
  const int nwg = gridDim.x, xcd = blockIdx.x & 7, q8 = nwg >> 3, r8 = nwg & 7;
  return (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (blockIdx.x >> 3);
}
// tile id -> (tile_m, tile_n) over ntn column tiles: row-major, or (panel > 1, 256-row tiles) in panels of that many row
// blocks, column tile outer — the host code that picks `panel` says when (launch_split_pipe)
struct TileMN { int m, n; };
__device__ __forceinline__ TileMN tile_coords(int tile, int ntn, int panel = 0, int M = 0) {
  TileMN t;
  if (panel > 1) {
    const int ntm = (M + 255) >> 8, per = panel * ntn, p = tile / per, w = tile - p * per;
    const int rows = min(panel, ntm - p * panel);
    t.n = w / rows;
    t.m = p * panel + (w - t.n * rows);
  } else {
    t.m = tile / ntn;
    t.n = tile % ntn;
  }
  return t;
}

// ---- convolution k-tile decode ---------------------------------------------------------------------------------------------
// k-tile kt of a convolution with cpt 16-channel chunks per tap and ntaps taps, in the order gemm_split.hpp documents (32-channel
// group outer, tap, the group's chunks): declares tap, chunk (the 16-channel chunk; weight k-tile = tap * cpt + chunk) and the
// intermediates cps, sup, rem.  A macro for the same reason split_epilogue_body.hpp is an include: it sits inside the k-loop.
#define GDRNPP_CONV_KTILE(kt, cpt, ntaps)                                                                                  \
  const int cps = ((cpt) & 1) ? 1 : 2, sup = (kt) / ((ntaps) * cps), rem = (kt) - sup * ((ntaps) * cps), tap = rem / cps; \
  const int chunk = sup * cps + (rem - tap * cps)

// ---- GroupNorm statistics in the epilogue ----------------------------------------------------------------------------------
// GroupNorm statistics of the result, taken in the epilogue of the convolution that produces it (GNS): every wave writes
// the fp64 (sum, sum of squares) of its 64 rows x 8-channel groups to part[image][P][G][2], P = 4 * (256-row tiles per
// image), slot 4 * tile + wave — the layout gn_apply_kernel (net_kernels.hip) reduces, so the separate statistics pass over
// the stored tensor is not needed.  Requires 8 channels per group and images of a multiple of 256 pixels.
struct GnStats { double* part; int G; int tiles_per_img; };

// (gs, gss): a lane's four columns over its 16 rows of the 64-column half that starts at column col0 of the tile at row m0
__device__ __forceinline__ void gn_stats_fold(double gs, double gss, const GnStats& gn, int hw, int m0, int col0, int wave, int lane) {
  // a group's 8 channels are the column quads of lanes 2k, 2k+1; its 64 rows sit in the four 16-lane row groups
  gs += __shfl_xor(gs, 1, 64);   gss += __shfl_xor(gss, 1, 64);
  gs += __shfl_xor(gs, 16, 64);  gss += __shfl_xor(gss, 16, 64);
  gs += __shfl_xor(gs, 32, 64);  gss += __shfl_xor(gss, 32, 64);
  if ((lane & 0x31) == 0) {
    const int img = m0 / hw, mt = (m0 - img * hw) >> 8;
    const int g = (col0 >> 3) + (lane >> 1);
    double* o = gn.part + (((size_t)img * (4 * gn.tiles_per_img) + 4 * mt + wave) * gn.G + g) * 2;
    o[0] = gs;
    o[1] = gss;
  }
}

}  // namespace splitgemm
}  // namespace gdrnpp
