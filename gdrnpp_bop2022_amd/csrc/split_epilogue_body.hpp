// The epilogue of every split-GEMM kernel, included once per kernel behind its k-loop (textual, not a function: a helper that is
// simplified on its own before inlining loses the known bits of `lane` and moves the register allocation of the k-loop,
// profiles/refactor_split_gemm_isa.md).  The wave's EPI_TILES_M x 2*EPI_HALVES MFMA 32x32 tiles go to C rows EPI_ROW0 ..,
// columns EPI_COL0 ..: a lane holds column (lane & 31) of rows (r&3) + 8*(r>>2) + 4*(lane>>5) of a tile.  Each wave parks one
// 16x64 slice at a time in its [16][65] floats of EPI_STAGE (the A stages, dead once the k-loop has ended on a barrier) and
// writes it back row-wise as float4 with bias / GELU / gamma * v + resid applied.
//
// From the kernel: EPI, lane, wave, gamma, resid, C, M, N.  The including kernel defines (all are undefined again below)
//   EPI_TILES_M, EPI_HALVES   32-row MFMA tiles per wave, 64-column halves per wave
//   EPI_ACC(i, j)             accumulator of row tile i, 32-column tile j
//   EPI_ROW0, EPI_COL0        first row / column of the wave's part of C
//   EPI_BIAS                  bias pointer (may be null)
//   EPI_STAGE, EPI_STAGE_BYTES  the dead A stages
// and optionally
//   EPI_SCALE                 the accumulator is multiplied by it (2^-e of a scaled packed weight)
//   EPI_N_STORE               columns >= it are not written
//   EPI_GN                    GnStats of the launch: under `if (GNS)` the fp64 statistics of the stored values (uses cg, m0)
//   EPI_RANGE_BAD             bool that collects "a stored value is inf / NaN"; with it, c_rows != 0 (bias / GELU epilogues)
//                             writes C as "f16x2 rows" (split2_common.hpp)
{
  static_assert(EPI_STAGE_BYTES >= 4 * 16 * 65 * sizeof(float), "epilogue staging fits the A images");
  float* T = reinterpret_cast<float*>(EPI_STAGE) + wave * 16 * 65;  // [16][65] per wave
  const int c4 = (lane & 15) * 4;
#pragma unroll
  for (int jh = 0; jh < EPI_HALVES; ++jh) {
    const int nb = EPI_COL0 + jh * 64 + c4;
    const float4 bv = EPI_BIAS ? *reinterpret_cast<const float4*>(EPI_BIAS + nb) : make_float4(0.f, 0.f, 0.f, 0.f);
    float4 gv = make_float4(1.f, 1.f, 1.f, 1.f);
    if (EPI == EPI_SCALE_RES) gv = *reinterpret_cast<const float4*>(gamma + nb);
#ifdef EPI_GN
    double gs = 0.0, gss = 0.0;  // GNS: this lane's four columns over its 16 rows
#endif
#pragma unroll
    for (int ih = 0; ih < 2 * EPI_TILES_M; ++ih) {
      const int i = ih >> 1, h = ih & 1;  // 32-row MFMA tile i, its 16-row half h (accumulator registers h*8 .. h*8+7)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int r = 0; r < 8; ++r)
          T[((r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)) * 65 + j * 32 + (lane & 31)] = EPI_ACC(i, jh * 2 + j)[h * 8 + r];
      __builtin_amdgcn_s_waitcnt(0xc07f);  // lgkmcnt(0): same wave reads back
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        const int row = rr * 4 + (lane >> 4);
        const float* t = T + row * 65 + c4;
#ifdef EPI_SCALE
        float4 v = make_float4(t[0] * EPI_SCALE + bv.x, t[1] * EPI_SCALE + bv.y, t[2] * EPI_SCALE + bv.z, t[3] * EPI_SCALE + bv.w);
#else
        float4 v = make_float4(t[0] + bv.x, t[1] + bv.y, t[2] + bv.z, t[3] + bv.w);
#endif
        const int grow = EPI_ROW0 + i * 32 + h * 16 + row;
#ifdef EPI_N_STORE
        if (grow >= M || nb >= EPI_N_STORE) continue;
#else
        if (grow >= M) continue;  // overhang of the last m-tile
#endif
        const size_t off = (size_t)grow * N + nb;
#ifdef EPI_GN
        if (GNS) {
          gs += ((double)v.x + (double)v.y) + ((double)v.z + (double)v.w);
          gss += ((double)v.x * v.x + (double)v.y * v.y) + ((double)v.z * v.z + (double)v.w * v.w);
        }
#endif
        if (EPI == EPI_GELU) { v.x = gelu_erf(v.x); v.y = gelu_erf(v.y); v.z = gelu_erf(v.z); v.w = gelu_erf(v.w); }
        if (EPI == EPI_SCALE_RES) {
          const float4 rs = *reinterpret_cast<const float4*>(resid + off);
          v.x = rs.x + gv.x * v.x; v.y = rs.y + gv.y * v.y; v.z = rs.z + gv.z * v.z; v.w = rs.w + gv.w * v.w;
        }
        // streaming stores: the result is not read again by this kernel, keep it from displacing the weights in L2
        // (-4 % on the fc1 shapes, whose output is 4x their input)
#ifdef EPI_RANGE_BAD
        constexpr unsigned kInfNan = 0x203u;   // v_cmp_class_f32: signalling / quiet NaN, -inf, +inf
        EPI_RANGE_BAD |= __builtin_amdgcn_class(v.x, kInfNan) | __builtin_amdgcn_class(v.y, kInfNan) |
                         __builtin_amdgcn_class(v.z, kInfNan) | __builtin_amdgcn_class(v.w, kInfNan);
        if (EPI != EPI_SCALE_RES && c_rows) {   // lanes 2k / 2k + 1 hold columns 8k .. 8k + 3 / 8k + 4 .. 8k + 7 of the same row
          const uint4 o = f16x2_rows_quad(v.x, v.y, v.z, v.w, lane & 1);
          const f32x4v t4 = {__uint_as_float(o.x), __uint_as_float(o.y), __uint_as_float(o.z), __uint_as_float(o.w)};
          __builtin_nontemporal_store(t4, reinterpret_cast<f32x4v*>(C + off));
        } else
#endif
#ifdef GDRNPP_TIMING_NO_STORE   // timing-only build (results invalid): the epilogue without its global stores
        if (v.x == 1.2345e38f) C[off] = v.y;
#else
        { const f32x4v t4 = {v.x, v.y, v.z, v.w}; __builtin_nontemporal_store(t4, reinterpret_cast<f32x4v*>(C + off)); }
#endif
      }
      __builtin_amdgcn_s_waitcnt(0xc07f);  // reads done before the next slice overwrites T
    }
#ifdef EPI_GN
    if (GNS) gn_stats_fold(gs, gss, EPI_GN, cg.H * cg.W, m0, EPI_COL0 + jh * 64, wave, lane);
#endif
  }
}
#undef EPI_TILES_M
#undef EPI_HALVES
#undef EPI_ACC
#undef EPI_ROW0
#undef EPI_COL0
#undef EPI_BIAS
#undef EPI_STAGE
#undef EPI_STAGE_BYTES
#undef EPI_SCALE
#undef EPI_N_STORE
#undef EPI_GN
#undef EPI_RANGE_BAD
