// GDRN's training losses on gfx950: the terms of gdrn_loss (core/gdrn_modeling/models/GDRN_double_mask.py:287-536) that every shipped
// config uses, with their gradients and no host synchronisation.
//
//   gdrnpp_gdrn_dense_losses           one pass over the geometry head's maps: the xyz terms (L1 or CE_coor), the two mask terms (L1 or
//                                      BCE with logits) and the region cross-entropy, as eight fp64 sums (six numerators, two mask counts)
//   gdrnpp_gdrn_dense_losses_backward  recomputes from the same inputs and writes d(loss)/d(map) for every map that is asked for
//   gdrnpp_gdrn_pose_losses            per ROI: the closest symmetric ground-truth rotation, the point-matching term, centroid and z
//
// Dense design: one lane per pixel of the flattened [B, o, o] plane (kPix pixels per lane at a stride of kThreads), so that at every step
// of the channel loop a wave reads 64 consecutive floats of one channel plane (NCHW: the channel stride is o * o floats).  A pixel whose
// mask is 0 has logits out * 0 = 0 whatever out holds, so its loads are predicated off: it costs log C and no traffic.  For C = 65, the only
// count a shipped config has, the 65 logits of a pixel live in registers between the maximum, the exponentials and (backward) the
// gradient, so each is read once; other C >= 2 walk the planes once per pass (maximum, sum, gradient).  The op is memory bound: the forward
// reads each map once, the backward reads each once and writes each gradient once.
//
// Arithmetic: per-pixel terms in fp32 as the reference forms them (out * m, gt * m, log-softmax as (l_t - max) - log(sum exp(l - max))),
// accumulated in fp64.  Every workgroup writes its eight partial sums to the workspace and a second kernel adds them in workgroup order:
// no floating-point atomics, two runs give the same bits.  A class target outside [0, C) is counted in an integer word and the pixel is
// left out of sum and gradient.
//
// Pose design: one workgroup per ROI, all arithmetic in fp64.  The candidates R_gt S_k are scored by the threads in parallel (re_deg of
// pair_error.hpp) and reduced to the (smallest re, then smallest index) pair, which is what the reference's sequential scan with a strict
// `<` arrives at; the unmodified R_gt is candidate -1.  The threads then walk the object's model points with a stride of kThreads and keep
// 13 accumulators (the term and its derivative with respect to R_pred and t_pred); per-ROI partials are added in ROI order by a second kernel.
#include "common.hpp"
#include "pair_error.hpp"

namespace {

using gdrnpp::wave::wave_sum_down;

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kPix = 1;                        // pixels per lane of the dense kernels: a batch of 48 ROIs is 3072 waves, under half of what
                                               // the chip holds, so every pixel gets a lane of its own (4 per lane left a SIMD under one wave)
constexpr int kTile = kThreads * kPix;         // pixels per workgroup
constexpr int kCols = 8;                       // x, y, z, mask, full mask, region numerators; xyz and region mask counts
constexpr int kRegC = 65;                      // the channel count that is held in registers

enum { kL1 = 0, kCE = 1, kBCE = 1 };

struct DenseArgs {
  const float *out_x, *out_y, *out_z, *out_mask, *out_full, *out_region;
  const float* gt_xyz;
  const unsigned char* gt_bin;
  const int* gt_region;
  const float* m[4];                           // trunc, visib, obj, full
  int Cx, Cr, xyz_type, xyz_mask, mask_type, mask_gt, full_type, region_mask;
  int n, hw;                                   // n = B * hw pixels
  // forward
  double* part;
  int* bad;
  // backward
  const double* sums;
  const float* scale;                          // [6] grad_output * weight per term
  float *g_x, *g_y, *g_z, *g_mask, *g_full, *g_region;
};

// ---- the masked cross-entropy of one pixel -------------------------------------------------------------------------------------------
// base: channel 0 of the pixel, stride: floats between channels, m: the mask value, t: the masked target (checked by the caller).
// kGrad: g (same layout as base) receives (softmax - onehot) * m * s.  Returns log(sum) - (l_t - max).

template <bool kGrad>
__device__ __forceinline__ float ce_regs(const float* __restrict__ base, size_t stride, float m, int t, float* __restrict__ g, float s) {
  float v[kRegC];
  const bool on = m != 0.f;
#pragma unroll
  for (int c = 0; c < kRegC; ++c) v[c] = on ? base[c * stride] * m : 0.f;
  float mx = v[0];
#pragma unroll
  for (int c = 1; c < kRegC; ++c) mx = fmaxf(mx, v[c]);
  float lt = 0.f;
#pragma unroll
  for (int c = 0; c < kRegC; ++c) lt = c == t ? v[c] : lt;
  float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
  for (int c = 0; c < kRegC; ++c) {
    v[c] = expf(v[c] - mx);
    if ((c & 3) == 0) a0 += v[c];
    else if ((c & 3) == 1) a1 += v[c];
    else if ((c & 3) == 2) a2 += v[c];
    else a3 += v[c];
  }
  const float sum = (a0 + a1) + (a2 + a3);
  if (kGrad) {
    const float inv = 1.f / sum, ms = m * s;
#pragma unroll
    for (int c = 0; c < kRegC; ++c) g[c * stride] = (v[c] * inv - (c == t ? 1.f : 0.f)) * ms;
  }
  return logf(sum) - (lt - mx);
}

template <bool kGrad>
__device__ __forceinline__ float ce_any(const float* __restrict__ base, size_t stride, int C, float m, int t, float* __restrict__ g, float s) {
  const bool on = m != 0.f;
  float mx = on ? base[0] * m : 0.f;
  for (int c = 1; c < C; ++c) mx = fmaxf(mx, on ? base[c * stride] * m : 0.f);
  float sum = 0.f;
  for (int c = 0; c < C; ++c) sum += expf((on ? base[c * stride] * m : 0.f) - mx);
  const float lt = on ? base[t * stride] * m : 0.f;
  if (kGrad) {
    const float inv = 1.f / sum, ms = m * s;
    for (int c = 0; c < C; ++c) g[c * stride] = (expf((on ? base[c * stride] * m : 0.f) - mx) * inv - (c == t ? 1.f : 0.f)) * ms;
  }
  return logf(sum) - (lt - mx);
}

// One cross-entropy term of pixel (b, q): value into acc (forward) or gradient into g (backward).  t_raw is the target before masking.
template <bool kGrad>
__device__ __forceinline__ void ce_term(const float* out, int C, int hw, int b, int q, float m, int t_raw, double& acc, int* bad, float* g,
                                        float s) {
  const size_t off = ((size_t)b * C) * hw + q;
  const int t = t_raw * (int)m;                // gt * mask.long()
  if (t < 0 || t >= C) {
    if (kGrad) {
      for (int c = 0; c < C; ++c) g[off + (size_t)c * hw] = 0.f;
    } else {
      atomicAdd(bad, 1);
    }
    return;
  }
  float v;
  if (C == kRegC) v = ce_regs<kGrad>(out + off, (size_t)hw, m, t, kGrad ? g + off : nullptr, s);
  else v = ce_any<kGrad>(out + off, (size_t)hw, C, m, t, kGrad ? g + off : nullptr, s);
  if (!kGrad) acc += (double)v;
}

__device__ __forceinline__ float sign_of(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }

// BCEWithLogits of one element: max(x, 0) - x z + log(1 + exp(-|x|))
__device__ __forceinline__ float bce_logits(float x, float z) { return (fmaxf(x, 0.f) - x * z) + log1pf(expf(-fabsf(x))); }

__device__ __forceinline__ float sigmoid_of(float x) {
  const float e = expf(-fabsf(x));
  return x >= 0.f ? 1.f / (1.f + e) : e / (1.f + e);
}

template <bool kGrad>
__global__ __launch_bounds__(kThreads) void dense_kernel(const DenseArgs a) {
  __shared__ double s_red[kWaves][kCols];
  const int tid = threadIdx.x, hw = a.hw;
  double acc[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) acc[c] = 0.0;
  float s_reg = 0.f, s_mask = 0.f, s_full = 0.f;
  float sc[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (kGrad) {
    const double d_xyz = fmax(a.sums[6], 1.0), d_reg = fmax(a.sums[7], 1.0), d_all = (double)a.n;
#pragma unroll
    for (int c = 0; c < 3; ++c) sc[c] = (float)((double)a.scale[c] / d_xyz);
    s_mask = (float)((double)a.scale[3] / d_all);
    s_full = (float)((double)a.scale[4] / d_all);
    s_reg = (float)((double)a.scale[5] / d_reg);
  }
  const float* outs[3] = {a.out_x, a.out_y, a.out_z};
  float* gs[3] = {a.g_x, a.g_y, a.g_z};
  const bool do_xyz = kGrad ? (a.g_x || a.g_y || a.g_z) : a.out_x != nullptr;
  const bool do_reg = kGrad ? a.g_region != nullptr : a.out_region != nullptr;
  const bool do_mask = kGrad ? a.g_mask != nullptr : a.out_mask != nullptr;
  const bool do_full = kGrad ? a.g_full != nullptr : a.out_full != nullptr;

  for (int k = 0; k < kPix; ++k) {
    const long long pl = (long long)blockIdx.x * kTile + (long long)k * kThreads + tid;
    if (pl >= a.n) break;
    const int p = (int)pl, b = p / hw, q = p - b * hw;
    if (do_xyz) {
      const float m = a.m[a.xyz_mask][p];
      if (!kGrad) acc[6] += (double)m;
      for (int c = 0; c < 3; ++c) {
        if (kGrad && !gs[c]) continue;
        if (a.xyz_type == kL1) {
          const size_t o1 = (size_t)b * hw + q;
          const float d = outs[c][o1] * m - a.gt_xyz[((size_t)b * 3 + c) * hw + q] * m;
          if (kGrad) gs[c][o1] = sign_of(d) * m * sc[c];
          else acc[c] += (double)fabsf(d);
        } else {
          ce_term<kGrad>(outs[c], a.Cx, hw, b, q, m, (int)a.gt_bin[((size_t)b * 3 + c) * hw + q], acc[c], a.bad, gs[c], sc[c]);
        }
      }
    }
    if (do_mask) {
      const float x = a.out_mask[p], z = a.m[a.mask_gt][p];
      if (a.mask_type == kL1) {
        if (kGrad) a.g_mask[p] = sign_of(x - z) * s_mask;
        else acc[3] += (double)fabsf(x - z);
      } else {
        if (kGrad) a.g_mask[p] = (sigmoid_of(x) - z) * s_mask;
        else acc[3] += (double)bce_logits(x, z);
      }
    }
    if (do_full) {
      const float x = a.out_full[p], z = a.m[3][p];
      if (a.full_type == kL1) {
        if (kGrad) a.g_full[p] = sign_of(x - z) * s_full;
        else acc[4] += (double)fabsf(x - z);
      } else {
        if (kGrad) a.g_full[p] = (sigmoid_of(x) - z) * s_full;
        else acc[4] += (double)bce_logits(x, z);
      }
    }
    if (do_reg) {
      const float m = a.m[a.region_mask][p];
      if (!kGrad) acc[7] += (double)m;
      ce_term<kGrad>(a.out_region, a.Cr, hw, b, q, m, a.gt_region[p], acc[5], a.bad, a.g_region, s_reg);
    }
  }
  if (kGrad) return;
  const int wave = tid >> 6, lane = tid & 63;
#pragma unroll
  for (int c = 0; c < kCols; ++c) {
    const double v = wave_sum_down(acc[c]);
    if (lane == 0) s_red[wave][c] = v;
  }
  __syncthreads();
  if (tid < kCols) {
    double v = s_red[0][tid];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) v += s_red[w][tid];
    a.part[(size_t)blockIdx.x * kCols + tid] = v;
  }
}

// sums[c] = part[0][c] + part[1][c] + ... in index order.  One wave per column: its lanes fetch 64 partials at a time (independent
// loads), then every lane adds them in index order, each read from its lane by v_readlane.  (One thread per column walking the
// workspace, a chain of dependent loads, took 0.16 us per partial.)
__global__ __launch_bounds__(64 * kCols) void sum_partials(const double* __restrict__ part, int n_part, int cols, double* __restrict__ sums) {
  const int c = threadIdx.x >> 6, lane = threadIdx.x & 63;
  if (c >= cols) return;      // wave-uniform
  double acc = 0.0;
  for (int i0 = 0; i0 < n_part; i0 += 64) {
    const int i = i0 + lane;
    const double v = i < n_part ? part[(size_t)i * cols + c] : 0.0;
    const int n = min(64, n_part - i0), lo = __double2loint(v), hi = __double2hiint(v);
    // l is wave-uniform: two v_readlane_b32 into scalar registers, no LDS crossbar
    if (n == 64) {
#pragma unroll
      for (int l = 0; l < 64; ++l) acc += __hiloint2double(__builtin_amdgcn_readlane(hi, l), __builtin_amdgcn_readlane(lo, l));
    } else {
      for (int l = 0; l < n; ++l) acc += __hiloint2double(__builtin_amdgcn_readlane(hi, l), __builtin_amdgcn_readlane(lo, l));
    }
  }
  if (lane == 0) sums[c] = acc;
}

int dense_checks(const char* fn, const DenseArgs& a, int B, int o, bool have_xyz, bool have_region) {
  GDRNPP_REQUIRE(B > 0 && o > 0, GDRNPP_EINVAL, "%s: B=%d o=%d", fn, B, o);
  GDRNPP_REQUIRE((long long)B * o * o <= 0x7fffffffLL / 256, GDRNPP_ELIMIT, "%s: B * o * o = %lld pixels > %d", fn, (long long)B * o * o,
                 0x7fffffff / 256);
  for (int sel : {a.xyz_mask, a.mask_gt, a.region_mask})
    GDRNPP_REQUIRE(sel >= 0 && sel <= 3, GDRNPP_EINVAL, "%s: mask selector %d outside 0..3 (trunc, visib, obj, full)", fn, sel);
  for (int ty : {a.xyz_type, a.mask_type, a.full_type}) GDRNPP_REQUIRE(ty == 0 || ty == 1, GDRNPP_EINVAL, "%s: loss type %d outside 0..1", fn, ty);
  if (have_xyz) {
    GDRNPP_REQUIRE(a.out_x && a.out_y && a.out_z, GDRNPP_EINVAL, "%s: out_x, out_y, out_z come together", fn);
    GDRNPP_REQUIRE(a.m[a.xyz_mask], GDRNPP_EINVAL, "%s: the xyz term selects mask %d, which is null", fn, a.xyz_mask);
    if (a.xyz_type == kL1) {
      GDRNPP_REQUIRE(a.Cx == 1, GDRNPP_EINVAL, "%s: the L1 xyz term takes Cx = 1, got %d", fn, a.Cx);
      GDRNPP_REQUIRE(a.gt_xyz, GDRNPP_EINVAL, "%s: gt_xyz is null", fn);
    } else {
      GDRNPP_REQUIRE(a.Cx >= 2 && a.Cx <= 256, GDRNPP_EINVAL, "%s: the CE_coor xyz term takes 2 <= Cx <= 256, got %d", fn, a.Cx);
      GDRNPP_REQUIRE(a.gt_bin, GDRNPP_EINVAL, "%s: gt_xyz_bin is null", fn);
    }
  }
  if (have_region) {
    GDRNPP_REQUIRE(a.Cr >= 2, GDRNPP_EINVAL, "%s: the region term takes Cr >= 2, got %d", fn, a.Cr);
    GDRNPP_REQUIRE(a.gt_region, GDRNPP_EINVAL, "%s: gt_region is null", fn);
    GDRNPP_REQUIRE(a.m[a.region_mask], GDRNPP_EINVAL, "%s: the region term selects mask %d, which is null", fn, a.region_mask);
  }
  return 0;
}

// ---- pose terms ------------------------------------------------------------------------------------------------------------------------

constexpr int kPoseAcc = 13;                   // the PM sum, d/dR_pred (9), d/dt_pred (3)
enum { kPmL1 = 0, kPmSmoothL1 = 1, kPmMSE = 2 };

struct PoseArgs {
  const float *R_pred, *R_gt, *t_pred, *t_gt;
  const int* obj;
  const float* points;
  int n_obj, P;
  const double* sym_rots;
  const int* sym_off;
  int n_sym_total;
  const float* extents;
  const float *pred_t_, *gt_trans_ratio, *gt_trans;
  int symmetric, r_only, z_type, pm_type;
  double beta;
  double* part;                                // [B, 3]
  float *R_sel, *dR, *dt, *dpt;
};

// R_gt S, each element (a0 s0 + a1 s1) + a2 s2 without contraction: tests/losses_ref.py forms the same expression
__device__ __forceinline__ void rot_times(const double* Rg, const double* S, double* X) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) X[3 * r + c] = (Rg[3 * r] * S[c] + Rg[3 * r + 1] * S[3 + c]) + Rg[3 * r + 2] * S[6 + c];
  }
}

__global__ __launch_bounds__(kThreads) void pose_kernel(const PoseArgs a) {
  __shared__ double s_best[kWaves];
  __shared__ int s_idx[kWaves];
  __shared__ double s_red[kWaves][kPoseAcc];
  const int i = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int o = a.obj[i];
  const bool obj_ok = o >= 0 && o < a.n_obj;
  double Rp[9], Rg[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) { Rp[k] = (double)a.R_pred[9 * (size_t)i + k]; Rg[k] = (double)a.R_gt[9 * (size_t)i + k]; }

  // ---- the closest symmetric ground truth: smallest re, earliest candidate; candidate -1 is R_gt itself
  int s0 = 0, ns = 0;
  if (a.symmetric && obj_ok && a.sym_rots && a.sym_off) {
    s0 = a.sym_off[o];
    const int s1 = a.sym_off[o + 1];
    if (s0 >= 0 && s1 <= a.n_sym_total && s1 > s0) ns = s1 - s0;   // workgroup-uniform
  }
  if (ns > 0) {
    double best = gdrnpp::pairs::re_deg(Rp, Rg);
    int idx = -1;
    for (int k = tid; k < ns; k += kThreads) {
      double S[9], X[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) S[e] = a.sym_rots[9 * (size_t)(s0 + k) + e];
      rot_times(Rg, S, X);
      const double r = gdrnpp::pairs::re_deg(Rp, X);
      if (r < best) { best = r; idx = k; }      // k ascends within a thread: strict < keeps the earliest
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const double ob = __shfl_xor(best, off, 64);
      const int oi = __shfl_xor(idx, off, 64);
      if (ob < best || (ob == best && oi < idx)) { best = ob; idx = oi; }
    }
    if (lane == 0) { s_best[wave] = best; s_idx[wave] = idx; }
    __syncthreads();
    best = s_best[0]; idx = s_idx[0];
#pragma unroll
    for (int w = 1; w < kWaves; ++w) {
      if (s_best[w] < best || (s_best[w] == best && s_idx[w] < idx)) { best = s_best[w]; idx = s_idx[w]; }
    }
    if (idx >= 0) {
      double S[9], X[9];
#pragma unroll
      for (int e = 0; e < 9; ++e) S[e] = a.sym_rots[9 * (size_t)(s0 + idx) + e];
      rot_times(Rg, S, X);
#pragma unroll
      for (int e = 0; e < 9; ++e) Rg[e] = X[e];
    }
  }
  if (tid < 9 && a.R_sel) a.R_sel[9 * (size_t)i + tid] = (float)Rg[tid];

  // ---- point matching
  double w = 1.0;
  if (a.extents && obj_ok) {
    const float* e = a.extents + 3 * (size_t)o;
    w = 1.0 / (double)fmaxf(e[0], fmaxf(e[1], e[2]));
  }
  double tp[3] = {0.0, 0.0, 0.0}, tg[3] = {0.0, 0.0, 0.0};
  if (!a.r_only) {
#pragma unroll
    for (int k = 0; k < 3; ++k) { tp[k] = (double)a.t_pred[3 * (size_t)i + k]; tg[k] = (double)a.t_gt[3 * (size_t)i + k]; }
  }
  double acc[kPoseAcc];
#pragma unroll
  for (int k = 0; k < kPoseAcc; ++k) acc[k] = 0.0;
  if (obj_ok) {
    const float* pts = a.points + (size_t)o * a.P * 3;
    for (int j = tid; j < a.P; j += kThreads) {
      const double p[3] = {(double)pts[3 * j], (double)pts[3 * j + 1], (double)pts[3 * j + 2]};
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        const double est = (Rp[3 * r] * p[0] + Rp[3 * r + 1] * p[1] + Rp[3 * r + 2] * p[2]) + tp[r];
        const double tgt = (Rg[3 * r] * p[0] + Rg[3 * r + 1] * p[1] + Rg[3 * r + 2] * p[2]) + tg[r];
        const double d = w * est - w * tgt, ad = fabs(d);
        double v, g;
        if (a.pm_type == kPmMSE) { v = d * d; g = 2.0 * d; }
        else if (a.pm_type == kPmSmoothL1 && a.beta >= 1e-5 && ad < a.beta) { v = 0.5 * d * d / a.beta; g = d / a.beta; }
        else {
          v = a.pm_type == kPmSmoothL1 && a.beta >= 1e-5 ? ad - 0.5 * a.beta : ad;
          g = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
        }
        const double gw = g * w;
        acc[0] += v;
        acc[1 + 3 * r] += gw * p[0];
        acc[2 + 3 * r] += gw * p[1];
        acc[3 + 3 * r] += gw * p[2];
        acc[10 + r] += gw;
      }
    }
  }
#pragma unroll
  for (int k = 0; k < kPoseAcc; ++k) {
    const double v = wave_sum_down(acc[k]);
    if (lane == 0) s_red[wave][k] = v;
  }
  __syncthreads();
  if (tid < kPoseAcc) {
    double v = s_red[0][tid];
#pragma unroll
    for (int wv = 1; wv < kWaves; ++wv) v += s_red[wv][tid];
    if (!obj_ok) v = tid == 0 ? __builtin_nan("") : 0.0;   // the binding checks obj; a ROI outside the table poisons the sum, reads nothing
    if (tid == 0) a.part[3 * (size_t)i] = v;
    else if (tid < 10) a.dR[9 * (size_t)i + tid - 1] = (float)v;
    else if (a.dt) a.dt[3 * (size_t)i + tid - 10] = a.r_only ? 0.f : (float)v;
  }

  // ---- centroid and z: L1 of pred_t_[:2] against gt_trans_ratio[:2], of pred_t_[2] against gt_trans_ratio[2] (REL) or gt_trans[2] (ABS)
  if (tid == 0) {
    double c = 0.0, z = 0.0;
    if (a.pred_t_) {
      const float* pt = a.pred_t_ + 3 * (size_t)i;
      const float* ratio = a.gt_trans_ratio + 3 * (size_t)i;
      const double d0 = (double)pt[0] - (double)ratio[0], d1 = (double)pt[1] - (double)ratio[1];
      const double gz = a.z_type == 0 ? (double)ratio[2] : (double)a.gt_trans[3 * (size_t)i + 2];
      const double d2 = (double)pt[2] - gz;
      c = fabs(d0) + fabs(d1);
      z = fabs(d2);
      a.dpt[3 * (size_t)i] = d0 > 0.0 ? 1.f : (d0 < 0.0 ? -1.f : 0.f);
      a.dpt[3 * (size_t)i + 1] = d1 > 0.0 ? 1.f : (d1 < 0.0 ? -1.f : 0.f);
      a.dpt[3 * (size_t)i + 2] = d2 > 0.0 ? 1.f : (d2 < 0.0 ? -1.f : 0.f);
    }
    a.part[3 * (size_t)i + 1] = c;
    a.part[3 * (size_t)i + 2] = z;
  }
}

}  // namespace

extern "C" {

size_t gdrnpp_gdrn_dense_losses_workspace_bytes(int B, int o) {
  if (B <= 0 || o <= 0 || (long long)B * o * o > 0x7fffffffLL / 256) return 0;
  const long long n = (long long)B * o * o;
  return sizeof(double) * kCols * (size_t)((n + kTile - 1) / kTile);
}

int gdrnpp_gdrn_dense_losses(const float* out_x, const float* out_y, const float* out_z, int Cx, const float* out_mask,
                             const float* out_mask_full, const float* out_region, int Cr, const float* gt_xyz,
                             const unsigned char* gt_xyz_bin, const int* gt_region, const float* mask_trunc, const float* mask_visib,
                             const float* mask_obj, const float* mask_full, int xyz_type, int xyz_mask, int mask_type, int mask_gt,
                             int full_type, int region_mask, int B, int o, double* sums, int* bad_targets, void* workspace,
                             size_t workspace_bytes, void* stream) {
  const char* const fn = "gdrnpp_gdrn_dense_losses";
  DenseArgs a{};
  a.out_x = out_x; a.out_y = out_y; a.out_z = out_z; a.out_mask = out_mask; a.out_full = out_mask_full; a.out_region = out_region;
  a.gt_xyz = gt_xyz; a.gt_bin = gt_xyz_bin; a.gt_region = gt_region;
  a.m[0] = mask_trunc; a.m[1] = mask_visib; a.m[2] = mask_obj; a.m[3] = mask_full;
  a.Cx = Cx; a.Cr = Cr; a.xyz_type = xyz_type; a.xyz_mask = xyz_mask; a.mask_type = mask_type; a.mask_gt = mask_gt; a.full_type = full_type;
  a.region_mask = region_mask;
  const bool have_xyz = out_x || out_y || out_z;
  if (int rc = dense_checks(fn, a, B, o, have_xyz, out_region != nullptr)) return rc;
  GDRNPP_REQUIRE(sums && bad_targets, GDRNPP_EINVAL, "%s: sums / bad_targets is null", fn);
  if (out_mask) GDRNPP_REQUIRE(a.m[mask_gt], GDRNPP_EINVAL, "%s: the mask term selects mask %d, which is null", fn, mask_gt);
  if (out_mask_full) GDRNPP_REQUIRE(mask_full, GDRNPP_EINVAL, "%s: the full-mask term needs mask_full, which is null", fn);
  const size_t need = gdrnpp_gdrn_dense_losses_workspace_bytes(B, o);
  GDRNPP_REQUIRE(workspace && workspace_bytes >= need, GDRNPP_EINVAL, "%s: workspace %zu < %zu bytes", fn, workspace ? workspace_bytes : (size_t)0,
                 need);
  a.n = B * o * o; a.hw = o * o;
  a.part = (double*)workspace; a.bad = bad_targets;
  const int n_part = (a.n + kTile - 1) / kTile;
  GDRNPP_HIP_TRY(hipMemsetAsync(bad_targets, 0, sizeof(int), (hipStream_t)stream));
  hipLaunchKernelGGL(dense_kernel<false>, dim3((unsigned)n_part), dim3(kThreads), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(sum_partials, dim3(1), dim3(64 * kCols), 0, (hipStream_t)stream, (const double*)a.part, n_part, kCols, sums);
  return gdrnpp::check_launch(fn);
}

int gdrnpp_gdrn_dense_losses_backward(const float* out_x, const float* out_y, const float* out_z, int Cx, const float* out_mask,
                                      const float* out_mask_full, const float* out_region, int Cr, const float* gt_xyz,
                                      const unsigned char* gt_xyz_bin, const int* gt_region, const float* mask_trunc,
                                      const float* mask_visib, const float* mask_obj, const float* mask_full, int xyz_type, int xyz_mask,
                                      int mask_type, int mask_gt, int full_type, int region_mask, int B, int o, const double* sums,
                                      const float* scale, float* grad_x, float* grad_y, float* grad_z, float* grad_mask,
                                      float* grad_mask_full, float* grad_region, void* stream) {
  const char* const fn = "gdrnpp_gdrn_dense_losses_backward";
  DenseArgs a{};
  a.out_x = out_x; a.out_y = out_y; a.out_z = out_z; a.out_mask = out_mask; a.out_full = out_mask_full; a.out_region = out_region;
  a.gt_xyz = gt_xyz; a.gt_bin = gt_xyz_bin; a.gt_region = gt_region;
  a.m[0] = mask_trunc; a.m[1] = mask_visib; a.m[2] = mask_obj; a.m[3] = mask_full;
  a.Cx = Cx; a.Cr = Cr; a.xyz_type = xyz_type; a.xyz_mask = xyz_mask; a.mask_type = mask_type; a.mask_gt = mask_gt; a.full_type = full_type;
  a.region_mask = region_mask;
  const bool want_xyz = grad_x || grad_y || grad_z;
  if (int rc = dense_checks(fn, a, B, o, want_xyz, grad_region != nullptr)) return rc;
  GDRNPP_REQUIRE(sums && scale, GDRNPP_EINVAL, "%s: sums / scale is null", fn);
  GDRNPP_REQUIRE(!grad_region || out_region, GDRNPP_EINVAL, "%s: grad_region without out_region", fn);
  if (grad_mask) GDRNPP_REQUIRE(out_mask && a.m[mask_gt], GDRNPP_EINVAL, "%s: grad_mask needs out_mask and mask %d", fn, mask_gt);
  if (grad_mask_full) GDRNPP_REQUIRE(out_mask_full && mask_full, GDRNPP_EINVAL, "%s: grad_mask_full needs out_mask_full and mask_full", fn);
  if (!(want_xyz || grad_mask || grad_mask_full || grad_region)) return 0;
  a.n = B * o * o; a.hw = o * o;
  a.sums = sums; a.scale = scale;
  a.g_x = grad_x; a.g_y = grad_y; a.g_z = grad_z; a.g_mask = grad_mask; a.g_full = grad_mask_full; a.g_region = grad_region;
  const int n_part = (a.n + kTile - 1) / kTile;
  hipLaunchKernelGGL(dense_kernel<true>, dim3((unsigned)n_part), dim3(kThreads), 0, (hipStream_t)stream, a);
  return gdrnpp::check_launch(fn);
}

size_t gdrnpp_gdrn_pose_losses_workspace_bytes(int B) { return B > 0 ? sizeof(double) * 3 * (size_t)B : 0; }

int gdrnpp_gdrn_pose_losses(const float* R_pred, const float* R_gt, const float* t_pred, const float* t_gt, const int* obj,
                            const float* points, int n_obj, int P, const double* sym_rots, const int* sym_off, int n_sym_total,
                            const float* extents, const float* pred_t_, const float* gt_trans_ratio, const float* gt_trans, int symmetric,
                            int r_only, int z_type, int pm_type, double beta, int B, double* sums, float* R_gt_sel, float* dR_pred,
                            float* dt_pred, float* dpred_t_, void* workspace, size_t workspace_bytes, void* stream) {
  const char* const fn = "gdrnpp_gdrn_pose_losses";
  GDRNPP_REQUIRE(B > 0 && B <= 0x7fffffff / 16, GDRNPP_EINVAL, "%s: B=%d", fn, B);
  GDRNPP_REQUIRE(n_obj > 0 && P > 0, GDRNPP_EINVAL, "%s: n_obj=%d P=%d", fn, n_obj, P);
  GDRNPP_REQUIRE((long long)n_obj * P <= 0x7fffffffLL / 3, GDRNPP_ELIMIT, "%s: n_obj * P = %lld points", fn, (long long)n_obj * P);
  GDRNPP_REQUIRE(R_pred && R_gt && obj && points, GDRNPP_EINVAL, "%s: R_pred / R_gt / obj / points is null", fn);
  GDRNPP_REQUIRE(sums && dR_pred, GDRNPP_EINVAL, "%s: sums / dR_pred is null", fn);
  GDRNPP_REQUIRE(r_only || (t_pred && t_gt && dt_pred), GDRNPP_EINVAL, "%s: r_only = 0 needs t_pred, t_gt and dt_pred", fn);
  GDRNPP_REQUIRE(!symmetric || (sym_rots && sym_off && n_sym_total >= 0) || n_sym_total == 0, GDRNPP_EINVAL,
                 "%s: symmetric needs sym_rots and sym_off", fn);
  GDRNPP_REQUIRE(z_type == 0 || z_type == 1, GDRNPP_EINVAL, "%s: z_type=%d outside 0..1 (REL, ABS)", fn, z_type);
  GDRNPP_REQUIRE(pm_type >= 0 && pm_type <= 2, GDRNPP_EINVAL, "%s: pm_type=%d outside 0..2 (L1, Smooth_L1, MSE)", fn, pm_type);
  if (pred_t_) {
    GDRNPP_REQUIRE(gt_trans_ratio && dpred_t_, GDRNPP_EINVAL, "%s: pred_t_ needs gt_trans_ratio and dpred_t_", fn);
    GDRNPP_REQUIRE(z_type == 0 || gt_trans, GDRNPP_EINVAL, "%s: z_type ABS needs gt_trans", fn);
  }
  const size_t need = gdrnpp_gdrn_pose_losses_workspace_bytes(B);
  GDRNPP_REQUIRE(workspace && workspace_bytes >= need, GDRNPP_EINVAL, "%s: workspace %zu < %zu bytes", fn, workspace ? workspace_bytes : (size_t)0,
                 need);
  PoseArgs a{};
  a.R_pred = R_pred; a.R_gt = R_gt; a.t_pred = t_pred; a.t_gt = t_gt; a.obj = obj; a.points = points; a.n_obj = n_obj; a.P = P;
  a.sym_rots = n_sym_total > 0 ? sym_rots : nullptr; a.sym_off = sym_off; a.n_sym_total = n_sym_total; a.extents = extents;
  a.pred_t_ = pred_t_; a.gt_trans_ratio = gt_trans_ratio; a.gt_trans = gt_trans;
  a.symmetric = symmetric; a.r_only = r_only; a.z_type = z_type; a.pm_type = pm_type; a.beta = beta;
  a.part = (double*)workspace; a.R_sel = R_gt_sel; a.dR = dR_pred; a.dt = dt_pred; a.dpt = dpred_t_;
  hipLaunchKernelGGL(pose_kernel, dim3((unsigned)B), dim3(kThreads), 0, (hipStream_t)stream, a);
  hipLaunchKernelGGL(sum_partials, dim3(1), dim3(64 * kCols), 0, (hipStream_t)stream, (const double*)a.part, B, 3, sums);
  return gdrnpp::check_launch(fn);
}

}  // extern "C"
