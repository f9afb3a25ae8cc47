// Pose errors of a batch of (estimate, ground truth) pairs on gfx950: ad (ADD or ADI), re, te, proj of the reference's
// GDRN_EvaluatorCustom (core/gdrn_modeling/engine/gdrn_custom_evaluator.py:672-730).
//
// Behavioural spec: lib/pysixd/pose_error.py:256-296 (add, adi), :359-374 (re), :406-417 (te), :440-445 (arp_2d),
// lib/pysixd/misc.py transform_pts_Rt / transform_pts_Rt_2d, core/utils/pose_utils.py:472-496 (get_closest_rot).
//
// Three kernels on one stream, every sum in a fixed order (no floating-point atomics: two runs are bit-equal):
//   pose_error_prologue   one thread per pair, fp64: te, the closest symmetric ground-truth rotation (symmetries visited in
//                         order, replaced on a strictly smaller re), re, and the ground-truth pose expressed in the
//                         estimate's model frame  Rrel = R_est^T R_gt,  trel = R_est^T (t_gt - t_est)
//   pose_error_points     a workgroup of 4 waves owns 256 model points of one pair, one per thread for the O(n) part in fp64:
//                         the ADD term |(R_est p + t_est) - (R_gt p + t_gt)| and the reprojection term.  A symmetric class runs
//                         the ADI search instead of the ADD term: rigid motions keep distances, so the nearest estimated-posed
//                         point of R_gt p_j + t_gt is as far away as the nearest RAW model point of q_j = Rrel p_j + trel.
//                         q_j is formed in fp64 and rounded once to fp32; the targets of every pair of a class are then the
//                         same resident model, object-sized coordinates, streamed through LDS in 1024-point float4 tiles as
//                         in nnd.hip: each wave scans its quarter of a tile with broadcast ds_read_b128 and the four minima
//                         merge in LDS (no index, so ties do not matter).  Unlike nnd.hip a lane carries four queries, so
//                         that one LDS read feeds four evaluations: with one query per lane the LDS set the pace (measured
//                         19 % of the fp32 VALU rate).  sqrt and the sum of the minima are fp64.  The per-point terms are
//                         added by a fixed shuffle tree per wave, the four waves in order; the workgroup's two partial sums
//                         go to the workspace.
//   pose_error_finalize   one thread per pair adds the partials in block order and divides by n.
// Workgroups beyond a pair's own point count exit; non-symmetric pairs skip the search on a workgroup-uniform branch.
// Roofline: the search is compute-side, 6.5 fp32 VALU operations per (query, target) (3 sub, 3 fma, half a min3); the O(n) part is
// ~60 fp64 operations per point.  Algorithmic HBM bytes: 12 n per model (L2-resident across the pairs of a class) + 16 per workgroup written.
#include "pair_error.hpp"
#include <cfloat>

using gdrnpp::pairs::re_deg;          // the trace form sym_error.hip takes its reS from
using gdrnpp::wave::wave_sum_down;

namespace {

constexpr int kWavesPerWG = 4;  // waves that split each target tile
constexpr int kPts = 256;       // model points per workgroup: one per thread in the O(n) part
constexpr int kQPerLane = 4;    // queries per lane in the search: every wave holds all kPts queries
static_assert(kPts == 64 * kWavesPerWG && kPts == 64 * kQPerLane, "one point per thread, kQPerLane per lane");
constexpr int kTile = 1024;     // targets per LDS tile (16 KiB as float4)
constexpr int kUnroll = 4;    // targets per trip of the scan loop (a tile and a wave's share of it are multiples)
constexpr int kPro = 24;        // doubles per pair of the prologue record
// prologue record: [0..8] R_gt_sym, [9..17] Rrel, [18..20] trel, [21] re (deg), [22] te, [23] unused

__global__ __launch_bounds__(64) void pose_error_prologue(
    const int* __restrict__ obj, int n_obj, const double* __restrict__ R_est, const double* __restrict__ t_est,
    const double* __restrict__ R_gt, const double* __restrict__ t_gt, const double* __restrict__ sym_rots,
    const int* __restrict__ sym_off, const unsigned char* __restrict__ symmetric, double* __restrict__ pro, int b) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= b) return;
  const double* Re = R_est + 9 * (size_t)i;
  const double* te_ = t_est + 3 * (size_t)i;
  const double* tg = t_gt + 3 * (size_t)i;
  double Rg[9], Rs[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rs[k] = Rg[k] = R_gt[9 * (size_t)i + k];
  double re = re_deg(Re, Rg);
  const int o = obj[i];
  if (o >= 0 && o < n_obj && symmetric && symmetric[o] && sym_rots && sym_off) {
    const int s1 = sym_off[o + 1];
    for (int s = sym_off[o]; s < s1; ++s) {
      const double* S = sym_rots + 9 * (size_t)s;
      double C[9];  // R_gt . S
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) C[3 * r + c] = (Rg[3 * r] * S[c] + Rg[3 * r + 1] * S[3 + c]) + Rg[3 * r + 2] * S[6 + c];
      const double cur = re_deg(Re, C);
      if (cur < re) {
        re = cur;
#pragma unroll
        for (int k = 0; k < 9; ++k) Rs[k] = C[k];
      }
    }
  }
  double* P = pro + kPro * (size_t)i;
#pragma unroll
  for (int k = 0; k < 9; ++k) P[k] = Rs[k];
  const double d0 = tg[0] - te_[0], d1 = tg[1] - te_[1], d2 = tg[2] - te_[2];
  // the ADI frame uses the UNMODIFIED R_gt (gdrn_custom_evaluator.py:699-705)
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) P[9 + 3 * r + c] = (Re[r] * Rg[c] + Re[3 + r] * Rg[3 + c]) + Re[6 + r] * Rg[6 + c];
    P[18 + r] = (Re[r] * d0 + Re[3 + r] * d1) + Re[6 + r] * d2;
  }
  P[21] = re;
  P[22] = sqrt((d0 * d0 + d1 * d1) + d2 * d2);
  P[23] = 0.0;
}

__global__ __launch_bounds__(kPts) void pose_error_points(
    const float* __restrict__ verts, const int* __restrict__ vert_off, int n_obj, const int* __restrict__ obj,
    const double* __restrict__ R_est, const double* __restrict__ t_est, const double* __restrict__ t_gt,
    const double* __restrict__ Kc, const unsigned char* __restrict__ symmetric, const double* __restrict__ pro,
    double* __restrict__ part, int nblk_max) {
  __shared__ float4 tile[kTile];
  __shared__ float4 s_q[kPts];
  __shared__ float s_d[kWavesPerWG][kPts];
  __shared__ double s_sum[kWavesPerWG][2];

  const size_t pair = blockIdx.x;
  const int blk = blockIdx.y;
  const int o = obj[pair];
  if (o < 0 || o >= n_obj) return;
  const int v0 = vert_off[o];
  const int n = vert_off[o + 1] - v0;
  if (blk * kPts >= n) return;  // workgroups beyond this pair's point count
  const bool sym = symmetric && symmetric[o];  // workgroup-uniform
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // tells the compiler that the scan bounds are wave-uniform

  const float* mv = verts + 3 * (size_t)v0;
  const double* P = pro + kPro * pair;
  const int j = blk * kPts + threadIdx.x;  // this thread's model point
  const bool live = j < n;
  double px = 0.0, py = 0.0, pz = 0.0;
  if (live) { px = (double)mv[3 * j]; py = (double)mv[3 * j + 1]; pz = (double)mv[3 * j + 2]; }

  float best = FLT_MAX;
  if (sym) {
    // the thread's point as a query in the estimate's model frame: fp64, rounded once
    s_q[threadIdx.x] = make_float4((float)(((P[9] * px + P[10] * py) + P[11] * pz) + P[18]),
                                   (float)(((P[12] * px + P[13] * py) + P[14] * pz) + P[19]),
                                   (float)(((P[15] * px + P[16] * py) + P[17] * pz) + P[20]), 0.f);
    __syncthreads();
    // every wave holds all kPts queries, kQPerLane per lane, and scans its quarter of each tile: one broadcast LDS read
    // serves kQPerLane distance evaluations per lane (with one query per lane the LDS, not the VALU, sets the pace)
    float qx[kQPerLane], qy[kQPerLane], qz[kQPerLane], bq[kQPerLane];
#pragma unroll
    for (int i = 0; i < kQPerLane; ++i) {
      const float4 q = s_q[lane + 64 * i];
      qx[i] = q.x; qy[i] = q.y; qz[i] = q.z; bq[i] = FLT_MAX;
    }
    for (int k0 = 0; k0 < n; k0 += kTile) {
      const int cnt = min(kTile, n - k0);
      const int cnt_up = (cnt + kUnroll - 1) & ~(kUnroll - 1);  // <= kTile; the tail is filled with entries that add infinity
      __syncthreads();
      for (int k = threadIdx.x; k < cnt_up; k += kPts) {
        const float* p = mv + 3 * (size_t)(k0 + k);
        // w is added to the squared distance: 0 for a model point, +inf for the padding
        tile[k] = k < cnt ? make_float4(p[0], p[1], p[2], 0.f) : make_float4(0.f, 0.f, 0.f, INFINITY);
      }
      __syncthreads();
      const int lo = wave * (kTile / kWavesPerWG);
      const int hi = min(cnt_up, lo + kTile / kWavesPerWG);
      for (int k = lo; k < hi; k += kUnroll) {  // no remainder loop: lo, hi and cnt_up are multiples of kUnroll
#pragma unroll
        for (int u = 0; u < kUnroll; u += 2) {
          const float4 p = tile[k + u], r = tile[k + u + 1];  // wave-uniform addresses: LDS broadcast, ds_read_b128
#pragma unroll
          for (int i = 0; i < kQPerLane; ++i) {
            const float dx = p.x - qx[i], dy = p.y - qy[i], dz = p.z - qz[i];
            const float ex = r.x - qx[i], ey = r.y - qy[i], ez = r.z - qz[i];
            // explicit fma (the build has -ffp-contract=off) and one three-way minimum per two targets: 6.5 VALU operations
            // per evaluation.  The minimum is written as the instruction because fminf's quieting of a possible signalling
            // NaN costs a v_max per operand; no operand can be a NaN unless the poses are.
            const float d = fmaf(dz, dz, fmaf(dy, dy, fmaf(dx, dx, p.w))), e = fmaf(ez, ez, fmaf(ey, ey, fmaf(ex, ex, r.w)));
            asm("v_min3_f32 %0, %0, %1, %2" : "+v"(bq[i]) : "v"(d), "v"(e));
          }
        }
      }
    }
#pragma unroll
    for (int i = 0; i < kQPerLane; ++i) s_d[wave][lane + 64 * i] = bq[i];
    __syncthreads();
    const int t = threadIdx.x;
    best = fminf(fminf(s_d[0][t], s_d[1][t]), fminf(s_d[2][t], s_d[3][t]));
  }

  // the per-point terms in fp64, one point per thread
  const double* Re = R_est + 9 * pair;
  const double* te_ = t_est + 3 * pair;
  const double* tg = t_gt + 3 * pair;
  const double* K = Kc + 9 * pair;
  double ad = 0.0, pj = 0.0;
  if (live) {
    const double ex = ((Re[0] * px + Re[1] * py) + Re[2] * pz) + te_[0];
    const double ey = ((Re[3] * px + Re[4] * py) + Re[5] * pz) + te_[1];
    const double ez = ((Re[6] * px + Re[7] * py) + Re[8] * pz) + te_[2];
    // R_gt_sym: equal to R_gt for a non-symmetric class, so ADD and proj share the transformed point
    const double gx = ((P[0] * px + P[1] * py) + P[2] * pz) + tg[0];
    const double gy = ((P[3] * px + P[4] * py) + P[5] * pz) + tg[1];
    const double gz = ((P[6] * px + P[7] * py) + P[8] * pz) + tg[2];
    if (sym) {
      ad = sqrt((double)best);
    } else {
      const double dx = ex - gx, dy = ey - gy, dz = ez - gz;
      ad = sqrt((dx * dx + dy * dy) + dz * dz);
    }
    // transform_pts_Rt_2d: K (R p + t), divided by its third row; z is not clamped
    const double eu = (K[0] * ex + K[1] * ey) + K[2] * ez, ev = (K[3] * ex + K[4] * ey) + K[5] * ez;
    const double ew = (K[6] * ex + K[7] * ey) + K[8] * ez;
    const double gu = (K[0] * gx + K[1] * gy) + K[2] * gz, gv = (K[3] * gx + K[4] * gy) + K[5] * gz;
    const double gw = (K[6] * gx + K[7] * gy) + K[8] * gz;
    const double du = eu / ew - gu / gw, dv = ev / ew - gv / gw;
    pj = sqrt(du * du + dv * dv);
  }
  // fixed order: a shuffle tree per wave, then the four waves in order
  ad = wave_sum_down(ad);
  pj = wave_sum_down(pj);
  if (lane == 0) { s_sum[wave][0] = ad; s_sum[wave][1] = pj; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* out = part + 2 * (pair * (size_t)nblk_max + blk);
    out[0] = ((s_sum[0][0] + s_sum[1][0]) + s_sum[2][0]) + s_sum[3][0];
    out[1] = ((s_sum[0][1] + s_sum[1][1]) + s_sum[2][1]) + s_sum[3][1];
  }
}

__global__ __launch_bounds__(64) void pose_error_finalize(const int* __restrict__ vert_off, int n_obj,
                                                          const int* __restrict__ obj, const double* __restrict__ pro,
                                                          const double* __restrict__ part, double* __restrict__ out,
                                                          int nblk_max, int b) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= b) return;
  const double* P = pro + kPro * (size_t)i;
  const int o = obj[i];
  const double nan = __builtin_nan("");
  double ad = nan, pj = nan;
  if (o >= 0 && o < n_obj) {
    const int n = vert_off[o + 1] - vert_off[o];
    const int nblk = (n + kPts - 1) / kPts;
    if (n > 0 && nblk <= nblk_max) {  // a model larger than the set's max_verts hint has no complete sum
      const double* p = part + 2 * ((size_t)i * nblk_max);
      double sa = 0.0, sp = 0.0;
      for (int k = 0; k < nblk; ++k) { sa += p[2 * k]; sp += p[2 * k + 1]; }
      ad = sa / (double)n;
      pj = sp / (double)n;
    }
  }
  double* r = out + 4 * (size_t)i;
  r[0] = ad;
  r[1] = P[21];
  r[2] = P[22];
  r[3] = pj;
}

inline int blocks_of(const gdrnpp_meshes* m) { return (m->max_verts + kPts - 1) / kPts; }

}  // namespace

extern "C" {

size_t gdrnpp_pose_errors_workspace_bytes(const gdrnpp_meshes* models, int b) {
  if (!models || b <= 0 || models->max_verts <= 0) return 0;
  return sizeof(double) * ((size_t)kPro * b + 2 * (size_t)b * blocks_of(models));
}

int gdrnpp_pose_errors(const gdrnpp_meshes* models, const int* obj, const double* R_est, const double* t_est,
                       const double* R_gt, const double* t_gt, const double* K, const double* sym_rots,
                       const int* sym_off, const unsigned char* symmetric, double* out, int b, void* workspace,
                       size_t workspace_bytes, void* stream) {
  GDRNPP_REQUIRE(models && models->verts && models->vert_off && models->n_obj > 0, GDRNPP_EINVAL,
                 "gdrnpp_pose_errors: no models");
  GDRNPP_REQUIRE(models->max_verts > 0, GDRNPP_EINVAL, "gdrnpp_pose_errors: models->max_verts must be set");
  GDRNPP_REQUIRE(obj && R_est && t_est && R_gt && t_gt && K && out, GDRNPP_EINVAL, "gdrnpp_pose_errors: null pointer");
  GDRNPP_REQUIRE((sym_rots == nullptr) == (sym_off == nullptr), GDRNPP_EINVAL,
                 "gdrnpp_pose_errors: sym_rots and sym_off come together");
  GDRNPP_REQUIRE(b > 0, GDRNPP_EINVAL, "gdrnpp_pose_errors: b=%d", b);
  const int nblk_max = blocks_of(models);
  GDRNPP_REQUIRE(nblk_max <= 65535, GDRNPP_ELIMIT, "gdrnpp_pose_errors: max_verts=%d > %d", models->max_verts, 65535 * kPts);
  const size_t need = gdrnpp_pose_errors_workspace_bytes(models, b);
  GDRNPP_REQUIRE(workspace && workspace_bytes >= need, GDRNPP_EINVAL, "gdrnpp_pose_errors: workspace %zu < %zu bytes",
                 workspace ? workspace_bytes : (size_t)0, need);
  hipStream_t st = (hipStream_t)stream;
  double* pro = (double*)workspace;
  double* part = pro + (size_t)kPro * b;
  const int nb = (b + 63) / 64;
  hipLaunchKernelGGL(pose_error_prologue, dim3(nb), dim3(64), 0, st, obj, models->n_obj, R_est, t_est, R_gt, t_gt, sym_rots,
                     sym_off, symmetric, pro, b);
  // pairs on grid.x (b above 65 535 is ordinary), the pair's 256-point blocks on grid.y
  hipLaunchKernelGGL(pose_error_points, dim3(b, nblk_max), dim3(kPts), 0, st, models->verts, models->vert_off,
                     models->n_obj, obj, R_est, t_est, t_gt, K, symmetric, pro, part, nblk_max);
  hipLaunchKernelGGL(pose_error_finalize, dim3(nb), dim3(64), 0, st, models->vert_off, models->n_obj, obj, pro, part, out,
                     nblk_max, b);
  return gdrnpp::check_launch("gdrnpp_pose_errors");
}

}  // extern "C"
