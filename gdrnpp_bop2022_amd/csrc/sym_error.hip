// Symmetry-aware reS / teS / projS of a batch of (estimate, ground truth) pairs on gfx950: the three errors the reference's
// BOP-toolkit fork adds beside re / te / proj and that its model configs ask for (VAL.ERROR_TYPES = "mspd,mssd,vsd,ad,reS,teS";
// lib/pysixd/scripts/eval_calc_errors.py:545-596 dispatches them, eval_pose_results_more.py:136-155 thresholds them at 2 / 5 / 10).
//
// Behavioural spec: lib/pysixd/pose_error.py:377-396 (re_sym), :420-437 (te_sym), :183-193 (arp_2d_sym) = :196-217 (proj_sym),
// lib/pysixd/misc.py:568-582 (project_pts: K (R p + t) divided by its third row, z not clamped).  For a pair with model points p and
// symmetries (S_R, S_t):
//   A_s = R_gt S_R,  b_s = R_gt S_t + t_gt
//   reS   = min_s rad2deg(acos(clamp(0.5 (min(trace(R_est A_s^T), 3) - 1), -1, 1)))
//   teS   = min_s | b_s - t_est |
//   projS = min_s mean_p | proj(R_est p + t_est) - proj(A_s p + b_s) |
//
// fp64 throughout (the results meet thresholds, the reference is fp64).  With K, two kernels on one stream, on the chunk scheme of
// pair_error.hpp (the composition into LDS, the walk over the model, the workspace, the host checks):
//   sym_error_points     the threads that compose the chunk's A_s, b_s take the O(1) errors of their symmetry there: re by re_deg, te as
//                        one norm.  Per (point, symmetry) ONE correctly rounded sqrt is added to that symmetry's running sum.  projS is
//                        a mean of norms, so the max-of-squares trick of bop_error.hip does not apply.  The sums have a fixed order: per
//                        thread in point order, a fixed shuffle tree per wave, the four waves in order; then one division by n per
//                        symmetry, and the minima over the chunk of all three errors go to the workspace.
//   pairs::finalize      one thread per pair takes the minima over the pair's chunks.
// Without K (projS not wanted) no work over the points is launched: ONE kernel,
//   sym_error_rt         a wave per pair, a lane per symmetry (stride 64), the same composition and the same re / te expressions
//                        (compose_rt below, one function for both paths: the two columns are bit-equal to the full call's), a minimum
//                        across the lanes, and NaN in the third column.  O(symmetries) per pair.
// No floating-point atomics; min does not depend on the order of its operands and every sum has one order, so two runs are bit-equal
// and a pair's result depends neither on its place in the launch nor on the other pairs.  A pair with equal poses and the identity among
// its symmetries gives projS == 0.0 and teS == 0.0 exactly.  Poses holding a NaN give unspecified results (a minimum drops a NaN operand).
// Roofline: compute-side.  Per (point, symmetry) evaluation ~58 fp64 VALU operations: 9 fma pose, 9 mul/fma for K, 13 for the IEEE
// reciprocal of the depth, 2 mul + 2 sub + 2 mul/fma for the squared 2-D distance (bop_error.hip's 2-D half, 37), then ~20 for the
// IEEE sqrt (v_rsq_f64, the scaling by ldexp, the Newton steps, the special-case selects) and 1 add; the per-point part (load,
// estimate pose, projection: ~35) is shared by the chunk's symmetries.  re / te: ~100 operations per (pair, symmetry), one thread
// each.  Algorithmic HBM bytes: 12 n per model (L2-resident across the pairs and chunks of a class), 96 per symmetry, 24 per
// workgroup written.
#include "pair_error.hpp"

using namespace gdrnpp::pairs;

namespace {

// X = [A_s | b_s] and, where it is composed, the two O(1) errors of the symmetry: re (degrees) from trace(R_est A_s^T)
// (pose_error.py:388-393), te = | b_s - t_est | (:433-435)
__device__ __forceinline__ void compose_rt(const double* __restrict__ Rg, const double* __restrict__ tg, const double* __restrict__ Re,
                                           const double* __restrict__ te_, const double* __restrict__ S, const double* __restrict__ St,
                                           double* X, double& re, double& te) {
  compose_xf(Rg, tg, S, St, X);
  re = re_deg(Re, X);
  const double d0 = X[9] - te_[0], d1 = X[10] - te_[1], d2 = X[11] - te_[2];
  te = sqrt(fma(d2, d2, fma(d1, d1, d0 * d0)));
}

__global__ __launch_bounds__(kThreads) void sym_error_points(
    const float* __restrict__ verts, const int* __restrict__ vert_off, int n_obj, const int* __restrict__ obj,
    const double* __restrict__ R_est, const double* __restrict__ t_est, const double* __restrict__ R_gt,
    const double* __restrict__ t_gt, const double* __restrict__ Kc, const double* __restrict__ sym_R,
    const double* __restrict__ sym_t, const int* __restrict__ sym_off, double* __restrict__ part, int nchunk_max) {
  __shared__ double s_xf[kSymChunk][kXf];
  __shared__ double s_rt[kSymChunk][2];
  __shared__ double s_sum[kWaves][kSymChunk];

  const size_t pair = blockIdx.x;
  const int chunk = blockIdx.y;
  const int o = obj[pair];
  if (o < 0 || o >= n_obj) return;
  const Chunk ck = chunk_of(o, sym_off, vert_off);
  if (ck.ns <= 0) return;
  const int ns = ck.ns;  // workgroup-uniform
  const int n = ck.n;    // an empty model still has its re / te; the finalize step gives it a NaN projS
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  if ((int)threadIdx.x < ns) {  // compose once per (pair, symmetry), and take re / te there
    double X[kXf], re, te;
    compose_rt(R_gt + 9 * pair, t_gt + 3 * pair, R_est + 9 * pair, t_est + 3 * pair, sym_R + 9 * (size_t)(ck.s0 + threadIdx.x),
               sym_t + 3 * (size_t)(ck.s0 + threadIdx.x), X, re, te);
#pragma unroll
    for (int k = 0; k < kXf; ++k) s_xf[threadIdx.x][k] = X[k];
    s_rt[threadIdx.x][0] = re;
    s_rt[threadIdx.x][1] = te;
  }
  __syncthreads();

  double E[kXf], K[9];
  load_est(R_est, t_est, Kc, pair, E, K);

  double acc[kSymChunk];  // this thread's sum of the 2-D distances, per symmetry, in point order
#pragma unroll
  for (int s = 0; s < kSymChunk; ++s) acc[s] = 0.0;

  walk_chunk(verts + 3 * (size_t)ck.v0, n, ns, E, K, s_xf,
             [](int s, double, double, double, double eu, double ev, double, double, double, double gu, double gv, double* acc)
                 __attribute__((always_inline)) {
               const double du = eu - gu, dv = ev - gv;
               acc[s] += sqrt(fma(dv, dv, du * du));  // IEEE sqrt: a mean of norms needs every one of them
             },
             acc);

  // fixed order: a shuffle tree per wave, then the four waves in order
#pragma unroll
  for (int s = 0; s < kSymChunk; ++s) {
    const double a = gdrnpp::wave::wave_sum_down(acc[s]);
    if (lane == 0) s_sum[wave][s] = a;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double best_re = INFINITY, best_te = INFINITY, best_pj = INFINITY;
    for (int s = 0; s < ns; ++s) {
      const double sum = ((s_sum[0][s] + s_sum[1][s]) + s_sum[2][s]) + s_sum[3][s];
      best_re = fmin(best_re, s_rt[s][0]);
      best_te = fmin(best_te, s_rt[s][1]);
      best_pj = fmin(best_pj, sum / (double)n);
    }
    double* out = part + 3 * (pair * (size_t)nchunk_max + chunk);
    out[0] = best_re;
    out[1] = best_te;
    out[2] = best_pj;
  }
}

// K == NULL: a wave per pair, a lane per symmetry, nothing over the points
__global__ __launch_bounds__(64) void sym_error_rt(int n_obj, const int* __restrict__ obj, const double* __restrict__ R_est,
                                                   const double* __restrict__ t_est, const double* __restrict__ R_gt,
                                                   const double* __restrict__ t_gt, const double* __restrict__ sym_R,
                                                   const double* __restrict__ sym_t, const int* __restrict__ sym_off,
                                                   double* __restrict__ out) {
  const size_t pair = blockIdx.x;
  const int o = obj[pair];
  const double nan = __builtin_nan("");
  double re = nan, te = nan;  // an obj outside [0, n_obj)
  if (o >= 0 && o < n_obj) {  // workgroup-uniform
    re = te = INFINITY;
    const int s1 = sym_off[o + 1];
    for (int s = sym_off[o] + (int)threadIdx.x; s < s1; s += 64) {
      double X[kXf], r, t;
      compose_rt(R_gt + 9 * pair, t_gt + 3 * pair, R_est + 9 * pair, t_est + 3 * pair, sym_R + 9 * (size_t)s, sym_t + 3 * (size_t)s, X, r, t);
      re = fmin(re, r);
      te = fmin(te, t);
    }
    re = gdrnpp::wave::wave_min(re);
    te = gdrnpp::wave::wave_min(te);
  }
  if (threadIdx.x == 0) {
    out[3 * pair] = re;
    out[3 * pair + 1] = te;
    out[3 * pair + 2] = nan;  // projS was not asked for
  }
}

}  // namespace

extern "C" {

size_t gdrnpp_sym_errors_workspace_bytes(const gdrnpp_meshes* models, const int* sym_off, int b) {
  return workspace_bytes(models, sym_off, b, 3);
}

int gdrnpp_sym_errors(const gdrnpp_meshes* models, const int* obj, const double* R_est, const double* t_est, const double* R_gt,
                      const double* t_gt, const double* K, const double* sym_R, const double* sym_t, const int* sym_off,
                      double* out, int b, void* workspace, size_t workspace_bytes, void* stream) {
  int* d_off;
  double* part;
  int nchunk_max;
  // K alone may be NULL: projS is then not computed
  const int rc = prepare("gdrnpp_sym_errors", models, obj && R_est && t_est && R_gt && t_gt && sym_R && sym_t && out, sym_off, b, 3,
                         workspace, workspace_bytes, stream, &d_off, &part, &nchunk_max);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (!K) {  // pairs on grid.x (b above 65 535 is ordinary)
    hipLaunchKernelGGL(sym_error_rt, dim3(b), dim3(64), 0, st, models->n_obj, obj, R_est, t_est, R_gt, t_gt, sym_R, sym_t, d_off, out);
    return gdrnpp::check_launch("gdrnpp_sym_errors");
  }
  // pairs on grid.x, the chunks of kSymChunk symmetries on grid.y
  hipLaunchKernelGGL(sym_error_points, dim3(b, nchunk_max), dim3(kThreads), 0, st, models->verts, models->vert_off, models->n_obj,
                     obj, R_est, t_est, R_gt, t_gt, K, sym_R, sym_t, d_off, part, nchunk_max);
  hipLaunchKernelGGL((finalize<3, 2>), dim3((b + 63) / 64), dim3(64), 0, st, models->vert_off, models->n_obj, obj, d_off, part, out,
                     nchunk_max, b);
  return gdrnpp::check_launch("gdrnpp_sym_errors");
}

}  // extern "C"
