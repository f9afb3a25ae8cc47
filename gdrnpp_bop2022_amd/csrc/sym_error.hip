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
// fp64 throughout (the results meet thresholds, the reference is fp64).  With K, two kernels on one stream:
//   sym_error_points     a workgroup of 4 waves owns one (pair, chunk of kSymChunk symmetries), as bop_error_points does.  Its first
//                        threads compose the chunk's A_s, b_s once (12 doubles each) into LDS and, where they compose them, take the
//                        O(1) errors of their symmetry: re by the trace form of pose_error.hip's re_deg, te as one norm.  Every thread
//                        then walks the model with stride 256: the estimate-posed point and its projection are formed once per point
//                        and stay in registers, each symmetry of the chunk is read from LDS at a wave-uniform address (a broadcast), and
//                        ONE correctly rounded sqrt per (point, symmetry) is added to that symmetry's running sum.  projS is a mean of
//                        norms, so the max-of-squares trick of bop_error.hip does not apply.  The sums have a fixed order: per thread in
//                        point order, a fixed shuffle tree per wave, the four waves in order; then one division by n per symmetry, and
//                        the minima over the chunk of all three errors go to the workspace.
//   sym_error_finalize   one thread per pair takes the minima over the pair's chunks.
// Without K (projS not wanted) no work over the points is launched: ONE kernel,
//   sym_error_rt         a wave per pair, a lane per symmetry (stride 64), the same composition and the same re / te expressions
//                        (compose_rt below, one function for both paths: the two columns are bit-equal to the full call's), a minimum
//                        across the lanes, and NaN in the third column.  O(symmetries) per pair.
// No floating-point atomics; min does not depend on the order of its operands and every sum has one order, so two runs are bit-equal
// and a pair's result depends neither on its place in the launch nor on the other pairs.  Workgroups beyond an object's symmetry
// count exit on a workgroup-uniform branch.  The estimate and the ground truth are posed and projected by the same expression, so a
// pair with equal poses and the identity among its symmetries gives projS == 0.0 and teS == 0.0 exactly.  Poses holding a NaN give
// unspecified results (a minimum drops a NaN operand).
// Roofline: compute-side.  Per (point, symmetry) evaluation ~58 fp64 VALU operations: 9 fma pose, 9 mul/fma for K, 13 for the IEEE
// reciprocal of the depth, 2 mul + 2 sub + 2 mul/fma for the squared 2-D distance (bop_error.hip's 2-D half, 37), then ~20 for the
// IEEE sqrt (v_rsq_f64, the scaling by ldexp, the Newton steps, the special-case selects) and 1 add; the per-point part (load,
// estimate pose, projection: ~35) is shared by the chunk's symmetries.  re / te: ~100 operations per (pair, symmetry), one thread
// each.  Algorithmic HBM bytes: 12 n per model (L2-resident across the pairs and chunks of a class), 96 per symmetry, 24 per
// workgroup written.
#include "common.hpp"
#include <cmath>

namespace {

constexpr int kThreads = 256;   // 4 waves; a thread's points are tid, tid + 256, ...
constexpr int kWaves = kThreads / 64;
constexpr int kSymChunk = 8;    // symmetries per workgroup: one running sum each per thread
constexpr int kXf = 12;         // doubles per composed transform: A_s row-major, then b_s

__device__ __forceinline__ double wave_sum_fixed(double v) {
  // fixed tree over the 64 lanes: the same order in every run
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ double wave_min(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
  return v;
}

// R p + t, one expression for the estimate and for every ground-truth transform
__device__ __forceinline__ void pose_pt(const double* __restrict__ X, double px, double py, double pz, double& x, double& y,
                                        double& z) {
  x = fma(X[0], px, fma(X[1], py, fma(X[2], pz, X[9])));
  y = fma(X[3], px, fma(X[4], py, fma(X[5], pz, X[10])));
  z = fma(X[6], px, fma(X[7], py, fma(X[8], pz, X[11])));
}

__device__ __forceinline__ void project_pt(const double* __restrict__ K, double x, double y, double z, double& u, double& v) {
  const double a = fma(K[0], x, fma(K[1], y, K[2] * z));
  const double c = fma(K[3], x, fma(K[4], y, K[5] * z));
  const double w = fma(K[6], x, fma(K[7], y, K[8] * z));
  const double inv = 1.0 / w;  // z is not clamped (misc.py:581)
  u = a * inv;
  v = c * inv;
}

// X = [A_s | b_s] = [R_gt S_R | R_gt S_t + t_gt] and, where it is composed, the two O(1) errors of the symmetry:
// re (degrees) from trace(R_est A_s^T) = sum_ik R_est[i][k] A_s[i][k] (pose_error.py:388-393), te = | b_s - t_est | (:433-435)
__device__ __forceinline__ void compose_rt(const double* __restrict__ Rg, const double* __restrict__ tg, const double* __restrict__ Re,
                                           const double* __restrict__ te_, const double* __restrict__ S, const double* __restrict__ St,
                                           double* X, double& re, double& te) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) X[3 * r + c] = fma(Rg[3 * r + 2], S[6 + c], fma(Rg[3 * r + 1], S[3 + c], Rg[3 * r] * S[c]));
    X[9 + r] = fma(Rg[3 * r + 2], St[2], fma(Rg[3 * r + 1], St[1], Rg[3 * r] * St[0])) + tg[r];
  }
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) tr += (Re[3 * i] * X[3 * i] + Re[3 * i + 1] * X[3 * i + 1]) + Re[3 * i + 2] * X[3 * i + 2];
  tr = tr <= 3.0 ? tr : 3.0;
  const double c = fmin(1.0, fmax(-1.0, 0.5 * (tr - 1.0)));
  re = acos(c) * (180.0 / 3.14159265358979323846);
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
  const int s0 = sym_off[o] + chunk * kSymChunk;
  const int ns = min(kSymChunk, sym_off[o + 1] - s0);  // workgroup-uniform
  if (ns <= 0) return;                                 // workgroups beyond this object's symmetry count
  const int v0 = vert_off[o];
  const int n = vert_off[o + 1] - v0;                  // an empty model still has its re / te; the finalize step gives it a NaN projS
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  if ((int)threadIdx.x < ns) {  // compose once per (pair, symmetry), and take re / te there
    double X[kXf], re, te;
    compose_rt(R_gt + 9 * pair, t_gt + 3 * pair, R_est + 9 * pair, t_est + 3 * pair, sym_R + 9 * (size_t)(s0 + threadIdx.x),
               sym_t + 3 * (size_t)(s0 + threadIdx.x), X, re, te);
#pragma unroll
    for (int k = 0; k < kXf; ++k) s_xf[threadIdx.x][k] = X[k];
    s_rt[threadIdx.x][0] = re;
    s_rt[threadIdx.x][1] = te;
  }
  __syncthreads();

  double E[kXf], K[9];  // the estimate's transform and the intrinsics: the same for every thread of the workgroup
#pragma unroll
  for (int k = 0; k < 9; ++k) { E[k] = R_est[9 * pair + k]; K[k] = Kc[9 * pair + k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) E[9 + k] = t_est[3 * pair + k];

  double acc[kSymChunk];  // this thread's sum of the 2-D distances, per symmetry, in point order
#pragma unroll
  for (int s = 0; s < kSymChunk; ++s) acc[s] = 0.0;

  const float* mv = verts + 3 * (size_t)v0;
  // as in bop_error_points: the next point is loaded before the current one is evaluated, and the chunk's independent symmetries
  // supply the parallelism
  int j = threadIdx.x;
  float fx = 0.f, fy = 0.f, fz = 0.f;
  if (j < n) { fx = mv[3 * j]; fy = mv[3 * j + 1]; fz = mv[3 * j + 2]; }
  for (; j < n; j += kThreads) {
    const double px = (double)fx, py = (double)fy, pz = (double)fz;
    if (j + kThreads < n) { fx = mv[3 * (j + kThreads)]; fy = mv[3 * (j + kThreads) + 1]; fz = mv[3 * (j + kThreads) + 2]; }
    double ex, ey, ez, eu, ev;
    pose_pt(E, px, py, pz, ex, ey, ez);
    project_pt(K, ex, ey, ez, eu, ev);
#pragma unroll
    for (int s = 0; s < kSymChunk; ++s) {
      if (s < ns) {  // wave-uniform
        double gx, gy, gz, gu, gv;
        pose_pt(s_xf[s], px, py, pz, gx, gy, gz);  // wave-uniform LDS address: a broadcast read
        project_pt(K, gx, gy, gz, gu, gv);
        const double du = eu - gu, dv = ev - gv;
        acc[s] += sqrt(fma(dv, dv, du * du));  // IEEE sqrt: a mean of norms needs every one of them
      }
    }
  }

  // fixed order: a shuffle tree per wave, then the four waves in order
#pragma unroll
  for (int s = 0; s < kSymChunk; ++s) {
    const double a = wave_sum_fixed(acc[s]);
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

__global__ __launch_bounds__(64) void sym_error_finalize(const int* __restrict__ vert_off, int n_obj, const int* __restrict__ obj,
                                                         const int* __restrict__ sym_off, const double* __restrict__ part,
                                                         double* __restrict__ out, int nchunk_max, int b) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= b) return;
  const int o = obj[i];
  const double nan = __builtin_nan("");
  double re = nan, te = nan, pj = nan;  // an obj outside [0, n_obj)
  if (o >= 0 && o < n_obj) {
    const int nchunk = (sym_off[o + 1] - sym_off[o] + kSymChunk - 1) / kSymChunk;
    const double* p = part + 3 * ((size_t)i * nchunk_max);
    re = te = pj = INFINITY;
    for (int k = 0; k < nchunk; ++k) { re = fmin(re, p[3 * k]); te = fmin(te, p[3 * k + 1]); pj = fmin(pj, p[3 * k + 2]); }
    if (vert_off[o + 1] - vert_off[o] <= 0) pj = nan;  // an empty model has no projections
  }
  out[3 * (size_t)i] = re;
  out[3 * (size_t)i + 1] = te;
  out[3 * (size_t)i + 2] = pj;
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
    re = wave_min(re);
    te = wave_min(te);
  }
  if (threadIdx.x == 0) {
    out[3 * pair] = re;
    out[3 * pair + 1] = te;
    out[3 * pair + 2] = nan;  // projS was not asked for
  }
}

// bytes of the device copy of sym_off at the head of the workspace, kept 16-byte aligned
inline size_t off_bytes(int n_obj) { return (sizeof(int) * ((size_t)n_obj + 1) + 15) & ~(size_t)15; }

// the largest symmetry count of an object, or -1 if the offsets do not start at 0, decrease, or leave an object without a transform
inline int max_syms(const int* sym_off, int n_obj) {
  if (sym_off[0] != 0) return -1;
  int m = 0;
  for (int o = 0; o < n_obj; ++o) {
    const int c = sym_off[o + 1] - sym_off[o];
    if (c <= 0) return -1;
    m = c > m ? c : m;
  }
  return m;
}

}  // namespace

extern "C" {

size_t gdrnpp_sym_errors_workspace_bytes(const gdrnpp_meshes* models, const int* sym_off, int b) {
  if (!models || !sym_off || b <= 0 || models->n_obj <= 0) return 0;
  const int m = max_syms(sym_off, models->n_obj);
  if (m <= 0) return 0;
  return off_bytes(models->n_obj) + sizeof(double) * 3 * (size_t)b * ((m + kSymChunk - 1) / kSymChunk);
}

int gdrnpp_sym_errors(const gdrnpp_meshes* models, const int* obj, const double* R_est, const double* t_est, const double* R_gt,
                      const double* t_gt, const double* K, const double* sym_R, const double* sym_t, const int* sym_off,
                      double* out, int b, void* workspace, size_t workspace_bytes, void* stream) {
  GDRNPP_REQUIRE(models && models->verts && models->vert_off && models->n_obj > 0, GDRNPP_EINVAL, "gdrnpp_sym_errors: no models");
  // K alone may be NULL: projS is then not computed
  GDRNPP_REQUIRE(obj && R_est && t_est && R_gt && t_gt && sym_R && sym_t && sym_off && out, GDRNPP_EINVAL,
                 "gdrnpp_sym_errors: null pointer");
  GDRNPP_REQUIRE(b > 0, GDRNPP_EINVAL, "gdrnpp_sym_errors: b=%d", b);
  const int m = max_syms(sym_off, models->n_obj);
  GDRNPP_REQUIRE(m > 0, GDRNPP_EINVAL,
                 "gdrnpp_sym_errors: sym_off must start at 0 and give every object at least one transform (the identity)");
  const int nchunk_max = (m + kSymChunk - 1) / kSymChunk;
  GDRNPP_REQUIRE(nchunk_max <= 65535, GDRNPP_ELIMIT, "gdrnpp_sym_errors: %d symmetries > %d", m, 65535 * kSymChunk);
  const size_t need = gdrnpp_sym_errors_workspace_bytes(models, sym_off, b);
  GDRNPP_REQUIRE(workspace && workspace_bytes >= need, GDRNPP_EINVAL, "gdrnpp_sym_errors: workspace %zu < %zu bytes",
                 workspace ? workspace_bytes : (size_t)0, need);
  hipStream_t st = (hipStream_t)stream;
  int* d_off = (int*)workspace;
  double* part = (double*)((char*)workspace + off_bytes(models->n_obj));
  // sym_off is a host array (it sizes the grid); the kernels read this copy.  Pageable source: staged before the call returns.
  hipError_t e = hipMemcpyAsync(d_off, sym_off, sizeof(int) * ((size_t)models->n_obj + 1), hipMemcpyHostToDevice, st);
  GDRNPP_REQUIRE(e == hipSuccess, (int)e, "gdrnpp_sym_errors: copying sym_off: %s", hipGetErrorString(e));
  if (!K) {  // pairs on grid.x (b above 65 535 is ordinary)
    hipLaunchKernelGGL(sym_error_rt, dim3(b), dim3(64), 0, st, models->n_obj, obj, R_est, t_est, R_gt, t_gt, sym_R, sym_t, d_off, out);
    return gdrnpp::check_launch("gdrnpp_sym_errors");
  }
  // pairs on grid.x, the chunks of kSymChunk symmetries on grid.y
  hipLaunchKernelGGL(sym_error_points, dim3(b, nchunk_max), dim3(kThreads), 0, st, models->verts, models->vert_off, models->n_obj,
                     obj, R_est, t_est, R_gt, t_gt, K, sym_R, sym_t, d_off, part, nchunk_max);
  hipLaunchKernelGGL(sym_error_finalize, dim3((b + 63) / 64), dim3(64), 0, st, models->vert_off, models->n_obj, obj, d_off, part,
                     out, nchunk_max, b);
  return gdrnpp::check_launch("gdrnpp_sym_errors");
}

}  // extern "C"
