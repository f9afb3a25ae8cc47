// BOP19 MSSD / MSPD of a batch of (estimate, ground truth) pairs on gfx950: the two symmetry-aware maximum distances the BOP
// toolkit scores a results file with (lib/pysixd/scripts/eval_calc_errors.py:397-423).
//
// Behavioural spec: lib/pysixd/pose_error.py:131-179 (mssd, mspd), lib/pysixd/misc.py:568-582 (project_pts: K (R p + t) divided by
// its third row, z not clamped) and :966-976 (transform_pts_Rt).  For a pair with model points p and symmetries (S_R, S_t):
//   A_s = R_gt S_R,  b_s = R_gt S_t + t_gt
//   mssd = min_s max_p | (R_est p + t_est) - (A_s p + b_s) |
//   mspd = min_s max_p | proj(R_est p + t_est) - proj(A_s p + b_s) |
//
// Two kernels on one stream, fp64 throughout (the results meet thresholds, the reference is fp64):
//   bop_error_points     a workgroup of 4 waves owns one (pair, chunk of kSymChunk symmetries).  Its first threads compose the chunk's
//                        A_s, b_s once (12 doubles each) into LDS.  Every thread then walks the model with stride 256: the
//                        estimate-posed point and its projection are formed once per point and stay in registers, each symmetry of the
//                        chunk is read from LDS at a wave-uniform address (a broadcast) and keeps two running maxima, of the SQUARED 3-D
//                        and 2-D distances, in registers.  The maxima merge by shuffles inside a wave and through LDS across the four
//                        waves; one sqrt per (pair, symmetry) follows (a correctly rounded sqrt is monotone: sqrt of the largest
//                        square is the largest distance), and the minimum over the chunk goes to the workspace.
//   bop_error_finalize   one thread per pair takes the minimum over the pair's chunks.
// max and min do not depend on the order of their operands, so two runs are bit-equal with no ordering machinery and no
// floating-point atomics.  Workgroups beyond an object's symmetry count exit on a workgroup-uniform branch.  The estimate and the
// ground truth are posed and projected by the same expression, so a pair with equal poses and the identity among its
// symmetries gives exactly 0.  Poses holding a NaN give unspecified results (a maximum drops a NaN operand).
// Roofline: compute-side.  Per (point, symmetry) evaluation 45 fp64 VALU operations: 9 fma pose, 3 sub + 3 mul/fma + 1 max for the
// 3-D term, 9 mul/fma for K, 13 for the IEEE reciprocal of the depth, 2 mul + 2 sub + 2 mul/fma + 1 max for the 2-D term; the
// per-point part (load, estimate pose, projection: ~35) is shared by the chunk's symmetries.  Algorithmic HBM bytes: 12 n per model
// (L2-resident across the pairs and chunks of a class), 96 per symmetry, 16 per workgroup written.
#include "common.hpp"
#include <cmath>

namespace {

constexpr int kThreads = 256;   // 4 waves; a thread's points are tid, tid + 256, ...
constexpr int kWaves = kThreads / 64;
constexpr int kSymChunk = 8;    // symmetries per workgroup: 2 running maxima each per thread (32 VGPRs)
constexpr int kXf = 12;         // doubles per composed transform: A_s row-major, then b_s

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, 64));
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

__global__ __launch_bounds__(kThreads) void bop_error_points(
    const float* __restrict__ verts, const int* __restrict__ vert_off, int n_obj, const int* __restrict__ obj,
    const double* __restrict__ R_est, const double* __restrict__ t_est, const double* __restrict__ R_gt,
    const double* __restrict__ t_gt, const double* __restrict__ Kc, const double* __restrict__ sym_R,
    const double* __restrict__ sym_t, const int* __restrict__ sym_off, double* __restrict__ part, int nchunk_max) {
  __shared__ double s_xf[kSymChunk][kXf];
  __shared__ double s_max[kWaves][2 * kSymChunk];

  const size_t pair = blockIdx.x;
  const int chunk = blockIdx.y;
  const int o = obj[pair];
  if (o < 0 || o >= n_obj) return;
  const int s0 = sym_off[o] + chunk * kSymChunk;
  const int ns = min(kSymChunk, sym_off[o + 1] - s0);  // workgroup-uniform
  if (ns <= 0) return;                                 // workgroups beyond this object's symmetry count
  const int v0 = vert_off[o];
  const int n = vert_off[o + 1] - v0;
  if (n <= 0) return;
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  if ((int)threadIdx.x < ns) {  // compose A_s = R_gt S_R, b_s = R_gt S_t + t_gt once per (pair, symmetry)
    const double* Rg = R_gt + 9 * pair;
    const double* tg = t_gt + 3 * pair;
    const double* S = sym_R + 9 * (size_t)(s0 + threadIdx.x);
    const double* St = sym_t + 3 * (size_t)(s0 + threadIdx.x);
    double* X = s_xf[threadIdx.x];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
#pragma unroll
      for (int c = 0; c < 3; ++c) X[3 * r + c] = fma(Rg[3 * r + 2], S[6 + c], fma(Rg[3 * r + 1], S[3 + c], Rg[3 * r] * S[c]));
      X[9 + r] = fma(Rg[3 * r + 2], St[2], fma(Rg[3 * r + 1], St[1], Rg[3 * r] * St[0])) + tg[r];
    }
  }
  __syncthreads();

  double E[kXf], K[9];  // the estimate's transform and the intrinsics: the same for every thread of the workgroup
#pragma unroll
  for (int k = 0; k < 9; ++k) { E[k] = R_est[9 * pair + k]; K[k] = Kc[9 * pair + k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) E[9 + k] = t_est[3 * pair + k];

  double m3[kSymChunk], m2[kSymChunk];  // running maxima of the squared 3-D / 2-D distances
#pragma unroll
  for (int s = 0; s < kSymChunk; ++s) m3[s] = m2[s] = 0.0;

  const float* mv = verts + 3 * (size_t)v0;
  // the compiler keeps the chunk's 96 doubles in registers across this loop, which leaves a SIMD one wave of this kernel: the next
  // point is loaded before the current one is evaluated, and the chunk's independent symmetries supply the parallelism
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
        const double dx = ex - gx, dy = ey - gy, dz = ez - gz;
        m3[s] = fmax(m3[s], fma(dz, dz, fma(dy, dy, dx * dx)));
        const double du = eu - gu, dv = ev - gv;
        m2[s] = fmax(m2[s], fma(dv, dv, du * du));
      }
    }
  }

#pragma unroll
  for (int s = 0; s < kSymChunk; ++s) {
    const double a = wave_max(m3[s]), c = wave_max(m2[s]);
    if (lane == 0) { s_max[wave][2 * s] = a; s_max[wave][2 * s + 1] = c; }
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double best3 = INFINITY, best2 = INFINITY;
    for (int s = 0; s < ns; ++s) {
      double a = s_max[0][2 * s], c = s_max[0][2 * s + 1];
      for (int w = 1; w < kWaves; ++w) { a = fmax(a, s_max[w][2 * s]); c = fmax(c, s_max[w][2 * s + 1]); }
      best3 = fmin(best3, sqrt(a));
      best2 = fmin(best2, sqrt(c));
    }
    double* out = part + 2 * (pair * (size_t)nchunk_max + chunk);
    out[0] = best3;
    out[1] = best2;
  }
}

__global__ __launch_bounds__(64) void bop_error_finalize(const int* __restrict__ vert_off, int n_obj, const int* __restrict__ obj,
                                                         const int* __restrict__ sym_off, const double* __restrict__ part,
                                                         double* __restrict__ out, int nchunk_max, int b) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= b) return;
  const int o = obj[i];
  const double nan = __builtin_nan("");
  double e3 = nan, e2 = nan;  // an obj outside [0, n_obj) or an empty model
  if (o >= 0 && o < n_obj && vert_off[o + 1] - vert_off[o] > 0) {
    const int nchunk = (sym_off[o + 1] - sym_off[o] + kSymChunk - 1) / kSymChunk;
    const double* p = part + 2 * ((size_t)i * nchunk_max);
    e3 = e2 = INFINITY;
    for (int k = 0; k < nchunk; ++k) { e3 = fmin(e3, p[2 * k]); e2 = fmin(e2, p[2 * k + 1]); }
  }
  out[2 * (size_t)i] = e3;
  out[2 * (size_t)i + 1] = e2;
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

size_t gdrnpp_bop_errors_workspace_bytes(const gdrnpp_meshes* models, const int* sym_off, int b) {
  if (!models || !sym_off || b <= 0 || models->n_obj <= 0) return 0;
  const int m = max_syms(sym_off, models->n_obj);
  if (m <= 0) return 0;
  return off_bytes(models->n_obj) + sizeof(double) * 2 * (size_t)b * ((m + kSymChunk - 1) / kSymChunk);
}

int gdrnpp_bop_errors(const gdrnpp_meshes* models, const int* obj, const double* R_est, const double* t_est, const double* R_gt,
                      const double* t_gt, const double* K, const double* sym_R, const double* sym_t, const int* sym_off,
                      double* out, int b, void* workspace, size_t workspace_bytes, void* stream) {
  GDRNPP_REQUIRE(models && models->verts && models->vert_off && models->n_obj > 0, GDRNPP_EINVAL, "gdrnpp_bop_errors: no models");
  GDRNPP_REQUIRE(obj && R_est && t_est && R_gt && t_gt && K && sym_R && sym_t && sym_off && out, GDRNPP_EINVAL,
                 "gdrnpp_bop_errors: null pointer");
  GDRNPP_REQUIRE(b > 0, GDRNPP_EINVAL, "gdrnpp_bop_errors: b=%d", b);
  const int m = max_syms(sym_off, models->n_obj);
  GDRNPP_REQUIRE(m > 0, GDRNPP_EINVAL,
                 "gdrnpp_bop_errors: sym_off must start at 0 and give every object at least one transform (the identity)");
  const int nchunk_max = (m + kSymChunk - 1) / kSymChunk;
  GDRNPP_REQUIRE(nchunk_max <= 65535, GDRNPP_ELIMIT, "gdrnpp_bop_errors: %d symmetries > %d", m, 65535 * kSymChunk);
  const size_t need = gdrnpp_bop_errors_workspace_bytes(models, sym_off, b);
  GDRNPP_REQUIRE(workspace && workspace_bytes >= need, GDRNPP_EINVAL, "gdrnpp_bop_errors: workspace %zu < %zu bytes",
                 workspace ? workspace_bytes : (size_t)0, need);
  hipStream_t st = (hipStream_t)stream;
  int* d_off = (int*)workspace;
  double* part = (double*)((char*)workspace + off_bytes(models->n_obj));
  // sym_off is a host array (it sizes the grid); the kernels read this copy.  Pageable source: staged before the call returns.
  hipError_t e = hipMemcpyAsync(d_off, sym_off, sizeof(int) * ((size_t)models->n_obj + 1), hipMemcpyHostToDevice, st);
  GDRNPP_REQUIRE(e == hipSuccess, (int)e, "gdrnpp_bop_errors: copying sym_off: %s", hipGetErrorString(e));
  // pairs on grid.x (b above 65 535 is ordinary), the chunks of kSymChunk symmetries on grid.y
  hipLaunchKernelGGL(bop_error_points, dim3(b, nchunk_max), dim3(kThreads), 0, st, models->verts, models->vert_off, models->n_obj,
                     obj, R_est, t_est, R_gt, t_gt, K, sym_R, sym_t, d_off, part, nchunk_max);
  hipLaunchKernelGGL(bop_error_finalize, dim3((b + 63) / 64), dim3(64), 0, st, models->vert_off, models->n_obj, obj, d_off, part,
                     out, nchunk_max, b);
  return gdrnpp::check_launch("gdrnpp_bop_errors");
}

}  // extern "C"
