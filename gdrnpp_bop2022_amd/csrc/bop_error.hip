// BOP19 MSSD / MSPD of a batch of (estimate, ground truth) pairs on gfx950: the two symmetry-aware maximum distances the BOP
// toolkit scores a results file with (lib/pysixd/scripts/eval_calc_errors.py:397-423).
//
// Behavioural spec: lib/pysixd/pose_error.py:131-179 (mssd, mspd), lib/pysixd/misc.py:568-582 (project_pts: K (R p + t) divided by
// its third row, z not clamped) and :966-976 (transform_pts_Rt).  For a pair with model points p and symmetries (S_R, S_t):
//   A_s = R_gt S_R,  b_s = R_gt S_t + t_gt
//   mssd = min_s max_p | (R_est p + t_est) - (A_s p + b_s) |
//   mspd = min_s max_p | proj(R_est p + t_est) - proj(A_s p + b_s) |
//
// Two kernels on one stream, fp64 throughout (the results meet thresholds, the reference is fp64), on the chunk scheme of pair_error.hpp
// (the composition into LDS, the walk over the model, the workspace, the host checks):
//   bop_error_points     per (point, symmetry) two running maxima, of the SQUARED 3-D and 2-D distances, in registers.  The maxima merge
//                        by shuffles inside a wave and through LDS across the four waves; one sqrt per (pair, symmetry) follows (a
//                        correctly rounded sqrt is monotone: sqrt of the largest square is the largest distance), and the minimum over
//                        the chunk goes to the workspace.
//   pairs::finalize      one thread per pair takes the minimum over the pair's chunks.
// max and min do not depend on the order of their operands, so two runs are bit-equal with no ordering machinery and no
// floating-point atomics.  A pair with equal poses and the identity among its symmetries gives exactly 0.  Poses holding a NaN give
// unspecified results (a maximum drops a NaN operand).
// Roofline: compute-side.  Per (point, symmetry) evaluation 45 fp64 VALU operations: 9 fma pose, 3 sub + 3 mul/fma + 1 max for the
// 3-D term, 9 mul/fma for K, 13 for the IEEE reciprocal of the depth, 2 mul + 2 sub + 2 mul/fma + 1 max for the 2-D term; the
// per-point part (load, estimate pose, projection: ~35) is shared by the chunk's symmetries.  Algorithmic HBM bytes: 12 n per model
// (L2-resident across the pairs and chunks of a class), 96 per symmetry, 16 per workgroup written.
#include "pair_error.hpp"

using namespace gdrnpp::pairs;

namespace {

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
  const Chunk ck = chunk_of(o, sym_off, vert_off);
  if (ck.ns <= 0 || ck.n <= 0) return;  // no points: nothing to take a maximum over, finalize gives NaN
  const int ns = ck.ns;  // workgroup-uniform
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;

  if ((int)threadIdx.x < ns)  // once per (pair, symmetry)
    compose_xf(R_gt + 9 * pair, t_gt + 3 * pair, sym_R + 9 * (size_t)(ck.s0 + threadIdx.x), sym_t + 3 * (size_t)(ck.s0 + threadIdx.x),
               s_xf[threadIdx.x]);
  __syncthreads();

  double E[kXf], K[9];
  load_est(R_est, t_est, Kc, pair, E, K);

  double m3[kSymChunk], m2[kSymChunk];  // running maxima of the squared 3-D / 2-D distances
#pragma unroll
  for (int s = 0; s < kSymChunk; ++s) m3[s] = m2[s] = 0.0;

  walk_chunk(verts + 3 * (size_t)ck.v0, ck.n, ns, E, K, s_xf,
             [](int s, double ex, double ey, double ez, double eu, double ev, double gx, double gy, double gz, double gu, double gv,
                double* m3, double* m2) __attribute__((always_inline)) {
               const double dx = ex - gx, dy = ey - gy, dz = ez - gz;
               m3[s] = fmax(m3[s], fma(dz, dz, fma(dy, dy, dx * dx)));
               const double du = eu - gu, dv = ev - gv;
               m2[s] = fmax(m2[s], fma(dv, dv, du * du));
             },
             m3, m2);

#pragma unroll
  for (int s = 0; s < kSymChunk; ++s) {
    const double a = gdrnpp::wave::wave_max(m3[s]), c = gdrnpp::wave::wave_max(m2[s]);
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

}  // namespace

extern "C" {

size_t gdrnpp_bop_errors_workspace_bytes(const gdrnpp_meshes* models, const int* sym_off, int b) {
  return workspace_bytes(models, sym_off, b, 2);
}

int gdrnpp_bop_errors(const gdrnpp_meshes* models, const int* obj, const double* R_est, const double* t_est, const double* R_gt,
                      const double* t_gt, const double* K, const double* sym_R, const double* sym_t, const int* sym_off,
                      double* out, int b, void* workspace, size_t workspace_bytes, void* stream) {
  int* d_off;
  double* part;
  int nchunk_max;
  const int rc = prepare("gdrnpp_bop_errors", models, obj && R_est && t_est && R_gt && t_gt && K && sym_R && sym_t && out, sym_off, b, 2,
                         workspace, workspace_bytes, stream, &d_off, &part, &nchunk_max);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  // pairs on grid.x (b above 65 535 is ordinary), the chunks of kSymChunk symmetries on grid.y
  hipLaunchKernelGGL(bop_error_points, dim3(b, nchunk_max), dim3(kThreads), 0, st, models->verts, models->vert_off, models->n_obj,
                     obj, R_est, t_est, R_gt, t_gt, K, sym_R, sym_t, d_off, part, nchunk_max);
  hipLaunchKernelGGL((finalize<2, 0>), dim3((b + 63) / 64), dim3(64), 0, st, models->vert_off, models->n_obj, obj, d_off, part, out,
                     nchunk_max, b);
  return gdrnpp::check_launch("gdrnpp_bop_errors");
}

}  // extern "C"
