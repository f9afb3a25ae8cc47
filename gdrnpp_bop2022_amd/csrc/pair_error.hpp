// The device and host layer shared by the pose-error kernels that score (estimate, ground truth) pairs over an object's symmetry
// transformations: bop_error.hip (MSSD / MSPD) and sym_error.hip (reS / teS / projS) in full, pose_error.hip for re_deg (their
// wave reductions are wave_ops.hpp's).  The bodies are those the three files were merged with, moved here unchanged as forceinline functions: every expression keeps its
// operand order and its fma / non-fma form, so the results are the same bits.
//
// The chunk scheme: a workgroup of kThreads owns one (pair, chunk of kSymChunk symmetries).  Its first threads compose the chunk's
//   A_s = R_gt S_R,  b_s = R_gt S_t + t_gt
// once (compose_xf, kXf doubles each) into LDS.  Every thread then walks the model with stride kThreads (walk_chunk): the estimate-posed
// point and its projection are formed once per point and stay in registers, each symmetry of the chunk is read from LDS at a wave-uniform
// address (a broadcast) and handed to the caller's term.  The caller merges its accumulators across the waves and writes kCols doubles per
// (pair, chunk) to the workspace; finalize takes the minimum over a pair's chunks.  Workgroups beyond an object's symmetry count exit on a
// workgroup-uniform branch.  The estimate and the ground truth are posed and projected by the same expression (pose_pt, project_pt), so a
// pair with equal poses and the identity among its symmetries has a zero distance at every point.
// Workspace: the device copy of sym_off (off_bytes), then cols doubles per (pair, chunk of the object with the most symmetries).
#pragma once
#include "common.hpp"
#include "wave_ops.hpp"
#include <cmath>

namespace gdrnpp {
namespace pairs {

constexpr int kThreads = 256;   // 4 waves; a thread's points are tid, tid + 256, ...
constexpr int kWaves = kThreads / 64;
constexpr int kSymChunk = 8;    // symmetries per workgroup: each keeps its accumulators in every thread's registers
constexpr int kXf = 12;         // doubles per composed transform: A_s row-major, then b_s

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

// X = [A_s | b_s] = [R_gt S_R | R_gt S_t + t_gt]
__device__ __forceinline__ void compose_xf(const double* __restrict__ Rg, const double* __restrict__ tg, const double* __restrict__ S,
                                           const double* __restrict__ St, double* X) {
#pragma unroll
  for (int r = 0; r < 3; ++r) {
#pragma unroll
    for (int c = 0; c < 3; ++c) X[3 * r + c] = fma(Rg[3 * r + 2], S[6 + c], fma(Rg[3 * r + 1], S[3 + c], Rg[3 * r] * S[c]));
    X[9 + r] = fma(Rg[3 * r + 2], St[2], fma(Rg[3 * r + 1], St[1], Rg[3 * r] * St[0])) + tg[r];
  }
}

__device__ __forceinline__ double re_deg(const double* __restrict__ Re, const double* Rg) {
  // trace(R_est R_gt^T) = sum_ik R_est[i][k] R_gt[i][k]   (pose_error.py:367-372, :388-393)
  double tr = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) tr += (Re[3 * i] * Rg[3 * i] + Re[3 * i + 1] * Rg[3 * i + 1]) + Re[3 * i + 2] * Rg[3 * i + 2];
  tr = tr <= 3.0 ? tr : 3.0;
  const double c = fmin(1.0, fmax(-1.0, 0.5 * (tr - 1.0)));
  return acos(c) * (180.0 / 3.14159265358979323846);
}

// What workgroup (blockIdx.x = pair, blockIdx.y = chunk) owns: symmetries [s0, s0 + ns) and the n model points from v0.
struct Chunk {
  int s0, ns, v0, n;
};

// The chunk of this workgroup for an obj o the caller has found inside [0, n_obj).  ns <= 0: a chunk beyond the object's symmetry count, the
// workgroup leaves (workgroup-uniform).  n may be 0: whether an empty model still has work is the caller's business.  No branch in here:
// the callers' two early returns stay the kernels' only exits, and after them the compiler knows 1 <= ns <= kSymChunk.
__device__ __forceinline__ Chunk chunk_of(int o, const int* sym_off, const int* vert_off) {
  const int chunk = blockIdx.y;
  Chunk c;
  c.s0 = sym_off[o] + chunk * kSymChunk;
  c.ns = min(kSymChunk, sym_off[o + 1] - c.s0);
  c.v0 = vert_off[o];
  c.n = vert_off[o + 1] - c.v0;
  return c;
}

// The estimate's transform E and the intrinsics K of a pair: the same for every thread of the workgroup
__device__ __forceinline__ void load_est(const double* R_est, const double* t_est, const double* Kc, size_t pair, double* E, double* K) {
#pragma unroll
  for (int k = 0; k < 9; ++k) { E[k] = R_est[9 * pair + k]; K[k] = Kc[9 * pair + k]; }
#pragma unroll
  for (int k = 0; k < 3; ++k) E[9 + k] = t_est[3 * pair + k];
}

// The walk over the n points at mv: calls term(s, ex, ey, ez, eu, ev, gx, gy, gz, gu, gv, acc...) for every (point of this thread, symmetry
// s < ns), with the point posed by E and by s_xf[s] (LDS) and both projected by K.  acc: the caller's accumulator arrays, kSymChunk doubles
// each.  They travel as arguments and term is a capture-less, always-inlined lambda: an array whose address sits in a closure object is not
// turned into a vector register tuple by the AMDGPU alloca promotion, and the loop then schedules worse (+2.5 % time, profiles/pair_error_refactor.txt).
// The compiler keeps the chunk's 96 doubles in registers across this loop, which leaves a SIMD one wave of such a kernel: the next point is
// loaded before the current one is evaluated, and the chunk's independent symmetries supply the parallelism.
template <class Term, class... Acc>
__device__ __forceinline__ void walk_chunk(const float* mv, int n, int ns, const double* E, const double* K, const double (*s_xf)[kXf],
                                           Term term, Acc*... acc) {
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
        term(s, ex, ey, ez, eu, ev, gx, gy, gz, gu, gv, acc...);
      }
    }
  }
}

// One thread per pair: the minimum over the pair's chunks of each of the kCols columns.  The row is NaN for an obj outside [0, n_obj);
// the columns from kFirstPointCol on, those formed over the model points, are NaN for an empty model.
template <int kCols, int kFirstPointCol>
__global__ __launch_bounds__(64) void finalize(const int* __restrict__ vert_off, int n_obj, const int* __restrict__ obj,
                                               const int* __restrict__ sym_off, const double* __restrict__ part,
                                               double* __restrict__ out, int nchunk_max, int b) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= b) return;
  const int o = obj[i];
  const double nan = __builtin_nan("");
  double e[kCols];
#pragma unroll
  for (int c = 0; c < kCols; ++c) e[c] = nan;
  if (o >= 0 && o < n_obj) {
    const bool empty = vert_off[o + 1] - vert_off[o] <= 0;
    if (kFirstPointCol > 0 || !empty) {  // with no other column, an empty model's workgroups wrote nothing
      const int nchunk = (sym_off[o + 1] - sym_off[o] + kSymChunk - 1) / kSymChunk;
      const double* p = part + kCols * ((size_t)i * nchunk_max);
#pragma unroll
      for (int c = 0; c < kCols; ++c) e[c] = INFINITY;
      for (int k = 0; k < nchunk; ++k) {
#pragma unroll
        for (int c = 0; c < kCols; ++c) e[c] = fmin(e[c], p[kCols * k + c]);
      }
      if (empty) {
#pragma unroll
        for (int c = kFirstPointCol; c < kCols; ++c) e[c] = nan;
      }
    }
  }
#pragma unroll
  for (int c = 0; c < kCols; ++c) out[kCols * (size_t)i + c] = e[c];
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

// what gdrnpp_{bop,sym}_errors_workspace_bytes return: 0 for arguments the entry point would refuse
inline size_t workspace_bytes(const gdrnpp_meshes* models, const int* sym_off, int b, int cols) {
  if (!models || !sym_off || b <= 0 || models->n_obj <= 0) return 0;
  const int m = max_syms(sym_off, models->n_obj);
  if (m <= 0) return 0;
  return off_bytes(models->n_obj) + sizeof(double) * cols * (size_t)b * ((m + kSymChunk - 1) / kSymChunk);
}

// The argument checks of an entry point named `what` (ptrs_ok: its own pointer arguments are there), the carving of its workspace into
// d_off and part, and the staging of sym_off on the stream.  Returns 0 or a GDRNPP_* / hipError_t code with the error text set.
inline int prepare(const char* what, const gdrnpp_meshes* models, bool ptrs_ok, const int* sym_off, int b, int cols, void* workspace,
                   size_t workspace_bytes_, void* stream, int** d_off, double** part, int* nchunk_max) {
  GDRNPP_REQUIRE(models && models->verts && models->vert_off && models->n_obj > 0, GDRNPP_EINVAL, "%s: no models", what);
  GDRNPP_REQUIRE(ptrs_ok && sym_off, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(b > 0, GDRNPP_EINVAL, "%s: b=%d", what, b);
  const int m = max_syms(sym_off, models->n_obj);
  GDRNPP_REQUIRE(m > 0, GDRNPP_EINVAL, "%s: sym_off must start at 0 and give every object at least one transform (the identity)", what);
  *nchunk_max = (m + kSymChunk - 1) / kSymChunk;
  GDRNPP_REQUIRE(*nchunk_max <= 65535, GDRNPP_ELIMIT, "%s: %d symmetries > %d", what, m, 65535 * kSymChunk);
  const size_t need = workspace_bytes(models, sym_off, b, cols);
  GDRNPP_REQUIRE(workspace && workspace_bytes_ >= need, GDRNPP_EINVAL, "%s: workspace %zu < %zu bytes", what,
                 workspace ? workspace_bytes_ : (size_t)0, need);
  *d_off = (int*)workspace;
  *part = (double*)((char*)workspace + off_bytes(models->n_obj));
  // sym_off is a host array (it sizes the grid); the kernels read this copy.  Pageable source: staged before the call returns.
  hipError_t e = hipMemcpyAsync(*d_off, sym_off, sizeof(int) * ((size_t)models->n_obj + 1), hipMemcpyHostToDevice, (hipStream_t)stream);
  GDRNPP_REQUIRE(e == hipSuccess, (int)e, "%s: copying sym_off: %s", what, hipGetErrorString(e));
  return 0;
}

}  // namespace pairs
}  // namespace gdrnpp
