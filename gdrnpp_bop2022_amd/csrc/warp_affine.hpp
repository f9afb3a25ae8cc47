// OpenCV's cv2.warpAffine, whole (restated as in oracle/warp_oracle.c): getAffineTransform (double LU), the inversion of a 2x3 map
// as warpAffine does it (host and device), the ROI's map solved once per workgroup, the 10-bit fixed-point source coordinate of an
// output pixel, and the 8-bit bilinear pixel: its 15-bit integer weights and the sum of four taps.  crop_resize.hip, roi_targets.hip
// (the ROI crops) and yolox_aug.hip (the YOLOX training batches' random affine) warp through these and bring their walk over the output,
// their loads and their border value; a rounding rule of the warp is stated nowhere else.  Internal linkage: one copy per translation unit.
#pragma once
#include "common.hpp"

namespace {

constexpr int AB_BITS = 10, AB_SCALE = 1 << AB_BITS, INTER_BITS = 5, INTER_TAB_SIZE = 1 << INTER_BITS;

__device__ __forceinline__ int cv_round(double v) { return __double2int_rn(v); }
__device__ __forceinline__ int sat_short(int v) { return v < -32768 ? -32768 : (v > 32767 ? 32767 : v); }

// cv::LUImpl, 6x6, one right-hand side (getAffineTransform).  Every index is a compile-time constant after unrolling (the
// pivot row is applied as a chain of predicated swaps), so the system lives in registers: with a run-time row index the
// arrays went to scratch memory and the solve took 20 us on the one lane that does it.  Same operations in the same order
// as the loop form (first maximal pivot, `>` comparison).
__device__ __forceinline__ bool lu_solve6(double (&A)[36], double (&b)[6]) {
  constexpr int m = 6;
#pragma unroll
  for (int i = 0; i < m; i++) {
    int k = i;
    double best = fabs(A[i * m + i]);
#pragma unroll
    for (int j = i + 1; j < m; j++) {
      const double v = fabs(A[j * m + i]);
      if (v > best) { best = v; k = j; }
    }
    if (best < 2.220446049250313e-16 * 100) return false;
#pragma unroll
    for (int r = i + 1; r < m; r++) {
      const bool sw = k == r;
#pragma unroll
      for (int j = i; j < m; j++) {
        const double ai = A[i * m + j], ar = A[r * m + j];
        A[i * m + j] = sw ? ar : ai;
        A[r * m + j] = sw ? ai : ar;
      }
      const double bi = b[i], br = b[r];
      b[i] = sw ? br : bi;
      b[r] = sw ? bi : br;
    }
    const double d = -1 / A[i * m + i];
#pragma unroll
    for (int j = i + 1; j < m; j++) {
      const double alpha = A[j * m + i] * d;
#pragma unroll
      for (int kk = i + 1; kk < m; kk++) A[j * m + kk] += alpha * A[i * m + kk];
      b[j] += alpha * b[i];
    }
  }
#pragma unroll
  for (int i = m - 1; i >= 0; i--) {
    double s = b[i];
#pragma unroll
    for (int k = i + 1; k < m; k++) s -= A[i * m + k] * b[k];
    b[i] = s / A[i * m + i];
  }
  return true;
}

// cv::warpAffine's inversion of the 2x3 map M, in place; false where the determinant is 0 (OpenCV goes on with D = 0, and M
// becomes the zero map).  Host and device: every user is compiled without contraction, the operation order is OpenCV's.
__host__ __device__ __forceinline__ bool invert_affine(double* M) {
  double D = M[0] * M[4] - M[1] * M[3];
  const bool regular = D != 0;
  D = D != 0 ? 1. / D : 0;
  const double A11 = M[4] * D, A22 = M[0] * D;
  M[0] = A11; M[1] *= -D;
  M[3] *= -D; M[4] = A22;
  const double b1 = -M[0] * M[2] - M[1] * M[5];
  const double b2 = -M[3] * M[2] - M[4] * M[5];
  M[2] = b1; M[5] = b2;
  return regular;
}

// get_affine_transform(center, scale, rot=0, (out,out)) -> inverse map M (dst -> src) as warpAffine forms it
__device__ void inverse_affine(double cx, double cy, double scale, int out, double* M) {
  float src[3][2], dst[3][2];
  const double src_dir1 = 0.0 * 0.0 + (scale * -0.5) * 1.0;
  const double src_dir0 = 0.0 * 1.0 - (scale * -0.5) * 0.0;
  src[0][0] = (float)(cx + scale * 0.0); src[0][1] = (float)(cy + scale * 0.0);
  src[1][0] = (float)(cx + src_dir0 + scale * 0.0); src[1][1] = (float)(cy + src_dir1 + scale * 0.0);
  dst[0][0] = (float)(out * 0.5); dst[0][1] = (float)(out * 0.5);
  dst[1][0] = (float)(out * 0.5) + 0.f; dst[1][1] = (float)(out * 0.5) + (float)(out * -0.5);
  float dx = src[0][0] - src[1][0], dy = src[0][1] - src[1][1];
  src[2][0] = src[1][0] + (-dy); src[2][1] = src[1][1] + dx;
  dx = dst[0][0] - dst[1][0]; dy = dst[0][1] - dst[1][1];
  dst[2][0] = dst[1][0] + (-dy); dst[2][1] = dst[1][1] + dx;
  double a[36], b[6];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const int j = i * 12, k = i * 12 + 6;
    a[j] = a[k + 3] = src[i][0];
    a[j + 1] = a[k + 4] = src[i][1];
    a[j + 2] = a[k + 5] = 1;
    a[j + 3] = a[j + 4] = a[j + 5] = 0;
    a[k] = a[k + 1] = a[k + 2] = 0;
    b[i * 2] = dst[i][0];
    b[i * 2 + 1] = dst[i][1];
  }
  if (!lu_solve6(a, b)) {
#pragma unroll
    for (int i = 0; i < 6; ++i) b[i] = 0.0;
  }
#pragma unroll
  for (int i = 0; i < 6; ++i) M[i] = b[i];
  invert_affine(M);
}

// A ROI's map, once per workgroup: thread 0 solves it into the workgroup's LDS slot `sM` (6 doubles), and behind a barrier every
// thread reads its own copy.  A kernel that stages other LDS data under the same barrier calls the two halves around its own barrier.
__device__ __forceinline__ void roi_map_solve(const double* __restrict__ centers, const double* __restrict__ scales, int bi, int out, double* sM) {
  if (threadIdx.x == 0) inverse_affine(centers[2 * bi], centers[2 * bi + 1], scales[bi], out, sM);
}

__device__ __forceinline__ void roi_map_read(const double* sM, double (&M)[6]) {
#pragma unroll
  for (int k = 0; k < 6; ++k) M[k] = sM[k];
}

__device__ __forceinline__ void roi_map(const double* __restrict__ centers, const double* __restrict__ scales, int bi, int out, double* sM, double (&M)[6]) {
  roi_map_solve(centers, scales, bi, out, sM);
  __syncthreads();
  roi_map_read(sM, M);
}

__device__ __forceinline__ void src_coord(const double* M, int x, int y, bool nearest, int& sx, int& sy, int& alpha) {
  const int adelta = cv_round(M[0] * x * AB_SCALE), bdelta = cv_round(M[3] * x * AB_SCALE);
  const int round_delta = nearest ? AB_SCALE / 2 : AB_SCALE / INTER_TAB_SIZE / 2;
  const int X0 = cv_round((M[1] * y + M[2]) * AB_SCALE) + round_delta;
  const int Y0 = cv_round((M[4] * y + M[5]) * AB_SCALE) + round_delta;
  if (nearest) {
    sx = sat_short((X0 + adelta) >> AB_BITS);
    sy = sat_short((Y0 + bdelta) >> AB_BITS);
    alpha = 0;
  } else {
    const int X = (X0 + adelta) >> (AB_BITS - INTER_BITS), Y = (Y0 + bdelta) >> (AB_BITS - INTER_BITS);
    sx = sat_short(X >> INTER_BITS);
    sy = sat_short(Y >> INTER_BITS);
    alpha = (Y & (INTER_TAB_SIZE - 1)) * INTER_TAB_SIZE + (X & (INTER_TAB_SIZE - 1));
  }
}

// The 8-bit bilinear pixel (INTER_LINEAR of CV_8U).  Weights of the fraction (fy, fx), both in 1/32: cv::initInterTab2D's table entry
// as 15-bit integers, taps in the order (y, x), (y, x + 1), (y + 1, x), (y + 1, x + 1).  Entry 0 is saturate_cast<short>(32768) with the
// table's sum fix-up.
__device__ __forceinline__ void bilinear_weights_u8(int fy, int fx, int w[4]) {
  w[0] = (32 - fy) * (32 - fx) * 32;
  w[1] = (32 - fy) * fx * 32;
  w[2] = fy * (32 - fx) * 32;
  w[3] = fy * fx * 32;
  if ((fy | fx) == 0) {
    w[0] = 32767;
    w[3] = 1;
  }
}

// ... and one channel from its four taps, which the caller has loaded with its border value where a tap lies outside the source
__device__ __forceinline__ int bilinear_u8(int v00, int v01, int v10, int v11, const int w[4]) {
  const int s = (v00 * w[0] + v01 * w[1] + v10 * w[2] + v11 * w[3] + (1 << 14)) >> 15;
  return s < 0 ? 0 : (s > 255 ? 255 : s);
}

}  // namespace
