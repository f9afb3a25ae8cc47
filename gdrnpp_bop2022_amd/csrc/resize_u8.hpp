// OpenCV's 8-bit cv2.resize(INTER_LINEAR), whole (modules/imgproc/src/resize.cpp, the generic fixed-point path): the three forms a
// call takes, the coefficients of one destination index, the pixel in each form, and on the host the request (sizes, form, scales)
// with its one check.  yolox_pre.hip (the letterbox), replace_bg.hip (the training backgrounds) and yolox_aug.hip (the YOLOX training
// batches) take their pixels from here and bring their walk over the output; a rounding rule of the resize is stated nowhere else.
#pragma once
#include "common.hpp"

#include <cstring>

namespace gdrnpp {
namespace resize_u8 {

enum { kModeCopy = 0, kModeArea = 1, kModeLinear = 2 };
constexpr int kCoefBits = 11, kCoefOne = 1 << kCoefBits;

struct Tap { int i0, i1, c0, c1; };

// OpenCV's coefficient of destination index d along an axis of n source samples
__device__ __forceinline__ Tap linear_tap(int d, double scale, int n, bool clamp_fraction) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (clamp_fraction) {                     // columns: the index is clamped and the fraction dropped
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= n - 1) { f = 0.f; s = n - 1; }
  }
  Tap t;
  t.c0 = __float2int_rn((1.f - f) * (float)kCoefOne);
  t.c1 = __float2int_rn(f * (float)kCoefOne);
  t.i0 = min(max(s, 0), n - 1);             // rows: the two row indices are clamped, the coefficients stay
  t.i1 = min(max(s + 1, 0), n - 1);
  return t;
}

// Taps: what the pixel functions read their source through, `taps(y, x, v)` -> the three channels of source pixel (y, x) as ints.
// This one is a u8 HWC image whose rows lie `stride` pixels apart: a dense image or a crop of a larger one.
struct StridedTaps {
  const uint8_t* img;
  size_t stride;
  __device__ __forceinline__ void operator()(int y, int x, int v[3]) const {
    const uint8_t* p = img + (size_t)y * stride * 3 + x * 3;      // the row's term is shared by the taps of a row
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (int)p[k];
  }
};

// destination pixel (r, c) in form `mode`; ty = linear_tap of r, tx = linear_tap of c, read by the linear form alone.  For a walk
// that makes several pixels of a row or a column and computes their shared tap once.
template <class Taps, class Out>
__device__ __forceinline__ void resize_px(const Taps& taps, int mode, const Tap& ty, const Tap& tx, int r, int c, Out v[3]) {
  if (mode == kModeCopy) {
    int p[3];
    taps(r, c, p);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (Out)p[k];
  } else if (mode == kModeArea) {
    int p00[3], p01[3], p10[3], p11[3];
    taps(2 * r, 2 * c, p00);
    taps(2 * r, 2 * c + 1, p01);
    taps(2 * r + 1, 2 * c, p10);
    taps(2 * r + 1, 2 * c + 1, p11);
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (Out)((p00[k] + p01[k] + p10[k] + p11[k] + 2) >> 2);
  } else {
    int p00[3], p01[3], p10[3], p11[3];
    taps(ty.i0, tx.i0, p00);
    taps(ty.i0, tx.i1, p01);
    taps(ty.i1, tx.i0, p10);
    taps(ty.i1, tx.i1, p11);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const int h0 = p00[k] * tx.c0 + p01[k] * tx.c1;
      const int h1 = p10[k] * tx.c0 + p11[k] * tx.c1;
      v[k] = (Out)(((((ty.c0 * (h0 >> 4)) >> 16) + ((ty.c1 * (h1 >> 4)) >> 16) + 2) >> 2) & 255);      // the cast to uchar
    }
  }
}

// cv2.resize(image of w x h, INTER_LINEAR) at destination (r, c)
template <class Taps, class Out>
__device__ __forceinline__ void resize_px(const Taps& taps, int w, int h, int mode, double scale_x, double scale_y, int r, int c, Out v[3]) {
  // pure arithmetic that only the linear form reads: the compiler moves it into that branch
  resize_px(taps, mode, linear_tap(r, scale_y, h, false), linear_tap(c, scale_x, w, true), r, c, v);
}

// host: a table's doubles travel as their bit patterns in its long long columns
template <class To, class From>
inline To bit_cast(From v) {
  To t;
  std::memcpy(&t, &v, sizeof t);
  return t;
}
inline double as_double(long long bits) { return bit_cast<double>(bits); }
inline long long as_bits(double d) { return bit_cast<long long>(d); }

// one resize: a w x h source into dw x dh in form `mode`, with the interpolation scales the linear form reads
struct ResizeRequest { long long w, h, dw, dh, mode; double scale_x, scale_y; };

// The request cv2.resize(src, dsize = (dw, dh)) makes: equal sizes are a copy, an exact 2:1 reduction on both axes is the area mean,
// the scale is 1 / inv_scale.  OpenCV asks whether the scale lies within DBL_EPSILON of 2 (hip_lib's resize_request says it that way);
// for integer sides below 32768 that is the question w == 2 dw: fl(dw / w) cannot come within an ulp of 0.5 without being 0.5.
inline ResizeRequest dsize_request(int w, int h, int dw, int dh) {
  const long long mode = (dh == h && dw == w) ? kModeCopy : (h == 2 * dh && w == 2 * dw) ? kModeArea : kModeLinear;
  return ResizeRequest{w, h, dw, dh, mode, 1. / ((double)dw / w), 1. / ((double)dh / h)};
}

// refuses a request the pixel functions cannot serve; `where` names the table row in the message ("row 3", "row 3 source 1")
inline int check_request(const char* what, const char* where, const ResizeRequest& q) {
  GDRNPP_REQUIRE(q.mode == kModeCopy || q.mode == kModeArea || q.mode == kModeLinear, GDRNPP_EINVAL, "%s: %s: mode=%lld", what, where, q.mode);
  GDRNPP_REQUIRE(q.mode != kModeCopy || (q.dw == q.w && q.dh == q.h), GDRNPP_EINVAL, "%s: %s: copy of %lld x %lld into %lld x %lld", what, where,
                 q.w, q.h, q.dw, q.dh);
  GDRNPP_REQUIRE(q.mode != kModeArea || (2 * q.dw <= q.w && 2 * q.dh <= q.h), GDRNPP_EINVAL,
                 "%s: %s: 2:1 area mean of %lld x %lld into %lld x %lld reads beyond the source", what, where, q.w, q.h, q.dw, q.dh);
  GDRNPP_REQUIRE(q.mode != kModeLinear || (q.scale_x > 0. && q.scale_y > 0. && q.scale_x * (double)q.dw < 1e9 && q.scale_y * (double)q.dh < 1e9),
                 GDRNPP_EINVAL, "%s: %s: scale_x=%g scale_y=%g", what, where, q.scale_x, q.scale_y);
  return 0;
}

}  // namespace resize_u8
}  // namespace gdrnpp
