// OpenCV's 8-bit INTER_LINEAR resize, the part its users here share: the three forms a call takes and the coefficients of one
// destination index (modules/imgproc/src/resize.cpp, the generic fixed-point path).  yolox_pre.hip (the letterbox) and
// replace_bg.hip (the training backgrounds) build their pixels from these; each keeps its own walk over the output.
#pragma once
#include <hip/hip_runtime.h>

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

}  // namespace resize_u8
}  // namespace gdrnpp
