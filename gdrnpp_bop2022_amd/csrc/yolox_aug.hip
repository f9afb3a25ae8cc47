// YOLOX training batches on the device: what `MosaicDetection.__getitem__` (det/yolox/data/datasets/mosaicdetection.py) and
// `TrainTransform` (det/yolox/data/data_augment.py) do to pixels, for a whole batch in one call.
//
// gdrnpp_yolox_train_inputs   The host makes every random draw and all size arithmetic (det/yolox/data/mosaic.py) and hands over one table
//   row per batch item (its columns: include/gdrnpp_hip.h); the kernels derive none of it and nothing is read back.  A row takes one of
//   three branches: plain (the source through TrainTransform), mosaic, mosaic + mixup.
//   Launch 1, mosaic rows only, one thread per canvas pixel: the 2H x 2W mosaic canvas of 114 with the four resized sources pasted
//   (later pastes win), and for mixup rows the H x W `cp` canvas of 114 with the resized mixup source top-left.  Canvases are 4 bytes a
//   pixel (b, g, r, 0): four pixels a thread and one 16-byte store here, one aligned 32-bit load per tap in launch 2.
//   Launch 2, one thread per output pixel (y, x), everything upstream addressed at the mirrored column where the row mirrors:
//   cv2.warpAffine's four canvas taps (inverse map inverted on the host as OpenCV does, 10-bit fixed-point coordinate of
//   warp_affine.hpp, 15-bit integer bilinear table, taps outside the canvas read 114), the mixup sample through the second resize, the
//   flip, the zero pad and the crop, the 0.5 / 0.5 blend truncated, then up to two HSV passes (8-bit RGB -> HSV in integers, three LUTs,
//   HSV -> RGB in singly rounded fp32: this file is compiled without contraction) and three coalesced f32 plane stores.  The plain
//   branch resizes its source per pixel from the source's own taps, each tap through the mirror and HSV pass 1, which the reference
//   applies before the resize.  The row's branch and flags are uniform over a workgroup: no lane diverges on them.
//   Memory-bound: per mosaic + mixup item the canvas launch writes 20 H W bytes and launch 2 reads about that (neighbours share taps
//   through L2) and writes 12 H W.
#include "common.hpp"
#include "resize_u8.hpp"
#include "warp_affine.hpp"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

using namespace gdrnpp::resize_u8;

// the table's columns, as include/gdrnpp_hip.h lists them
enum { cBranch = 0, cFlags, cM0, cJw = cM0 + 6, cJh, cMode2, cScale2X, cScale2Y, cXOff, cYOff, cSrc0 };
enum { sOff = 0, sW, sH, sDw, sDh, sMode, sScaleX, sScaleY, sLx, sLy, sSx, sSy, sPw, sPh, kSrcCols };
constexpr int kSources = 5, kMixSource = 4;         // four mosaic tiles (the plain branch uses the first), then the mixup image
constexpr int kCols = cSrc0 + kSources * kSrcCols;
static_assert(kCols == 85, "the header's column count");
enum { kPlain = 0, kMosaic = 1, kMixup = 2 };
enum { fHsv1 = 1, fHsv1Rgb = 2, fMirror = 4, fFallback = 8, fHsv2 = 16, fHsv2Rgb = 32, fMixFlip = 64, fSingular = 128, fAll = 255 };
constexpr int kPad = 114;
constexpr uint32_t kPadPixel = 114u | (114u << 8) | (114u << 16);
constexpr int kDivInts = 512;                        // sdiv[256], hdiv[256] behind the staged table

__device__ __forceinline__ uint32_t pack_px(const int v[3]) { return (uint32_t)v[0] | ((uint32_t)v[1] << 8) | ((uint32_t)v[2] << 16); }
__device__ __forceinline__ void unpack_px(uint32_t p, int v[3]) {
  v[0] = (int)(p & 255u);
  v[1] = (int)((p >> 8) & 255u);
  v[2] = (int)((p >> 16) & 255u);
}

// cv2.cvtColor(RGB|BGR -> HSV), cv2.LUT x 3, cv2.cvtColor(HSV -> RGB|BGR) on one 8-bit pixel; hue range 180.  v is in the image's
// channel order; lut = u8[3][256] (hue, saturation, value).
__device__ __forceinline__ void hsv_pass(int v[3], const uint8_t* __restrict__ lut, bool rgb, const int* __restrict__ sdiv,
                                         const int* __restrict__ hdiv) {
  const int b = rgb ? v[2] : v[0], g = v[1], r = rgb ? v[0] : v[2];
  const int vmax = max(b, max(g, r)), vmin = min(b, min(g, r)), diff = vmax - vmin;
  int s = (diff * sdiv[vmax] + (1 << 11)) >> 12;
  int h = vmax == r ? g - b : (vmax == g ? b - r + 2 * diff : r - g + 4 * diff);
  h = (h * hdiv[diff] + (1 << 11)) >> 12;
  h += h < 0 ? 180 : 0;
  h = (int)lut[min(h, 255)];
  s = (int)lut[256 + min(s, 255)];
  const int val = (int)lut[512 + vmax];
  const float vf = __fmul_rn((float)val, 1.f / 255.f);
  float fb = vf, fg = vf, fr = vf;
  if (s != 0) {
    const float sf = __fmul_rn((float)s, 1.f / 255.f);
    float hf = __fmul_rn((float)h, 6.f / 180.f);
    while (hf >= 6.f) hf = __fsub_rn(hf, 6.f);
    const int sector = (int)floorf(hf);
    const float f = __fsub_rn(hf, (float)sector);
    const float t0 = vf;
    const float t1 = __fmul_rn(vf, __fsub_rn(1.f, sf));
    const float t2 = __fmul_rn(vf, __fsub_rn(1.f, __fmul_rn(sf, f)));
    const float t3 = __fmul_rn(vf, __fsub_rn(1.f, __fmul_rn(sf, __fsub_rn(1.f, f))));
    // (b, g, r) = tab[{1,3,0},{1,0,2},{3,0,1},{0,2,1},{0,1,3},{2,1,0}][sector], as selects: no indexed array, no scratch
    fb = sector == 0 ? t1 : sector == 1 ? t1 : sector == 2 ? t3 : sector == 3 ? t0 : sector == 4 ? t0 : t2;
    fg = sector == 0 ? t3 : sector == 1 ? t0 : sector == 2 ? t0 : sector == 3 ? t2 : sector == 4 ? t1 : t1;
    fr = sector == 0 ? t0 : sector == 1 ? t2 : sector == 2 ? t1 : sector == 3 ? t1 : sector == 4 ? t3 : t0;
  }
  const int ob = min(max(__float2int_rn(__fmul_rn(fb, 255.f)), 0), 255);
  const int og = min(max(__float2int_rn(__fmul_rn(fg, 255.f)), 0), 255);
  const int orr = min(max(__float2int_rn(__fmul_rn(fr, 255.f)), 0), 255);
  v[0] = rgb ? orr : ob;
  v[1] = og;
  v[2] = rgb ? ob : orr;
}

// a dense u8 HWC image; mirror and HSV pass 1 act on the tap (the plain branch: TrainTransform applies both before preproc's resize)
struct SourceTaps {
  const uint8_t* img;
  int w;
  bool mirror, hsv, rgb;
  const uint8_t* lut;
  const int *sdiv, *hdiv;
  __device__ __forceinline__ void operator()(int y, int x, int v[3]) const {
    const uint8_t* p = img + ((size_t)y * w + (mirror ? w - 1 - x : x)) * 3;
#pragma unroll
    for (int k = 0; k < 3; ++k) v[k] = (int)p[k];
    if (hsv) hsv_pass(v, lut, rgb, sdiv, hdiv);
  }
};

// a 4-byte-a-pixel canvas of this file
struct CanvasTaps {
  const uint32_t* img;
  int w;
  __device__ __forceinline__ void operator()(int y, int x, int v[3]) const { unpack_px(img[(size_t)y * w + x], v); }
};

// pixel (r, c) of source `s` (a table row's source block) after its resize
__device__ __forceinline__ void source_px(const uint8_t* __restrict__ src, const long long* __restrict__ s, int r, int c, int v[3]) {
  const StridedTaps taps{src + (size_t)s[sOff], (size_t)s[sW]};
  resize_px(taps, (int)s[sW], (int)s[sH], (int)s[sMode], __longlong_as_double(s[sScaleX]), __longlong_as_double(s[sScaleY]), r, c, v);
}

// pixel (x, y) of the mosaic canvas: the last of the four pastes that covers it, else 114
__device__ __forceinline__ uint32_t mosaic_px(const uint8_t* __restrict__ src, const long long* __restrict__ row, int x, int y) {
  int hit = -1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {             // later pastes overwrite earlier ones
    const long long* s = row + cSrc0 + k * kSrcCols;
    const int lx = (int)s[sLx], ly = (int)s[sLy];
    if (x >= lx && x < lx + (int)s[sPw] && y >= ly && y < ly + (int)s[sPh]) hit = k;
  }
  if (hit < 0) return kPadPixel;
  const long long* s = row + cSrc0 + hit * kSrcCols;
  int v[3];
  source_px(src, s, y - (int)s[sLy] + (int)s[sSy], x - (int)s[sLx] + (int)s[sSx], v);
  return pack_px(v);
}

// pixel (x, y) of the cp canvas: the resized mixup image top-left, else 114
__device__ __forceinline__ uint32_t cp_px(const uint8_t* __restrict__ src, const long long* __restrict__ s, int x, int y) {
  if (y >= (int)s[sPh] || x >= (int)s[sPw]) return kPadPixel;
  int v[3];
  source_px(src, s, y, x, v);
  return pack_px(v);
}

// launch 1: canvas rows [0, 2H) are the mosaic canvas (2W wide), rows [2H, 3H) the cp canvas (W wide) of mixup rows.  A thread makes
// four neighbouring pixels of a row and stores them as one 16-byte vector where the row's width and alignment allow.
constexpr int kCanvasPx = 4;
__global__ __launch_bounds__(256) void canvas_kernel(const uint8_t* __restrict__ src, const long long* __restrict__ table,
                                                     uint32_t* __restrict__ canvases, int H, int W) {
  const int b = blockIdx.z;
  const long long* row = table + (size_t)b * kCols;
  const int branch = (int)row[cBranch];
  if (branch == kPlain) return;             // the whole workgroup
  const int x0 = (blockIdx.x * 64 + threadIdx.x) * kCanvasPx, y = blockIdx.y * 4 + threadIdx.y;
  uint32_t* base = canvases + (size_t)b * 5 * H * W;
  const bool mosaic = y < 2 * H;
  const int yy = mosaic ? y : y - 2 * H, width = mosaic ? 2 * W : W;
  if ((!mosaic && (branch != kMixup || yy >= H)) || x0 >= width) return;
  uint32_t* dst = mosaic ? base + (size_t)yy * width : base + (size_t)4 * H * W + (size_t)yy * width;
  const long long* mix = row + cSrc0 + kMixSource * kSrcCols;
  uint32_t px[kCanvasPx];
#pragma unroll
  for (int k = 0; k < kCanvasPx; ++k) {
    const int x = x0 + k;
    px[k] = x >= width ? 0u : (mosaic ? mosaic_px(src, row, x, yy) : cp_px(src, mix, x, yy));
  }
  if (x0 + kCanvasPx <= width && ((uintptr_t)(dst + x0) & 15) == 0) {
    *reinterpret_cast<uint4*>(dst + x0) = make_uint4(px[0], px[1], px[2], px[3]);
  } else {
#pragma unroll
    for (int k = 0; k < kCanvasPx; ++k)
      if (x0 + k < width) dst[x0 + k] = px[k];
  }
}

// cv2.warpAffine(canvas of cw x ch, M, INTER_LINEAR, borderValue 114) at (x, y); Minv is the inverted map
__device__ __forceinline__ void warp_px(const uint32_t* __restrict__ canvas, int cw, int ch, const double* Minv, int x, int y, int v[3]) {
  int sx, sy, alpha;
  src_coord(Minv, x, y, false, sx, sy, alpha);
  int w[4], p[4][3];
  bilinear_weights_u8(alpha >> INTER_BITS, alpha & (INTER_TAB_SIZE - 1), w);
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const int xx = sx + (t & 1), yy = sy + (t >> 1);
    const bool in = xx >= 0 && xx < cw && yy >= 0 && yy < ch;
    unpack_px(in ? canvas[(size_t)yy * cw + xx] : kPadPixel, p[t]);
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) v[k] = bilinear_u8(p[0][k], p[1][k], p[2][k], p[3][k], w);
}

// launch 2: one output pixel per thread
__global__ __launch_bounds__(256) void output_kernel(const uint8_t* __restrict__ src, const long long* __restrict__ table,
                                                     const uint32_t* __restrict__ canvases, const uint8_t* __restrict__ lut,
                                                     float* __restrict__ out, int* __restrict__ flags, int H, int W) {
  const int b = blockIdx.z, B = gridDim.z;
  const long long* row = table + (size_t)b * kCols;
  const int* sdiv = reinterpret_cast<const int*>(table + (size_t)B * kCols);
  const int* hdiv = sdiv + 256;
  const int branch = (int)row[cBranch], f = (int)row[cFlags];
  if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0) flags[b] = (f & fSingular) ? 1 : 0;
  const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y * 4 + threadIdx.y;
  if (x >= W || y >= H) return;
  const bool fallback = (f & fFallback) != 0;          // preproc(image_o): the image before HSV pass 1 and the mirror
  const bool hsv1 = (f & fHsv1) != 0 && !fallback, mirror = (f & fMirror) != 0 && !fallback;
  const uint8_t* lut_b = lut + (size_t)b * 2 * 768;
  int v[3] = {kPad, kPad, kPad};
  if (branch == kPlain) {
    const long long* s = row + cSrc0;
    if (y < (int)s[sDh] && x < (int)s[sDw]) {
      const SourceTaps taps{src + (size_t)s[sOff], (int)s[sW], mirror, hsv1, (f & fHsv1Rgb) != 0, lut_b, sdiv, hdiv};
      resize_px(taps, (int)s[sW], (int)s[sH], (int)s[sMode], __longlong_as_double(s[sScaleX]), __longlong_as_double(s[sScaleY]), y, x, v);
    }
  } else {
    const uint32_t* base = canvases + (size_t)b * 5 * H * W;
    const int xs = mirror ? W - 1 - x : x;
    double Minv[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) Minv[k] = __longlong_as_double(row[cM0 + k]);
    warp_px(base, 2 * W, 2 * H, Minv, xs, y, v);
    if (branch == kMixup) {
      int m[3] = {0, 0, 0};                 // outside the jittered image: the zeros it was placed on
      const int jw = (int)row[cJw], jh = (int)row[cJh];
      const int py = y + (int)row[cYOff], px = xs + (int)row[cXOff];
      if (py < jh && px < jw) {
        const CanvasTaps taps{base + (size_t)4 * H * W, W};
        resize_px(taps, W, H, (int)row[cMode2], __longlong_as_double(row[cScale2X]), __longlong_as_double(row[cScale2Y]), py,
                  (f & fMixFlip) ? jw - 1 - px : px, m);
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) v[k] = (int)__fadd_rn(__fmul_rn(0.5f, (float)v[k]), __fmul_rn(0.5f, (float)m[k]));
    }
    if (hsv1) hsv_pass(v, lut_b, (f & fHsv1Rgb) != 0, sdiv, hdiv);
  }
  if (f & fHsv2) hsv_pass(v, lut_b + 768, (f & fHsv2Rgb) != 0, sdiv, hdiv);
  const size_t plane = (size_t)H * W;
  float* o = out + (size_t)b * 3 * plane + (size_t)y * W + x;
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k * plane] = (float)v[k];
}

size_t table_bytes(int B) { return (size_t)B * kCols * sizeof(long long) + kDivInts * sizeof(int); }

// checks one source block; cw x ch is the canvas it is pasted on
int check_source(const char* what, int b, int k, const long long* s, long long src_bytes, long long cw, long long ch) {
  const long long off = s[sOff], w = s[sW], h = s[sH], dw = s[sDw], dh = s[sDh];
  GDRNPP_REQUIRE(w >= 1 && h >= 1 && w < 32768 && h < 32768 && off >= 0 && off <= src_bytes && w * h * 3 <= src_bytes - off, GDRNPP_EINVAL,
                 "%s: row %d source %d: a %lld x %lld image at offset %lld lies outside the %lld bytes of src", what, b, k, w, h, off, src_bytes);
  GDRNPP_REQUIRE(dw >= 1 && dh >= 1 && dw < 32768 && dh < 32768, GDRNPP_EINVAL, "%s: row %d source %d: resized to %lld x %lld", what, b, k, dw, dh);
  char where[48];
  std::snprintf(where, sizeof where, "row %d source %d", b, k);
  if (int e = check_request(what, where, ResizeRequest{w, h, dw, dh, s[sMode], as_double(s[sScaleX]), as_double(s[sScaleY])})) return e;
  const long long lx = s[sLx], ly = s[sLy], px = s[sSx], py = s[sSy], pw = s[sPw], ph = s[sPh];
  GDRNPP_REQUIRE(pw >= 0 && ph >= 0 && px >= 0 && py >= 0 && px + pw <= dw && py + ph <= dh && lx >= 0 && ly >= 0 && lx + pw <= cw && ly + ph <= ch,
                 GDRNPP_EINVAL, "%s: row %d source %d: paste of %lld x %lld from (%lld, %lld) of %lld x %lld to (%lld, %lld) of %lld x %lld", what,
                 b, k, pw, ph, px, py, dw, dh, lx, ly, cw, ch);
  return 0;
}

}  // namespace

extern "C" size_t gdrnpp_yolox_train_inputs_workspace_bytes(int B, int H, int W) {
  if (B <= 0 || H <= 0 || W <= 0) return 0;
  return ((table_bytes(B) + 15) / 16) * 16 + (size_t)B * 5 * H * W * sizeof(uint32_t);
}

extern "C" int gdrnpp_yolox_train_inputs(const unsigned char* src, long long src_bytes, const long long* table, const unsigned char* lut,
                                         int B, int H, int W, float* out, int* flags, void* workspace, size_t workspace_bytes,
                                         void* stream) {
  const char* what = "gdrnpp_yolox_train_inputs";
  GDRNPP_REQUIRE(B >= 0, GDRNPP_EINVAL, "%s: B=%d", what, B);
  if (B == 0) return 0;
  GDRNPP_REQUIRE(src && table && lut && out && flags && workspace, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(H > 0 && W > 0 && src_bytes >= 0, GDRNPP_EINVAL, "%s: H=%d W=%d src_bytes=%lld", what, H, W, src_bytes);
  // the warp's source coordinate saturates to a short: the 2H x 2W canvas has to stay below it
  GDRNPP_REQUIRE(H <= 16383 && W <= 16383 && B <= 65535, GDRNPP_ELIMIT, "%s: B=%d H=%d W=%d (B <= 65535, H and W <= 16383)", what, B, H, W);
  GDRNPP_REQUIRE(workspace_bytes >= gdrnpp_yolox_train_inputs_workspace_bytes(B, H, W) && ((uintptr_t)workspace & 15) == 0, GDRNPP_EINVAL,
                 "%s: workspace of %zu bytes (needs %zu, 16-byte aligned)", what, workspace_bytes,
                 gdrnpp_yolox_train_inputs_workspace_bytes(B, H, W));
  const size_t n_tab = (size_t)B * kCols;
  std::vector<long long> host(n_tab + kDivInts / 2);
  std::memcpy(host.data(), table, n_tab * sizeof(long long));
  bool any_canvas = false;
  for (int b = 0; b < B; ++b) {
    long long* t = host.data() + (size_t)b * kCols;
    const long long branch = t[cBranch], f = t[cFlags];
    GDRNPP_REQUIRE(branch >= kPlain && branch <= kMixup, GDRNPP_EINVAL, "%s: row %d: branch=%lld", what, b, branch);
    GDRNPP_REQUIRE(f >= 0 && (f & ~(long long)(fAll & ~fSingular)) == 0, GDRNPP_EINVAL, "%s: row %d: flags=%lld", what, b, f);
    if (branch == kPlain) {
      GDRNPP_REQUIRE((f & (fHsv2 | fHsv2Rgb | fMixFlip)) == 0, GDRNPP_EINVAL, "%s: row %d: flags=%lld on the plain branch, which has no HSV pass 2 and no mixup",
                     what, b, f);
      if (int e = check_source(what, b, 0, t + cSrc0, src_bytes, W, H)) return e;
      const long long* s = t + cSrc0;
      GDRNPP_REQUIRE(s[sLx] == 0 && s[sLy] == 0 && s[sSx] == 0 && s[sSy] == 0 && s[sPw] == s[sDw] && s[sPh] == s[sDh], GDRNPP_EINVAL,
                     "%s: row %d: the plain branch pastes the whole resized source top-left", what, b);
      continue;
    }
    any_canvas = true;
    for (int k = 0; k < 4; ++k)
      if (int e = check_source(what, b, k, t + cSrc0 + k * kSrcCols, src_bytes, 2LL * W, 2LL * H)) return e;
    double M[6];
    for (int k = 0; k < 6; ++k) {
      M[k] = as_double(t[cM0 + k]);
      GDRNPP_REQUIRE(std::isfinite(M[k]) && std::fabs(M[k]) < 1e6, GDRNPP_EINVAL, "%s: row %d: M[%d]=%g", what, b, k, M[k]);
    }
    if (!invert_affine(M)) t[cFlags] |= fSingular;      // warp_affine.hpp; this file is compiled without contraction
    // cvRound of the 10-bit fixed-point coordinate has to stay an int: each of its two terms below 1e6 pixels
    GDRNPP_REQUIRE(std::fabs(M[0]) * W < 1e6 && std::fabs(M[3]) * W < 1e6 && std::fabs(M[1]) * H + std::fabs(M[2]) < 1e6 &&
                       std::fabs(M[4]) * H + std::fabs(M[5]) < 1e6,
                   GDRNPP_EINVAL, "%s: row %d: inverse map [%g %g %g; %g %g %g] leaves the fixed-point range", what, b, M[0], M[1], M[2], M[3],
                   M[4], M[5]);
    for (int k = 0; k < 6; ++k) t[cM0 + k] = as_bits(M[k]);
    if (branch == kMixup) {
      const long long* s = t + cSrc0 + kMixSource * kSrcCols;
      if (int e = check_source(what, b, kMixSource, s, src_bytes, W, H)) return e;
      GDRNPP_REQUIRE(s[sLx] == 0 && s[sLy] == 0 && s[sSx] == 0 && s[sSy] == 0 && s[sPw] == s[sDw] && s[sPh] == s[sDh], GDRNPP_EINVAL,
                     "%s: row %d: the mixup source is pasted whole, top-left", what, b);
      const long long jw = t[cJw], jh = t[cJh], xo = t[cXOff], yo = t[cYOff];
      GDRNPP_REQUIRE(jw >= 1 && jh >= 1 && jw < 65536 && jh < 65536, GDRNPP_EINVAL, "%s: row %d: jittered size %lld x %lld", what, b, jw, jh);
      char where[48];
      std::snprintf(where, sizeof where, "row %d jitter", b);      // the second resize, of the cp canvas: mode2, scale2_x, scale2_y
      if (int e = check_request(what, where, ResizeRequest{W, H, jw, jh, t[cMode2], as_double(t[cScale2X]), as_double(t[cScale2Y])})) return e;
      GDRNPP_REQUIRE(xo >= 0 && yo >= 0 && xo + W <= (jw > W ? jw : W) && yo + H <= (jh > H ? jh : H), GDRNPP_EINVAL,
                     "%s: row %d: crop offset (%lld, %lld) leaves the padded image", what, b, xo, yo);
    }
  }
  // OpenCV's division tables of RGB -> HSV (hue range 180), behind the table in the same staged copy
  int* div = reinterpret_cast<int*>(host.data() + n_tab);
  div[0] = div[256] = 0;
  for (int i = 1; i < 256; ++i) {
    div[i] = (int)std::nearbyint((double)(255 << 12) / (1.0 * i));
    div[256 + i] = (int)std::nearbyint((double)(180 << 12) / (6.0 * i));
  }
  hipStream_t st = (hipStream_t)stream;
  // pageable source: staged before the call returns
  GDRNPP_HIP_TRY(hipMemcpyAsync(workspace, host.data(), table_bytes(B), hipMemcpyHostToDevice, st));
  const long long* d_table = (const long long*)workspace;
  uint32_t* d_canvas = reinterpret_cast<uint32_t*>((char*)workspace + ((table_bytes(B) + 15) / 16) * 16);
  if (any_canvas)
    hipLaunchKernelGGL(canvas_kernel, dim3((2 * W + 64 * kCanvasPx - 1) / (64 * kCanvasPx), (3 * H + 3) / 4, B), dim3(64, 4), 0, st, src, d_table,
                       d_canvas, H, W);
  hipLaunchKernelGGL(output_kernel, dim3((W + 63) / 64, (H + 3) / 4, B), dim3(64, 4), 0, st, src, d_table, (const uint32_t*)d_canvas, lut, out,
                     flags, H, W);
  return gdrnpp::check_launch(what);
}
