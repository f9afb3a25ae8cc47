// Background replacement of the training loader, for a batch of images in one call.
//
// gdrnpp_replace_bg   `replace_bg` + `trunc_mask` of core/base_data_loader.py:413-478 on top of `get_bg_image` / `get_bg_image_v2`
//   (:480-579) and `resize_short_edge` (core/utils/data_utils.py:208-235): wherever the (possibly truncated) instance mask is 0 the
//   image takes the pixel of a background that is a crop of a pool image, resized by cv2.resize(INTER_LINEAR) and pasted top-left
//   onto zeros.  The host makes every random draw and all size arithmetic (gdrn_modeling/train_inputs.py) and hands over one table
//   row per image (its columns: include/gdrnpp_hip.h); nothing is read back.
//   Phase 1, images with a cut only: min / max row and column of the non-zero mask bytes.  A wave walks a row 64 bytes at a time,
//   shuffles reduce the wave, LDS the four waves, and one lane issues the workgroup's four vector atomicMin / atomicMax on extents
//   the host staged as (INT_MAX, -1, INT_MAX, -1) together with the table.  Min and max do not depend on order.
//   Phase 2, one thread per pixel: the cut line a + (b - a) u in fp64 from correctly rounded single operations (Python's
//   random.uniform, truncated by int()), keep = mask != 0 and the pixel's side of the line, mask_trunc = keep, and where !keep the
//   background pixel at (r, c): the resize restated per pixel from its four source taps (resize_u8.hpp; copy and 2:1 area mean are
//   OpenCV's two shortcuts), 0 outside the dh x dw paste.  Bytes of kept pixels are never written.  Bytes are read and written one
//   by one: rows are 3 W bytes, no alignment to assume.  Memory-bound: reads H W mask bytes (twice with a cut) and the taps, which
//   neighbours share through L2; writes at most 4 H W bytes.
#include "common.hpp"
#include "resize_u8.hpp"

#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

namespace {

using namespace gdrnpp::resize_u8;

constexpr int kCols = 14;                  // the table's columns, as include/gdrnpp_hip.h lists them
enum { cDo = 0, cOff, cStride, cX0, cY0, cCw, cCh, cDw, cDh, cMode, cScaleX, cScaleY, cCut, cU };
static_assert(cU + 1 == kCols, "one name per column");
enum { kCutNone = 0, kCutUpper = 1, kCutBottom = 2, kCutLeft = 3, kCutRight = 4 };
constexpr int kExtentRows = 16;             // rows of one phase-1 workgroup: four per wave

// phase 1: ext[b] = (min row, max row, min column, max column) of the non-zero bytes of mask b
__global__ __launch_bounds__(256) void mask_extent_kernel(const uint8_t* __restrict__ masks, const long long* __restrict__ table, int H,
                                                          int W, int* __restrict__ ext) {
  __shared__ int s_part[4][4];
  const int b = blockIdx.y, lane = threadIdx.x, wave = threadIdx.y;
  const long long* row = table + (size_t)b * kCols;
  if (row[cDo] == 0 || row[cCut] == kCutNone) return;      // the whole workgroup
  const uint8_t* m = masks + (size_t)b * H * W;
  int rmin = INT_MAX, rmax = -1, cmin = INT_MAX, cmax = -1;
  const int r_end = min(H, ((int)blockIdx.x + 1) * kExtentRows);
  for (int r = blockIdx.x * kExtentRows + wave; r < r_end; r += 4) {
    const uint8_t* p = m + (size_t)r * W;
    for (int c = lane; c < W; c += 64) {
      if (p[c] != 0) {
        rmin = min(rmin, r);
        rmax = max(rmax, r);
        cmin = min(cmin, c);
        cmax = max(cmax, c);
      }
    }
  }
  for (int off = 32; off >= 1; off >>= 1) {
    rmin = min(rmin, __shfl_xor(rmin, off, 64));
    rmax = max(rmax, __shfl_xor(rmax, off, 64));
    cmin = min(cmin, __shfl_xor(cmin, off, 64));
    cmax = max(cmax, __shfl_xor(cmax, off, 64));
  }
  if (lane == 0) {
    s_part[wave][0] = rmin;
    s_part[wave][1] = rmax;
    s_part[wave][2] = cmin;
    s_part[wave][3] = cmax;
  }
  __syncthreads();
  if (wave == 0 && lane == 0) {
    for (int w = 1; w < 4; ++w) {
      rmin = min(rmin, s_part[w][0]);
      rmax = max(rmax, s_part[w][1]);
      cmin = min(cmin, s_part[w][2]);
      cmax = max(cmax, s_part[w][3]);
    }
    if (rmax >= 0) {
      atomicMin(ext + 4 * b + 0, rmin);
      atomicMax(ext + 4 * b + 1, rmax);
      atomicMin(ext + 4 * b + 2, cmin);
      atomicMax(ext + 4 * b + 3, cmax);
    }
  }
}

// phase 2: the cut, mask_trunc and the composite
__global__ __launch_bounds__(256) void replace_bg_kernel(uint8_t* __restrict__ images, const uint8_t* __restrict__ masks,
                                                         uint8_t* __restrict__ mask_trunc, const uint8_t* __restrict__ bg,
                                                         const long long* __restrict__ table, const int* __restrict__ ext,
                                                         int* __restrict__ flags, int H, int W) {
  const int b = blockIdx.z;
  const long long* row = table + (size_t)b * kCols;
  const bool first = blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && threadIdx.y == 0;
  if (row[cDo] == 0) {                      // left untouched, mask_trunc not written
    if (first) flags[b] = 0;
    return;
  }
  int cut = (int)row[cCut], line = 0;
  bool empty = false;
  if (cut != kCutNone) {
    // the reference's names: x1 / x2 are rows, y1 / y2 are columns
    const int x1 = ext[4 * b + 0], x2 = ext[4 * b + 1], y1 = ext[4 * b + 2], y2 = ext[4 * b + 3];
    if (x2 < 0) {                           // np.min of nothing raises in the reference; here: the flag, and no cut
      empty = true;
      cut = kCutNone;
    } else {
      const double u = __longlong_as_double(row[cU]);
      const double c_h = __dmul_rn(0.5, (double)(x1 + x2)), c_w = __dmul_rn(0.5, (double)(y1 + y2));
      double lo, hi;
      if (cut == kCutUpper) { lo = (double)x1; hi = c_h; }
      else if (cut == kCutBottom) { lo = c_h; hi = (double)x2; }
      else if (cut == kCutLeft) { lo = (double)y1; hi = c_w; }
      else { lo = c_w; hi = (double)y2; }
      line = (int)__dadd_rn(lo, __dmul_rn(__dsub_rn(hi, lo), u));      // int(random.uniform(lo, hi)): no FMA, one ulp moves the line
    }
  }
  if (first) flags[b] = empty ? 1 : 0;
  const int c = blockIdx.x * 64 + threadIdx.x, r = blockIdx.y * 4 + threadIdx.y;
  if (c >= W || r >= H) return;
  const size_t px = ((size_t)b * H + r) * W + c;
  bool keep = masks[px] != 0;
  if (cut == kCutUpper) keep = keep && r >= line;
  else if (cut == kCutBottom) keep = keep && r < line;
  else if (cut == kCutLeft) keep = keep && c >= line;
  else if (cut == kCutRight) keep = keep && c < line;
  mask_trunc[px] = keep ? 1 : 0;
  if (keep) return;
  int v[3] = {0, 0, 0};                     // outside the paste: the zeros it was pasted on
  if (r < (int)row[cDh] && c < (int)row[cDw]) {
    // cv2.resize(crop, INTER_LINEAR) at (r, c): the crop is cw x ch pixels of a pool image whose rows lie `stride` pixels apart
    const size_t stride = (size_t)row[cStride];
    const StridedTaps crop{bg + (size_t)row[cOff] + ((size_t)row[cY0] * stride + (size_t)row[cX0]) * 3, stride};
    resize_px(crop, (int)row[cCw], (int)row[cCh], (int)row[cMode], __longlong_as_double(row[cScaleX]), __longlong_as_double(row[cScaleY]), r,
              c, v);
  }
  uint8_t* o = images + px * 3;
#pragma unroll
  for (int k = 0; k < 3; ++k) o[k] = (uint8_t)v[k];
}

}  // namespace

extern "C" size_t gdrnpp_replace_bg_workspace_bytes(int B) {
  if (B <= 0) return 0;
  return (size_t)B * kCols * sizeof(long long) + (size_t)B * 4 * sizeof(int);
}

extern "C" int gdrnpp_replace_bg(unsigned char* images, const unsigned char* masks, unsigned char* mask_trunc, int B, int H, int W,
                                 const unsigned char* bg, long long bg_bytes, const long long* table, int* flags, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  const char* what = "gdrnpp_replace_bg";
  GDRNPP_REQUIRE(B >= 0, GDRNPP_EINVAL, "%s: B=%d", what, B);
  if (B == 0) return 0;
  GDRNPP_REQUIRE(images && masks && mask_trunc && table && flags && workspace, GDRNPP_EINVAL, "%s: null pointer", what);
  GDRNPP_REQUIRE(H > 0 && W > 0, GDRNPP_EINVAL, "%s: H=%d W=%d", what, H, W);
  GDRNPP_REQUIRE(H < 32768 && W < 32768 && B <= 65535, GDRNPP_ELIMIT, "%s: B=%d H=%d W=%d (B <= 65535, H and W < 32768)", what, B, H, W);
  GDRNPP_REQUIRE(bg_bytes >= 0 && (bg || bg_bytes == 0), GDRNPP_EINVAL, "%s: bg_bytes=%lld", what, bg_bytes);
  GDRNPP_REQUIRE(workspace_bytes >= gdrnpp_replace_bg_workspace_bytes(B) && ((uintptr_t)workspace & 7) == 0, GDRNPP_EINVAL,
                 "%s: workspace of %zu bytes (needs %zu, 8-byte aligned)", what, workspace_bytes, gdrnpp_replace_bg_workspace_bytes(B));
  bool any_cut = false;
  for (int b = 0; b < B; ++b) {
    const long long* t = table + (size_t)b * kCols;
    if (t[cDo] == 0) continue;
    const long long off = t[cOff], stride = t[cStride], x0 = t[cX0], y0 = t[cY0], cw = t[cCw], ch = t[cCh], dw = t[cDw], dh = t[cDh];
    GDRNPP_REQUIRE(stride >= 1 && stride < 32768 && x0 >= 0 && y0 >= 0 && y0 < 32768 && cw >= 1 && ch >= 1 && ch < 32768 &&
                       x0 + cw <= stride,
                   GDRNPP_EINVAL, "%s: row %d: crop x0=%lld y0=%lld cw=%lld ch=%lld leaves its image of row stride %lld", what, b, x0, y0,
                   cw, ch, stride);
    GDRNPP_REQUIRE(off >= 0 && off <= bg_bytes && ((y0 + ch - 1) * stride + x0 + cw) * 3 <= bg_bytes - off, GDRNPP_EINVAL,
                   "%s: row %d: offset %lld with a crop ending %lld bytes on lies outside the %lld bytes of bg", what, b, off,
                   ((y0 + ch - 1) * stride + x0 + cw) * 3, bg_bytes);
    GDRNPP_REQUIRE(dw >= 1 && dh >= 1 && dw <= W && dh <= H, GDRNPP_EINVAL,
                   "%s: row %d: resized background %lld x %lld does not fit the %d x %d image (the reference's own paste fails here)",
                   what, b, dw, dh, W, H);
    char where[32];
    std::snprintf(where, sizeof where, "row %d", b);
    if (int e = check_request(what, where, ResizeRequest{cw, ch, dw, dh, t[cMode], as_double(t[cScaleX]), as_double(t[cScaleY])})) return e;
    const long long cut = t[cCut];
    const double u = as_double(t[cU]);
    GDRNPP_REQUIRE(cut >= kCutNone && cut <= kCutRight, GDRNPP_EINVAL, "%s: row %d: cut=%lld", what, b, cut);
    GDRNPP_REQUIRE(cut == kCutNone || (u >= 0. && u < 1.), GDRNPP_EINVAL, "%s: row %d: u=%g outside [0, 1)", what, b, u);
    any_cut = any_cut || cut != kCutNone;
  }
  // one staged copy: the table, then per image the extents phase 1 reduces into.  Pageable source: staged before the call returns.
  const size_t n_tab = (size_t)B * kCols;
  std::vector<long long> host(n_tab + (size_t)B * 2);
  std::memcpy(host.data(), table, n_tab * sizeof(long long));
  int* init = reinterpret_cast<int*>(host.data() + n_tab);
  for (int b = 0; b < B; ++b) {
    init[4 * b + 0] = init[4 * b + 2] = INT_MAX;
    init[4 * b + 1] = init[4 * b + 3] = -1;
  }
  hipStream_t st = (hipStream_t)stream;
  GDRNPP_HIP_TRY(hipMemcpyAsync(workspace, host.data(), host.size() * sizeof(long long), hipMemcpyHostToDevice, st));
  const long long* d_table = (const long long*)workspace;
  int* d_ext = (int*)((long long*)workspace + n_tab);
  if (any_cut)
    hipLaunchKernelGGL(mask_extent_kernel, dim3((H + kExtentRows - 1) / kExtentRows, B), dim3(64, 4), 0, st, masks, d_table, H, W, d_ext);
  hipLaunchKernelGGL(replace_bg_kernel, dim3((W + 63) / 64, (H + 3) / 4, B), dim3(64, 4), 0, st, images, masks, mask_trunc, bg, d_table,
                     (const int*)d_ext, flags, H, W);
  return gdrnpp::check_launch(what);
}
