// GDRN's per-ROI training targets on gfx950: what GDRN_DatasetFromList.read_data_train forms per instance from its xyz_crop record
// and its masks (core/gdrn_modeling/datasets/data_loader.py:448-612 with TRAIN.VIS off):
//   xyz        = zeros((H, W, 3), float32); xyz[y1:y2+1, x1:x2+1] = xyz_crop (float16)                                  :449-454
//   mask_obj   = xyz has a non-zero component; mask_visib = segmentation * mask_obj; mask_trunc = mask_visib [* trunc]    :456, :526-531
//   roi_mask_* = cv2.warpAffine(mask[:, :, None], M, (out, out), INTER_NEAREST)                                           :539-557
//   roi_xyz    = cv2.warpAffine(xyz, M, (out, out), INTER_NEAREST); roi_region = xyz_to_region(roi_xyz, fps_points)       :560-566
//   roi_xyz[c] = roi_xyz[c] / extent[c] + 0.5; clip to [0, 0.999999], bin = uint8(clipped * n_bin), n_bin where the mask is 0   :568-605
// A nearest-neighbour warp of a product of masks is the product of the masks' bytes at the one source pixel, so nothing of the
// full-image maps is materialised: the kernel reads, per output pixel, three fp16 values of the packed crop (zero outside its box)
// and up to three mask bytes, and writes every target of the batch in one launch.
//
// Design: grid (pixel tiles, ROI), thread = one output pixel, x fastest: every output plane is written as coalesced rows.  The ROI's
// inverse affine map is solved once per workgroup by one lane (warp_affine.hpp, as crop_resize.hip does) while the others stage the
// object's farthest-point-sampling points in LDS (at most 256 x 3 doubles = 6 KB, read by every lane at the same address: a broadcast).
// The op is bound by launch latency and its writes (29 bytes per output pixel against <= 9 bytes read through L2), not by arithmetic.
//
// Exactness: the source pixel is OpenCV's integer arithmetic; the region is the argmin over the fp64 distances
// sqrt((dx dx + dy dy) + dz dz) of scipy's cdist (differences taken in fp64 from the float32 value of the fp16 source, no contraction,
// correctly rounded square root, first index on ties, np.argmin's first NaN).  sqrt is monotone, so a candidate whose squared sum is not
// below the best one's cannot have a smaller root and is dismissed without a root; the others compare their rounded roots.  roi_xyz is
// one IEEE float32 division and one addition.
#include "common.hpp"
#include "warp_affine.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxFps = 256;
constexpr int kMaxOut = 4096;

struct RoiTargetArgs {
  const _Float16* xyz;
  const long long* xyz_off;
  const int* xyz_box;
  long long xyz_px;
  const unsigned char* masks;
  const int *visib_idx, *trunc_idx, *full_idx;
  int n_masks, H, W;
  const double *centers, *scales;
  const int* obj;
  const float* extents;
  const double* fps;
  int n_obj, F, out, n_bin, bin_mask;
  float *m_obj, *m_visib, *m_trunc, *m_full;
  int* region;
  float* roi_xyz;
  unsigned char* xyz_bin;
};

__global__ __launch_bounds__(kThreads) void roi_targets_kernel(const RoiTargetArgs a) {
  __shared__ double sM[6];
  __shared__ double sF[kMaxFps * 3];
  const int bi = blockIdx.y, tid = threadIdx.x;
  const int out = a.out, F = a.F;
  const bool need_obj = a.roi_xyz || a.xyz_bin || (a.region && F > 0);
  const int o = need_obj ? a.obj[bi] : 0;
  const bool obj_ok = o >= 0 && o < a.n_obj;   // the binding checks it; a ROI whose obj is outside the tables gets zeros
  roi_map_solve(a.centers, a.scales, bi, out, sM);
  if (a.region && F > 0 && obj_ok) {
    const double* f = a.fps + (size_t)o * F * 3;
    for (int i = tid; i < F * 3; i += kThreads) sF[i] = f[i];
  }
  __syncthreads();                             // one barrier for the map and the points
  const int p = blockIdx.x * kThreads + tid;
  if (p >= out * out) return;
  double M[6];
  roi_map_read(sM, M);
  const int y = p / out, x = p - y * out;
  int sx, sy, alpha;
  src_coord(M, x, y, true, sx, sy, alpha);
  const bool inside = sx >= 0 && sx < a.W && sy >= 0 && sy < a.H;

  // the xyz source: the pose's box of the packed buffer, zero outside it (and outside the image: the border)
  const int x1 = a.xyz_box[4 * bi], y1 = a.xyz_box[4 * bi + 1], x2 = a.xyz_box[4 * bi + 2], y2 = a.xyz_box[4 * bi + 3];
  float v[3] = {0.f, 0.f, 0.f};
  if (inside && sx >= x1 && sx <= x2 && sy >= y1 && sy <= y2) {
    const long long px = a.xyz_off[bi] + (long long)(sy - y1) * (x2 - x1 + 1) + (sx - x1);
    if (px >= 0 && px < a.xyz_px) {
      const _Float16* s = a.xyz + px * 3;
      v[0] = (float)s[0]; v[1] = (float)s[1]; v[2] = (float)s[2];
    }
  }
  const bool is_obj = v[0] != 0.f || v[1] != 0.f || v[2] != 0.f;

  // the masks: a byte counts as 1 if it is not 0; an index of -1 (or no masks) selects the documented stand-in
  const size_t plane = (size_t)a.H * a.W, spix = inside ? (size_t)sy * a.W + sx : 0;
  const int vi = a.masks ? a.visib_idx[bi] : -1, ti = a.masks ? a.trunc_idx[bi] : -1, fi = a.masks ? a.full_idx[bi] : -1;
  const bool b_visib = vi < 0 ? true : (inside && vi < a.n_masks && a.masks[vi * plane + spix] != 0);
  const bool b_trunc = ti < 0 ? true : (inside && ti < a.n_masks && a.masks[ti * plane + spix] != 0);
  const bool b_full = fi < 0 ? false : (inside && fi < a.n_masks && a.masks[fi * plane + spix] != 0);
  const bool is_visib = b_visib && is_obj, is_trunc = b_trunc && is_visib;

  const size_t q = (size_t)bi * out * out + p;
  if (a.m_obj) a.m_obj[q] = is_obj ? 1.f : 0.f;
  if (a.m_visib) a.m_visib[q] = is_visib ? 1.f : 0.f;
  if (a.m_trunc) a.m_trunc[q] = is_trunc ? 1.f : 0.f;
  if (a.m_full) a.m_full[q] = b_full ? 1.f : 0.f;

  if (a.region && F > 0) {
    int best_j = -1;
    if (is_obj && obj_ok) {  // the background's region is 0 whatever its argmin
      const double px = (double)v[0], py = (double)v[1], pz = (double)v[2];
      double best2, best;
      {
        const double dx = px - sF[0], dy = py - sF[1], dz = pz - sF[2];
        best2 = (dx * dx + dy * dy) + dz * dz;
        best = __dsqrt_rn(best2);
        best_j = 0;
      }
      for (int j = 1; j < F; ++j) {
        const double dx = px - sF[3 * j], dy = py - sF[3 * j + 1], dz = pz - sF[3 * j + 2];
        const double d2 = (dx * dx + dy * dy) + dz * dz;
        if (d2 < best2) {
          const double d = __dsqrt_rn(d2);
          if (d < best) { best = d; best2 = d2; best_j = j; }
        } else if (d2 != d2 && best2 == best2) {  // np.argmin: the first NaN
          best = best2 = d2; best_j = j;
        }
      }
    }
    a.region[q] = best_j + 1;
  }

  if (a.roi_xyz || a.xyz_bin) {
    const bool sel = a.bin_mask == 0 ? is_trunc : a.bin_mask == 1 ? is_visib : a.bin_mask == 2 ? is_obj : b_full;
    const float* e = a.extents + 3 * (size_t)(obj_ok ? o : 0);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float r = obj_ok ? v[c] / e[c] + 0.5f : 0.f;  // IEEE division, no fused multiply-add: the background holds 0.5
      const size_t qc = ((size_t)bi * 3 + c) * out * out + p;
      if (a.n_bin > 0) {
        r = r < 0.f ? 0.f : r;  // roi_x_norm is a view of roi_xyz[0]: the clipping lands in roi_xyz too (:579-592)
        r = r > 0.999999f ? 0.999999f : r;
        if (a.xyz_bin) a.xyz_bin[qc] = (sel && obj_ok) ? (unsigned char)(int)(r * (float)a.n_bin) : (unsigned char)(obj_ok ? a.n_bin : 0);
      }
      if (a.roi_xyz) a.roi_xyz[qc] = r;
    }
  }
}

}  // namespace

extern "C" {

int gdrnpp_roi_train_targets(const unsigned short* xyz_packed, long long xyz_px, const long long* xyz_off, const int* xyz_box,
                             const unsigned char* masks, int n_masks, const int* visib_idx, const int* trunc_idx, const int* full_idx,
                             int H, int W, const double* centers, const double* scales, const int* obj, const float* extents, int n_obj,
                             const double* fps, int F, int out_res, int n_bin, int bin_mask, float* roi_mask_obj, float* roi_mask_visib,
                             float* roi_mask_trunc, float* roi_mask_full, int* roi_region, float* roi_xyz, unsigned char* roi_xyz_bin,
                             int n, void* stream) {
  const char* const fn = "gdrnpp_roi_train_targets";
  GDRNPP_REQUIRE(n >= 0, GDRNPP_EINVAL, "%s: n=%d", fn, n);
  GDRNPP_REQUIRE(H > 0 && W > 0, GDRNPP_EINVAL, "%s: H=%d W=%d", fn, H, W);
  GDRNPP_REQUIRE(H < 32767 && W < 32767, GDRNPP_ELIMIT, "%s: H=%d W=%d: an image side must be below SHRT_MAX", fn, H, W);
  GDRNPP_REQUIRE(out_res > 0, GDRNPP_EINVAL, "%s: out_res=%d", fn, out_res);
  GDRNPP_REQUIRE(out_res <= kMaxOut, GDRNPP_ELIMIT, "%s: out_res=%d > %d", fn, out_res, kMaxOut);
  GDRNPP_REQUIRE(F >= 0, GDRNPP_EINVAL, "%s: F=%d", fn, F);
  GDRNPP_REQUIRE(F <= kMaxFps, GDRNPP_ELIMIT, "%s: F=%d > %d points per object", fn, F, kMaxFps);
  GDRNPP_REQUIRE(n_bin >= 0 && n_bin <= 255, GDRNPP_EINVAL, "%s: n_bin=%d outside [0, 255]", fn, n_bin);
  GDRNPP_REQUIRE(bin_mask >= 0 && bin_mask <= 3, GDRNPP_EINVAL, "%s: bin_mask=%d outside 0..3 (trunc, visib, obj, full)", fn, bin_mask);
  GDRNPP_REQUIRE(n_masks >= 0 && n_obj >= 0 && xyz_px >= 0, GDRNPP_EINVAL, "%s: n_masks=%d n_obj=%d xyz_px=%lld", fn, n_masks, n_obj, xyz_px);
  GDRNPP_REQUIRE(n <= 65535, GDRNPP_ELIMIT, "%s: n=%d > 65535", fn, n);
  if (n == 0) return 0;
  GDRNPP_REQUIRE(centers, GDRNPP_EINVAL, "%s: centers is null", fn);
  GDRNPP_REQUIRE(scales, GDRNPP_EINVAL, "%s: scales is null", fn);
  GDRNPP_REQUIRE(xyz_packed || xyz_px == 0, GDRNPP_EINVAL, "%s: xyz_packed is null", fn);
  GDRNPP_REQUIRE(xyz_off, GDRNPP_EINVAL, "%s: xyz_off is null", fn);
  GDRNPP_REQUIRE(xyz_box, GDRNPP_EINVAL, "%s: xyz_box is null", fn);
  if (masks) {
    GDRNPP_REQUIRE(visib_idx, GDRNPP_EINVAL, "%s: visib_idx is null", fn);
    GDRNPP_REQUIRE(trunc_idx, GDRNPP_EINVAL, "%s: trunc_idx is null", fn);
    GDRNPP_REQUIRE(full_idx, GDRNPP_EINVAL, "%s: full_idx is null", fn);
  }
  const bool want_bins = roi_xyz_bin && n_bin > 0, want_region = roi_region && F > 0;
  GDRNPP_REQUIRE(!(want_bins && bin_mask == 3) || masks, GDRNPP_EINVAL, "%s: bin_mask=3 (full) needs masks, which is null", fn);
  if (roi_xyz || want_bins || want_region) GDRNPP_REQUIRE(obj, GDRNPP_EINVAL, "%s: obj is null", fn);
  if (roi_xyz || want_bins) GDRNPP_REQUIRE(extents, GDRNPP_EINVAL, "%s: extents is null", fn);
  if (want_region) GDRNPP_REQUIRE(fps, GDRNPP_EINVAL, "%s: fps is null", fn);
  RoiTargetArgs a{};
  a.xyz = reinterpret_cast<const _Float16*>(xyz_packed); a.xyz_off = xyz_off; a.xyz_box = xyz_box; a.xyz_px = xyz_px;
  a.masks = masks; a.visib_idx = visib_idx; a.trunc_idx = trunc_idx; a.full_idx = full_idx; a.n_masks = n_masks; a.H = H; a.W = W;
  a.centers = centers; a.scales = scales; a.obj = obj; a.extents = extents; a.fps = fps; a.n_obj = n_obj; a.F = F; a.out = out_res;
  a.n_bin = n_bin; a.bin_mask = bin_mask;
  a.m_obj = roi_mask_obj; a.m_visib = roi_mask_visib; a.m_trunc = roi_mask_trunc; a.m_full = roi_mask_full;
  a.region = want_region ? roi_region : nullptr; a.roi_xyz = roi_xyz; a.xyz_bin = want_bins ? roi_xyz_bin : nullptr;
  const dim3 grid((unsigned)((out_res * out_res + kThreads - 1) / kThreads), (unsigned)n);
  hipLaunchKernelGGL(roi_targets_kernel, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
  return gdrnpp::check_launch(fn);
}

}  // extern "C"
