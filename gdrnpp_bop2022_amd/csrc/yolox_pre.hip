// The two ends of the detector that were host work: the image on its way in and the boxes on their way to the pose path.
//
// gdrnpp_yolox_letterbox   `preproc` of det/yolox/data/data_augment.py:161-177 (ValTransform, legacy=False): u8 BGR image ->
//   cv2.resize(INTER_LINEAR) to rh x rw, placed top-left on a canvas of 114, as float.  The resize restates OpenCV's 8-bit
//   path: coefficients (float)((d + 0.5) * scale - 0.5) with scale = 1 / (dst / src) in double, floor, the fraction rounded to
//   11 bits (half to even), source index clamped at both borders with the fraction dropped, horizontal pass in int, vertical
//   pass ((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2; equal sizes are a copy and an exact 2:1 reduction in
//   both axes is the area mean (a + b + c + d + 2) >> 2 — OpenCV's two shortcuts.  One thread makes a 2x2 output block: two
//   float2 stores per plane (NCHW, what YOLOX.forward takes) or three float4 stores (the Focus stem's 12-channel NHWC cell,
//   channel 3 q + c with q = top-left, bottom-left, top-right, bottom-right, as gdrnpp_yolox_focus writes it).  Bytes are read
//   one by one: image rows are 3 W bytes long, no alignment to assume.  No LDS, no atomics; reads 3 H W bytes, writes 12 Ht Wt.
//
// gdrnpp_rois_from_dets   gdrnpp_yolox_postprocess output -> the per-ROI table of roi_stream.roi_host_arrays, on the device:
//   boxes / ratio in float (detections_from_yolox), ROI parameters in double (rois_from_detections), selection as
//   load_detections_into_dataset (core/utils/dataset_utils.py:146-227).  Phase 1, one workgroup per image: rank every detection
//   by counting the ones ordered in front of it (max_det is small); phase 2: exclusive scan of the images' counts, rows written
//   at base + rank.  Positions are functions of the input alone: the order is deterministic, no atomics.
#include "common.hpp"
#include "resize_u8.hpp"

#include <cstdint>

namespace {

using namespace gdrnpp::resize_u8;          // the resize itself: forms, taps, pixel, request
constexpr float kPad = 114.f;

template <bool FOCUS>
__global__ __launch_bounds__(256) void letterbox_kernel(const uint8_t* __restrict__ img, int H, int W, int rh, int rw, int mode,
                                                        double scale_y, double scale_x, float* __restrict__ out, int Ht, int Wt,
                                                        int ldy) {
  const int cx = blockIdx.x * 64 + threadIdx.x, cy = blockIdx.y * 4 + threadIdx.y, b = blockIdx.z;
  if (cx >= (Wt >> 1) || cy >= (Ht >> 1)) return;
  const StridedTaps taps{img + (size_t)b * H * W * 3, (size_t)W};
  float v[2][2][3];                         // [row of the cell][column of the cell][colour]
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int oy = 2 * cy + r;
    Tap ty{0, 0, 0, 0};
    if (oy < rh && mode == kModeLinear) ty = linear_tap(oy, scale_y, H, false);
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int ox = 2 * cx + q;
      if (oy >= rh || ox >= rw) {
        v[r][q][0] = v[r][q][1] = v[r][q][2] = kPad;
        continue;
      }
      resize_px(taps, mode, ty, linear_tap(ox, scale_x, W, true), oy, ox, v[r][q]);
    }
  }
  if (FOCUS) {
    float4* y = reinterpret_cast<float4*>(out + (((size_t)b * (Ht >> 1) + cy) * (Wt >> 1) + cx) * ldy);
    y[0] = make_float4(v[0][0][0], v[0][0][1], v[0][0][2], v[1][0][0]);
    y[1] = make_float4(v[1][0][1], v[1][0][2], v[0][1][0], v[0][1][1]);
    y[2] = make_float4(v[0][1][2], v[1][1][0], v[1][1][1], v[1][1][2]);
  } else {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      float* plane = out + ((size_t)b * 3 + c) * Ht * Wt + (size_t)(2 * cy) * Wt + 2 * cx;
      *reinterpret_cast<float2*>(plane) = make_float2(v[0][0][c], v[0][1][c]);
      *reinterpret_cast<float2*>(plane + Wt) = make_float2(v[1][0][c], v[1][1][c]);
    }
  }
}

// ---- detections -> ROI table ------------------------------------------------------------------------------------------------
constexpr int kMaxDet = 1024;

// phase 1: slot[b][j] = position of detection j among image b's selected ROIs, or -1; n_sel[b] = how many
__global__ __launch_bounds__(256) void roi_rank_kernel(const float* __restrict__ dets, const int* __restrict__ count, int max_det,
                                                       int C, double score_thr, int top_k, int* __restrict__ slot,
                                                       int* __restrict__ n_sel) {
  __shared__ float s_score[kMaxDet];
  __shared__ int s_cls[kMaxDet];            // -1: dropped
  __shared__ unsigned char s_sel[kMaxDet];
  __shared__ int s_part[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int n = min(max(count[b], 0), max_det);
  const float* d = dets + (size_t)b * max_det * 7;
  for (int j = tid; j < n; j += 256) {
    const float sc = d[j * 7 + 4] * d[j * 7 + 5];
    const float cf = d[j * 7 + 6];
    const bool ok = cf >= 0.f && cf < (float)C && !((double)sc < score_thr);
    s_score[j] = sc;
    s_cls[j] = ok ? (int)cf : -1;
  }
  __syncthreads();
  for (int j = tid; j < n; j += 256) {
    bool sel = s_cls[j] >= 0;
    if (sel && top_k > 0) {                 // rank within the class: higher scores first, ties in NMS order
      int rank = 0;
      for (int i = 0; i < n; ++i)
        rank += (s_cls[i] == s_cls[j] && (s_score[i] > s_score[j] || (s_score[i] == s_score[j] && i < j))) ? 1 : 0;
      sel = rank < top_k;
    }
    s_sel[j] = sel ? 1 : 0;
  }
  __syncthreads();
  int mine = 0;
  for (int j = tid; j < n; j += 256) {
    int pos = -1;
    if (s_sel[j]) {
      pos = 0;
      ++mine;
      for (int i = 0; i < n; ++i) {
        if (!s_sel[i]) continue;
        const bool before = top_k > 0 ? (s_cls[i] < s_cls[j] || (s_cls[i] == s_cls[j] && (s_score[i] > s_score[j] ||
                                                                                       (s_score[i] == s_score[j] && i < j))))
                                      : i < j;
        pos += before ? 1 : 0;
      }
    }
    slot[(size_t)b * max_det + j] = pos;
  }
  for (int j = n + tid; j < max_det; j += 256) slot[(size_t)b * max_det + j] = -1;
  for (int off = 32; off >= 1; off >>= 1) mine += __shfl_xor(mine, off, 64);
  if ((tid & 63) == 0) s_part[tid >> 6] = mine;
  __syncthreads();
  if (tid == 0) n_sel[b] = s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// phase 2: base = sum of the counts of the images in front, rows written at base + slot (below cap)
__global__ __launch_bounds__(256) void roi_write_kernel(const float* __restrict__ dets, int max_det, const int* __restrict__ slot,
                                                        const int* __restrict__ n_sel, int B, float ratio, int H, int W,
                                                        double dzi_pad_scale, double out_res, const float* __restrict__ cam,
                                                        int cam_stride, const float* __restrict__ extents, int cap,
                                                        gdrnpp_roi_table t, int* __restrict__ n_rois, int* __restrict__ per_image) {
  __shared__ int s_part[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  int acc = 0;
  for (int i = tid; i < b; i += 256) acc += n_sel[i];
  for (int off = 32; off >= 1; off >>= 1) acc += __shfl_xor(acc, off, 64);
  if ((tid & 63) == 0) s_part[tid >> 6] = acc;
  __syncthreads();
  const int base = s_part[0] + s_part[1] + s_part[2] + s_part[3];
  const int mine = n_sel[b];
  if (tid == 0) {
    per_image[b] = min(base + mine, cap) - min(base, cap);
    if (b == B - 1) n_rois[0] = min(base + mine, cap);
  }
  const float* d = dets + (size_t)b * max_det * 7;
  const float* K = cam + (size_t)b * cam_stride;
  for (int j = tid; j < max_det; j += 256) {
    const int pos = slot[(size_t)b * max_det + j];
    if (pos < 0 || base + pos >= cap) continue;
    const size_t r = (size_t)(base + pos);
    const float* p = d + j * 7;
    const double x1 = (double)(p[0] / ratio), y1 = (double)(p[1] / ratio), x2 = (double)(p[2] / ratio), y2 = (double)(p[3] / ratio);
    const double cx = 0.5 * (x1 + x2), cy = 0.5 * (y1 + y2);
    double bw = x2 - x1, bh = y2 - y1;
    bw = bw > 1.0 ? bw : 1.0;
    bh = bh > 1.0 ? bh : 1.0;
    const double side = (bh > bw ? bh : bw) * dzi_pad_scale, lim = (double)(H > W ? H : W);
    const double scale = side < lim ? side : lim;
    const int cls = (int)p[6];
    t.center64[2 * r] = cx;
    t.center64[2 * r + 1] = cy;
    t.scale64[r] = scale;
    t.im_idx[r] = b;
    t.roi_cls[r] = (long long)cls;
    for (int k = 0; k < 9; ++k) t.roi_cam[9 * r + k] = K[k];
    t.roi_center[2 * r] = (float)cx;
    t.roi_center[2 * r + 1] = (float)cy;
    t.roi_wh[2 * r] = (float)bw;
    t.roi_wh[2 * r + 1] = (float)bh;
    t.scale[r] = (float)scale;
    t.resize_ratio[r] = (float)(out_res / scale);
    for (int k = 0; k < 3; ++k) t.roi_extent[3 * r + k] = extents[3 * cls + k];
    t.score[r] = p[4] * p[5];
    t.roi_id[r] = (int)r;
  }
}

}  // namespace

extern "C" int gdrnpp_yolox_letterbox(const unsigned char* images_u8, int B, int H, int W, int rh, int rw, float* out, int Ht, int Wt,
                                      int focus, int ldy, int y_off, void* stream) {
  GDRNPP_REQUIRE(images_u8 && out, GDRNPP_EINVAL, "gdrnpp_yolox_letterbox: null pointer");
  GDRNPP_REQUIRE(B > 0 && B <= 65535 && H > 0 && W > 0, GDRNPP_EINVAL, "gdrnpp_yolox_letterbox: B=%d H=%d W=%d", B, H, W);
  GDRNPP_REQUIRE(Ht > 0 && Wt > 0 && Ht % 32 == 0 && Wt % 32 == 0, GDRNPP_EINVAL,
                 "gdrnpp_yolox_letterbox: target %d x %d must be positive multiples of 32", Ht, Wt);
  GDRNPP_REQUIRE(rh > 0 && rw > 0 && rh <= Ht && rw <= Wt, GDRNPP_EINVAL,
                 "gdrnpp_yolox_letterbox: resized image %d x %d does not fit the %d x %d target", rh, rw, Ht, Wt);
  GDRNPP_REQUIRE((long)H * W * 3 < (1l << 31), GDRNPP_ELIMIT, "gdrnpp_yolox_letterbox: image too large");
  if (focus) {
    GDRNPP_REQUIRE(y_off >= 0 && y_off + 12 <= ldy && y_off % 4 == 0 && ldy % 4 == 0, GDRNPP_EINVAL,
                   "gdrnpp_yolox_letterbox: Focus slice y_off=%d ldy=%d (12 channels inside ldy, both multiples of 4)", y_off, ldy);
    GDRNPP_REQUIRE(((uintptr_t)out & 15) == 0, GDRNPP_EINVAL, "gdrnpp_yolox_letterbox: the Focus buffer must be 16-byte aligned");
  } else {
    GDRNPP_REQUIRE(((uintptr_t)out & 7) == 0, GDRNPP_EINVAL, "gdrnpp_yolox_letterbox: the output must be 8-byte aligned");
  }
  const ResizeRequest q = dsize_request(W, H, rw, rh);
  const dim3 grid((Wt / 2 + 63) / 64, (Ht / 2 + 3) / 4, B), block(64, 4);
  hipStream_t st = (hipStream_t)stream;
  if (focus)
    hipLaunchKernelGGL(letterbox_kernel<true>, grid, block, 0, st, images_u8, H, W, rh, rw, (int)q.mode, q.scale_y, q.scale_x, out + y_off, Ht, Wt, ldy);
  else
    hipLaunchKernelGGL(letterbox_kernel<false>, grid, block, 0, st, images_u8, H, W, rh, rw, (int)q.mode, q.scale_y, q.scale_x, out, Ht, Wt, 0);
  return gdrnpp::check_launch("gdrnpp_yolox_letterbox");
}

extern "C" size_t gdrnpp_rois_from_dets_workspace_bytes(int B, int max_det) {
  if (B <= 0 || max_det <= 0) return 0;
  return ((size_t)B * max_det + (size_t)B) * sizeof(int);
}

extern "C" int gdrnpp_rois_from_dets(const float* dets, const int* count, int B, int max_det, int num_classes, float ratio, int H, int W,
                                     double dzi_pad_scale, int out_res, const float* cam, int cam_per_image, const float* extents,
                                     double score_thr, int top_k_per_obj, int cap, const gdrnpp_roi_table* table, int* n_rois,
                                     int* per_image, void* workspace, size_t workspace_bytes, void* stream) {
  GDRNPP_REQUIRE(dets && count && cam && extents && table && n_rois && per_image && workspace, GDRNPP_EINVAL,
                 "gdrnpp_rois_from_dets: null pointer");
  GDRNPP_REQUIRE(B > 0 && max_det > 0 && max_det <= kMaxDet && num_classes > 0 && cap > 0 && top_k_per_obj >= 0, GDRNPP_EINVAL,
                 "gdrnpp_rois_from_dets: B=%d max_det=%d (<= %d) num_classes=%d cap=%d top_k_per_obj=%d", B, max_det, kMaxDet,
                 num_classes, cap, top_k_per_obj);
  GDRNPP_REQUIRE(ratio > 0.f && H > 0 && W > 0 && out_res > 0, GDRNPP_EINVAL, "gdrnpp_rois_from_dets: ratio=%g H=%d W=%d out_res=%d",
                 (double)ratio, H, W, out_res);
  GDRNPP_REQUIRE((long)B * max_det < (1l << 30), GDRNPP_ELIMIT, "gdrnpp_rois_from_dets: problem too large");
  const gdrnpp_roi_table t = *table;
  GDRNPP_REQUIRE(t.center64 && t.scale64 && t.im_idx && t.roi_cls && t.roi_cam && t.roi_center && t.roi_wh && t.scale &&
                     t.resize_ratio && t.roi_extent && t.score && t.roi_id,
                 GDRNPP_EINVAL, "gdrnpp_rois_from_dets: null table column");
  GDRNPP_REQUIRE(workspace_bytes >= gdrnpp_rois_from_dets_workspace_bytes(B, max_det), GDRNPP_EINVAL,
                 "gdrnpp_rois_from_dets: workspace too small");
  int* slot = (int*)workspace;
  int* n_sel = slot + (size_t)B * max_det;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(roi_rank_kernel, dim3(B), dim3(256), 0, st, dets, count, max_det, num_classes, score_thr, top_k_per_obj, slot, n_sel);
  hipLaunchKernelGGL(roi_write_kernel, dim3(B), dim3(256), 0, st, dets, max_det, (const int*)slot, (const int*)n_sel, B, ratio, H, W,
                     dzi_pad_scale, (double)out_res, cam, cam_per_image ? 9 : 0, extents, cap, t, n_rois, per_image);
  return gdrnpp::check_launch("gdrnpp_rois_from_dets");
}
