// YOLOX training: SimOTA label assignment and the detection losses with their gradient (include/gdrnpp_hip.h, "YOLOX training").
// Restates get_in_boxes_info / get_assignments / dynamic_k_matching / get_losses of det/yolox/models/yolo_head.py for the whole batch
// without a host round trip.
//
// Assignment, a memset of matched_gt to -1 and three kernels:
//   prep_kernel     one thread per (image, anchor): decoded box, sum_c -log(1 - p_c), sigmoid(obj) and the candidate flag ("inside any
//                   gt box or any 2.5-stride centre square of this image") -> pre f32[B,A,8].  The workgroups of an image count its
//                   gts themselves (rows with sum > 0), so the flag needs no earlier launch.
//   match_kernel    one workgroup per (gt, image) walks the candidates.  Since dynamic_k <= 10, no G x A matrix exists: every lane keeps
//                   its 10 largest IoUs and its 10 lowest (cost, anchor) pairs sorted in LDS, and the workgroup merges the lane lists by
//                   at most 10 + 10 rounds of "best head of any lane".  A chosen anchor's matched_gt goes -1 -> gt -> -2 (chosen twice).
//   resolve_kernel  one thread per (image, anchor): -2 is replaced by the argmin of the cost over ALL gts of the image (the reference's
//                   torch.min over cost[:, multiply chosen]), recomputed with pair_terms(), the device function match_kernel used: the
//                   two passes see identical bits.  Writes matched_iou and counts num_fg (integer atomics: order-free).
// Selections are fp32 in the reference's operation order (-ffp-contract=off); ties go to the lowest index.
//
// Losses: per-anchor terms in fp64 from the fp32 inputs (decode included), per-workgroup partials added in a fixed tree, the partials
// added in workgroup order: equal bits on every run.  The backward recomputes from the same inputs.
#include "common.hpp"
#include "wave_ops.hpp"
#include <cfloat>
#include <climits>
#include <cmath>

namespace {

constexpr int kThreads = 256;
constexpr int kTopK = 10;          // n_candidate_k of dynamic_k_matching, and so the largest dynamic_k
constexpr int kPre = 8;            // floats per anchor of the pre-pass: cx, cy, w, h, negsum, sigmoid(obj), candidate, unused
constexpr int kMulti = -2;         // matched_gt between match_kernel and resolve_kernel: chosen by more than one gt

struct Gt {
  float cls, cx, cy, w, h;
};

__device__ __forceinline__ Gt load_gt(const float* __restrict__ labels, int G, int b, int g) {
  const float* r = labels + ((size_t)b * G + g) * 5;
  return Gt{r[0], r[1], r[2], r[3], r[4]};
}

// nlabel of get_losses: rows whose five values sum to more than 0.  Counted by a whole workgroup; every thread gets the count.
__device__ int count_gt(const float* __restrict__ labels, int G, int b, int* lds_count) {
  if (threadIdx.x == 0) *lds_count = 0;
  __syncthreads();
  for (int g = threadIdx.x; g < G; g += blockDim.x) {
    const Gt t = load_gt(labels, G, b, g);
    if ((((t.cls + t.cx) + t.cy) + t.w) + t.h > 0.f) atomicAdd(lds_count, 1);
  }
  __syncthreads();
  const int n = *lds_count;
  __syncthreads();
  return n;
}

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

// get_in_boxes_info for one (gt, anchor): bit 0 = centre of the anchor's cell inside the gt box, bit 1 = inside the 2.5-stride square.
__device__ __forceinline__ int in_flags(const Gt& t, float xs, float ys, float s) {
  const float xc = xs * s + 0.5f * s, yc = ys * s + 0.5f * s;
  const float bl = xc - (t.cx - 0.5f * t.w), br = (t.cx + 0.5f * t.w) - xc;
  const float bt = yc - (t.cy - 0.5f * t.h), bb = (t.cy + 0.5f * t.h) - yc;
  const float r = 2.5f * s;
  const float cl = xc - (t.cx - r), cr = (t.cx + r) - xc, ct = yc - (t.cy - r), cb = (t.cy + r) - yc;
  const int in_box = fminf(fminf(bl, bt), fminf(br, bb)) > 0.f;
  const int in_ctr = fminf(fminf(cl, ct), fminf(cr, cb)) > 0.f;
  return in_box | (in_ctr << 1);
}

// bboxes_iou(..., xyxy=False) of det/yolox/utils/boxes.py for one pair
__device__ __forceinline__ float pair_iou(const Gt& t, float px, float py, float pw, float ph) {
  const float tlx = fmaxf(t.cx - t.w / 2.f, px - pw / 2.f), tly = fmaxf(t.cy - t.h / 2.f, py - ph / 2.f);
  const float brx = fminf(t.cx + t.w / 2.f, px + pw / 2.f), bry = fminf(t.cy + t.h / 2.f, py + ph / 2.f);
  const float en = (tlx < brx ? 1.f : 0.f) * (tly < bry ? 1.f : 0.f);
  const float area_i = ((brx - tlx) * (bry - tly)) * en;
  return area_i / ((t.w * t.h + pw * ph) - area_i);
}

// IoU and SimOTA cost of (gt t, candidate anchor a of image b).  pre: the anchor's 8 floats; cls_logits: its C class logits.
// A class outside [0, C) (the reference's one_hot raises there) has no positive term.
__device__ __forceinline__ void pair_terms(const Gt& t, const float* __restrict__ pre, const float* __restrict__ cls_logits, int C, float xs,
                                           float ys, float s, float* iou_out, float* cost_out) {
  const float iou = pair_iou(t, pre[0], pre[1], pre[2], pre[3]);
  float cls_cost = pre[4];
  const int k = (int)t.cls;
  if (k >= 0 && k < C) {
    const float p = sqrtf(sigmoid_f(cls_logits[k]) * pre[5]);
    const float pos = -fmaxf(logf(p), -100.f), neg = -fmaxf(logf(1.f - p), -100.f);
    cls_cost = cls_cost + (pos - neg);
  }
  const float penalty = in_flags(t, xs, ys, s) == 3 ? 0.f : 1.f;
  *iou_out = iou;
  *cost_out = (cls_cost + 3.0f * (-logf(iou + 1e-8f))) + 100000.0f * penalty;
}

__global__ __launch_bounds__(kThreads) void prep_kernel(const float* __restrict__ raw, const float* __restrict__ anchors,
                                                        const float* __restrict__ labels, int A, int C, int G, float* __restrict__ pre,
                                                        int* __restrict__ num_gt, int* __restrict__ num_fg) {
  __shared__ int lds_count;
  const int b = blockIdx.y, a = blockIdx.x * kThreads + threadIdx.x;
  const int n_gt = count_gt(labels, G, b, &lds_count);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    num_gt[b] = n_gt;
    num_fg[b] = 0;
  }
  if (a >= A) return;
  const float* row = raw + ((size_t)b * A + a) * (5 + C);
  const float xs = anchors[3 * a], ys = anchors[3 * a + 1], s = anchors[3 * a + 2];
  float* o = pre + ((size_t)b * A + a) * kPre;
  o[0] = (row[0] + xs) * s;
  o[1] = (row[1] + ys) * s;
  o[2] = expf(row[2]) * s;
  o[3] = expf(row[3]) * s;
  const float sobj = sigmoid_f(row[4]);
  float negsum = 0.f;
  for (int c = 0; c < C; ++c) {
    const float p = sqrtf(sigmoid_f(row[5 + c]) * sobj);
    negsum += -fmaxf(logf(1.f - p), -100.f);
  }
  int cand = 0;
  for (int g = 0; g < n_gt; ++g) cand |= in_flags(load_gt(labels, G, b, g), xs, ys, s);
  o[4] = negsum;
  o[5] = sobj;
  o[6] = cand ? 1.f : 0.f;
  o[7] = 0.f;
}

// The best (value, key) of the workgroup, to every thread.  kMax: largest value, else smallest; ties: the smallest key.
template <bool kMax>
__device__ __forceinline__ bool better(float v, int k, float v2, int k2) {
  return (kMax ? v > v2 : v < v2) || (v == v2 && k < k2);
}

template <bool kMax>
__device__ void block_best(float& v, int& key, float* lds_v, int* lds_k) {
  for (int off = 32; off > 0; off >>= 1) {
    const float v2 = __shfl_xor(v, off, 64);
    const int k2 = __shfl_xor(key, off, 64);
    if (better<kMax>(v2, k2, v, key)) {
      v = v2;
      key = k2;
    }
  }
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    lds_v[wave] = v;
    lds_k[wave] = key;
  }
  __syncthreads();
  v = lds_v[0];
  key = lds_k[0];
  for (int w = 1; w < kThreads / 64; ++w)
    if (better<kMax>(lds_v[w], lds_k[w], v, key)) {
      v = lds_v[w];
      key = lds_k[w];
    }
  __syncthreads();
}

__global__ __launch_bounds__(kThreads) void match_kernel(const float* __restrict__ raw, const float* __restrict__ anchors,
                                                         const float* __restrict__ labels, const float* __restrict__ pre,
                                                         const int* __restrict__ num_gt, int A, int C, int G, int* __restrict__ matched_gt) {
  __shared__ float l_iou[kTopK][kThreads];
  __shared__ float l_cost[kTopK][kThreads];
  __shared__ int l_idx[kTopK][kThreads];
  __shared__ float red_v[kThreads / 64];
  __shared__ int red_k[kThreads / 64];
  const int g = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
  if (g >= num_gt[b]) return;       // uniform over the workgroup
  const Gt t = load_gt(labels, G, b, g);
  int n_iou = 0, n_cost = 0;
  for (int a = tid; a < A; a += kThreads) {
    const float* p = pre + ((size_t)b * A + a) * kPre;
    if (p[6] == 0.f) continue;
    float iou, cost;
    pair_terms(t, p, raw + ((size_t)b * A + a) * (5 + C) + 5, C, anchors[3 * a], anchors[3 * a + 1], anchors[3 * a + 2], &iou, &cost);
    if (n_iou < kTopK || iou > l_iou[kTopK - 1][tid]) {          // the lane's largest IoUs, descending
      int j = n_iou < kTopK ? n_iou : kTopK - 1;
      for (; j > 0 && l_iou[j - 1][tid] < iou; --j) l_iou[j][tid] = l_iou[j - 1][tid];
      l_iou[j][tid] = iou;
      if (n_iou < kTopK) ++n_iou;
    }
    if (n_cost < kTopK || cost < l_cost[kTopK - 1][tid]) {       // the lane's lowest costs, ascending; equal costs keep anchor order
      int j = n_cost < kTopK ? n_cost : kTopK - 1;
      for (; j > 0 && l_cost[j - 1][tid] > cost; --j) {
        l_cost[j][tid] = l_cost[j - 1][tid];
        l_idx[j][tid] = l_idx[j - 1][tid];
      }
      l_cost[j][tid] = cost;
      l_idx[j][tid] = a;
      if (n_cost < kTopK) ++n_cost;
    }
  }
  // sum of the top-min(10, n_cand) IoUs, largest first
  float sum = 0.f;
  int head = 0;
  for (int r = 0; r < kTopK; ++r) {
    float v = head < n_iou ? l_iou[head][tid] : -FLT_MAX;
    int key = tid;
    if (!(v == v)) v = -FLT_MAX;
    block_best<true>(v, key, red_v, red_k);
    if (v == -FLT_MAX) break;        // uniform: the broadcast result
    sum += v;
    if (key == tid) ++head;
  }
  int dynamic_k = sum >= 1.f ? (int)fminf(sum, (float)kTopK) : 1;
  head = 0;
  for (int r = 0; r < dynamic_k; ++r) {
    float v = head < n_cost ? l_cost[head][tid] : FLT_MAX;
    int key = head < n_cost ? l_idx[head][tid] : INT_MAX;
    if (!(v == v)) {
      v = FLT_MAX;
      key = INT_MAX;
    }
    block_best<false>(v, key, red_v, red_k);
    if (key == INT_MAX) break;       // no candidate left: this gt gets no further anchor
    if ((key & (kThreads - 1)) == tid) {
      ++head;
      int* m = matched_gt + (size_t)b * A + key;
      if (atomicCAS(m, -1, g) != -1) atomicExch(m, kMulti);
    }
  }
}

__global__ __launch_bounds__(kThreads) void resolve_kernel(const float* __restrict__ raw, const float* __restrict__ anchors,
                                                           const float* __restrict__ labels, const float* __restrict__ pre,
                                                           const int* __restrict__ num_gt, int A, int C, int G, int* __restrict__ matched_gt,
                                                           float* __restrict__ matched_iou, int* __restrict__ num_fg) {
  const int b = blockIdx.y, a = blockIdx.x * kThreads + threadIdx.x;
  int fg = 0;
  if (a < A) {
    const size_t i = (size_t)b * A + a;
    int m = matched_gt[i];
    float iou = 0.f;
    if (m != -1) {
      const float* p = pre + i * kPre;
      const float* cls = raw + i * (5 + C) + 5;
      const float xs = anchors[3 * a], ys = anchors[3 * a + 1], s = anchors[3 * a + 2];
      float cost;
      if (m == kMulti) {
        const int n_gt = num_gt[b];
        float best = 0.f;
        m = -1;
        for (int g = 0; g < n_gt; ++g) {
          float iou_g, cost_g;
          pair_terms(load_gt(labels, G, b, g), p, cls, C, xs, ys, s, &iou_g, &cost_g);
          if (m < 0 || cost_g < best) {
            best = cost_g;
            m = g;
            iou = iou_g;
          }
        }
        matched_gt[i] = m;
      } else {
        pair_terms(load_gt(labels, G, b, m), p, cls, C, xs, ys, s, &iou, &cost);
      }
      fg = m >= 0;
    }
    matched_iou[i] = iou;
  }
  const int n = __syncthreads_count(fg);
  if (threadIdx.x == 0 && n) atomicAdd(num_fg + b, n);
}

// ---- losses -----------------------------------------------------------------------------------------------------------------------

struct LossArgs {
  const float* raw;
  const float* anchors;
  const float* labels;
  const int* matched_gt;
  int n, A, C, G;
  int iou_type, cls_type, use_l1;
  double alpha, gamma;
};

__device__ __forceinline__ double bce_logits(double x, double z) { return fmax(x, 0.0) - x * z + log1p(exp(-fabs(x))); }
__device__ __forceinline__ double sigmoid_d(double x) { return 1.0 / (1.0 + exp(-x)); }
__device__ __forceinline__ double sel_gt(double a, double b) { return a > b ? 1.0 : (a == b ? 0.5 : 0.0); }   // d max(a, b) / d a

// IOUloss (det/yolox/models/losses.py) of the decoded box p against the target t: the loss and its gradient by (px, py, pw, ph).
template <bool kGrad>
__device__ double iou_loss(const double* p, const double* t, int giou, double* d) {
  double tl[2], br[2], dtl[2], dbr[2];      // dtl: d tl / d (p - w/2), dbr: d br / d (p + w/2)
  for (int k = 0; k < 2; ++k) {
    const double pl = p[k] - p[2 + k] / 2, pr = p[k] + p[2 + k] / 2, gl = t[k] - t[2 + k] / 2, gr = t[k] + t[2 + k] / 2;
    tl[k] = fmax(pl, gl);
    br[k] = fmin(pr, gr);
    dtl[k] = sel_gt(pl, gl);
    dbr[k] = sel_gt(gr, pr);
  }
  const double area_p = p[2] * p[3], area_g = t[2] * t[3];
  const double en = (tl[0] < br[0] ? 1.0 : 0.0) * (tl[1] < br[1] ? 1.0 : 0.0);
  const double wi = br[0] - tl[0], hi = br[1] - tl[1];
  const double area_i = wi * hi * en, area_u = area_p + area_g - area_i, den = area_u + 1e-16;
  const double iou = area_i / den;
  // gradients of area_i, area_u by (px, py, pw, ph)
  double dai[4], dau[4], diou[4];
  if (kGrad) {
    dai[0] = (dbr[0] - dtl[0]) * hi * en;
    dai[1] = (dbr[1] - dtl[1]) * wi * en;
    dai[2] = 0.5 * (dbr[0] + dtl[0]) * hi * en;
    dai[3] = 0.5 * (dbr[1] + dtl[1]) * wi * en;
    const double dap[4] = {0.0, 0.0, p[3], p[2]};
    for (int k = 0; k < 4; ++k) {
      dau[k] = dap[k] - dai[k];
      diou[k] = (dai[k] * den - area_i * dau[k]) / (den * den);
    }
  }
  if (!giou) {
    if (kGrad)
      for (int k = 0; k < 4; ++k) d[k] = -2.0 * iou * diou[k];
    return 1.0 - iou * iou;
  }
  double ctl[2], cbr[2], dctl[2], dcbr[2];
  for (int k = 0; k < 2; ++k) {
    const double pl = p[k] - p[2 + k] / 2, pr = p[k] + p[2 + k] / 2, gl = t[k] - t[2 + k] / 2, gr = t[k] + t[2 + k] / 2;
    ctl[k] = fmin(pl, gl);
    cbr[k] = fmax(pr, gr);
    dctl[k] = sel_gt(gl, pl);
    dcbr[k] = sel_gt(pr, gr);
  }
  const double wc = cbr[0] - ctl[0], hc = cbr[1] - ctl[1], area_c = wc * hc, acc = fmax(area_c, 1e-16);
  const double g = iou - (area_c - area_u) / acc;
  if (kGrad) {
    const double dac[4] = {(dcbr[0] - dctl[0]) * hc, (dcbr[1] - dctl[1]) * wc, 0.5 * (dcbr[0] + dctl[0]) * hc, 0.5 * (dcbr[1] + dctl[1]) * wc};
    const double pass = (g >= -1.0 && g <= 1.0) ? 1.0 : 0.0, cpass = area_c >= 1e-16 ? 1.0 : 0.0;
    for (int k = 0; k < 4; ++k) {
      const double dg = diou[k] - ((dac[k] - dau[k]) * acc - (area_c - area_u) * dac[k] * cpass) / (acc * acc);
      d[k] = -dg * pass;
    }
  }
  return 1.0 - fmin(fmax(g, -1.0), 1.0);
}

// The terms of anchor i.  term[4] = IOUloss, objectness BCE, L1, class loss (unscaled).  kGrad: grad[5 + C] = the gradient of
// w[0] * 5 IOUloss + w[1] obj + w[2] l1 + w[3] cls by the raw row.
template <bool kGrad>
__device__ void anchor_terms(const LossArgs& a, int i, double* term, const double* w, float* grad) {
  const int S = 5 + a.C, an = i % a.A, b = i / a.A;
  const float* row = a.raw + (size_t)i * S;
  const int m = a.matched_gt[i];
  const bool fg = m >= 0 && m < a.G;
  const double xo = row[4];
  term[1] = bce_logits(xo, fg ? 1.0 : 0.0);
  term[0] = term[2] = term[3] = 0.0;
  if (kGrad) {
    for (int k = 0; k < S; ++k) grad[k] = 0.f;
    grad[4] = (float)((sigmoid_d(xo) - (fg ? 1.0 : 0.0)) * w[1]);
  }
  if (!fg) return;
  const float* lab = a.labels + ((size_t)b * a.G + m) * 5;
  const double xs = a.anchors[3 * an], ys = a.anchors[3 * an + 1], s = a.anchors[3 * an + 2];
  const double t[4] = {lab[1], lab[2], lab[3], lab[4]};
  const double p[4] = {(row[0] + xs) * s, (row[1] + ys) * s, exp((double)row[2]) * s, exp((double)row[3]) * s};
  double d[4] = {0.0, 0.0, 0.0, 0.0};
  term[0] = iou_loss<kGrad>(p, t, a.iou_type, d);
  double greg[4];
  if (kGrad) {
    greg[0] = 5.0 * w[0] * d[0] * s;
    greg[1] = 5.0 * w[0] * d[1] * s;
    greg[2] = 5.0 * w[0] * d[2] * p[2];
    greg[3] = 5.0 * w[0] * d[3] * p[3];
  }
  if (a.use_l1) {
    const double l1t[4] = {t[0] / s - xs, t[1] / s - ys, log(t[2] / s + 1e-8), log(t[3] / s + 1e-8)};
    for (int k = 0; k < 4; ++k) {
      const double e = (double)row[k] - l1t[k];
      term[2] += fabs(e);
      if (kGrad) greg[k] += w[2] * (e > 0.0 ? 1.0 : (e < 0.0 ? -1.0 : 0.0));
    }
  }
  if (kGrad)
    for (int k = 0; k < 4; ++k) grad[k] = (float)greg[k];
  // the class target: onehot * IoU of the match (bboxes_iou's form, no epsilon), a constant of the gradient
  double tiou;
  {
    const double tlx = fmax(t[0] - t[2] / 2, p[0] - p[2] / 2), tly = fmax(t[1] - t[3] / 2, p[1] - p[3] / 2);
    const double brx = fmin(t[0] + t[2] / 2, p[0] + p[2] / 2), bry = fmin(t[1] + t[3] / 2, p[1] + p[3] / 2);
    const double en = (tlx < brx ? 1.0 : 0.0) * (tly < bry ? 1.0 : 0.0);
    const double ai = (brx - tlx) * (bry - tly) * en;
    tiou = ai / (t[2] * t[3] + p[2] * p[3] - ai);
  }
  const int cls = (int)lab[0];
  for (int c = 0; c < a.C; ++c) {
    const double x = row[5 + c], z = c == cls ? tiou : 0.0;
    if (a.cls_type == 0) {
      term[3] += bce_logits(x, z);
      if (kGrad) grad[5 + c] = (float)((sigmoid_d(x) - z) * w[3]);
    } else {     // fvcore sigmoid_focal_loss
      const double pr = sigmoid_d(x), ce = bce_logits(x, z), pt = pr * z + (1.0 - pr) * (1.0 - z), om = 1.0 - pt;
      const double at = a.alpha >= 0.0 ? a.alpha * z + (1.0 - a.alpha) * (1.0 - z) : 1.0;
      const double mod = pow(om, a.gamma);
      term[3] += at * ce * mod;
      if (kGrad) {
        const double dmod = a.gamma == 0.0 ? 0.0 : a.gamma * pow(om, a.gamma - 1.0) * (-(pr * (1.0 - pr) * (2.0 * z - 1.0)));
        grad[5 + c] = (float)(at * ((pr - z) * mod + ce * dmod) * w[3]);
      }
    }
  }
}

// Sum of v over the workgroup in a fixed tree; the result in thread 0.
__device__ double block_sum(double v, double* lds) {
  const double r = gdrnpp::wave::block_sum_halving<kThreads>(v, lds);
  __syncthreads();   // the next call writes the slots again
  return r;
}

__global__ __launch_bounds__(kThreads) void loss_kernel(const LossArgs a, double* __restrict__ part) {
  __shared__ double lds[kThreads];
  const int i = blockIdx.x * kThreads + threadIdx.x;
  double term[4] = {0.0, 0.0, 0.0, 0.0};
  if (i < a.n) anchor_terms<false>(a, i, term, nullptr, nullptr);
  for (int k = 0; k < 4; ++k) {
    const double r = block_sum(term[k], lds);
    if (threadIdx.x == 0) part[4 * (size_t)blockIdx.x + k] = r;
  }
}

// out f64[6] = loss_iou (5 x), loss_conf, loss_l1, loss_cls, max(sum num_fg, 1), sum num_gt
__global__ __launch_bounds__(kThreads) void finish_kernel(const double* __restrict__ part, int n_part, const int* __restrict__ num_fg,
                                                          const int* __restrict__ num_gt, int B, double* __restrict__ out) {
  __shared__ double lds[kThreads];
  double total[4];
  for (int k = 0; k < 4; ++k) {
    double v = 0.0;
    for (int j = threadIdx.x; j < n_part; j += kThreads) v += part[4 * (size_t)j + k];
    total[k] = block_sum(v, lds);
  }
  if (threadIdx.x == 0) {
    long long nf = 0, ng = 0;
    for (int b = 0; b < B; ++b) {
      nf += num_fg[b];
      ng += num_gt[b];
    }
    const double den = nf > 1 ? (double)nf : 1.0;
    out[0] = 5.0 * total[0] / den;
    out[1] = total[1] / den;
    out[2] = total[2] / den;
    out[3] = total[3] / den;
    out[4] = den;
    out[5] = (double)ng;
  }
}

__global__ __launch_bounds__(kThreads) void loss_backward_kernel(const LossArgs a, const double* __restrict__ out,
                                                                 const float* __restrict__ scale, float* __restrict__ grad_raw) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n) return;
  const double den = out[4];
  const double w[4] = {scale[0] / den, scale[1] / den, scale[2] / den, scale[3] / den};
  double term[4];
  anchor_terms<true>(a, i, term, w, grad_raw + (size_t)i * (5 + a.C));
}

int common_checks(const char* fn, const void* raw, const void* anchors, const void* labels, int B, int A, int C, int G) {
  GDRNPP_REQUIRE(raw && anchors && labels, GDRNPP_EINVAL, "%s: raw / anchors / labels is null", fn);
  GDRNPP_REQUIRE(B > 0 && A > 0 && C > 0 && G >= 0, GDRNPP_EINVAL, "%s: B = %d, A = %d, C = %d, G = %d", fn, B, A, C, G);
  GDRNPP_REQUIRE(B <= 65535 && G <= 65535 && (long long)B * A * ((long long)C + kPre) <= 0x7fffffffLL, GDRNPP_ELIMIT,
                 "%s: B = %d, A = %d, C = %d, G = %d: above one launch (B, G <= 65535, B A (C + 8) < 2^31)", fn, B, A, C, G);
  return 0;
}

LossArgs loss_args(const float* raw, const float* anchors, const float* labels, const int* matched_gt, int B, int A, int C, int G,
                   int iou_type, int cls_type, float fl_alpha, float fl_gamma, int use_l1) {
  LossArgs a{};
  a.raw = raw; a.anchors = anchors; a.labels = labels; a.matched_gt = matched_gt;
  a.n = B * A; a.A = A; a.C = C; a.G = G;
  a.iou_type = iou_type; a.cls_type = cls_type; a.use_l1 = use_l1;
  a.alpha = fl_alpha; a.gamma = fl_gamma;
  return a;
}

}  // namespace

extern "C" {

size_t gdrnpp_yolox_assign_workspace_bytes(int B, int A) {
  if (B <= 0 || A <= 0 || (long long)B * A * kPre > 0x7fffffffLL) return 0;
  return sizeof(float) * kPre * (size_t)B * A;
}

int gdrnpp_yolox_assign(const float* raw, const float* anchors, const float* labels, int B, int A, int C, int G, int* matched_gt,
                        float* matched_iou, int* num_fg, int* num_gt, void* workspace, size_t workspace_bytes, void* stream) {
  const char* const fn = "gdrnpp_yolox_assign";
  if (int rc = common_checks(fn, raw, anchors, labels, B, A, C, G)) return rc;
  GDRNPP_REQUIRE(matched_gt && matched_iou && num_fg && num_gt, GDRNPP_EINVAL, "%s: an output is null", fn);
  const size_t need = gdrnpp_yolox_assign_workspace_bytes(B, A);
  GDRNPP_REQUIRE(workspace && workspace_bytes >= need, GDRNPP_EINVAL, "%s: workspace %zu < %zu bytes", fn, workspace ? workspace_bytes : (size_t)0,
                 need);
  hipStream_t st = (hipStream_t)stream;
  float* pre = (float*)workspace;
  const dim3 per_anchor((unsigned)((A + kThreads - 1) / kThreads), (unsigned)B);
  GDRNPP_HIP_TRY(hipMemsetAsync(matched_gt, 0xff, sizeof(int) * (size_t)B * A, st));       // -1: background
  hipLaunchKernelGGL(prep_kernel, per_anchor, dim3(kThreads), 0, st, raw, anchors, labels, A, C, G, pre, num_gt, num_fg);
  if (G > 0)
    hipLaunchKernelGGL(match_kernel, dim3((unsigned)G, (unsigned)B), dim3(kThreads), 0, st, raw, anchors, labels, (const float*)pre,
                       (const int*)num_gt, A, C, G, matched_gt);
  hipLaunchKernelGGL(resolve_kernel, per_anchor, dim3(kThreads), 0, st, raw, anchors, labels, (const float*)pre, (const int*)num_gt, A, C, G,
                     matched_gt, matched_iou, num_fg);
  return gdrnpp::check_launch(fn);
}

size_t gdrnpp_yolox_losses_workspace_bytes(int B, int A) {
  if (B <= 0 || A <= 0 || (long long)B * A > 0x7fffffffLL) return 0;
  return sizeof(double) * 4 * (size_t)(((long long)B * A + kThreads - 1) / kThreads);
}

int gdrnpp_yolox_losses(const float* raw, const float* anchors, const float* labels, const int* matched_gt, const int* num_fg,
                        const int* num_gt, int B, int A, int C, int G, int iou_type, int cls_type, float fl_alpha, float fl_gamma, int use_l1,
                        double* out, void* workspace, size_t workspace_bytes, void* stream) {
  const char* const fn = "gdrnpp_yolox_losses";
  if (int rc = common_checks(fn, raw, anchors, labels, B, A, C, G)) return rc;
  GDRNPP_REQUIRE(matched_gt && num_fg && num_gt && out, GDRNPP_EINVAL, "%s: matched_gt / num_fg / num_gt / out is null", fn);
  GDRNPP_REQUIRE((iou_type == 0 || iou_type == 1) && (cls_type == 0 || cls_type == 1), GDRNPP_EINVAL,
                 "%s: iou_type %d (0 iou, 1 giou), cls_type %d (0 bce, 1 focal)", fn, iou_type, cls_type);
  const size_t need = gdrnpp_yolox_losses_workspace_bytes(B, A);
  GDRNPP_REQUIRE(workspace && workspace_bytes >= need, GDRNPP_EINVAL, "%s: workspace %zu < %zu bytes", fn, workspace ? workspace_bytes : (size_t)0,
                 need);
  const LossArgs a = loss_args(raw, anchors, labels, matched_gt, B, A, C, G, iou_type, cls_type, fl_alpha, fl_gamma, use_l1);
  const int n_part = (a.n + kThreads - 1) / kThreads;
  double* part = (double*)workspace;
  hipLaunchKernelGGL(loss_kernel, dim3((unsigned)n_part), dim3(kThreads), 0, (hipStream_t)stream, a, part);
  hipLaunchKernelGGL(finish_kernel, dim3(1), dim3(kThreads), 0, (hipStream_t)stream, (const double*)part, n_part, num_fg, num_gt, B, out);
  return gdrnpp::check_launch(fn);
}

int gdrnpp_yolox_losses_backward(const float* raw, const float* anchors, const float* labels, const int* matched_gt, const double* out,
                                 const float* scale, int B, int A, int C, int G, int iou_type, int cls_type, float fl_alpha, float fl_gamma,
                                 int use_l1, float* grad_raw, void* stream) {
  const char* const fn = "gdrnpp_yolox_losses_backward";
  if (int rc = common_checks(fn, raw, anchors, labels, B, A, C, G)) return rc;
  GDRNPP_REQUIRE(matched_gt && out && scale && grad_raw, GDRNPP_EINVAL, "%s: matched_gt / out / scale / grad_raw is null", fn);
  GDRNPP_REQUIRE((iou_type == 0 || iou_type == 1) && (cls_type == 0 || cls_type == 1), GDRNPP_EINVAL,
                 "%s: iou_type %d (0 iou, 1 giou), cls_type %d (0 bce, 1 focal)", fn, iou_type, cls_type);
  const LossArgs a = loss_args(raw, anchors, labels, matched_gt, B, A, C, G, iou_type, cls_type, fl_alpha, fl_gamma, use_l1);
  hipLaunchKernelGGL(loss_backward_kernel, dim3((unsigned)((a.n + kThreads - 1) / kThreads)), dim3(kThreads), 0, (hipStream_t)stream, a, out,
                     scale, grad_raw);
  return gdrnpp::check_launch(fn);
}

}  // extern "C"
