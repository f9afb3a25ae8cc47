// BOP ground-truth info and masks of a batch of ground-truth poses on gfx950: what the toolkit's calc_gt_info.py and calc_gt_masks.py
// compute per pose with one GL render and half a dozen full-image NumPy passes (px_count_all / valid / visib, the boxes behind bbox_obj
// and bbox_visib, and the mask / mask_visib images), as the one-pose case of vsd_error.hip's tiled render-and-compare.
//
// Behavioural spec: lib/pysixd/scripts/calc_gt_info.py:98-173, calc_gt_masks.py:83-111, lib/pysixd/visibility.py:9-54 (visib_mode
// "bop19"), lib/pysixd/misc.py:628-647 (depth_im_to_dist_im_fast) and the render rule raster.hpp states: pixel (row j, col i) sampled at
// (i+0.5, j+0.5), both faces, depth = camera-space Z rounded to float32, background 0.  The toolkit hands the renderer fx, fy, cx, cy only.
// Canvas: calc_gt_info.py renders on a 3W x 3H canvas with the principal point moved to (cx + W, cy + H) and crops the central W x H
// window; calc_gt_masks.py renders on the plain image.  Here one offset (ox, oy): the render uses K' = [fx 0 cx+ox; 0 fy cy+oy; 0 0 1]
// over (W + 2 ox) x (H + 2 oy) canvas pixels, with the canvas's own pixel indices in the raster expressions (not an algebraically equal
// shifted form: the coverage decisions are the reference's), and the window is the canvas region [ox, ox+W) x [oy, oy+H).
// Per window pixel (x, y) in image coordinates, Z_g the render there, D the scene depth (float32 mm, 0 = missing), pX = (x - cx) / fx,
// pY = (y - cy) / fy at the INTEGER pixel with the image's own cx, cy (the toolkit's half-pixel inconsistency, as in VSD):
//   dist(Z) = sqrt(((pX Z)^2 + (pY Z)^2) + Z^2)                                          fp64, NumPy's order, no contraction
//   mask    = dist_g > 0
//   visib   = ((f32(dist_g) - f32(dist_t) <= delta) || dist_t == 0) && dist_g > 0        the subtraction in float32
//   valid   = mask && dist_t > 0
// Output per pose, i32[11]: px_count_all = #(canvas pixels with Z_g > 0), px_count_valid = #valid, px_count_visib = #visib (window),
// the inclusive extents x_min, y_min, x_max, y_max of the canvas silhouette in image coordinates (canvas index minus offset: they can
// be negative or reach beyond the image), and the same of visib.  Empty extents are INT_MAX, INT_MAX, INT_MIN, INT_MIN (x_min > x_max).
// Optionally the window's mask and visib as bytes 0 / 255, u8[n,H,W] each.  The host forms visib_fract and the boxes.
//
// Two kernels on one stream, the buffers of the masks cleared on that stream before them:
//   gt_project    one workgroup per pose.  Stages per vertex h = K' (R v + t), u = h0 / h2, v = h1 / h2 in the workspace, reduces the
//                 pose's conservative pixel box in canvas coordinates (the whole canvas once a vertex is nearer than z_near) and
//                 initialises the pose's row: zeros and empty extents, or eleven times -1 for a pose the device refuses (obj outside
//                 [0, n_obj), im_idx outside [0, n_im), an object without faces or vertices or above max_verts).
//   gt_tiles      the grid is (pose, tile) over ALL 64x64 tiles of the canvas, so no host read-back sizes it; a workgroup whose tile
//                 misses the box leaves on a workgroup-uniform branch.  A surviving workgroup (256 threads) keeps one z-buffer of
//                 float-Z bits in LDS (16 KiB), walks the object's faces once (tile_raster.hpp: the face walk of vsd_tiles, with its
//                 early box rejection and its whole-wave path for faces above 32 candidate centres) and then every pixel of tile & box
//                 evaluates the recipe.  The three counters are summed and the eight extents reduced in registers, across a wave by
//                 shuffles, across waves by LDS atomics; each non-zero counter costs one global integer atomic add per workgroup and
//                 each extent of a workgroup that saw a pixel one global integer atomic min / max.  A mask byte is a plain store by the
//                 one thread that owns the pixel.
// The staging, the box reduction and the face walk are vsd_error.hip's, shared through tile_raster.hpp (moved, not changed: VSD's
// generated code keeps its floating-point instructions and its 101 / 42 VGPRs, and computes the same bits).
// Deterministic: coverage and depth are fixed fp64 expressions, the z-buffer an integer minimum; everything written is an integer sum,
// a minimum, a maximum or a byte owned by one thread: two runs are bit-equal.  sqrt and division are the IEEE correctly rounded ones.
// Roofline.  Per covered pixel of the window: 1 division (pY; pX is a per-thread constant), 2 distances of 5 mul + 2 add + 1 sqrt, 1
// float subtraction: ~65 fp64 VALU operations with the division and roots expanded (division ~13, sqrt ~17), 4 B of the scene depth
// read, 0 - 2 B of masks written; a covered pixel of the canvas outside the window costs its z-buffer read and integer work only.  Per
// (face, surviving tile): 12 B of indices + 3 x 24 B (z, u, v) for the box test, and for a face that reaches the tile 3 x 24 B more and
// ~60 operations; per candidate centre 18 operations, 3 compares, 1 division.  Per vertex: 31 operations and 2 divisions, 12 B read, 40 B
// written.  Algorithmic HBM bytes per pose: 40 V staged once and re-read per surviving tile from L2, 12 F + 12 V of the model
// (L2-resident across the poses of an object), 4 B per covered window pixel of the depth image, 44 B out, and with masks 2 H W bytes
// cleared plus the covered bytes.  By these counts the face walk (L2 gathers of 84 - 156 B per face per tile against ~60 operations)
// bounds a 5 k-face model without masks, and the clearing of 2 H W mask bytes per pose (614 KB at 640 x 480, against ~10^4 covered
// pixels) bounds the call with masks: HBM writes.  The measured fractions are in DESIGN.md (tools/gt_info_bench.py).
#include "common.hpp"
#include "tile_raster.hpp"
#include "wave_ops.hpp"
#include <climits>

namespace {

using namespace gdrnpp;
using namespace gdrnpp::tiles;
using wave::wave_max, wave::wave_min, wave::wave_sum;

constexpr int kInfo = 11;  // all, valid, visib, obj x0 y0 x1 y1, visib x0 y0 x1 y1

struct GtArgs {
  const float* verts; const int* faces; const int* vert_off; const int* face_off; int n_obj, max_verts;
  const int* obj; const int* im_idx;
  const double *R, *t, *K;
  const float* depth; int n_im, H, W, ox, oy, Wc, Hc;
  float delta;
  double z_near, z_far;
  int* info;
  unsigned char* mask;        // [n][H][W] or null
  unsigned char* mask_visib;  // [n][H][W] or null
  double* hv;                 // [n][max_verts][kVtx]
  int* box;                   // [n][4] = i_lo, i_hi, j_lo, j_hi on the canvas (inclusive; empty when lo > hi)
};

// what only the device can see: such a pose's row is -1 and nothing of it is staged, rendered or read
__device__ __forceinline__ bool pose_ok(const GtArgs& a, size_t pose, int& o) {
  o = a.obj[pose];
  if (o < 0 || o >= a.n_obj) return false;
  const int im = a.im_idx[pose];
  if (im < 0 || im >= a.n_im) return false;
  const int nv = a.vert_off[o + 1] - a.vert_off[o], nf = a.face_off[o + 1] - a.face_off[o];
  return nv > 0 && nv <= a.max_verts && nf > 0;
}

__global__ __launch_bounds__(kThreads) void gt_project(const GtArgs a) {
  __shared__ double s_red[kWaves][6];
  const size_t pose = blockIdx.x;
  const int tid = threadIdx.x;
  int o;
  const bool ok = pose_ok(a, pose, o);
  if (tid < kInfo) a.info[pose * kInfo + tid] = !ok ? -1 : tid < 3 ? 0 : ((tid - 3) & 2) ? INT_MIN : INT_MAX;
  int* box = a.box + 4 * pose;
  if (!ok) {
    if (tid == 0) { box[0] = 1; box[1] = 0; box[2] = 1; box[3] = 0; }
    return;
  }
  const int v0 = a.vert_off[o], nv = a.vert_off[o + 1] - v0;
  double K[9], R[9], t[3];
  render_K(a.K + 9 * pose, K);
  K[2] = K[2] + (double)a.ox;  // the canvas's principal point, formed as the reference forms it: cx + offset in fp64
  K[5] = K[5] + (double)a.oy;
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = a.R[9 * pose + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = a.t[3 * pose + k];
  stage_vertices_and_box(a.verts + 3 * (size_t)v0, nv, K, R, t, a.hv + (pose * (size_t)a.max_verts) * kVtx, a.z_near, a.z_far, a.Wc, a.Hc,
                         s_red, box);
}

__global__ __launch_bounds__(kThreads) void gt_tiles(const GtArgs a, int tiles_x, int ntiles) {
  __shared__ unsigned zb[kTilePix];
  __shared__ int s_cnt[3];
  __shared__ int s_ext[8];

  const size_t pose = blockIdx.x / (unsigned)ntiles;
  const int tile = (int)(blockIdx.x - pose * (unsigned)ntiles);
  int o;
  if (!pose_ok(a, pose, o)) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int Wc = a.Wc, Hc = a.Hc;
  const int tx0 = (tile % tiles_x) * kTile, ty0 = (tile / tiles_x) * kTile;
  const int tx1 = min(tx0 + kTile, Wc) - 1, ty1 = min(ty0 + kTile, Hc) - 1;
  // this tile & the pose's box; a tile that misses it leaves (workgroup-uniform)
  const int* bx = a.box + 4 * pose;
  const int ci0 = max(bx[0], tx0), ci1 = min(bx[1], tx1), cj0 = max(bx[2], ty0), cj1 = min(bx[3], ty1);
  if (ci0 > ci1 || cj0 > cj1) return;

  for (int p = tid; p < kTilePix; p += kThreads) zb[p] = kInfBits;
  if (tid < 3) s_cnt[tid] = 0;
  if (tid < 8) s_ext[tid] = (tid & 2) ? INT_MIN : INT_MAX;
  __syncthreads();

  const int nv = a.vert_off[o + 1] - a.vert_off[o];
  const int* mfaces = a.faces + 3 * (size_t)a.face_off[o];
  const int nfaces = a.face_off[o + 1] - a.face_off[o];
  raster_faces_tile(a.hv + (pose * (size_t)a.max_verts) * kVtx, mfaces, nfaces, nv, ci0, ci1, cj0, cj1, tx0, ty0, Wc, Hc, a.z_near, a.z_far,
                    zb);
  __syncthreads();

  // ---- the recipe: the pixels of tile & box; (x, y) are image coordinates, inside the window where 0 <= x < W and 0 <= y < H ---------
  const int W = a.W, H = a.H;
  const double* Kp = a.K + 9 * pose;
  const double fx = Kp[0], cx = Kp[2], fy = Kp[4], cy = Kp[5];
  const float delta = a.delta;
  const size_t plane = (size_t)H * W;
  const float* dt = a.depth + (size_t)a.im_idx[pose] * plane;
  unsigned char* mk = a.mask ? a.mask + pose * plane : nullptr;
  unsigned char* mv = a.mask_visib ? a.mask_visib + pose * plane : nullptr;
  int n_all = 0, n_valid = 0, n_visib = 0;
  int ox0 = INT_MAX, oy0 = INT_MAX, ox1 = INT_MIN, oy1 = INT_MIN, vx0 = INT_MAX, vy0 = INT_MAX, vx1 = INT_MIN, vy1 = INT_MIN;
  const int xc = tx0 + lane;  // the thread's canvas column in every row it visits
  if (xc >= ci0 && xc <= ci1) {
    const int x = xc - a.ox;
    const bool in_x = x >= 0 && x < W;
    const double pX = ((double)x - cx) / fx;
    for (int ly = tid >> 6; ly < kTile; ly += kWaves) {
      const int yc = ty0 + ly;
      if (yc < cj0 || yc > cj1) continue;
      const unsigned bg = zb[ly * kTile + lane];
      if (bg == kInfBits) continue;  // background: Z_g = 0, in no count and no mask
      const double Zg = (double)__uint_as_float(bg);
      if (!(Zg > 0.0)) continue;
      const int y = yc - a.oy;
      ++n_all;
      ox0 = min(ox0, x); ox1 = max(ox1, x); oy0 = min(oy0, y); oy1 = max(oy1, y);
      if (!in_x || y < 0 || y >= H) continue;
      const size_t at = (size_t)y * W + x;
      const double Zt = (double)dt[at];
      const double pY = ((double)y - cy) / fy;
      double ax = pX * Zg, ay = pY * Zg;
      const double dist_g = sqrt((ax * ax + ay * ay) + Zg * Zg);
      ax = pX * Zt; ay = pY * Zt;
      const double dist_t = sqrt((ax * ax + ay * ay) + Zt * Zt);
      const bool in_mask = dist_g > 0.0;
      const bool visib = (((float)dist_g - (float)dist_t <= delta) || dist_t == 0.0) && in_mask;
      n_valid += (in_mask && dist_t > 0.0) ? 1 : 0;
      if (in_mask && mk) mk[at] = 255;
      if (visib) {
        ++n_visib;
        vx0 = min(vx0, x); vx1 = max(vx1, x); vy0 = min(vy0, y); vy1 = max(vy1, y);
        if (mv) mv[at] = 255;
      }
    }
  }
  n_all = wave_sum(n_all);
  n_valid = wave_sum(n_valid);
  n_visib = wave_sum(n_visib);
  ox0 = wave_min(ox0); oy0 = wave_min(oy0); ox1 = wave_max(ox1); oy1 = wave_max(oy1);
  vx0 = wave_min(vx0); vy0 = wave_min(vy0); vx1 = wave_max(vx1); vy1 = wave_max(vy1);
  if (lane == 0) {
    if (n_all) {
      atomicAdd(&s_cnt[0], n_all);
      atomicMin(&s_ext[0], ox0); atomicMin(&s_ext[1], oy0); atomicMax(&s_ext[2], ox1); atomicMax(&s_ext[3], oy1);
    }
    if (n_valid) atomicAdd(&s_cnt[1], n_valid);
    if (n_visib) {
      atomicAdd(&s_cnt[2], n_visib);
      atomicMin(&s_ext[4], vx0); atomicMin(&s_ext[5], vy0); atomicMax(&s_ext[6], vx1); atomicMax(&s_ext[7], vy1);
    }
  }
  __syncthreads();
  int* row = a.info + pose * kInfo;
  if (tid < 3) {
    if (s_cnt[tid]) atomicAdd(&row[tid], s_cnt[tid]);
  } else if (tid < kInfo) {
    const int e = tid - 3;  // 0..3 the silhouette's extents (counter 0), 4..7 the visible part's (counter 2)
    if (s_cnt[e < 4 ? 0 : 2]) {
      if (e & 2) atomicMax(&row[tid], s_ext[e]);
      else atomicMin(&row[tid], s_ext[e]);
    }
  }
}

inline size_t stage_bytes(const gdrnpp_meshes* m, int n) { return (size_t)n * (size_t)m->max_verts * kVtx * sizeof(double); }

}  // namespace

extern "C" {

size_t gdrnpp_gt_visibility_workspace_bytes(const gdrnpp_meshes* models, int n) {
  if (!models || n <= 0 || models->max_verts <= 0) return 0;
  return stage_bytes(models, n) + (size_t)n * 4 * sizeof(int);
}

int gdrnpp_gt_visibility(const gdrnpp_meshes* models, const int* obj, const int* im_idx, const double* R, const double* t, const double* K,
                         const float* depth, int n_im, int H, int W, int ox, int oy, float delta, double z_near, double z_far, int* info,
                         unsigned char* mask, unsigned char* mask_visib, int n, void* workspace, size_t workspace_bytes, void* stream) {
  GDRNPP_REQUIRE(models && models->verts && models->faces && models->vert_off && models->face_off && models->n_obj > 0, GDRNPP_EINVAL,
                 "gdrnpp_gt_visibility: invalid mesh set (the models need faces)");
  GDRNPP_REQUIRE(models->max_verts > 0, GDRNPP_EINVAL, "gdrnpp_gt_visibility: gdrnpp_meshes.max_verts must be set");
  GDRNPP_REQUIRE(n >= 0, GDRNPP_EINVAL, "gdrnpp_gt_visibility: n=%d", n);
  if (n == 0) return 0;
  GDRNPP_REQUIRE(obj && im_idx && R && t && K && depth && info, GDRNPP_EINVAL, "gdrnpp_gt_visibility: null pointer");
  GDRNPP_REQUIRE(n_im > 0 && H > 0 && W > 0, GDRNPP_EINVAL, "gdrnpp_gt_visibility: n_im=%d H=%d W=%d", n_im, H, W);
  GDRNPP_REQUIRE(ox >= 0 && oy >= 0, GDRNPP_EINVAL, "gdrnpp_gt_visibility: canvas offset ox=%d oy=%d must not be negative", ox, oy);
  GDRNPP_REQUIRE(z_near > 0.0 && z_far >= z_near, GDRNPP_EINVAL, "gdrnpp_gt_visibility: z_near=%g z_far=%g (0 < z_near <= z_far)", z_near,
                 z_far);
  const long long Wc = (long long)W + 2LL * ox, Hc = (long long)H + 2LL * oy;
  GDRNPP_REQUIRE(Wc * Hc <= INT_MAX, GDRNPP_ELIMIT, "gdrnpp_gt_visibility: a canvas of %lld x %lld pixels exceeds the 32-bit counters", Wc, Hc);
  const int tiles_x = (int)((Wc + kTile - 1) / kTile), tiles_y = (int)((Hc + kTile - 1) / kTile);
  const long long ntiles = (long long)tiles_x * tiles_y;
  GDRNPP_REQUIRE(ntiles * n <= INT_MAX, GDRNPP_ELIMIT, "gdrnpp_gt_visibility: %d poses x %lld tiles exceed one launch (split the poses)", n,
                 ntiles);
  const size_t need = gdrnpp_gt_visibility_workspace_bytes(models, n);
  GDRNPP_REQUIRE(workspace && workspace_bytes >= need, GDRNPP_EINVAL, "gdrnpp_gt_visibility: workspace %zu < %zu bytes",
                 workspace ? workspace_bytes : (size_t)0, need);
  GtArgs a{};
  a.verts = models->verts; a.faces = models->faces; a.vert_off = models->vert_off; a.face_off = models->face_off;
  a.n_obj = models->n_obj; a.max_verts = models->max_verts;
  a.obj = obj; a.im_idx = im_idx; a.R = R; a.t = t; a.K = K;
  a.depth = depth; a.n_im = n_im; a.H = H; a.W = W; a.ox = ox; a.oy = oy; a.Wc = (int)Wc; a.Hc = (int)Hc;
  a.delta = delta; a.z_near = z_near; a.z_far = z_far; a.info = info; a.mask = mask; a.mask_visib = mask_visib;
  a.hv = (double*)workspace;
  a.box = (int*)((char*)workspace + stage_bytes(models, n));
  hipStream_t st = (hipStream_t)stream;
  // the kernels store the covered bytes only: a skipped tile, a refused pose and the background are the zeros written here
  const size_t mask_bytes = (size_t)n * H * W;
  if (mask) {
    hipError_t e = hipMemsetAsync(mask, 0, mask_bytes, st);
    GDRNPP_REQUIRE(e == hipSuccess, (int)e, "gdrnpp_gt_visibility: clearing mask: %s", hipGetErrorString(e));
  }
  if (mask_visib) {
    hipError_t e = hipMemsetAsync(mask_visib, 0, mask_bytes, st);
    GDRNPP_REQUIRE(e == hipSuccess, (int)e, "gdrnpp_gt_visibility: clearing mask_visib: %s", hipGetErrorString(e));
  }
  hipLaunchKernelGGL(gt_project, dim3((unsigned)n), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(gt_tiles, dim3((unsigned)(ntiles * n)), dim3(kThreads), 0, st, a, tiles_x, (int)ntiles);
  return gdrnpp::check_launch("gdrnpp_gt_visibility");
}

}  // extern "C"
