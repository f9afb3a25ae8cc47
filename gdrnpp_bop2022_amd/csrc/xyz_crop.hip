// The xyz_crop training targets of a batch of ground-truth poses on gfx950: the object-space coordinate map the reference's
// core/gdrn_modeling/tools/*/*_1_gen_xyz.py store per ground-truth instance (one full-image EGL frame, mask.sum(), nonzero(), four .item()
// read-backs, a full-image calc_xyz_bp_torch, a crop and a pickle per pose), as the third consumer of tile_raster.hpp: a pose is rendered
// once, its covered pixels are back-projected as the reference back-projects them, and only the pose's box is written, packed pose after
// pose.  No full-frame tensor, no clear pass, no per-pose host synchronisation.
//
// Behavioural spec: core/gdrn_modeling/tools/tless/tless_pbr_1_gen_xyz.py:95-187.  The tudl, icbin and itodd *_pbr_1_gen_xyz.py were
// compared with it: they differ in the dataset paths, IM_H / IM_W and the class list only.  lm/lm_egl_1_gen_xyz.py:100-180 reads one
// gt.json whose "pose" is already [R | t] in metres, uses one fixed K, has no scene directory and its skip of existing files commented
// out; from the render to the record (its :122-178) it is the same text.  near = 0.01, far = 6.5 and vertex_scale = 0.001 in all five.
// Further lib/pysixd/misc.py:381-409 (calc_xyz_bp_torch) and
// the render rule raster.hpp states: pixel (row j, col i) sampled at (i+0.5, j+0.5), both faces, depth = camera-space Z rounded to
// float32, background 0.  The render is the plain W x H image under fx, fy, cx, cy (render_K: no skew, no canvas offset); R, t, K are fp64,
// t in the unit of the vertices (the tools: metres).
// Per covered pixel (x, y), d = (float)Z of the z-buffer, everything below in fp32 with no contraction and IEEE division:
//   gx = (float)x - (float)cx, gy = (float)y - (float)cy     the INTEGER pixel, as calc_xyz_bp_torch's meshgrid; the raster samples at
//                                                            +0.5: the inconsistency is the reference's and it is kept
//   c0 = (gx d) / fx, c1 = (gy d) / fy, c2 = d;  e_j = c_j - (float)t_j
//   xyz_i = (R_0i e_0 + R_1i e_1) + R_2i e_2,  R_ji = (float)R[j][i]      R^T (c - t); the reference's einsum leaves the order of the
//                                                                         three products to the BLAS, here it is this one
//   fp16, round to nearest even, subnormals kept (NumPy's astype(float16)), at out[(off + (y - j_lo) bw + (x - i_lo)) 3 + i]
// A background pixel of the box is three +0 (the reference's xyz * mask can leave -0 there).
//
// Three kernels on one stream:
//   xyz_project   one workgroup per pose.  stage_vertices_and_box as it stands: h = K (R v + t), u, v per vertex into the workspace and the
//                 pose's conservative pixel box (it contains every covered pixel; the whole image once a vertex is nearer than z_near;
//                 empty for a pose outside the image or behind the camera) into the pose's row.  Initialises the row: status 0, count 0,
//                 empty extents; or twelve times -1, which every later reader takes as "no box", for a pose the device refuses (obj
//                 outside [0, n_obj), an object without faces or vertices or above max_verts).
//   xyz_offsets   one workgroup.  Exclusive scan, 64-bit and in pose order, of the box areas bw bh into the rows' offsets (pixels).  The
//                 inclusive ends never decrease, so "the first pose whose end exceeds the capacity and every pose after it" is
//                 end > capacity: those rows get status 1 (deferred); totals = the number of poses in front of them and the pixels they
//                 use.  A refused or empty pose occupies nothing.  capacity >= H W, so the first pose of a call always fits.
//   xyz_tiles     the grid is (pose, tile) over ALL 64x64 tiles, so no host read-back sizes it; a workgroup of a deferred or refused pose,
//                 or whose tile misses the box, leaves on a workgroup-uniform branch.  A surviving workgroup (256 threads) clears its
//                 16 KiB LDS z-buffer, walks the faces (raster_faces_tile) and then every pixel of tile & box writes its three halves.
//                 Count and extents (those of seg > 0 in the tool) as gt_tiles: registers, wave shuffles, LDS atomics, then one global
//                 integer atomic add / min / max per workgroup that saw a pixel.
// Packed output: every element of a served pose's box is written exactly once, by the thread that owns the pixel (the tiles partition the
// image, the box is inside it), so the buffer needs no clearing; nothing at or beyond totals[1] pixels is touched.
// Deterministic: coverage and depth are fixed fp64 expressions and the z-buffer an integer minimum (tile_raster.hpp); the back-projection
// is a fixed sequence of correctly rounded fp32 operations of one thread per pixel; offsets are integer sums in pose order; count and
// extents are an integer sum, minima and maxima.  No value depends on the order in which workgroups or atomics run: two runs are bit-equal.
// Roofline.  Per covered pixel: 2 int->float conversions, 2 subtractions, 2 multiplications, 2 divisions (~10 operations each expanded),
// 3 subtractions, 9 multiply / adds, 3 conversions to fp16: ~40 fp32 VALU operations, 6 B written; a background pixel of the box writes 6 B
// and computes nothing.  Per (face, surviving tile), per candidate centre and per vertex: gt_visib.hip's figures (84 - 156 B of L2 gathers
// and ~60 fp64 operations per face and tile; 18 operations and a division per centre; 31 operations, 2 divisions, 12 B read and 40 B
// written per vertex).  Algorithmic HBM bytes per pose: 6 B per box pixel written, 40 V staged once (re-read per surviving tile from L2),
// 12 F + 12 V of the model (L2-resident across the poses of an object), 48 B of the row.  A 5 k-face, 2.5 k-vertex model 50 - 100 px across
// at 640 x 480: a box of 3 10^3 - 10^4 px = 17 - 60 KB, staging 100 KB, together 0.12 - 0.16 MB or 0.015 - 0.02 us of HBM time per pose,
// against 5 120 faces x 2 - 4 tiles x 84 - 156 B = 1 - 3 MB of L2 gathers (0.06 - 0.2 us at 17 TB/s) and ~1 M fp64 operations (0.03 us):
// by these counts the face walk's L2 gathers bound it, as they bound gt_visib.hip without masks, and the HBM write roofline is an order of
// magnitude above what a pose can reach.  The measured figure is in DESIGN.md (tools/xyz_crop_bench.py).
#include "common.hpp"
#include "tile_raster.hpp"
#include "wave_ops.hpp"
#include <climits>

namespace {

using namespace gdrnpp;
using namespace gdrnpp::tiles;
using wave::wave_max, wave::wave_min, wave::wave_sum;

constexpr int kRow = 12;  // status, count, x1 y1 x2 y2, box i_lo i_hi j_lo j_hi, offset in pixels (low, high word)
constexpr int kBox = 6, kOff = 10;

struct XyzArgs {
  const float* verts; const int* faces; const int* vert_off; const int* face_off; int n_obj, max_verts;
  const int* obj;
  const double *R, *t, *K;
  int H, W;
  double z_near, z_far;
  unsigned short* out;     // packed fp16 bits, capacity x 3
  long long capacity;      // pixels
  int* rows;               // [n][kRow]
  long long* totals;       // n_done, used pixels
  double* hv;              // [n][max_verts][kVtx]
  int n;
};

__device__ __forceinline__ bool pose_ok(const XyzArgs& a, size_t pose, int& o) {
  o = a.obj[pose];
  if (o < 0 || o >= a.n_obj) return false;
  const int nv = a.vert_off[o + 1] - a.vert_off[o], nf = a.face_off[o + 1] - a.face_off[o];
  return nv > 0 && nv <= a.max_verts && nf > 0;
}

__global__ __launch_bounds__(kThreads) void xyz_project(const XyzArgs a) {
  __shared__ double s_red[kWaves][6];
  const size_t pose = blockIdx.x;
  const int tid = threadIdx.x;
  int o;
  const bool ok = pose_ok(a, pose, o);
  int* row = a.rows + pose * kRow;
  if (!ok) {
    if (tid < kRow) row[tid] = -1;
    return;
  }
  // the box columns are written by stage_vertices_and_box, everything else here
  if (tid < kRow && (tid < kBox || tid >= kOff)) row[tid] = (tid == 2 || tid == 3) ? INT_MAX : (tid == 4 || tid == 5) ? INT_MIN : 0;
  const int v0 = a.vert_off[o], nv = a.vert_off[o + 1] - v0;
  double K[9], R[9], t[3];
  render_K(a.K + 9 * pose, K);
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = a.R[9 * pose + k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = a.t[3 * pose + k];
  stage_vertices_and_box(a.verts + 3 * (size_t)v0, nv, K, R, t, a.hv + (pose * (size_t)a.max_verts) * kVtx, a.z_near, a.z_far, a.W, a.H, s_red,
                         row + kBox);
}

// pixels of a row's box; 0 for the empty box and for a refused pose's row of -1
__device__ __forceinline__ long long box_area(const int* row) {
  const int bw = row[kBox + 1] - row[kBox] + 1, bh = row[kBox + 3] - row[kBox + 2] + 1;
  return row[0] < 0 || bw <= 0 || bh <= 0 ? 0LL : (long long)bw * bh;
}

__global__ __launch_bounds__(kThreads) void xyz_offsets(const XyzArgs a) {
  __shared__ long long s_wave[kWaves];
  __shared__ long long s_base;
  __shared__ int s_done;
  __shared__ unsigned long long s_used;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  if (tid == 0) { s_base = 0; s_done = 0; s_used = 0ULL; }
  __syncthreads();
  for (int p0 = 0; p0 < a.n; p0 += kThreads) {  // the trip count is workgroup-uniform
    const int p = p0 + tid;
    int* row = a.rows + (size_t)p * kRow;
    const long long area = p < a.n ? box_area(row) : 0LL;
    long long incl = area;  // inclusive scan across the wave, then across the waves
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long up = __shfl_up(incl, off, 64);
      if (lane >= off) incl += up;
    }
    if (lane == 63) s_wave[wave] = incl;
    __syncthreads();
    long long base = s_base;
    for (int w = 0; w < wave; ++w) base += s_wave[w];
    const long long end = base + incl;
    if (p < a.n) {
      const long long start = end - area;
      if (end > a.capacity) {
        if (row[0] == 0) row[0] = 1;
      } else {
        atomicAdd(&s_done, 1);
        atomicMax(&s_used, (unsigned long long)end);
        if (row[0] == 0) { row[kOff] = (int)(unsigned)(start & 0xffffffffLL); row[kOff + 1] = (int)(start >> 32); }
      }
    }
    __syncthreads();
    if (tid == kThreads - 1) s_base = end;
    __syncthreads();
  }
  if (tid == 0) { a.totals[0] = s_done; a.totals[1] = (long long)s_used; }
}

__device__ __forceinline__ unsigned short half_bits(float v) {
  const _Float16 h = (_Float16)v;  // v_cvt_f16_f32: round to nearest even, subnormal results kept
  return __builtin_bit_cast(unsigned short, h);
}

__global__ __launch_bounds__(kThreads) void xyz_tiles(const XyzArgs a, int tiles_x, int ntiles) {
  __shared__ unsigned zb[kTilePix];
  __shared__ int s_cnt;
  __shared__ int s_ext[4];

  const size_t pose = blockIdx.x / (unsigned)ntiles;
  const int tile = (int)(blockIdx.x - pose * (unsigned)ntiles);
  int* row = a.rows + pose * kRow;
  if (row[0] != 0) return;  // refused (-1) or deferred (1): nothing of it is rendered or written
  const int tid = threadIdx.x, lane = tid & 63;
  const int W = a.W, H = a.H;
  const int tx0 = (tile % tiles_x) * kTile, ty0 = (tile / tiles_x) * kTile;
  const int tx1 = min(tx0 + kTile, W) - 1, ty1 = min(ty0 + kTile, H) - 1;
  const int i_lo = row[kBox], i_hi = row[kBox + 1], j_lo = row[kBox + 2], j_hi = row[kBox + 3];
  const int ci0 = max(i_lo, tx0), ci1 = min(i_hi, tx1), cj0 = max(j_lo, ty0), cj1 = min(j_hi, ty1);
  if (ci0 > ci1 || cj0 > cj1) return;
  const long long off = (long long)(((unsigned long long)(unsigned)row[kOff + 1] << 32) | (unsigned)row[kOff]);

  for (int p = tid; p < kTilePix; p += kThreads) zb[p] = kInfBits;
  if (tid == 0) s_cnt = 0;
  if (tid < 4) s_ext[tid] = (tid & 2) ? INT_MIN : INT_MAX;
  __syncthreads();

  const int o = a.obj[pose];  // in range: the row's status is 0
  const int nv = a.vert_off[o + 1] - a.vert_off[o];
  const int* mfaces = a.faces + 3 * (size_t)a.face_off[o];
  const int nfaces = a.face_off[o + 1] - a.face_off[o];
  raster_faces_tile(a.hv + (pose * (size_t)a.max_verts) * kVtx, mfaces, nfaces, nv, ci0, ci1, cj0, cj1, tx0, ty0, W, H, a.z_near, a.z_far, zb);
  __syncthreads();

  // ---- the recipe: the pixels of tile & box ---------------------------------------------------------------------------------------------
  const double* Kp = a.K + 9 * pose;
  const double* Rp = a.R + 9 * pose;
  const double* tp = a.t + 3 * pose;
  const float fx = (float)Kp[0], cx = (float)Kp[2], fy = (float)Kp[4], cy = (float)Kp[5];
  float R[9], t[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = (float)Rp[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = (float)tp[k];
  const int bw = i_hi - i_lo + 1;
  int n_cov = 0, x0 = INT_MAX, y0 = INT_MAX, x1 = INT_MIN, y1 = INT_MIN;
  const int x = tx0 + lane;  // the thread's column in every row it visits
  if (x >= ci0 && x <= ci1) {
    const float gx = (float)x - cx;
    for (int ly = tid >> 6; ly < kTile; ly += kWaves) {
      const int y = ty0 + ly;
      if (y < cj0 || y > cj1) continue;
      // (y - j_lo) bw + (x - i_lo) < bw bh <= capacity - off: inside the pose's share of the packed buffer
      unsigned short* dst = a.out + (size_t)(off + (long long)(y - j_lo) * bw + (x - i_lo)) * 3;
      const unsigned bits = zb[ly * kTile + lane];
      unsigned short h0 = 0, h1 = 0, h2 = 0;
      if (bits != kInfBits) {
        const float d = __uint_as_float(bits);
        const float gy = (float)y - cy;
        const float e0 = (gx * d) / fx - t[0];
        const float e1 = (gy * d) / fy - t[1];
        const float e2 = d - t[2];
        h0 = half_bits((R[0] * e0 + R[3] * e1) + R[6] * e2);
        h1 = half_bits((R[1] * e0 + R[4] * e1) + R[7] * e2);
        h2 = half_bits((R[2] * e0 + R[5] * e1) + R[8] * e2);
        ++n_cov;
        x0 = min(x0, x); x1 = max(x1, x); y0 = min(y0, y); y1 = max(y1, y);
      }
      dst[0] = h0; dst[1] = h1; dst[2] = h2;
    }
  }
  n_cov = wave_sum(n_cov);
  x0 = wave_min(x0); y0 = wave_min(y0); x1 = wave_max(x1); y1 = wave_max(y1);
  if (lane == 0 && n_cov) {
    atomicAdd(&s_cnt, n_cov);
    atomicMin(&s_ext[0], x0); atomicMin(&s_ext[1], y0); atomicMax(&s_ext[2], x1); atomicMax(&s_ext[3], y1);
  }
  __syncthreads();
  if (s_cnt) {
    if (tid == 0) atomicAdd(&row[1], s_cnt);
    else if (tid < 3) atomicMin(&row[1 + tid], s_ext[tid - 1]);
    else if (tid < 5) atomicMax(&row[1 + tid], s_ext[tid - 1]);
  }
}

inline size_t stage_bytes(const gdrnpp_meshes* m, int n) { return (size_t)n * (size_t)m->max_verts * kVtx * sizeof(double); }

}  // namespace

extern "C" {

size_t gdrnpp_gt_xyz_crop_workspace_bytes(const gdrnpp_meshes* models, int n) {
  if (!models || n <= 0 || models->max_verts <= 0) return 0;
  return stage_bytes(models, n);
}

int gdrnpp_gt_xyz_crop(const gdrnpp_meshes* models, const int* obj, const double* R, const double* t, const double* K, int H, int W,
                       double z_near, double z_far, unsigned short* out, long long capacity_px, int* rows, long long* totals, int n,
                       void* workspace, size_t workspace_bytes, void* stream) {
  GDRNPP_REQUIRE(models && models->verts && models->faces && models->vert_off && models->face_off && models->n_obj > 0, GDRNPP_EINVAL,
                 "gdrnpp_gt_xyz_crop: invalid mesh set (the models need faces)");
  GDRNPP_REQUIRE(models->max_verts > 0, GDRNPP_EINVAL, "gdrnpp_gt_xyz_crop: gdrnpp_meshes.max_verts must be set");
  GDRNPP_REQUIRE(n >= 0, GDRNPP_EINVAL, "gdrnpp_gt_xyz_crop: n=%d", n);
  if (n == 0) return 0;
  GDRNPP_REQUIRE(obj && R && t && K && out && rows && totals, GDRNPP_EINVAL, "gdrnpp_gt_xyz_crop: null pointer");
  GDRNPP_REQUIRE(H > 0 && W > 0, GDRNPP_EINVAL, "gdrnpp_gt_xyz_crop: H=%d W=%d", H, W);
  GDRNPP_REQUIRE(z_near > 0.0 && z_far >= z_near, GDRNPP_EINVAL, "gdrnpp_gt_xyz_crop: z_near=%g z_far=%g (0 < z_near <= z_far)", z_near, z_far);
  GDRNPP_REQUIRE((long long)W * H <= INT_MAX, GDRNPP_ELIMIT, "gdrnpp_gt_xyz_crop: an image of %d x %d pixels exceeds the 32-bit counters", W, H);
  GDRNPP_REQUIRE(capacity_px >= (long long)W * H, GDRNPP_EINVAL,
                 "gdrnpp_gt_xyz_crop: capacity of %lld pixels is below one image of %d x %d (a pose's box can be the whole image)", capacity_px, W, H);
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  const long long ntiles = (long long)tiles_x * tiles_y;
  GDRNPP_REQUIRE(ntiles * n <= INT_MAX, GDRNPP_ELIMIT, "gdrnpp_gt_xyz_crop: %d poses x %lld tiles exceed one launch (split the poses)", n, ntiles);
  const size_t need = gdrnpp_gt_xyz_crop_workspace_bytes(models, n);
  GDRNPP_REQUIRE(workspace && workspace_bytes >= need, GDRNPP_EINVAL, "gdrnpp_gt_xyz_crop: workspace %zu < %zu bytes",
                 workspace ? workspace_bytes : (size_t)0, need);
  XyzArgs a{};
  a.verts = models->verts; a.faces = models->faces; a.vert_off = models->vert_off; a.face_off = models->face_off;
  a.n_obj = models->n_obj; a.max_verts = models->max_verts;
  a.obj = obj; a.R = R; a.t = t; a.K = K; a.H = H; a.W = W; a.z_near = z_near; a.z_far = z_far;
  a.out = out; a.capacity = capacity_px; a.rows = rows; a.totals = totals; a.hv = (double*)workspace; a.n = n;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(xyz_project, dim3((unsigned)n), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(xyz_offsets, dim3(1), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(xyz_tiles, dim3((unsigned)(ntiles * n)), dim3(kThreads), 0, st, a, tiles_x, (int)ntiles);
  return gdrnpp::check_launch("gdrnpp_gt_xyz_crop");
}

}  // extern "C"
