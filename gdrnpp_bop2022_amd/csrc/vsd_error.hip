// BOP19 VSD (Visible Surface Discrepancy) of a batch of (estimate, ground truth) pairs on gfx950: the third error the BOP toolkit
// scores a results file with (lib/pysixd/scripts/eval_calc_errors.py:376-395), as a tiled render-and-compare.
//
// Behavioural spec: lib/pysixd/pose_error.py:22-128 (vsd, cost_type "step"), lib/pysixd/visibility.py:9-74 (visib_mode "bop19"),
// lib/pysixd/misc.py:604-647 (depth_im_to_dist_im_fast) and the render rule of lib/pysixd/renderer_vispy.py:432-539 as raster.hpp
// states it: pixel (row j, col i) sampled at (i+0.5, j+0.5), both faces, depth = camera-space Z rounded to float32, background 0.
// The toolkit hands the renderer fx, fy, cx, cy only, so the render uses K = [fx 0 cx; 0 fy cy; 0 0 1] whatever else K holds.
// For a pair with test depth D_t (float32, 0 = missing), renders D_e, D_g and pX = (x - cx) / fx, pY = (y - cy) / fy at the INTEGER
// pixel (x, y) (the toolkit's half-pixel inconsistency with its renderer is part of the spec):
//   dist(Z)  = sqrt(((pX Z)^2 + (pY Z)^2) + Z^2)                                         fp64, NumPy's order, no contraction
//   visib_g  = ((f32(dist_g) - f32(dist_t) <= delta) || dist_t == 0) && dist_g > 0       the subtraction in float32
//   visib_e  = (((f32(dist_e) - f32(dist_t) <= delta) || dist_t == 0) && dist_e > 0) || (visib_g && dist_e > 0)
//   union = #(visib_g || visib_e),  inter = #(visib_g && visib_e),  cost_k = #(inter pixels with |dist_g - dist_e| / diameter >= tau_k)
// The kernels output these integers only, i32[b, 2 + n_tau] = union, inter, cost_0 ..; the caller forms (cost_k + (union - inter)) /
// union in fp64, as the toolkit does.
//
// Two kernels on one stream:
//   vsd_project   one workgroup per (pair, pose).  Stages per vertex h = K (R v + t) and u = h0 / h2, v = h1 / h2 (5 doubles: the
//                 operands setup_triangle forms per corner, formed once per vertex) in the workspace, reduces the pose's conservative
//                 pixel box (shuffles, then LDS; the whole image once a vertex is nearer than z_near) and writes it behind the vertices.
//                 The workgroup of the estimate also initialises the pair's output row: 0, or -1 for a pair the device refuses
//                 (obj outside [0, n_obj), im_idx outside [0, n_im), an object without faces or vertices or above max_verts).
//   vsd_tiles     the grid is (pair, tile) over ALL 64x64 tiles of the image, so no host read-back sizes it; a workgroup whose tile
//                 misses both boxes leaves on a workgroup-uniform branch.  A surviving workgroup (256 threads) keeps two z-buffers of
//                 float-Z bits in LDS (32 KiB), walks the object's faces once per pose (face -> thread, staged corners read from L2),
//                 drops a face whose projected box misses tile & pose box before its fp64 vectors are read, and rasterises the rest
//                 with raster.hpp's unchanged expressions inside tile & box by ds_min_u32 (rounding to float is monotone, so the
//                 minimum of the rounded values is the rounded minimum).  A face with more than 32 candidate centres is rasterised by
//                 its whole wave (ballot, shfl_setup).  Then every pixel of the tile inside the boxes' hull evaluates the recipe;
//                 the 2 + n_tau counters are summed in registers, across a wave by shuffles, across waves by LDS atomics, and added to
//                 the pair's row with one global integer atomic per non-zero counter per workgroup.
// Deterministic: coverage and depth are decided by fixed fp64 expressions, the z-buffer by an integer minimum, and the outputs are
// integer sums, which do not depend on order: two runs are bit-equal with no ordering machinery.  sqrt and division are the IEEE
// correctly rounded ones, so dist equals NumPy's to the bit where the operands do.
// Roofline.  Per rendered pixel that some pose covers: 1 division (pY; pX is a per-thread constant: the thread's column is fixed), 3
// distances of 5 mul + 2 add + 1 sqrt, 2 float subtractions, and per tau 1 compare on the one division |dist_g - dist_e| / diameter:
// ~110 fp64 VALU operations with the divisions and roots expanded (division ~13, sqrt ~17), 4 B of the test depth read.  Per (face,
// pose, surviving tile): 12 B of indices + 3 x 24 B (z, u, v) for the box test, and for a face that reaches the tile 3 x 24 B more and
// ~60 operations (27 for the three cross products, 5 for D, the box); per candidate centre 18 operations, 3 compares, 1 division.
// Per (vertex, pose): 31 operations and 2 divisions, 12 B read, 40 B written.  Algorithmic HBM bytes per pair: 2 x 40 V staged once
// and re-read per surviving tile from L2, 12 F + 12 V of the model (L2-resident across the pairs of an object), 4 B per pixel of the
// test image under the boxes' hull, 4 (2 + n_tau) out.  By these counts the face walk (L2 gathers of 84 - 156 B per face and pose per
// tile against ~60 operations) bounds a 5 k-face model and the per-pixel fp64 recipe a small one; measured (tools/vsd_bench.py)
// the call reaches 0.26 / 0.05 of those bounds at 512 pairs: one wave per SIMD per workgroup (101 VGPRs) does not hide the dependent loads
// of the face walk and of the compare loop.
#include "common.hpp"
#include "tile_raster.hpp"
#include "wave_ops.hpp"
#include <climits>

namespace {

using namespace gdrnpp;
using namespace gdrnpp::tiles;   // tile_raster.hpp: kThreads, kTile, kVtx ..., the staging and the face walk shared with gt_visib.hip
using wave::wave_sum;

constexpr int kMaxTau = 16;

struct VsdArgs {
  const float* verts; const int* faces; const int* vert_off; const int* face_off; int n_obj, max_verts;
  const int* obj; const int* im_idx;
  const double *R_est, *t_est, *R_gt, *t_gt, *K, *diameter;
  const float* depth_test; int n_im, H, W;
  const double* taus; int n_tau; float delta;
  double z_near, z_far;
  int* counts;
  double* hv;   // [b][2][max_verts][kVtx]
  int* box;     // [b][2][4] = i_lo, i_hi, j_lo, j_hi (inclusive; empty when lo > hi)
};

// what only the device can see: such a pair's row is -1 and nothing of it is staged, rendered or read
__device__ __forceinline__ bool pair_ok(const VsdArgs& a, size_t pair, int& o) {
  o = a.obj[pair];
  if (o < 0 || o >= a.n_obj) return false;
  const int im = a.im_idx[pair];
  if (im < 0 || im >= a.n_im) return false;
  const int nv = a.vert_off[o + 1] - a.vert_off[o], nf = a.face_off[o + 1] - a.face_off[o];
  return nv > 0 && nv <= a.max_verts && nf > 0;
}

__global__ __launch_bounds__(kThreads) void vsd_project(const VsdArgs a) {
  __shared__ double s_red[kWaves][6];
  const size_t pair = blockIdx.x >> 1;
  const int pose = blockIdx.x & 1, tid = threadIdx.x;
  int o;
  const bool ok = pair_ok(a, pair, o);
  const int ncnt = 2 + a.n_tau;
  if (pose == 0 && tid < ncnt) a.counts[pair * ncnt + tid] = ok ? 0 : -1;
  int* box = a.box + 4 * (2 * pair + pose);
  if (!ok) {
    if (tid == 0) { box[0] = 1; box[1] = 0; box[2] = 1; box[3] = 0; }
    return;
  }
  const int v0 = a.vert_off[o], nv = a.vert_off[o + 1] - v0;
  double K[9], R[9], t[3];
  render_K(a.K + 9 * pair, K);
  const double* Rp = (pose ? a.R_gt : a.R_est) + 9 * pair;
  const double* tp = (pose ? a.t_gt : a.t_est) + 3 * pair;
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = Rp[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) t[k] = tp[k];
  double* hv = a.hv + ((2 * pair + pose) * (size_t)a.max_verts) * kVtx;
  const float* mv = a.verts + 3 * (size_t)v0;
  stage_vertices_and_box(mv, nv, K, R, t, hv, a.z_near, a.z_far, a.W, a.H, s_red, box);
}

__global__ __launch_bounds__(kThreads) void vsd_tiles(const VsdArgs a, int tiles_x, int ntiles) {
  __shared__ unsigned zb[2][kTilePix];
  __shared__ int s_cnt[2 + kMaxTau];

  const size_t pair = blockIdx.x / (unsigned)ntiles;
  const int tile = (int)(blockIdx.x - pair * (unsigned)ntiles);
  int o;
  if (!pair_ok(a, pair, o)) return;
  const int tid = threadIdx.x, lane = tid & 63;
  const int W = a.W, H = a.H;
  const int tx0 = (tile % tiles_x) * kTile, ty0 = (tile / tiles_x) * kTile;
  const int tx1 = min(tx0 + kTile, W) - 1, ty1 = min(ty0 + kTile, H) - 1;
  // this tile & each pose's box; a tile that misses both leaves (workgroup-uniform)
  int c[2][4];
  bool hit[2];
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int* bx = a.box + 4 * (2 * pair + p);
    c[p][0] = max(bx[0], tx0); c[p][1] = min(bx[1], tx1); c[p][2] = max(bx[2], ty0); c[p][3] = min(bx[3], ty1);
    hit[p] = c[p][0] <= c[p][1] && c[p][2] <= c[p][3];
  }
  if (!hit[0] && !hit[1]) return;

  for (int p = tid; p < 2 * kTilePix; p += kThreads) (&zb[0][0])[p] = kInfBits;
  if (tid < 2 + kMaxTau) s_cnt[tid] = 0;
  __syncthreads();

  const int nv = a.vert_off[o + 1] - a.vert_off[o];
  const int* mfaces = a.faces + 3 * (size_t)a.face_off[o];
  const int nfaces = a.face_off[o + 1] - a.face_off[o];
  const double zn = a.z_near, zf = a.z_far;

  for (int pose = 0; pose < 2; ++pose) {
    if (!hit[pose]) continue;  // workgroup-uniform
    const int ci0 = c[pose][0], ci1 = c[pose][1], cj0 = c[pose][2], cj1 = c[pose][3];
    const double* hv = a.hv + ((2 * pair + pose) * (size_t)a.max_verts) * kVtx;
    unsigned* z = zb[pose];
    raster_faces_tile(hv, mfaces, nfaces, nv, ci0, ci1, cj0, cj1, tx0, ty0, W, H, zn, zf, z);
  }
  __syncthreads();

  // ---- compare: the pixels of the tile inside the hull of the two boxes ---------------------------------------------------------
  int x_lo = tx1 + 1, x_hi = tx0 - 1, y_lo = ty1 + 1, y_hi = ty0 - 1;
#pragma unroll
  for (int p = 0; p < 2; ++p)
    if (hit[p]) { x_lo = min(x_lo, c[p][0]); x_hi = max(x_hi, c[p][1]); y_lo = min(y_lo, c[p][2]); y_hi = max(y_hi, c[p][3]); }
  const double* Kp = a.K + 9 * pair;
  const double fx = Kp[0], cx = Kp[2], fy = Kp[4], cy = Kp[5];
  const double diameter = a.diameter[pair];
  const float delta = a.delta;
  const int n_tau = a.n_tau;
  double tau[kMaxTau];
#pragma unroll
  for (int k = 0; k < kMaxTau; ++k) tau[k] = k < n_tau ? a.taus[k] : 0.0;
  int n_union = 0, n_inter = 0, n_cost[kMaxTau];
#pragma unroll
  for (int k = 0; k < kMaxTau; ++k) n_cost[k] = 0;
  const float* dt = a.depth_test + (size_t)a.im_idx[pair] * H * W;
  const int x = tx0 + lane;  // the thread's column in every row it visits
  if (x >= x_lo && x <= x_hi) {
    const double pX = ((double)x - cx) / fx;
    for (int ly = tid >> 6; ly < kTile; ly += kWaves) {
      const int y = ty0 + ly;
      if (y < y_lo || y > y_hi) continue;
      const unsigned be = zb[0][ly * kTile + lane], bg = zb[1][ly * kTile + lane];
      if (be == kInfBits && bg == kInfBits) continue;  // neither pose covers the pixel: in no mask
      const double Ze = be == kInfBits ? 0.0 : (double)__uint_as_float(be);
      const double Zg = bg == kInfBits ? 0.0 : (double)__uint_as_float(bg);
      const double Zt = (double)dt[(size_t)y * W + x];
      const double pY = ((double)y - cy) / fy;
      double ax = pX * Ze, ay = pY * Ze;
      const double dist_e = sqrt((ax * ax + ay * ay) + Ze * Ze);
      ax = pX * Zg; ay = pY * Zg;
      const double dist_g = sqrt((ax * ax + ay * ay) + Zg * Zg);
      ax = pX * Zt; ay = pY * Zt;
      const double dist_t = sqrt((ax * ax + ay * ay) + Zt * Zt);
      const float ft = (float)dist_t;
      const bool no_t = dist_t == 0.0;
      const bool vg = (((float)dist_g - ft <= delta) || no_t) && dist_g > 0.0;
      const bool ve = ((((float)dist_e - ft <= delta) || no_t) && dist_e > 0.0) || (vg && dist_e > 0.0);
      n_union += (vg || ve) ? 1 : 0;
      if (vg && ve) {
        ++n_inter;
        const double d = fabs(dist_g - dist_e) / diameter;
#pragma unroll
        for (int k = 0; k < kMaxTau; ++k) n_cost[k] += (k < n_tau && d >= tau[k]) ? 1 : 0;
      }
    }
  }
  n_union = wave_sum(n_union);
  n_inter = wave_sum(n_inter);
#pragma unroll
  for (int k = 0; k < kMaxTau; ++k) n_cost[k] = wave_sum(n_cost[k]);
  if (lane == 0) {
    if (n_union) atomicAdd(&s_cnt[0], n_union);
    if (n_inter) atomicAdd(&s_cnt[1], n_inter);
#pragma unroll
    for (int k = 0; k < kMaxTau; ++k)
      if (n_cost[k]) atomicAdd(&s_cnt[2 + k], n_cost[k]);
  }
  __syncthreads();
  if (tid < 2 + n_tau && s_cnt[tid]) atomicAdd(&a.counts[pair * (2 + n_tau) + tid], s_cnt[tid]);
}

inline size_t stage_bytes(const gdrnpp_meshes* m, int b) { return (size_t)b * 2 * (size_t)m->max_verts * kVtx * sizeof(double); }

}  // namespace

extern "C" {

size_t gdrnpp_vsd_counts_workspace_bytes(const gdrnpp_meshes* models, int b) {
  if (!models || b <= 0 || models->max_verts <= 0) return 0;
  return stage_bytes(models, b) + (size_t)b * 8 * sizeof(int);
}

int gdrnpp_vsd_counts(const gdrnpp_meshes* models, const int* obj, const int* im_idx, const double* R_est, const double* t_est,
                      const double* R_gt, const double* t_gt, const double* K, const double* diameter, const float* depth_test,
                      int n_im, int H, int W, const double* taus, int n_tau, float delta, double z_near, double z_far, int* counts,
                      int b, void* workspace, size_t workspace_bytes, void* stream) {
  GDRNPP_REQUIRE(models && models->verts && models->faces && models->vert_off && models->face_off && models->n_obj > 0, GDRNPP_EINVAL,
                 "gdrnpp_vsd_counts: invalid mesh set (the models need faces)");
  GDRNPP_REQUIRE(models->max_verts > 0, GDRNPP_EINVAL, "gdrnpp_vsd_counts: gdrnpp_meshes.max_verts must be set");
  GDRNPP_REQUIRE(obj && im_idx && R_est && t_est && R_gt && t_gt && K && diameter && depth_test && taus && counts, GDRNPP_EINVAL,
                 "gdrnpp_vsd_counts: null pointer");
  GDRNPP_REQUIRE(b > 0, GDRNPP_EINVAL, "gdrnpp_vsd_counts: b=%d", b);
  GDRNPP_REQUIRE(n_im > 0 && H > 0 && W > 0, GDRNPP_EINVAL, "gdrnpp_vsd_counts: n_im=%d H=%d W=%d", n_im, H, W);
  GDRNPP_REQUIRE(n_tau >= 1 && n_tau <= kMaxTau, GDRNPP_ELIMIT, "gdrnpp_vsd_counts: n_tau=%d outside 1..%d", n_tau, kMaxTau);
  GDRNPP_REQUIRE(z_near > 0.0 && z_far >= z_near, GDRNPP_EINVAL, "gdrnpp_vsd_counts: z_near=%g z_far=%g (0 < z_near <= z_far)", z_near,
                 z_far);
  const int tiles_x = (W + kTile - 1) / kTile, tiles_y = (H + kTile - 1) / kTile;
  const long long ntiles = (long long)tiles_x * tiles_y;
  GDRNPP_REQUIRE(ntiles * b <= INT_MAX && 2LL * b <= INT_MAX, GDRNPP_ELIMIT,
                 "gdrnpp_vsd_counts: %d pairs x %lld tiles exceed one launch (split the pairs)", b, ntiles);
  const size_t need = gdrnpp_vsd_counts_workspace_bytes(models, b);
  GDRNPP_REQUIRE(workspace && workspace_bytes >= need, GDRNPP_EINVAL, "gdrnpp_vsd_counts: workspace %zu < %zu bytes",
                 workspace ? workspace_bytes : (size_t)0, need);
  VsdArgs a{};
  a.verts = models->verts; a.faces = models->faces; a.vert_off = models->vert_off; a.face_off = models->face_off;
  a.n_obj = models->n_obj; a.max_verts = models->max_verts;
  a.obj = obj; a.im_idx = im_idx; a.R_est = R_est; a.t_est = t_est; a.R_gt = R_gt; a.t_gt = t_gt; a.K = K; a.diameter = diameter;
  a.depth_test = depth_test; a.n_im = n_im; a.H = H; a.W = W; a.taus = taus; a.n_tau = n_tau; a.delta = delta;
  a.z_near = z_near; a.z_far = z_far; a.counts = counts;
  a.hv = (double*)workspace;
  a.box = (int*)((char*)workspace + stage_bytes(models, b));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(vsd_project, dim3(2 * (unsigned)b), dim3(kThreads), 0, st, a);
  hipLaunchKernelGGL(vsd_tiles, dim3((unsigned)(ntiles * b)), dim3(kThreads), 0, st, a, tiles_x, (int)ntiles);
  return gdrnpp::check_launch("gdrnpp_vsd_counts");
}

}  // extern "C"
