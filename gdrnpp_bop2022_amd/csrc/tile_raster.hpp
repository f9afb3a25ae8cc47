// The full-image tiled render shared by vsd_error.hip (two poses per pair) and gt_visib.hip (one pose, optionally on a canvas larger than
// the image): the per-vertex staging with the pose's conservative pixel box, and the face walk of one 64x64 tile into an LDS z-buffer.
// The bodies are those vsd_error.hip was merged with, moved here unchanged as forceinline functions: raster.hpp's expressions decide
// coverage and depth, so both callers render the same bits for the same K, R, t and image size.
#pragma once
#include "raster.hpp"

namespace gdrnpp {
namespace tiles {

constexpr int kThreads = 256;   // 4 waves
constexpr int kWaves = kThreads / 64;
constexpr int kTile = 64;       // tile edge in pixels; a thread's column inside the tile is tid & 63
constexpr int kTilePix = kTile * kTile;
constexpr int kVtx = 5;         // staged doubles per vertex: h0, h1, h2, u, v
constexpr int kLargeArea = 32;  // candidate centres above which a face is rasterised by its whole wave
constexpr unsigned kInfBits = 0x7f800000u;

// what the toolkit's renderer sees of K: fx, fy, cx, cy
__device__ __forceinline__ void render_K(const double* __restrict__ Kp, double* K) {
  K[0] = Kp[0]; K[1] = 0.0; K[2] = Kp[2];
  K[3] = 0.0; K[4] = Kp[4]; K[5] = Kp[5];
  K[6] = 0.0; K[7] = 0.0; K[8] = 1.0;
}

// One workgroup of kThreads: stages h = K (R v + t), u = h0 / h2, v = h1 / h2 of the nv vertices at mv into hv[nv][kVtx] and writes the
// pose's conservative pixel box of a W x H render to box[4] = i_lo, i_hi, j_lo, j_hi (inclusive; empty when lo > hi; the whole render
// once a vertex is nearer than z_near).  s_red: kWaves x 6 doubles of LDS.  Holds one __syncthreads: every thread of the workgroup calls.
__device__ __forceinline__ void stage_vertices_and_box(const float* mv, int nv, const double* K, const double* R,
                                                       const double* t, double* hv, double z_near, double z_far, int W,
                                                       int H, double (*s_red)[6], int* box) {
  const int tid = threadIdx.x;
  // projections of the vertices at or beyond z_near, and the z range of all of them
  double umin = 1e300, umax = -1e300, vmin = 1e300, vmax = -1e300, zmin = 1e300, zmax = -1e300;
  for (int v = tid; v < nv; v += kThreads) {
    double h[3];
    project_vertex(mv + 3 * (size_t)v, K, R, t, h);
    const double pu = h[0] / h[2], pv = h[1] / h[2];
    double* dst = hv + (size_t)v * kVtx;
    dst[0] = h[0]; dst[1] = h[1]; dst[2] = h[2]; dst[3] = pu; dst[4] = pv;
    zmin = fmin(zmin, h[2]); zmax = fmax(zmax, h[2]);
    if (h[2] >= z_near) { umin = fmin(umin, pu); umax = fmax(umax, pu); vmin = fmin(vmin, pv); vmax = fmax(vmax, pv); }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
    umin = fmin(umin, __shfl_xor(umin, off, 64)); umax = fmax(umax, __shfl_xor(umax, off, 64));
    vmin = fmin(vmin, __shfl_xor(vmin, off, 64)); vmax = fmax(vmax, __shfl_xor(vmax, off, 64));
    zmin = fmin(zmin, __shfl_xor(zmin, off, 64)); zmax = fmax(zmax, __shfl_xor(zmax, off, 64));
  }
  if ((tid & 63) == 0) {
    double* r = s_red[tid >> 6];
    r[0] = umin; r[1] = umax; r[2] = vmin; r[3] = vmax; r[4] = zmin; r[5] = zmax;
  }
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < kWaves; ++w) {
      umin = fmin(umin, s_red[w][0]); umax = fmax(umax, s_red[w][1]); vmin = fmin(vmin, s_red[w][2]);
      vmax = fmax(vmax, s_red[w][3]); zmin = fmin(zmin, s_red[w][4]); zmax = fmax(zmax, s_red[w][5]);
    }
    int b0 = 1, b1 = 0, b2 = 1, b3 = 0;
    if (!(zmax < z_near || zmin > z_far || !(umin <= umax) || !(vmin <= vmax))) {
      if (zmin < z_near) {  // a face may cross the near plane: its clipped outline is not bounded by the vertices in front
        b0 = 0; b1 = W - 1; b2 = 0; b3 = H - 1;
      } else {              // every covered centre lies in a face's box (triangle_bbox), every face's box in this one
        b0 = clampi(ceil(umin - 0.5 - 1e-6), 0, W); b1 = clampi(floor(umax - 0.5 + 1e-6), -1, W - 1);
        b2 = clampi(ceil(vmin - 0.5 - 1e-6), 0, H); b3 = clampi(floor(vmax - 0.5 + 1e-6), -1, H - 1);
      }
    }
    box[0] = b0; box[1] = b1; box[2] = b2; box[3] = b3;
  }
}

// One workgroup of kThreads walks the nfaces faces at mfaces once (face -> thread, staged corners hv read from L2) and rasterises them
// into z[kTilePix] (LDS, float-Z bits, kInfBits = empty) of the tile whose first pixel is (tx0, ty0), inside [ci0, ci1] x [cj0, cj1] (tile
// & pose box, not empty) of a W x H render, by an unsigned minimum (rounding to float is monotone, so the minimum of the rounded values
// is the rounded minimum).  A face whose projected box misses that window leaves before its fp64 vectors are read; a face with more than
// kLargeArea candidate centres is rasterised by its whole wave.  No barrier inside: the caller synchronises before z is read.
__device__ __forceinline__ void raster_faces_tile(const double* hv, const int* mfaces, int nfaces, int nv,
                                                  int ci0, int ci1, int cj0, int cj1, int tx0, int ty0, int W, int H, double zn,
                                                  double zf, unsigned* z) {
  const int tid = threadIdx.x, lane = tid & 63;
  for (int f0 = 0; f0 < nfaces; f0 += kThreads) {
    const int f = f0 + tid;
    bool large = false;
    TriSetup s;
#pragma unroll
    for (int k = 0; k < 3; ++k) s.e0[k] = s.e1[k] = s.e2[k] = 0.0;
    s.D = 0.0; s.i_lo = 1; s.i_hi = 0; s.j_lo = 1; s.j_hi = 0;
    if (f < nfaces) {
      const int i0 = mfaces[3 * f], i1 = mfaces[3 * f + 1], i2 = mfaces[3 * f + 2];
      if ((unsigned)i0 < (unsigned)nv && (unsigned)i1 < (unsigned)nv && (unsigned)i2 < (unsigned)nv) {
        const double* p0 = hv + (size_t)i0 * kVtx;
        const double* p1 = hv + (size_t)i1 * kVtx;
        const double* p2 = hv + (size_t)i2 * kVtx;
        const double uv0[2] = {p0[3], p0[4]}, uv1[2] = {p1[3], p1[4]}, uv2[2] = {p2[3], p2[4]};
        const double z0 = p0[2], z1 = p1[2], z2 = p2[2];
        // a face wholly in front whose projected box (widened as triangle_bbox widens it) holds no centre of tile & box has no
        // candidate here; the comparisons are written so that a NaN passes on to the exact test
        bool cand = true;
        if (fmin(z0, fmin(z1, z2)) >= zn) {
          const double ulo = fmin(uv0[0], fmin(uv1[0], uv2[0])), uhi = fmax(uv0[0], fmax(uv1[0], uv2[0]));
          const double vlo = fmin(uv0[1], fmin(uv1[1], uv2[1])), vhi = fmax(uv0[1], fmax(uv1[1], uv2[1]));
          cand = !(uhi + 1e-6 < (double)ci0 + 0.5 || ulo - 1e-6 > (double)ci1 + 0.5 || vhi + 1e-6 < (double)cj0 + 0.5 ||
                   vlo - 1e-6 > (double)cj1 + 0.5);
        }
        if (cand) {
          const double h0[3] = {p0[0], p0[1], z0}, h1[3] = {p1[0], p1[1], z1}, h2[3] = {p2[0], p2[1], z2};
          if (triangle_bbox(h0, h1, h2, uv0, uv1, uv2, W, H, zn, zf, s)) {
            s.i_lo = max(s.i_lo, ci0); s.i_hi = min(s.i_hi, ci1); s.j_lo = max(s.j_lo, cj0); s.j_hi = min(s.j_hi, cj1);
            if (s.i_lo <= s.i_hi && s.j_lo <= s.j_hi && triangle_edges(h0, h1, h2, s)) {
              if ((s.i_hi - s.i_lo + 1) * (s.j_hi - s.j_lo + 1) > kLargeArea) large = true;
              else
                for (int j = s.j_lo; j <= s.j_hi; ++j)
                  for (int i = s.i_lo; i <= s.i_hi; ++i) {
                    double Z;
                    if (sample_triangle(s, i, j, zn, zf, Z, nullptr))
                      atomicMin(&z[(j - ty0) * kTile + (i - tx0)], __float_as_uint((float)Z));
                  }
            }
          }
        }
      }
    }
    // faces that cover much of the tile: all 64 lanes of the wave rasterise one (the trip count f0 is workgroup-uniform)
    unsigned long long bal = __ballot(large);
    while (bal) {
      const int src = __ffsll((long long)bal) - 1;
      bal &= bal - 1;
      const TriSetup s2 = shfl_setup(s, src);
      const int bw = s2.i_hi - s2.i_lo + 1, bh = s2.j_hi - s2.j_lo + 1;  // inside the tile: bw * bh <= 4096
      for (int p = lane; p < bw * bh; p += 64) {
        const int j = s2.j_lo + p / bw, i = s2.i_lo + p % bw;
        double Z;
        if (sample_triangle(s2, i, j, zn, zf, Z, nullptr))
          atomicMin(&z[(j - ty0) * kTile + (i - tx0)], __float_as_uint((float)Z));
      }
    }
  }
}

}  // namespace tiles
}  // namespace gdrnpp
