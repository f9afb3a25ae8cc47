/*
 * gdrnpp_hip.h — flat C ABI of libgdrnpp_hip.so (MI355X / gfx950).
 *
 * This is the drop-in boundary for the GDRNPP inference hot path
 * (SURVEY.md §8b).  Two groups of entry points:
 *
 *  (1) Reference-ABI symbols: byte-for-byte the prototypes the reference's
 *      cffi modules bind (host pointers, synchronous, no status):
 *        core/csrc/fps/src/ext.h:1-14
 *        core/csrc/uncertainty_pnp/src/ext.h:1-9
 *  (2) gdrnpp_* symbols: device-pointer, stream-ordered, batched entry points
 *      that replace the reference's torch extensions (ransac_voting.cpp:112-117,
 *      nnd_cuda.cpp:86-89) and its per-ROI CPU/GL post-processing
 *      (gdrn_evaluator.py:115-153,461-573, engine_utils.py:295-333,
 *      pose_from_pred_centroid_z.py:56-154, lib/render_vispy/renderer.py).
 *
 * Conventions for group (2):
 *   - every pointer is a DEVICE pointer unless its name starts with h_;
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream);
 *   - return 0 = ok, negative = argument error (GDRNPP_E*), positive = hipError_t;
 *   - no allocation inside; scratch is passed in, sized by *_workspace_bytes();
 *   - no global state apart from the process-wide tuning switches of gdrnpp_set_option; safe from several host
 *     threads on different streams.
 */
#ifndef GDRNPP_HIP_H_
#define GDRNPP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GDRNPP_EINVAL (-1) /* bad size / null pointer */
#define GDRNPP_ELIMIT (-2) /* size above what the kernel supports */

/* library/ABI version: major*10000 + minor*100 + patch */
int gdrnpp_version(void);
/* message for the last non-zero status returned on this host thread */
const char* gdrnpp_last_error(void);
/* process-wide tuning switches, read on the launch path (no environment lookups there):
 *   "split_gemm_glds"  0 / 1   256-row tiles of the split GEMM / convolution use the register-staged kernel / the
 *                              LDS-DMA kernel (default 1; results are bitwise identical)
 *   "split_gemm_pipe"  0 / 2 / 3   256-row tiles of the linear form use the software-pipelined LDS-DMA kernel with two /
 *                              three A stages (default 3; bitwise identical to the other kernels); 0 = off
 *   "split_gemm_big_tiles"  >= 1    256x128 output tiles (pipelined / LDS-DMA kernels) when the problem has at least this many
 *                                   of them (default 256 = one per CU), 128x128 tiles below
 *   "split_gemm_panel"      0, 2..64  wide layers (packed weight > 2 MB, N >= 1024) walk their tiles in panels of that many
 *                                   256-row blocks, column tile outer, for L2 reuse of both operands (default 4; 0: row-major)
 *   "split_gemm_mi4"   -1 / 0 / 1   tile height by tile count (default) / force 128 rows / force 256 rows
 *   "dwconv_tile"      -1 / 0 / 1 / 2   output pixels per thread of the depthwise 7x7 kernel: by launch size (default: 2x8 at
 *                                   the headline batch, 2x4 / 1x4 when a launch has too few tiles for the chip) / force 2x8 / 2x4 / 1x4
 *   "mlp_fused_pipe"   0 / 1       fused stage-0 MLP (gdrnpp_convnext_mlp_f32_fused): software-pipelined tile loop (default 1) or the plain loop (A/B switch)
 *   "dwconv_lds_w"     0 / 1       depthwise 7x7 + LayerNorm: [49][C] weights in LDS with persistent workgroups where they fit (default 1) or
 *                                   through L1 / L2 without LDS (A/B switch: which of two kernels sharing the chip yields is decided by the LDS
 *                                   a workgroup holds, profiles/r06_dwconv_shared.txt; bitwise identical)
 *   "dwconv_specialise" 0 / 1      depthwise 7x7 + LayerNorm: C = 128 / 256 / 512 / 1024 run the kernel compiled for that width (default 1) or
 *                                   every C runs the run-time-width form (A/B switch; bitwise identical)
 *   "dwconv_lds_pad"   bytes      experiment only: dynamic LDS the no-LDS form allocates without using it (default 0)
 *   "upconv_lowres"    0 / 1       read by the callers' routing, not by a launch: a 3x3 convolution behind a bilinear x2 upsampling runs
 *                                   as a tap GEMM at the low resolution + gdrnpp_upconv_gather_gn_nhwc (default 1) or as the upsampling
 *                                   and the convolution of the high-resolution tensor (0)
 *   "conv3x3_window"   0 / 1       three-product 3x3 / stride 1 / pad 1 convolution (gdrnpp_conv3x3_f32_split2) at W = 16 / 32 / 64 with
 *                                   H % (256 / W) == 0: a workgroup stages the input window of its 256 pixels once per 16-channel chunk and
 *                                   reads the nine taps from it (default 1) or stages one operand image per tap (0; every other shape runs
 *                                   that form).  Same products, another summation order: results differ in their last bits
 * unknown name -> GDRNPP_EINVAL. */
int gdrnpp_set_option(const char* name, int value);
/* the value gdrnpp_set_option left (clamped as that entry point clamps it) or the default */
int gdrnpp_get_option(const char* name, int* value);

/* ------------------------------------------------------------------------ */
/* (1) reference-ABI symbols (host pointers)                                 */
/* ------------------------------------------------------------------------ */

/* core/csrc/fps/src/ext.h:1-6 — random start point (time-seeded like
 * farthest_point_sampling.cpp:93-94); pts f32[pn,3], idxs i32[sn]. */
void farthest_point_sampling(float* pts, int* idxs, int pn, int sn);
/* core/csrc/fps/src/ext.h:9-14 — start = farthest from bbox centre
 * (farthest_point_sampling.cpp:122-160). */
void farthest_point_sampling_init_center(float* pts, int* idxs, int pn, int sn);

/* core/csrc/uncertainty_pnp/src/ext.h:1-9 — covariance-weighted reprojection
 * LM (uncertainty_pnp.cpp:61-92).  pts2d f64[pn,2], pts3d f64[pn,3],
 * wgt2d f64[pn,3]=(wxx,wxy,wyy), K f64[9], init_rt/result_rt f64[6]
 * = (angle-axis, t). */
void uncertainty_pnp(double* pts2d, double* pts3d, double* wgt2d, double* K,
                     double* init_rt, double* result_rt, int pn);

/* ------------------------------------------------------------------------ */
/* (2) device-pointer entry points                                           */
/* ------------------------------------------------------------------------ */

/* ---- farthest point sampling (a9) ---------------------------------------
 * pts f32[b,pn,3]; idxs i32[b,sn]; start_idx i32[b] or NULL.
 * mode 0: start from start_idx[b] (farthest_point_sampling.cpp:76-105 with the
 *         random draw made explicit); mode 1: init-center (…:122-160).
 * workspace: gdrnpp_fps_workspace_bytes(b,pn) bytes (may be 0). */
size_t gdrnpp_fps_workspace_bytes(int b, int pn);
int gdrnpp_fps(const float* pts, int* idxs, const int* start_idx, int b, int pn,
               int sn, int mode, void* workspace, void* stream);

/* ---- bidirectional NN distance / chamfer (a12) ---------------------------
 * nnd_cuda.cpp:37-60 (forward), :63-84 (backward).
 * xyz1 f32[b,n,3], xyz2 f32[b,m,3] -> dist1 f32[b,n], idx1 i32[b,n],
 * dist2 f32[b,m], idx2 i32[b,m]; first minimum wins (nnd_cpu.cpp:3-25). */
int gdrnpp_nnd_forward(const float* xyz1, const float* xyz2, float* dist1,
                       float* dist2, int* idx1, int* idx2, int b, int n, int m,
                       void* stream);
/* grad buffers are overwritten (zeroed inside), like nnd_cuda_kernel.cu:185-222 */
int gdrnpp_nnd_backward(const float* xyz1, const float* xyz2, float* gradxyz1,
                        float* gradxyz2, const float* graddist1,
                        const float* graddist2, const int* idx1, const int* idx2,
                        int b, int n, int m, void* stream);

/* ---- PVNet-style RANSAC voting (a10) -------------------------------------
 * ransac_voting.cpp:30-41,51-65,74-85,95-109.
 * direct f32[tn,vn,2], coords f32[tn,2], idxs i32[hn,vn,2],
 * hypo_pts f32[hn,vn,2] (vanishing point: [hn,vn,3]); the kernels overwrite
 * the whole of hypo_pts (degenerate pairs -> 0, like at::zeros + skip);
 * inliers u8[hn,vn,tn] must be pre-zeroed by the caller exactly as in the
 * reference (ransac_voting_gpu.py:58) — only 1s are written. */
int gdrnpp_generate_hypothesis(const float* direct, const float* coords,
                               const int* idxs, float* hypo_pts, int tn, int vn,
                               int hn, void* stream);
int gdrnpp_voting_for_hypothesis(const float* direct, const float* coords,
                                 const float* hypo_pts, unsigned char* inliers,
                                 int tn, int vn, int hn, float inlier_thresh,
                                 void* stream);
int gdrnpp_generate_hypothesis_vanishing_point(const float* direct,
                                               const float* coords,
                                               const int* idxs, float* hypo_pts,
                                               int tn, int vn, int hn,
                                               void* stream);
int gdrnpp_voting_for_hypothesis_vanishing_point(
    const float* direct, const float* coords, const float* hypo_pts,
    unsigned char* inliers, int tn, int vn, int hn, float inlier_thresh,
    void* stream);
/* fused vote + count: counts i32[hn,vn] = sum_t inlier(hi,vi,ti) without
 * materialising the [hn,vn,tn] tensor (replaces voting + torch.sum(...,2),
 * ransac_voting_gpu.py:58-62).  homogeneous=1 -> vanishing-point variant. */
int gdrnpp_vote_count(const float* direct, const float* coords,
                      const float* hypo_pts, int* counts, int tn, int vn, int hn,
                      float inlier_thresh, int homogeneous, void* stream);

/* ---- uncertainty-PnP, batched (a11) --------------------------------------
 * One problem per workgroup; same cost and LM schedule as the host symbol.
 * pts2d f64[b,pn,2], pts3d f64[b,pn,3], wgt f64[b,pn,3], K f64[b,9],
 * init f64[b,6] -> result f64[b,6]; info i32[b,2] = (iterations, status) or NULL. */
int gdrnpp_uncertainty_pnp_batched(const double* pts2d, const double* pts3d,
                                   const double* wgt2d, const double* K,
                                   const double* init_rt, double* result_rt,
                                   int* info, int b, int pn, void* stream);

/* ---- EPnP + RANSAC on the decoded correspondences (a7: "ransac_pnp", "net_ransac_pnp", "net_ransac_pnp_rot") ------
 * cv2.solvePnPRansac(objectPoints, imagePoints, K, dist = 0, flags = SOLVEPNP_EPNP, reprojectionError, iterationsCount,
 * confidence = 0.99) as called at lib/pysixd/misc.py:182-193 (reprojErr 3, 100 iterations) and
 * gdrn_evaluator.py:319-330 (20 iterations), for every ROI of the batch.  OpenCV is a third-party dependency that is not
 * in the reference tree: its published algorithms are restated (calib3d epnp.cpp, ptsetreg.cpp, solvepnp.cpp) — 5-point
 * minimal sets, float32 squared reprojection error <= reprojErr^2, best = strictly more inliers, adaptive iteration
 * count, final EPnP over the inliers of the best hypothesis; count == 5: one EPnP over all five; count == 4: one P3P solve
 * (OpenCV switches to SOLVEPNP_P3P there: the poses consistent with the first three points, the fourth picks), all inliers.
 * img_pts f32[b,stride,2], mdl_pts f32[b,stride,3], count i32[b]: outputs of gdrnpp_decode_correspondences; K f32[b,9].
 * draws: NULL -> every ROI draws from cv::RNG(2^64-1) like OpenCV does; else u32[b,n_draws] words consumed in order
 * (index = word % count, redrawn while it repeats), n_draws >= 5*iters.
 * R_out f32[b,9], t_out f32[b,3], n_inliers i32[b], status i32[b] (1 = pose found; 0 = fewer than 4 points, no
 * hypothesis with at least 5 inliers, or a degenerate system: R = I, t = 0 and the caller applies the reference's
 * fallback), inlier_mask u8[b,stride].  workspace: gdrnpp_epnp_ransac_workspace_bytes(b, stride, iters). */
size_t gdrnpp_epnp_ransac_workspace_bytes(int b, int stride, int iters);
int gdrnpp_epnp_ransac(const float* img_pts, const float* mdl_pts, const int* count, int stride, const float* K,
                       const unsigned* draws, int n_draws, int iters, float reproj_err, double confidence,
                       float* R_out, float* t_out, int* n_inliers, int* status, unsigned char* inlier_mask,
                       int b, void* workspace, size_t workspace_bytes, void* stream);
/* plain EPnP on all n >= 4 points of each problem (cv2.solvePnP(flags=SOLVEPNP_EPNP); un_pnp_utils.py:27-44 runs it on the
 * four best-weighted keypoints to initialise uncertainty-PnP): img_pts f32[b,n,2], mdl_pts f32[b,n,3], K f32[b,9]. */
int gdrnpp_epnp_batched(const float* img_pts, const float* mdl_pts, int n, const float* K, float* R_out,
                        float* t_out, int* status, int b, void* stream);

/* ---- net-initialised iterative PnP on the decoded correspondences (a7, "net_iter_pnp") ------------------------
 * gdrn_evaluator.py:241-371 with pnp_type="iter": cv2.solvePnP(SOLVEPNP_ITERATIVE, useExtrinsicGuess=True) seeded
 * with the network pose = Levenberg-Marquardt on the plain reprojection error.  OpenCV's own LM is third-party and
 * not in the tree; the same restated LM as gdrnpp_uncertainty_pnp_batched is used with identity weights (both
 * converge to the minimiser of the same cost).  img_pts f32[b,stride,2], mdl_pts f32[b,stride,3] and count i32[b]
 * are the outputs of gdrnpp_decode_correspondences (stride = hw); a count above stride is clamped to stride, as in
 * gdrnpp_epnp_ransac, so a problem never reads another problem's rows.  Reference fallbacks kept: count < 4 -> network
 * pose (:355-358); |t_est - t_net| > 1 m -> network translation (:347-351, info status += 100).
 * K f32[b,9], R_net f32[b,9], t_net f32[b,3] -> R_out f32[b,9], t_out f32[b,3], info i32[b,2] or NULL. */
int gdrnpp_pnp_iter_from_correspondences(const float* img_pts, const float* mdl_pts,
                                         const int* count, int stride, const float* K,
                                         const float* R_net, const float* t_net,
                                         float* R_out, float* t_out, int* info, int b,
                                         void* stream);

/* ---- map decoding + 2D-3D correspondences (a4 + a6) ----------------------
 * engine_utils.py:295-333 (regression xyz, mask_type: 0=L1 min-max, 1=sigmoid)
 * and gdrn_evaluator.py:115-153.  coor f32[b,3,64*64] (x,y,z planes, may be
 * three separate [b,1,h,w] tensors laid out contiguously or passed via
 * strides = plane stride in floats), mask_raw f32[b,hw], coord2d f32[b,2,hw],
 * extent f32[b,3], imwh f32[b,2]=(im_W, im_H).
 * outputs: out_mask f32[b,hw] (normalised mask, may be NULL), count i32[b],
 * sel_idx i32[b,hw] (row-major pixel index of every selected pixel, in
 * order), img_pts f32[b,hw,2], mdl_pts f32[b,hw,3]; rows >= count[b] are left
 * untouched. */
int gdrnpp_decode_correspondences(const float* coor_x, const float* coor_y,
                                  const float* coor_z, const float* mask_raw,
                                  const float* coord2d, const float* extent,
                                  const float* imwh, float* out_mask, int* count,
                                  int* sel_idx, float* img_pts, float* mdl_pts,
                                  int b, int hw, int mask_type, float mask_thr,
                                  void* stream);

/* ---- allocentric->egocentric pose from Patch-PnP output (a3.4 + a3.5) -----
 * rot_reps.py:34-55 + pose_from_pred_centroid_z.py:56-154 + utils.py:31-75.
 * rot6d f32[b,6] (allo), t_ f32[b,3] = (dx,dy,z_rel), cams f32[b,9],
 * centers f32[b,2], whs f32[b,2], resize_ratios f32[b] -> rot f32[b,9] (ego),
 * trans f32[b,3].  z_type 0=REL 1=ABS; is_allo 0/1. */
int gdrnpp_pose_from_pred_centroid_z(const float* rot6d, const float* t_,
                                     const float* cams, const float* centers,
                                     const float* whs, const float* resize_ratios,
                                     float* rot, float* trans, int b, int z_type,
                                     int is_allo, void* stream);
/* the other ROT_TYPE / TRANS_TYPE variants of GDRN_double_mask.py:162-200 through the same kernel:
 * rot_mode 0 = 6-d representation f32[b,6], 1 = quaternion (w,x,y,z) f32[b,4] (quat2mat_torch, pose_utils.py:349-400),
 *          2 = rotation matrix f32[b,9], 3 = log-quaternion f32[b,3] (quaternion_lf.qexp, core/utils/quaternion_lf.py:294-318,
 *          then quat2mat_torch), 4 = Lie vector / angle-axis f32[b,3] (lie_algebra.lie_vec_to_rot, core/utils/lie_algebra.py:7-77)
 *          — get_rot_mat, model_utils.py:347-359;
 * t_mode   0 = centroid_z with relative z, 1 = centroid_z with absolute z, 2 = centroid_z_abs (absolute 2-d centre and z,
 *          pose_from_pred_centroid_z_abs.py:44-76; centers / whs / resize_ratios unused), 3 = trans (t_ is the translation,
 *          pose_from_pred.py:25-27). */
int gdrnpp_pose_from_pred(const float* rot_in, int rot_mode, const float* t_, int t_mode, const float* cams,
                          const float* centers, const float* whs, const float* resize_ratios, float* rot, float* trans,
                          int b, int is_allo, void* stream);

/* Patch-PnP's two output layers in one launch (row a3.3): rot_ = fc_r(x), t_ = fc_t(x) of ConvPnPNet.forward,
 * core/gdrn_modeling/models/heads/conv_pnp_net.py:99-101,178-182 (two nn.Linear on the same [b,256] feature).
 * x f32[b,K] (K <= 1024), w_r f32[rot_dim,K] (rot_dim <= 9), b_r f32[rot_dim] | NULL, w_t f32[3,K], b_t f32[3] | NULL
 * -> rot_ f32[b,rot_dim], t_ f32[b,3]; fp32 fma chains, one wavefront per ROI, fixed summation order. */
int gdrnpp_pnp_fc_heads(const float* x, const float* w_r, const float* b_r, const float* w_t, const float* b_t, float* rot_,
                        float* t_, int b, int K, int rot_dim, void* stream);
/* the same launch followed, per ROI, by gdrnpp_pose_from_pred on the values just computed (GDRN_double_mask.py:162-200 behind
 * conv_pnp_net.py:178-182): the network's last kernel.  rot_dim follows from rot_mode (6 / 4 / 9 / 3 / 3); rot_ f32[b,rot_dim] and
 * t_ f32[b,3] are written as well (forward returns them to the losses / tests).  Pose arguments as gdrnpp_pose_from_pred. */
int gdrnpp_pnp_fc_heads_pose(const float* x, const float* w_r, const float* b_r, const float* w_t, const float* b_t, float* rot_,
                             float* t_, int b, int K, int rot_mode, int t_mode, const float* cams, const float* centers,
                             const float* whs, const float* resize_ratios, float* rot, float* trans, int is_allo, void* stream);

/* ---- SimplePointPnPNet (core/gdrn_modeling/models/heads/point_pnp_net.py:208-293), use_softpool=False ---------------------
 * The point-wise MLP conv1 -> LeakyReLU(0.1) -> conv2 -> LeakyReLU(0.1) -> conv3 (1x1 Conv1d, cin -> 128 -> 128 -> 1024) over
 * the hw points of each ROI with the global max over the points in the last layer's epilogue: neither hidden layer nor the
 * [b,1024,hw] tensor leaves the chip.  Exact-f32 matrix instructions (a k-ordered fmaf chain per output).
 *   x  f32[b*hw][pitch]  NHWC, the first cin channels of a row are used; pitch % 32 == 0, cin <= pitch, cin <= 128
 *   w1 f32[128][cin], b1 f32[128], w2 f32[128][128], b2 f32[128], w3 f32[1024][128], b3 f32[1024]   (Conv1d weights, kernel 1)
 *   hw % 128 == 0: one workgroup per (ROI, tile of 128 points)
 *   workspace: gdrnpp_point_pnp_workspace_bytes(b, hw) bytes (0 for sizes the kernel does not take); receives the per-tile
 *              maxima f32[b][hw/128][1024] that gdrnpp_point_pnp_fc reads
 *   pooled f32[b][1024] | NULL: the max over the ROI's points of W3 lrelu(W2 lrelu(W1 x + b1) + b2) + b3, written by a second
 *              small launch; NULL when only gdrnpp_point_pnp_fc follows
 * fp32 max is order-independent: results are bit-reproducible, no atomics, any number of streams.
 * Argument errors (null pointer, b <= 0, hw % 128 != 0, cin > pitch, pitch % 32 != 0, small workspace) return a negative
 * status before anything is launched. */
size_t gdrnpp_point_pnp_workspace_bytes(int b, int hw);
int gdrnpp_point_pnp_pool(const float* x, int pitch, int cin, const float* w1, const float* b1, const float* w2, const float* b2,
                          const float* w3, const float* b3, float* pooled, int b, int hw, void* workspace, size_t workspace_bytes,
                          void* stream);
/* feat f32[b][256] = lrelu(fc2(lrelu(fc1(max over the tiles of the workspace)))), LeakyReLU slope 0.1 (point_pnp_net.py:287-288).
 * w_fc1 f32[512][1024], b_fc1 f32[512], w_fc2 f32[256][512], b_fc2 f32[256] (nn.Linear layout).  fp32 fmaf chains in a fixed
 * order, four ROIs per workgroup.  The last layer (fc_pose) is gdrnpp_pnp_fc_heads / gdrnpp_pnp_fc_heads_pose on feat with the
 * rows [0, rot_dim) and [rot_dim, rot_dim + 3) of its weight. */
int gdrnpp_point_pnp_fc(const void* workspace, size_t workspace_bytes, const float* w_fc1, const float* b_fc1, const float* w_fc2,
                        const float* b_fc2, float* feat, int b, int hw, void* stream);

/* ---- crop-resize intrinsics (a8.2) — camera_geometry.py:6-21 --------------
 * K f32[b,9], centers f32[b,2], scales f32[b] -> K_crop f32[b,9],
 * with crop_xy = center - scale/2 and ratio = out_res/scale
 * (engine_utils.py:260-264). */
int gdrnpp_zoom_K(const float* K, const float* centers, const float* scales,
                  float* K_crop, int b, float out_res, void* stream);

/* ---- mesh set for the depth rasteriser -----------------------------------
 * A flat, caller-owned description of all object models resident in HBM:
 * verts f32[sum V,3], faces i32[sum F,3] (indices local to the object),
 * vert_off i32[n_obj+1], face_off i32[n_obj+1]. */
typedef struct gdrnpp_meshes {
  const float* verts;
  const int* faces;
  const int* vert_off;
  const int* face_off;
  int n_obj;
  int max_verts; /* host-side hint: max vertices of any object (0 = unknown -> no LDS staging) */
  int max_faces; /* host-side hint: max faces of any object (0 = unknown) */
} gdrnpp_meshes;

/* ---- depth render (a8.1 / a14) — lib/render_vispy/renderer.py:126-130,
 * 155-182,363-407,461-477 restated without GL: depth f32[b,res,res] in metres,
 * 0 = background; optional xyz f32[b,res,res,3] = object-space surface point
 * (the PCObject attachment of egl_renderer, egl_renderer_v3.py:1185-1225),
 * NULL to skip.  K f32[b,9], R f32[b,9], t f32[b,3], obj i32[b]. */
int gdrnpp_render_depth(const gdrnpp_meshes* meshes, const int* obj,
                        const float* K, const float* R, const float* t,
                        float* depth, float* xyz, int b, int res, float z_near,
                        float z_far, void* stream);

/* ---- fast depth refinement (a8) — gdrn_evaluator.py:461-573 ---------------
 * One workgroup per ROI runs all iterations (render -> query map -> threshold
 * -> median -> weighted centroid -> ray update) on chip.
 * coor_{x,y,z} f32[b,hw] normalised xyz maps; mask_raw f32[b,hw];
 * roi_depth f32[b,in_res,in_res] sensor depth crop, in_res must be 4*res (256x256 for res=64: the kernel reads the 2x2
 * centre of every 4x4 block like cv2.resize at scale 4; anything else is refused);
 * K_crop f32[b,9]; R f32[b,9]; t_in f32[b,3]; obj i32[b] -> t_out f64[b,3].  An obj id outside [0, n_obj) leaves t = t_in.
 * mask_type as in gdrnpp_decode_correspondences; use_coor_z: TEST.USE_COOR_Z_REFINE.
 * debug_depth (f32[b,iters,hw]) receives each iteration's render or NULL.
 * workspace: gdrnpp_depth_refine_workspace_bytes(meshes, b) — 0 unless a mesh has more than 4096 vertices (their
 * transformed vertices are then staged in this workspace instead of LDS; same kernel, same arithmetic). */
size_t gdrnpp_depth_refine_workspace_bytes(const gdrnpp_meshes* meshes, int b);
int gdrnpp_depth_refine(const gdrnpp_meshes* meshes, const int* obj,
                        const float* coor_x, const float* coor_y,
                        const float* coor_z, const float* mask_raw,
                        const float* roi_depth, const float* K_crop,
                        const float* R, const float* t_in, double* t_out,
                        float* debug_depth, int b, int res, int in_res, int iters,
                        float threshold, int mask_type, int use_coor_z,
                        float z_near, float z_far, void* workspace, size_t workspace_bytes, void* stream);
/* The post-processing tail of the refine configuration in ONE launch: get_K_crop_resize (camera_geometry.py:6-21, from
 * cam f32[b,9], center f32[b,2], scale f32[b] and OUTPUT_RES = res) -> the refinement above -> the f32[b,16] pose records
 * R(9) | t(3, metres) | score | obj | roi_id | valid of gdrnpp_pack_pose_records (score / roi_id nullable; valid = 0 for
 * an obj id outside the mesh set). */
int gdrnpp_refine_to_records(const gdrnpp_meshes* meshes, const int* obj, const float* coor_x, const float* coor_y,
                             const float* coor_z, const float* mask_raw, const float* roi_depth, const float* cam,
                             const float* center, const float* scale, const float* R, const float* t_in,
                             const float* score, const int* roi_id, float* rec, int b, int res, int in_res, int iters,
                             float threshold, int mask_type, int use_coor_z, float z_near, float z_far, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- pose errors of the custom evaluator — gdrn_custom_evaluator.py:672-730 with lib/pysixd/pose_error.py:256-296 (add,
 * adi), :359-374 (re), :406-417 (te), :440-445 (arp_2d) and pose_utils.py:472-496 (get_closest_rot) ----------------------
 * All b (estimate, ground truth) pairs of a dataset in one call, pairs of different classes mixed.  Device pointers:
 * obj i32[b] class index into `models` (whose verts are the model points; the float64 values of those float32 numbers);
 * R_est, R_gt, K f64[b,9]; t_est, t_gt f64[b,3] in metres; sym_rots f64[n_sym_total,9] with sym_off i32[n_obj+1] (both NULL:
 * no class has a symmetry list); symmetric u8[n_obj] (NULL: none), 1 = the class takes adi and the closest symmetric
 * ground-truth rotation (symmetries visited in order, replaced on a strictly smaller re) for re and proj, while adi itself
 * keeps the unmodified R_gt.  out f64[b,4] = ad, re (degrees), te, proj (pixels).  An obj outside [0, n_obj), an empty model
 * or one with more vertices than models->max_verts gives NaN for ad and proj.  models->max_verts must be set (> 0).
 * Sums have a fixed order: two calls give bit-equal output.  workspace: gdrnpp_pose_errors_workspace_bytes(models, b) =
 * 8 * b * (24 + 2 * ceil(max_verts / 256)) bytes.  Argument errors return GDRNPP_EINVAL / GDRNPP_ELIMIT and launch nothing. */
size_t gdrnpp_pose_errors_workspace_bytes(const gdrnpp_meshes* models, int b);
int gdrnpp_pose_errors(const gdrnpp_meshes* models, const int* obj, const double* R_est, const double* t_est,
                       const double* R_gt, const double* t_gt, const double* K, const double* sym_rots,
                       const int* sym_off, const unsigned char* symmetric, double* out, int b, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- BOP19 MSSD / MSPD — lib/pysixd/pose_error.py:131-179 with misc.py:568-582 (project_pts), the two errors that
 * eval_calc_errors.py:397-423 computes for every (estimate, ground truth of the same object in the same image) pair -------
 * All b pairs of a dataset in one call, objects mixed.  Device pointers: obj i32[b] index into `models` (the eval-model
 * vertices in the unit of the translations, millimetres for a BOP results file); R_est, R_gt, K f64[b,9]; t_est, t_gt
 * f64[b,3]; sym_R f64[n_sym_total,9], sym_t f64[n_sym_total,3]: the symmetry transformations of every object, object after
 * object (misc.get_symmetry_transformations).  sym_off i32[n_obj+1] is a HOST array: it sizes the grid, and the kernels read
 * a copy placed in the workspace.  It starts at 0, and every object holds at least one transformation (the identity for an
 * object without symmetries): an empty range is an argument error.  out f64[b,2] = mssd, mspd (pixels; z is not clamped).
 * An obj outside [0, n_obj) or an empty model gives NaN.  fp64 throughout; maxima and minima only, so two calls give
 * bit-equal output.  workspace: gdrnpp_bop_errors_workspace_bytes(models, sym_off, b) = round_up(4 (n_obj + 1), 16) +
 * 16 * b * ceil(max symmetries of an object / 8) bytes (0 for arguments that gdrnpp_bop_errors refuses).  Argument errors
 * return GDRNPP_EINVAL / GDRNPP_ELIMIT and launch nothing. */
size_t gdrnpp_bop_errors_workspace_bytes(const gdrnpp_meshes* models, const int* sym_off, int b);
int gdrnpp_bop_errors(const gdrnpp_meshes* models, const int* obj, const double* R_est, const double* t_est,
                      const double* R_gt, const double* t_gt, const double* K, const double* sym_R, const double* sym_t,
                      const int* sym_off, double* out, int b, void* workspace, size_t workspace_bytes, void* stream);

/* ---- symmetry-aware reS / teS / projS — lib/pysixd/pose_error.py:377-396 (re_sym), :420-437 (te_sym), :183-217 (arp_2d_sym =
 * proj_sym), the errors eval_calc_errors.py:545-596 computes for every pair: each the minimum over the object's symmetry
 * transformations, of the rotation error (degrees), of the translation error, and of the MEAN over the model points of the projected
 * distance (pixels; z is not clamped) --------------------------------------------------------------------------------------------
 * Arguments as gdrnpp_bop_errors (sym_off is a HOST array, starts at 0, no empty range), except that K may be NULL: projS is then
 * not wanted, no work over the model points is launched and the call is O(symmetries) per pair.  out f64[b,3] = reS, teS (unit of
 * t), projS (NaN without K, and for an empty model); an obj outside [0, n_obj) gives a NaN row.  Columns 0 and 1 do not depend on
 * whether K was given.  fp64 throughout; every sum has a fixed order and there are no floating-point atomics: two calls give
 * bit-equal output, and a pair's result does not depend on the other pairs of the call.  workspace:
 * gdrnpp_sym_errors_workspace_bytes(models, sym_off, b) = round_up(4 (n_obj + 1), 16) + 24 * b * ceil(max symmetries of an object
 * / 8) bytes (0 for arguments that gdrnpp_sym_errors refuses), with or without K.  Argument errors return GDRNPP_EINVAL /
 * GDRNPP_ELIMIT and launch nothing. */
size_t gdrnpp_sym_errors_workspace_bytes(const gdrnpp_meshes* models, const int* sym_off, int b);
int gdrnpp_sym_errors(const gdrnpp_meshes* models, const int* obj, const double* R_est, const double* t_est,
                      const double* R_gt, const double* t_gt, const double* K, const double* sym_R, const double* sym_t,
                      const int* sym_off, double* out, int b, void* workspace, size_t workspace_bytes, void* stream);

/* ---- BOP19 VSD — lib/pysixd/pose_error.py:22-128 (cost_type "step") with visibility.py:9-74 ("bop19") and misc.py:604-647, the error
 * eval_calc_errors.py:376-395 computes per (estimate, ground truth) pair from two full-image depth renders and the test depth image.
 * Device pointers: obj i32[b] class index into `models` (which need faces; used as gdrnpp_render_depth uses them); im_idx i32[b]
 * index into depth_test f32[n_im,H,W] (millimetres, 0 = missing); R_est, R_gt, K f64[b,9] (of K only fx, fy, cx, cy are used, as the
 * toolkit passes them); t_est, t_gt f64[b,3] in the unit of the vertices; diameter f64[b], the divisor of the pixel-wise distances
 * (1.0 = not normalised: x / 1.0 is exact); taus f64[n_tau], 1 <= n_tau <= 16; delta: the visibility tolerance; only fragments with
 * 0 < z_near <= Z <= z_far are rendered.  counts i32[b, 2 + n_tau] = union, inter, cost_0 .. cost_{n_tau-1} (pixel counts); the
 * error at tau_k is (cost_k + (union - inter)) / (double)union, or 1.0 when union is 0.  What only the device can see — an obj outside
 * [0, n_obj), an im_idx outside [0, n_im), an object without faces or vertices, or with more vertices than models->max_verts —
 * gives that pair's whole row -1.  Integer sums only: two calls give bit-equal output.  models->max_verts must be set (> 0).
 * workspace: gdrnpp_vsd_counts_workspace_bytes(models, b) = b * (2 * max_verts * 40 + 32) bytes (the projected vertices of both
 * poses and their pixel boxes).  Argument errors return GDRNPP_EINVAL / GDRNPP_ELIMIT and launch nothing. */
size_t gdrnpp_vsd_counts_workspace_bytes(const gdrnpp_meshes* models, int b);
int gdrnpp_vsd_counts(const gdrnpp_meshes* models, const int* obj, const int* im_idx, const double* R_est, const double* t_est,
                      const double* R_gt, const double* t_gt, const double* K, const double* diameter, const float* depth_test,
                      int n_im, int H, int W, const double* taus, int n_tau, float delta, double z_near, double z_far, int* counts,
                      int b, void* workspace, size_t workspace_bytes, void* stream);

/* ---- BOP ground-truth info and masks — lib/pysixd/scripts/calc_gt_info.py:98-173 and calc_gt_masks.py:83-111 with visibility.py:9-54
 * ("bop19") and misc.py:628-647: per ground-truth pose one full-canvas depth render compared with the scene's depth image.
 * Device pointers: obj i32[n] class index into `models` (which need faces); im_idx i32[n] index into depth f32[n_im,H,W] (millimetres,
 * 0 = missing); R, K f64[n,9] (of K only fx, fy, cx, cy are used); t f64[n,3] in the unit of the vertices.  (ox, oy) >= 0 is the canvas
 * offset: the render covers (W + 2 ox) x (H + 2 oy) pixels with the principal point at (cx + ox, cy + oy), and the image is the window
 * [ox, ox + W) x [oy, oy + H) of it — (W, H) for calc_gt_info.py's 3W x 3H canvas, (0, 0) for calc_gt_masks.py's plain image.  delta:
 * the visibility tolerance; only fragments with 0 < z_near <= Z <= z_far are rendered.  info i32[n,11] = px_count_all (canvas),
 * px_count_valid, px_count_visib (window), then the inclusive extents x_min, y_min, x_max, y_max of the canvas silhouette and of the
 * visible part, in image coordinates (canvas index minus offset; they may be negative or reach beyond the image); empty extents are
 * INT_MAX, INT_MAX, INT_MIN, INT_MIN (x_min > x_max).  mask, mask_visib u8[n,H,W] or NULL: the silhouette and its visible part in the
 * window as bytes 0 / 255; the call clears them on `stream` before it renders.  What only the device can see — an obj outside
 * [0, n_obj), an im_idx outside [0, n_im), an object without faces or vertices, or with more vertices than models->max_verts — gives
 * that pose's whole row -1 and leaves its mask planes zero.  Integer sums, minima, maxima and bytes with one owner only: two calls give
 * bit-equal output.  models->max_verts must be set (> 0).  workspace: gdrnpp_gt_visibility_workspace_bytes(models, n) = n * (max_verts
 * * 40 + 16) bytes (the projected vertices and the pixel boxes).  n = 0 succeeds and touches nothing.  Argument errors return
 * GDRNPP_EINVAL / GDRNPP_ELIMIT, launch nothing and touch no output. */
size_t gdrnpp_gt_visibility_workspace_bytes(const gdrnpp_meshes* models, int n);
int gdrnpp_gt_visibility(const gdrnpp_meshes* models, const int* obj, const int* im_idx, const double* R, const double* t,
                         const double* K, const float* depth, int n_im, int H, int W, int ox, int oy, float delta, double z_near,
                         double z_far, int* info, unsigned char* mask, unsigned char* mask_visib, int n, void* workspace,
                         size_t workspace_bytes, void* stream);

/* ---- xyz_crop training targets — core/gdrn_modeling/tools/tless/tless_pbr_1_gen_xyz.py:95-187 (and its lm, tudl, icbin, itodd
 * siblings) with lib/pysixd/misc.py:381-409 (calc_xyz_bp_torch): per ground-truth pose one render of the plain W x H image, the covered
 * pixels back-projected to object space in float32 and stored as float16, only the pose's pixel box written, pose after pose.
 * Device pointers: obj i32[n] class index into `models` (which need faces); R, K f64[n,9] (of K only fx, fy, cx, cy are used); t
 * f64[n,3] in the unit of the vertices.  Only fragments with 0 < z_near <= Z <= z_far are rendered.  rows i32[n,12] = status (0 served,
 * 1 deferred, -1 refused), the covered-pixel count, the inclusive extents x1, y1, x2, y2 of coverage (empty: INT_MAX, INT_MAX, INT_MIN,
 * INT_MIN), the conservative box i_lo, i_hi, j_lo, j_hi (inclusive, empty when lo > hi; it contains the extents) and the pose's offset
 * into `out` in pixels (low word, high word).  out: fp16 bits, capacity_px x 3; pixel (x, y) of a served pose's box is at
 * out[(offset + (y - j_lo) (i_hi - i_lo + 1) + (x - i_lo)) 3 + c], three +0 where the pixel is not covered.  Every element of a served
 * pose's box is written exactly once and nothing at or beyond totals[1] pixels is touched: `out` needs no clearing.  The first pose whose
 * box would end beyond capacity_px and every pose after it are deferred (status 1, nothing written): totals i64[2] = the number of poses
 * in front of them, the pixels those use.  capacity_px >= H W, so a call serves at least its first pose; call again from pose
 * totals[0].  What only the device can see — an obj outside [0, n_obj), an object without faces or vertices, or with more vertices
 * than models->max_verts — gives that pose's whole row -1 and no space.  Fixed fp32 expressions, one owner per element, integer sums,
 * minima and maxima: two calls give bit-equal output.  models->max_verts must be set (> 0).  workspace:
 * gdrnpp_gt_xyz_crop_workspace_bytes(models, n) = n * max_verts * 40 bytes (the projected vertices).  n = 0 succeeds and touches
 * nothing.  Argument errors return GDRNPP_EINVAL / GDRNPP_ELIMIT, launch nothing and touch no output. */
size_t gdrnpp_gt_xyz_crop_workspace_bytes(const gdrnpp_meshes* models, int n);
int gdrnpp_gt_xyz_crop(const gdrnpp_meshes* models, const int* obj, const double* R, const double* t, const double* K, int H, int W,
                       double z_near, double z_far, unsigned short* out, long long capacity_px, int* rows, long long* totals, int n,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- per-ROI training targets — GDRN_DatasetFromList.read_data_train, core/gdrn_modeling/datasets/data_loader.py:448-612 with
 * TRAIN.VIS off, for n ROIs over images of H x W in one launch.  Device pointers; outputs contiguous; an output passed as NULL is
 * not wanted.  centers f64[n,2], scales f64[n], out_res: the convention of gdrnpp_crop_resize_roi; every crop is a nearest-neighbour
 * fetch at OpenCV's source pixel, border 0.
 *   The xyz source is what gdrnpp_gt_xyz_crop packs: xyz_packed f16 bits [xyz_px,3]; per ROI xyz_off i64 (in pixels) and
 * xyz_box i32[n,4] = x1, y1, x2, y2 inclusive in image space, row pitch x2 - x1 + 1.  A source pixel outside the box is (0, 0, 0); a
 * box with x2 < x1 or y2 < y1 is an instance without a covered pixel.  masks u8[n_masks,H,W] (a byte counts as 1 if it is not 0), per ROI
 * visib_idx (-1: visib = obj), trunc_idx (-1: trunc = visib, the reference's `mask_trunc is None`), full_idx (-1: roi_mask_full all 0);
 * masks == NULL stands for three columns of -1.  obj i32[n] indexes extents f32[n_obj,3] and fps f64[n_obj,F,3]; F = 0: no region
 * output; F > 256 is refused (GDRNPP_ELIMIT).  n_bin = 0: no bins; bin_mask selects the mask of the bins: 0 trunc, 1 visib, 2 obj, 3 full.
 *   roi_mask_obj f32[n,o,o] (o = out_res) = 1 where the fetched xyz has a non-zero component; roi_mask_visib = visib byte x obj;
 * roi_mask_trunc = trunc byte x that; roi_mask_full = full byte.  roi_region i32[n,o,o] = xyz_to_region (core/utils/data_utils.py:
 * 267-280): 1 + argmin over the object's F points of the fp64 distance sqrt((dx dx + dy dy) + dz dz), the differences taken in fp64
 * from the float32 value of the fp16 source, nothing contracted, first index on ties, times the obj mask.  roi_xyz f32[n,3,o,o] =
 * x / extent[c] + 0.5 in float32 (one IEEE division, one addition; the background holds 0.5).  roi_xyz_bin u8[n,3,o,o] (n_bin > 0) =
 * trunc(clip(roi_xyz, 0, float32(0.999999)) x n_bin), n_bin where the selected mask is 0; with n_bin > 0 roi_xyz holds the clipped values,
 * as in the reference, where the clipping works on a view of it (:579-592).  Every element of every wanted output of the n ROIs is
 * written once, nothing else is touched, the inputs are only read: two calls are bit-equal.  Indices are device data the host cannot
 * see: a mask index >= n_masks reads as a byte of 0, an offset outside [0, xyz_px) as a zero pixel, and a ROI whose obj is outside
 * [0, n_obj) gets region, xyz and bins of 0.  n = 0 succeeds and launches nothing.  Refused, naming the argument, with nothing launched:
 * n < 0, H or W <= 0 (GDRNPP_EINVAL) or >= 32767 (GDRNPP_ELIMIT), out_res <= 0 or > 4096 (ELIMIT), F < 0, n_bin outside [0, 255],
 * bin_mask outside 0..3, bin_mask = 3 with bins wanted and masks NULL, n > 65535 (ELIMIT), and a NULL among centers, scales, xyz_packed,
 * xyz_off, xyz_box, the three index columns when masks is given, and obj / extents / fps when an output needs them. */
int gdrnpp_roi_train_targets(const unsigned short* xyz_packed, long long xyz_px, const long long* xyz_off, const int* xyz_box,
                             const unsigned char* masks, int n_masks, const int* visib_idx, const int* trunc_idx, const int* full_idx,
                             int H, int W, const double* centers, const double* scales, const int* obj, const float* extents, int n_obj,
                             const double* fps, int F, int out_res, int n_bin, int bin_mask, float* roi_mask_obj, float* roi_mask_visib,
                             float* roi_mask_trunc, float* roi_mask_full, int* roi_region, float* roi_xyz, unsigned char* roi_xyz_bin,
                             int n, void* stream);

/* ---- background replacement of the training loader (csrc/replace_bg.hip) — `replace_bg` and `trunc_mask` of
 * core/base_data_loader.py:413-478 over `get_bg_image` / `get_bg_image_v2` (:480-579) and `resize_short_edge`
 * (core/utils/data_utils.py:208-235), for B images of H x W in one call.  Device pointers: images u8[B,H,W,3], composited IN PLACE
 * (bytes of kept pixels are never written); masks u8[B,H,W], the instance masks (non-zero = foreground); mask_trunc u8[B,H,W], written
 * as 0 / 1; bg: bg_bytes bytes holding the decoded backgrounds, 3 bytes per pixel, rows dense; flags i32[B].
 *   table is a HOST array i64[B,14], one row per image, with the columns (hip_lib.REPLACE_BG_COLUMNS)
 *     0  do        0: the image and its mask_trunc are left untouched, the rest of the row is not read
 *     1  bg_off    byte offset of the background image in bg
 *     2  bg_stride its row length in pixels
 *     3  x0        4  y0     origin of the crop in that image
 *     5  cw        6  ch     size of the crop
 *     7  dw        8  dh     size the crop is resized to; pasted top-left on zeros, so dw <= W and dh <= H
 *     9  mode      0 copy (dw x dh == cw x ch), 1 the 2:1 area mean, 2 linear: OpenCV's forms of an 8-bit INTER_LINEAR cv2.resize
 *    10  scale_x  11  scale_y   the bits of an fp64: OpenCV's interpolation scale, 1 / fx for cv2.resize(im, None, None, fx, fy) and
 *                  1 / (dst / src) for cv2.resize(im, dsize); the host's arithmetic, the kernel derives none (mode 2 only)
 *    12  cut       0 none, 1 block upper, 2 block bottom, 3 block left, 4 block right (trunc_mask's branches)
 *    13  u         the bits of an fp64 in [0, 1): the random.random() behind trunc_mask's random.uniform (cut != 0 only)
 * Every value the kernels index with is checked here, before the table is staged into the workspace in one copy: a crop that leaves its
 * image or bg, dw > W, dh > H, a copy or area mean whose sizes do not agree, a mode, cut, scale or u out of range return GDRNPP_EINVAL
 * naming the row, and nothing is launched.  H, W < 32768 and B <= 65535, or GDRNPP_ELIMIT.  B = 0 succeeds and launches nothing.
 *   Phase 1 (images with a cut): the extents x1 <= x2 (rows) and y1 <= y2 (columns) of the non-zero mask bytes, by atomicMin / atomicMax.
 * Phase 2, per pixel (r, c): line = int(lo + (hi - lo) u) in fp64, nothing contracted, with (lo, hi) = (x1, c_h), (c_h, x2), (y1, c_w),
 * (c_w, y2) for cuts 1..4, c_h = 0.5 (x1 + x2), c_w = 0.5 (y1 + y2); keep = mask != 0, and r >= line, r < line, c >= line, c < line for
 * cuts 1..4; mask_trunc = keep; where !keep the pixel becomes the resized crop's pixel at (r, c) if r < dh and c < dw, else 0.  An empty
 * mask under a cut (the reference raises in np.min) sets flags[b] = 1 and the cut is skipped; every other flags[b] is written 0.
 * workspace: gdrnpp_replace_bg_workspace_bytes(B) bytes of device memory, 8-byte aligned, used by this call alone. */
size_t gdrnpp_replace_bg_workspace_bytes(int B);
int gdrnpp_replace_bg(unsigned char* images, const unsigned char* masks, unsigned char* mask_trunc, int B, int H, int W,
                      const unsigned char* bg, long long bg_bytes, const long long* table, int* flags, void* workspace,
                      size_t workspace_bytes, void* stream);

/* ---- YOLOX training batches (csrc/yolox_aug.hip) — the pixel work of `MosaicDetection.__getitem__`
 * (det/yolox/data/datasets/mosaicdetection.py) over `TrainTransform` (det/yolox/data/data_augment.py) for B items in one call: mosaic,
 * cv2.warpAffine, mixup, augment_hsv, mirror, preproc.  Device pointers: src, src_bytes bytes holding the decoded source images, u8 HWC,
 * 3 bytes per pixel, rows dense; lut u8[B,2,3,256], the (hue, saturation, value) LUTs of HSV pass 1 and pass 2; out f32[B,3,H,W], integer
 * values 0..255; flags i32[B].
 *   table is a HOST array i64[B,85], one row per item, with the columns (hip_lib.YOLOX_AUG_COLUMNS)
 *     0  branch    0 plain (source 0 through TrainTransform), 1 mosaic, 2 mosaic + mixup
 *     1  flags     1 HSV pass 1, 2 pass 1 reads RGB (else BGR), 4 mirror, 8 fallback (TrainTransform kept no box and re-ran
 *                  preproc(image_o): pass 1 and the mirror are dropped), 16 HSV pass 2, 32 pass 2 reads RGB, 64 mixup flip
 *     2..7  m00 m01 m02 m10 m11 m12   the bits of six fp64: the affine matrix handed to cv2.warpAffine (branches 1, 2)
 *     8  mix_w     9  mix_h      size of the second, jittered resize of the H x W cp canvas (branch 2)
 *    10  mix_mode  11 mix_scale_x  12 mix_scale_y   its form and scales, as for a source
 *    13  mix_x_off 14 mix_y_off  origin of the H x W crop of the zero-padded, jittered image
 *    15 + 14 k ..  source k = 0..3: the mosaic tiles in paste order (branch 0 reads source 0 only); k = 4: the mixup image
 *      +0 off      byte offset of the image in src        +1 w   +2 h   its size
 *      +3 dw  +4 dh   size it is resized to      +5 mode   0 copy, 1 the 2:1 area mean, 2 linear: OpenCV's forms of an 8-bit cv2.resize
 *      +6 scale_x  +7 scale_y   the bits of an fp64: OpenCV's interpolation scale 1 / (dst / src) (mode 2 only)
 *      +8 l_x  +9 l_y   where the paste lands on its canvas      +10 s_x  +11 s_y   where it starts in the resized image
 *      +12 pw  +13 ph   size of the pasted rectangle (0: nothing is pasted)
 * The host does all size arithmetic and the affine matrix in the reference's Python floats; the kernels derive none.  Every value the
 * kernels index with is checked here before the table is staged into the workspace in one copy: an image outside src, a paste outside
 * its canvas (2W x 2H for the tiles, W x H for source 4 and the plain branch, whose paste is whole and top-left), sizes that do not fit
 * their form, an offset outside the padded image, a matrix whose inverse leaves the fixed-point range return GDRNPP_EINVAL naming the
 * row, and nothing is launched.  H, W <= 16383 and B <= 65535, or GDRNPP_ELIMIT.  B = 0 succeeds and launches nothing.
 *   The matrix is inverted here as cv::warpAffine does; the tap coordinates are those of gdrnpp_crop_resize's warp (10-bit fixed point,
 * 5 fractional bits), the 8-bit bilinear weights are integers of 15 bits, and a tap outside the canvas reads 114.  Mixup blends
 * uint8(0.5f a + 0.5f b).  An HSV pass is 8-bit RGB -> HSV in integers (hue range 180), the three LUTs, and HSV -> RGB in fp32 with every
 * operation rounded on its own.  flags[b] = 1 where the matrix was singular (OpenCV then warps with a zero map), else 0.
 * workspace: gdrnpp_yolox_train_inputs_workspace_bytes(B, H, W) bytes of device memory, 16-byte aligned, used by this call alone. */
size_t gdrnpp_yolox_train_inputs_workspace_bytes(int B, int H, int W);
int gdrnpp_yolox_train_inputs(const unsigned char* src, long long src_bytes, const long long* table, const unsigned char* lut, int B, int H,
                              int W, float* out, int* flags, void* workspace, size_t workspace_bytes, void* stream);

/* device-to-device copy into a raw device pointer on `stream` — the transfer CppEGLRenderer::map_tensor performs with
 * cudaMemcpy2DFromArray in the reference (lib/egl_renderer/cpp/egl_renderer.cpp:262-298): attachment -> caller's tensor */
int gdrnpp_copy_d2d(void* dst, const void* src, size_t bytes, void* stream);

/* debug aid: PMC calibration stream — reads n floats with 4- or 16-byte lanes (a known byte count) */
int gdrnpp_debug_stream_read(const float* p, size_t n, int lane_bytes, float* out_blocks,
                             int blocks, void* stream);

/* debug aid: ONE wave busy-waits `micros` microseconds of the device's constant-rate wall clock on `stream` and computes nothing — the
 * probe engine.streams_overlap_ratio launches on two streams to learn whether they sit on different hardware queues (replaces
 * the private torch.cuda._sleep).  1 <= micros <= 1 000 000. */
int gdrnpp_debug_spin(int micros, void* stream);

/* debug aid: 16 s_memtime stamps written by workgroup 0 of the last gdrnpp_depth_refine launch (LDS-staged
 * kernel): [0] start, [1] prologue, then per iteration staged/rastered/reduced/median/updated. Host pointer. */
int gdrnpp_debug_refine_profile(long long* h_out16);

/* ---- network-side layers of GDRN_Net (a3), NHWC fp32 ----------------------------------------
 * Memory-bound layers that PyTorch-ROCm runs far from the HBM roofline: all tensors are
 * channels-last (N,H,W,C contiguous), C % 4 == 0.
 *  dwconv7x7_ln : timm ConvNeXtBlock.conv_dw (depthwise 7x7, pad 3) + bias, fused with the LayerNorm(C, eps)
 *                 that follows it when ln_w/ln_b are non-NULL.  w49c f32[49,C] = weight[C,1,7,7] tap-major.
 *  upsample_bilinear2x : nn.UpsamplingBilinear2d(scale_factor=2) (align_corners=True) of the geometry head
 *                 (top_down_doublemask_xyz_region_head.py:80).
 *  groupnorm_act : nn.GroupNorm(G, C, eps) [+ exact-erf GELU] of ConvModule / ConvPnPNet
 *                 (lib/torch_utils/layers/conv_module.py:222-236, conv_pnp_net.py:59-72); workspace sized by
 *                 gdrnpp_groupnorm_workspace_bytes.
 *  layernorm    : LayerNorm over C of n_pix NHWC pixels (timm LayerNorm2d of the ConvNeXt stem and downsample
 *                 layers): biased variance, eps inside the sqrt. */
int gdrnpp_layernorm_nhwc(const float* x, const float* weight, const float* bias, float* y,
                          long n_pix, int C, float eps, void* stream);
int gdrnpp_dwconv7x7_ln_nhwc(const float* x, const float* w49c, const float* bias,
                             const float* ln_w, const float* ln_b, float* y, int N,
                             int H, int W, int C, float eps, void* stream);
/* ... with y written as an "f16x2 rows" tensor when y_rows != 0 (C % 8 == 0; see gdrnpp_linear_f32_split2_rows): the block's
 * LayerNorm output then reaches fc1 already split. */
int gdrnpp_dwconv7x7_ln_nhwc_rows(const float* x, const float* w49c, const float* bias,
                                  const float* ln_w, const float* ln_b, float* y, int N,
                                  int H, int W, int C, float eps, int y_rows, void* stream);
/* Backward of dwconv7x7 + LayerNorm (ln_w non-NULL) for grad_y = dL/dy f32[N,H,W,C]: dx f32[N,H,W,C], dw f32[C,49] (the layout
 * of conv.weight [C,1,7,7], not tap-major), db, dln_w, dln_b f32[C].  u and the LayerNorm statistics are recomputed from x
 * with the forward's own fma chain; nothing of the forward is kept.  An output given as NULL is not computed, and the pass
 * that only it needs is not launched (dx: one pass, dw: one pass).  No atomics: partial sums go to fixed slots of the
 * workspace, whose count depends on the shape alone, and are added in slot order in fp64 — two calls give equal bits.
 * workspace: gdrnpp_dwconv7x7_ln_backward_workspace_bytes(N,H,W,C) bytes, 16-byte aligned = one f32[N,H,W,C] (du) +
 * at most 512 x 3C + 64 x 49C doubles; 0 for a shape the kernels do not take (C % 4, C / 4 no power of two <= 256). */
size_t gdrnpp_dwconv7x7_ln_backward_workspace_bytes(int N, int H, int W, int C);
int gdrnpp_dwconv7x7_ln_backward(const float* x, const float* w49c, const float* bias, const float* ln_w,
                                 const float* grad_y, float* dx, float* dw, float* db, float* dln_w,
                                 float* dln_b, int N, int H, int W, int C, float eps, void* workspace,
                                 size_t workspace_bytes, void* stream);
/* Training kernels of the ConvNeXt stem and downsample layers (csrc/backbone_bwd.hip).  No atomics: partial sums go to fixed slots
 * of the workspace, whose count depends on the shape alone, and are added in fp64 in a fixed order — two calls give equal bits.
 *  stem_conv4x4_ln_backward : the parameter gradients of gdrnpp_stem_conv4x4_ln for grad_y = dL/dy f32 NHWC [N,H/4,W/4,128]: dw
 *                 f32[128,3,4,4], db, dln_w, dln_b f32[128]; an output given as NULL is not computed (dw NULL: the kernel without its
 *                 matrix instructions).  The pre-norm activation and the LayerNorm statistics are recomputed from x with the forward's
 *                 own fma chain in (ci, ky, kx) order, carried in fp64; du, the LayerNorm backward of grad_y, stays in LDS; x and grad_y are read once.
 *                 dw = du^T patches(x), [128 x M] [M x 48] with M = N H/4 W/4, on the exact-f32 matrix instruction with
 *                 gemm_tn_f32's sums: fp32 chains of 32 rows (at most 128 is that kernel's rule) carried in fp64, the rows dealt to at
 *                 most 256 slots (256-row chunks), an fp64 finalize.  ln_w == NULL: no LayerNorm, du = grad_y (weight and bias are then not read, dln_w and
 *                 dln_b must be NULL).  bias may be NULL.  The gradient with respect to x is not formed.  Shapes of the forward:
 *                 H % 4 == 0, W % 16 == 0, W <= 1024, Cout = 128.  workspace: gdrnpp_stem_conv4x4_ln_backward_workspace_bytes(N,H,W,Cout)
 *                 bytes (slots x 6528 doubles), 16-byte aligned; 0 for a shape outside the kernel.
 *  layernorm_patch2x2_nhwc : x f32 NHWC [N,H,W,C] -> A f32[N H/2 W/2, 4 C], row = output pixel of a 2x2 / stride 2 convolution, column
 *                 = (ky, kx, ci): the values of gdrnpp_layernorm_nhwc bit for bit, stored in patch order.  ln_w == ln_b == NULL: the
 *                 space-to-depth copy alone.  H, W even; C = 128, 256, 512 or 1024; N H W < 2^31 - 4096.  Every pointer of this and of
 *                 the next entry point 16-byte aligned.
 *  layernorm_patch2x2_backward : its adjoint for dA in the same layout: dx f32 NHWC, dln_w, dln_b f32[C] (each may be NULL), the
 *                 statistics recomputed from x in fp64.  ln_w == NULL: the inverse copy (dx alone; x is not read, no workspace).
 *                 workspace: gdrnpp_layernorm_patch2x2_backward_workspace_bytes(N,H,W,C) bytes (at most 512 x 2 C doubles), 16-byte
 *                 aligned; 0 for a shape outside the kernel. */
size_t gdrnpp_stem_conv4x4_ln_backward_workspace_bytes(int N, int H, int W, int Cout);
int gdrnpp_stem_conv4x4_ln_backward(const float* x_nchw, const float* weight, const float* bias, const float* ln_w,
                                    const float* grad_y, float* dw, float* db, float* dln_w, float* dln_b, int N, int H,
                                    int W, int Cout, float eps, void* workspace, size_t workspace_bytes, void* stream);
int gdrnpp_layernorm_patch2x2_nhwc(const float* x, const float* ln_w, const float* ln_b, float* A, int N, int H, int W,
                                   int C, float eps, void* stream);
size_t gdrnpp_layernorm_patch2x2_backward_workspace_bytes(int N, int H, int W, int C);
int gdrnpp_layernorm_patch2x2_backward(const float* x, const float* ln_w, const float* dA, float* dx, float* dln_w,
                                       float* dln_b, int N, int H, int W, int C, float eps, void* workspace,
                                       size_t workspace_bytes, void* stream);
/* Backward of the ConvNeXt MLP tail y = s + gamma (.) (gelu(x W1^T + b1) W2^T + b2) (csrc/mlp_bwd.hip): the kernels beside
 * gdrnpp_linear_f32_split, which runs the two data-gradient products dh = g (diag(gamma) W2) and dx = dpre W1 as it is.
 *  pack_weight_bf16x3_t : the image gdrnpp_pack_weight_bf16x3 makes of T = (diag(row_scale) W)^T, f32[K,R], read from W f32[R,K]
 *                 (row_scale f32[R] or NULL; K % 128 == 0, R % 32 == 0): byte for byte that of the transposed, scaled copy.
 *  gelu_f32     : h = gelu(pre), n elements (n % 4 == 0), with the function of the split GEMMs' GELU epilogue.
 *  colsum_f32   : column sums of x f32[M,cols] (cols % 4 == 0) in fp64 through fixed partial slots: sum64[cols] (fp64) and / or
 *                 sum32[c] = fl(scale[c] sum[c]) (scale f32[cols] or NULL).  workspace: gdrnpp_colsum_workspace_bytes(M, cols) bytes
 *                 (at most 256 x cols doubles), 16-byte aligned.
 *  mlp_bwd_act  : one pass over [M,cols]: dh_dpre holds dh on entry and dpre = dh gelu'(pre) on return, gelu'(x) = Phi(x) +
 *                 x phi(x); h (or NULL) receives gelu(pre), recomputed; db1 (or NULL) f32[cols] the column sums of dpre.  The
 *                 workspace of colsum_f32.
 *  gemm_tn_f32  : G[N1,N2] = sum_m A[m,N1] B[m,N2], A f32[M,N1], B f32[M,N2] row-major, N1 % 128 == 0, N2 % 128 == 0, any M >= 1,
 *                 on the exact-f32 matrix instruction.  fp32 chains of at most 128 rows are carried in fp64; the rows are dealt to at
 *                 most 64 slots (512-row chunks; no more slots than bring the grid to 512 workgroups; the count from the shape
 *                 alone) whose fp64 tiles the finalize adds in slot order and
 *                 rounds once: no atomics, two calls give equal bits.  row_scale (f32[N1] or NULL): G[c,:] = fl(row_scale[c] sum).
 *                 drow (f32[N1] or NULL; needs W f32[N1,N2], b f32[N1], sg f64[N1]): drow[c] = fl(sum_k W[c,k] sum[c,k] + b[c]
 *                 sg[c]) from the fp64 sums — the layer-scale gradient.  G may be NULL when drow is asked for.  workspace:
 *                 gdrnpp_gemm_tn_f32_workspace_bytes(M, N1, N2) bytes (slots x N1 x N2 doubles), 16-byte aligned; 0 for a shape
 *                 outside the kernel. */
 /* linear_f32_exact : out[M,N] = epilogue(A[M,K] Bop) on the exact-f32 matrix instruction with gemm_tn_f32's sums (fp32 chains of 128,
 *                 fp64 carries, one rounding): the deep products of the tail (K >= 512), where the six-product kernel's fp32
 *                 accumulation is past twice a CPU sgemm's error.  b_is_nk != 0: B f32[N,K] (an nn.Linear weight, out = A B^T);
 *                 else B f32[K,N], times row_scale[k] (f32[K] or NULL).  bias f32[N] or NULL; gamma f32[N] and resid f32[M,N]
 *                 together or both NULL: out = resid + gamma (sum + bias).  N % 128 == 0, K % 32 == 0, any M >= 1.  A launch
 *                 with fewer than 256 output tiles cuts K into slots (multiples of 128, their count from the shape alone) whose
 *                 fp64 tiles a finalize adds in slot order: workspace of gdrnpp_linear_f32_exact_workspace_bytes(M, N, K) bytes
 *                 (slots x M x N doubles; 0 with one slot, and the workspace may then be NULL), 16-byte aligned. */
size_t gdrnpp_linear_f32_exact_workspace_bytes(int M, int N, int K);
int gdrnpp_linear_f32_exact(const float* A, const float* B, int b_is_nk, const float* row_scale, const float* bias,
                            const float* gamma, const float* resid, float* out, int M, int N, int K, void* workspace,
                            size_t workspace_bytes, void* stream);
int gdrnpp_pack_weight_bf16x3_t(const float* W, const float* row_scale, void* packed, int R, int K, void* stream);
int gdrnpp_gelu_f32(const float* pre, float* h, size_t n, void* stream);
size_t gdrnpp_colsum_workspace_bytes(long M, int cols);
int gdrnpp_colsum_f32(const float* x, const float* scale, double* sum64, float* sum32, long M, int cols,
                      void* workspace, size_t workspace_bytes, void* stream);
int gdrnpp_mlp_bwd_act(const float* pre, float* dh_dpre, float* h, float* db1, long M, int cols,
                       void* workspace, size_t workspace_bytes, void* stream);
size_t gdrnpp_gemm_tn_f32_workspace_bytes(int M, int N1, int N2);
int gdrnpp_gemm_tn_f32(const float* A, const float* B, float* G, int M, int N1, int N2, const float* row_scale,
                       const float* W, const float* b, const double* sg, float* drow, void* workspace,
                       size_t workspace_bytes, void* stream);
int gdrnpp_upsample_bilinear2x_nhwc(const float* x, float* y, int N, int H, int W,
                                    int C, void* stream);
size_t gdrnpp_groupnorm_workspace_bytes(int N, int HW, int G);
int gdrnpp_groupnorm_act_nhwc(const float* x, const float* gamma, const float* beta,
                              float* y, void* workspace, int N, int HW, int C, int G,
                              float eps, int act_gelu, void* stream);

/* ---- ROI crop-resize (a1) — read_data_test, data_loader.py:754-797 ---------------------------------
 * cv2.warpAffine restated (data_utils.py:115-184): images u8[n_im,H,W,3] (BGR), depths f32[n_im,H,W] or NULL,
 * im_idx i32[b] (NULL = image 0), centers f64[b,2] = bbox centre, scales f64[b] (float64 like the reference's
 * call site) -> roi_img f32[b,3,out,out] = (bilinear u8 - mean[c]) / std[c] (float64 math, float32 store);
 * roi_depth f32[b,1,out,out] (nearest); roi_coord2d f32[b,2,out_small,out_small] = bilinear crop of the
 * analytic coord_2d map.  Any output pointer may be NULL.  h_mean3/h_std3 are HOST pointers to 3 doubles
 * (MODEL.PIXEL_MEAN / PIXEL_STD). */
int gdrnpp_crop_resize_roi(const unsigned char* images, const float* depths, int n_im,
                           int H, int W, const int* im_idx, const double* centers,
                           const double* scales, float* roi_img, float* roi_depth,
                           float* roi_coord2d, int b, int out_res, int out_res_small,
                           const double* h_mean3, const double* h_std3, void* stream);

/* ---- ROIAlign crop-resize (a1b) — detectron2 ROIAlign(output_size, spatial_scale, sampling_ratio, aligned)
 * as called at core/utils/data_utils.py:65-112 and core/utils/zoom_utils.py:80-96.
 * x f32[B,C,H,W] (NCHW), rois f32[N,5] = (batch idx, x1, y1, x2, y2) -> out f32[N,C,pooled_h,pooled_w]. */
int gdrnpp_roi_align(const float* x, const float* rois, float* out, int n_rois, int C,
                     int H, int W, int pooled_h, int pooled_w, float spatial_scale,
                     int sampling_ratio, int aligned, void* stream);

/* the "nearest" flavour of batch_crop_resize (core/utils/zoom_utils.py:92-93): torchvision RoIPool(output_size, spatial_scale)
 * forward — max over integer pixel bins, 0 for an empty bin.  Same tensor conventions as gdrnpp_roi_align. */
int gdrnpp_roi_pool(const float* x, const float* rois, float* out, int n_rois, int C, int H, int W, int pooled_h, int pooled_w,
                    float spatial_scale, void* stream);

/* ---- fp32 linear layer with fused epilogue (ConvNeXt Mlp of GDRN_Net, a3) --------------------------------------
 * C[M,N] = A[M,K] * W[N,K]^T + bias[N]; epilogue 0 = none, 1 = exact-erf GELU (timm Mlp.fc1 + act),
 * 2 = resid[M,N] + gamma[N] * C (Mlp.fc2 + layer scale + residual). */

/* ---- fp32-accurate linear layer on the bf16 matrix cores (a3) -------------------------------------------------
 * Every fp32 operand is split EXACTLY into three bf16 values (x = h + m + l);
 * six of the nine partial products (all terms above 2^-26 relative) are accumulated in fp32 by
 * v_mfma_f32_32x32x16_bf16.  Error against an fp64 product is below that of the fp32 fma chain.
 * gdrnpp_pack_weight_bf16x3: W f32[N][K] (nn.Linear weight) -> bf16[N/128][K/16][3][2][128][8]: the three splits
 * (h | m | l) of every 128x16 tile in the order the kernel stages them (split, k-block of 8, row); 6*N*K bytes,
 * done once per weight.  gdrnpp_linear_f32_split: A stays fp32 and is split on the way into LDS.
 * N multiple of 128, K multiple of 32; any M >= 1 (the last row tile is clamped on load and masked on store). */
int gdrnpp_pack_weight_bf16x3(const float* W, void* packed, int N, int K, void* stream);
/* Split-K form for problems with too few output tiles to fill the chip (the Patch-PnP fc layers: one row per ROI,
 * K = 8192; the stage-2/3 ConvNeXt MLPs at small ROI counts): K is cut into chunks so that every CU gets about three
 * workgroups, partial products go to the workspace (gdrnpp_linear_f32_splitk_workspace_bytes) and are summed in a
 * fixed order; bias and the epilogue (0 none, 1 GELU, 2 resid + gamma * y) are applied by the reduction. */
size_t gdrnpp_linear_f32_splitk_workspace_bytes(int M, int N, int K);
int gdrnpp_linear_f32_splitk(const float* A, const void* W_packed, const float* bias, const float* gamma,
                             const float* resid, float* C, int M, int N, int K, int epilogue, void* workspace,
                             size_t workspace_bytes, void* stream);
int gdrnpp_linear_f32_split(const float* A, const void* W_packed, const float* bias, const float* gamma,
                            const float* resid, float* C, int M, int N, int K, int epilogue,
                            void* stream);
/* ConvNeXt stem (timm stem_0 + stem_1): Conv2d(3 -> 128, kernel 4, stride 4) + bias + LayerNorm2d over the channels in one
 * pass.  x f32 NCHW [N,3,H,W] (H % 4 == 0, W % 16 == 0, W <= 1024), weight f32[128,3,4,4], bias f32[128] or NULL ->
 * y f32 NHWC [N,H/4,W/4,128].  fp32 fma chain in (ci, ky, kx) order; LayerNorm as gdrnpp_layernorm_nhwc. */
int gdrnpp_stem_conv4x4_ln(const float* x_nchw, const float* weight, const float* bias, const float* ln_weight,
                           const float* ln_bias, float* y_nhwc, int N, int H, int W, int Cout, float eps, void* stream);
/* Grouped form for the class-sliced 1x1 output layer of the geometry head (GDRN_double_mask.py:107-126 folded into the
 * weights): W_packed_stack holds one gdrnpp_pack_weight_bf16x3 image per group (all [N,K]), bias_stack f32[groups][N];
 * rows [g*rows_per_group, (g+1)*rows_per_group) of A use slice group_sel[g] (device i32[M / rows_per_group]); rows_per_group a
 * multiple of 256 dividing M.  C is f32[M][N]; columns >= n_store (multiple of 4) are not written.  Bias epilogue only.
 * n_groups = slices in the stack: rows whose selector lies outside [0, n_groups) are written as NaN (the reference's
 * t.view(B,C,k,h,w)[arange(B), roi_classes] raises an index error for such a label, GDRN_double_mask.py:107-126; a stream-ordered
 * launch cannot raise, so the result is poisoned instead of read out of bounds). */
int gdrnpp_linear_f32_split_grouped(const float* A, const void* W_packed_stack, const float* bias_stack, const int* group_sel,
                                    int n_groups, int rows_per_group, float* C, int M, int N, int K, int n_store, void* stream);
/* Tail of the geometry head on that NHWC result (GDRN_double_mask.py:128-160, conv_pnp_net.py:120-134): out_nhwc
 * f32[b*hw][pitch] with channels [vis | full (double_mask) | x | y | z | region bg, 1..64] ->
 *   pnp_in f32[b*hw][96] = [(xyz - 0.5) * extent | coord2d (f32[b,2,hw]) | softmax(region[1..64]) | 27 zeros]  (Patch-PnP input, NHWC,
 *          Cin padded to a multiple of 32), planes f32[3 + (double_mask ? 2 : 1)][b*hw] = vis, (full,) x, y, z of out_dict. */
int gdrnpp_head_tail_nhwc(const float* out_nhwc, int pitch, const float* coord2d, const float* extents, float* pnp_in,
                          float* planes, int b, int hw, int double_mask, void* stream);
/* Backward of those two launches for training (csrc/head_tail_bwd.hip).  No atomics; every sum over rows goes through slots whose
 * count depends on the shape alone and is finished in fp64 in index order: two calls give equal bits.
 *
 * Adjoint of gdrnpp_head_tail_nhwc: d_out f32[b*hw][pitch] from out_nhwc (the forward's input: the region softmax is rebuilt from it
 * with the forward's own expression), extents f32[b][3] and any of
 *   g_pnp_in f32[b*hw][96]   gradient of pnp_in (channels 3, 4 and 69..95 — coord2d and the padding — are ignored),
 *   g_planes f32[3 + (double_mask ? 2 : 1)][b*hw]   gradient of planes,
 *   g_out    f32[b*hw][pitch]   a gradient that reached out_nhwc directly (the region map is a view of it); added in.
 * Each may be NULL: it contributes nothing and is not read (out_nhwc and extents are read only with g_pnp_in).  With kx = the first
 * xyz channel and p = softmax(region[1..64]):  d_vis, d_full = their planes;  d_xyz[c] = g_planes[kx + c] + g_pnp_in[c] extent[c];
 * d_region[0] = 0;  d_region[j] = p_j (g_pnp_in[4 + j] - sum_i p_i g_pnp_in[4 + i]) — sums and combination in fp64, one rounding.
 * Columns n_out = kx + 68 .. pitch-1 of d_out are written 0; those columns of g_out are never read.  pitch >= 72, a multiple of 4;
 * hw a multiple of 64. */
int gdrnpp_head_tail_backward_nhwc(const float* out_nhwc, int pitch, const float* extents, const float* g_pnp_in, const float* g_planes,
                                   const float* g_out, float* d_out, int b, int hw, int double_mask, void* stream);
/* Data gradient of gdrnpp_linear_f32_split_grouped:  dfeat[m][0..K) = sum_{c < n_out} d_out[m][c] W[group_sel[m / rows_per_group]][c][:]
 * with W f32[n_slices][n_out][K] — the sliced weight as it lies, no packed image — and d_out f32[M][pitch] read at its pitch; columns
 * >= n_out are never used (they may hold anything).  Exact-f32 matrix instruction, one fp32 chain in column order.  A group whose
 * selector lies outside [0, n_slices) gets NaN rows, as the forward poisons it; nothing is read out of bounds.
 * rows_per_group a multiple of 256 dividing M, K a multiple of 128, n_out <= 72 <= pitch, pitch a multiple of 4. */
int gdrnpp_grouped_linear_dinput_f32(const float* d_out, int pitch, int n_out, const float* W, const int* group_sel, int n_slices,
                                     int rows_per_group, float* dfeat, int M, int K, void* stream);
/* Weight and bias gradient of gdrnpp_linear_f32_split_grouped by slice, written into tensors shaped like the layer's own parameters:
 * for every slice c and channel j < n_out
 *   dW[cls_rows[c][j]][0..K) = sum over the groups r with group_sel[r] == c of  d_out[r]^T feat[r]  (row j),   db[cls_rows[c][j]] =
 *   the column sums of those d_out[r] — groups in index order, each group's row slots in index order, in fp64, rounded once.
 * d_out f32[B*hw][pitch] (columns >= n_out never used), feat f32[B*hw][K], cls_rows device i64[n_slices][n_out] with values in
 * [0, out_rows) (others are skipped), dW f32[out_rows][K] or NULL, db f32[out_rows] or NULL: with both NULL nothing is launched.
 * The rows of a slice no group selects are written 0; groups with a selector outside [0, n_slices) are left out; rows of dW / db
 * outside cls_rows are not written.  The slot count depends on (B, hw, K) alone.  hw a multiple of 256, K of 128, n_out <= 72 <= pitch.
 * workspace: gdrnpp_grouped_linear_wgrad_f32_workspace_bytes (0 = a shape outside the kernel), 16-byte aligned. */
size_t gdrnpp_grouped_linear_wgrad_f32_workspace_bytes(int B, int hw, int K, int n_out);
int gdrnpp_grouped_linear_wgrad_f32(const float* d_out, int pitch, int n_out, const float* feat, const int* group_sel, int n_slices,
                                    const long long* cls_rows, int out_rows, float* dW, float* db, int B, int hw, int K, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* 3x3 / stride 1 / zero-pad 1 convolution of the geometry head (a3) as an implicit GEMM on the same kernel:
 * x f32 NHWC [n_img,H,W,Cin] -> y f32 NHWC [n_img,H,W,Cout]; W_packed = gdrnpp_pack_weight_bf16x3 of the weight
 * reordered to [Cout][ky][kx][Cin] (N = Cout, K = 9*Cin); bias may be NULL; epilogue 0 = none, 1 = GELU.
 * Cout multiple of 128, Cin multiple of 32; any n_img*H*W. */
/* General form: KH x KW taps, stride, symmetric zero padding (pad < KH, KW); W_packed = gdrnpp_pack_weight_bf16x3 of the
 * weight reordered to [Cout][ky][kx][Cin].  Used for the 2x2/2 downsample convolutions of ConvNeXt and the 3x3/2
 * convolutions of Patch-PnP as well.  OH = (H + 2 pad - KH) / stride + 1 (likewise OW); y is [n_img,OH,OW,Cout]. */
int gdrnpp_conv2d_f32_split(const float* x_nhwc, const void* W_packed, const float* bias, float* y_nhwc,
                            int n_img, int H, int W, int Cin, int Cout, int KH, int KW, int stride, int pad,
                            int epilogue, void* stream);
/* Split-K form for launches with too few output tiles for the chip (few ROIs x small maps, K = KH*KW*Cin long): K cut into
 * chunks, partial sums in `workspace` (gdrnpp_conv2d_f32_splitk_workspace_bytes; 0 = the shape runs as one launch and needs
 * none), fixed-order reduction with bias / GELU.  Same arguments and result as gdrnpp_conv2d_f32_split. */
size_t gdrnpp_conv2d_f32_splitk_workspace_bytes(int n_img, int OH, int OW, int Cin, int Cout, int KH, int KW);
int gdrnpp_conv2d_f32_splitk(const float* x_nhwc, const void* W_packed, const float* bias, float* y_nhwc, int n_img, int H, int W,
                             int Cin, int Cout, int KH, int KW, int stride, int pad, int epilogue, void* workspace,
                             size_t workspace_bytes, void* stream);
int gdrnpp_conv3x3_f32_split(const float* x_nhwc, const void* W_packed, const float* bias, float* y_nhwc,
                             int n_img, int H, int W, int Cin, int Cout, int epilogue, void* stream);
/* The ConvModule pair conv3x3 -> GroupNorm of the geometry head (lib/torch_utils/layers/conv_module.py:222-236,
 * top_down_doublemask_xyz_region_head.py:84-107) with the GroupNorm statistics taken in the convolution's epilogue:
 * gn_partials f64[n_img, P, groups, 2] (sum, sum of squares; P = gdrnpp_conv3x3_gnstats_partials(H, W), 0 = shape not
 * supported) is fully written; gdrnpp_groupnorm_apply_nhwc then normalises y (+ affine, optional GELU) from them, the
 * same second pass gdrnpp_groupnorm_act_nhwc runs after its own statistics pass.  Needs H*W % 256 == 0 and
 * Cout == 8 * groups; no activation between convolution and norm. */
/* nn.ConvTranspose2d (the head's first upsampling step, top_down_doublemask_xyz_region_head.py:62-78) = one
 * gdrnpp_linear_f32_split of the NHWC input [n*H*W, Cin] with the weight reordered to [(ky, kx, co), ci]
 * (N = KS*KS*Cout columns) -> cols f32[n, H, W, KS*KS, Cout], then this gather: y f32 NHWC [n, OH, OW, Cout],
 * OH = (H-1)*stride - 2*pad + KS + out_pad; every output pixel adds its <= ceil(KS/stride)^2 taps in (ky, kx) order
 * (+ bias, may be NULL).  Cout % 4 == 0. */
/* y = act(x + bias[c] (+ resid)) over n_pix NHWC pixels of C channels (C % 4 == 0; resid may be NULL; relu 0 / 1; y may be
 * x): the [BatchNorm2d (inference), residual add, ReLU] tail of a ResNet BasicBlock (timm resnet.py BasicBlock.forward)
 * once the BatchNorm is folded into the convolution in front of it (hip_layers.conv_bn_act). */
int gdrnpp_bias_act_nhwc(const float* x, const float* bias, const float* resid, float* y, long n_pix, int C, int relu,
                         void* stream);
int gdrnpp_deconv_col2im_nhwc(const float* cols, const float* bias, float* y, int N, int H, int W, int C, int KS,
                              int stride, int pad, int out_pad, void* stream);
/* the same gather + the GroupNorm(G) statistics of its result (the head's ConvTranspose2d -> GroupNorm -> GELU,
 * top_down_doublemask_xyz_region_head.py:53-75): gn_partials f64[N, P, G, 2] with P = gdrnpp_groupnorm_workspace_bytes(N, OH*OW, G)
 * / (16 N G), bitwise what gdrnpp_groupnorm_act_nhwc's own statistics pass writes; follow with gdrnpp_groupnorm_apply_nhwc.
 * (C / G) % 4 == 0, C / 4 divides 256, G <= 64. */
int gdrnpp_deconv_col2im_gn_nhwc(const float* cols, const float* bias, float* y, double* gn_partials, int N, int H, int W, int C,
                                 int KS, int stride, int pad, int out_pad, int G, void* stream);
/* [nn.UpsamplingBilinear2d(2), conv3x3 / stride 1 / zero pad 1] of the geometry head (top_down_doublemask_xyz_region_head.py:80-107)
 * at the LOW resolution: channel mixing and per-channel interpolation commute, so one gdrnpp_linear_f32_split of the NHWC input
 * [N*H*W, Cin] with the weight reordered to [(ky, kx, co), ci] gives y_taps f32[N, H, W, 9, C] with a quarter of the convolution's
 * matrix work, and this gather writes out f32 NHWC [N, 2H, 2W, C]: per output pixel bias (may be NULL), then taps 0..8, each the
 * align_corners=True interpolation of its tap plane at the neighbouring high-resolution position (nothing where that position is
 * outside 2H x 2W: zero padding applies there).  gn_partials f64[N, P, G, 2], P = gdrnpp_upconv_gather_partials (0 = shape not
 * supported), holds the GroupNorm(G) sums of the result for gdrnpp_groupnorm_apply_nhwc; an image's result and partials do not
 * depend on the other images of the launch.  (C / G) % 4 == 0, C / 4 divides 256, G <= 64. */
int gdrnpp_upconv_gather_partials(int H, int W, int C);
int gdrnpp_upconv_gather_gn_nhwc(const float* y_taps, const float* bias, float* out, double* gn_partials, int N, int H, int W,
                                 int C, int G, void* stream);
int gdrnpp_conv3x3_gnstats_partials(int H, int W);
int gdrnpp_conv3x3_f32_split_gnstats(const float* x_nhwc, const void* W_packed, const float* bias, float* y_nhwc,
                                     double* gn_partials, int n_img, int H, int W, int Cin, int Cout, int groups,
                                     void* stream);
int gdrnpp_groupnorm_apply_nhwc(const float* x, const double* partials, int P, const float* gamma, const float* beta,
                                float* y, int N, int HW, int C, int G, float eps, int act_gelu, void* stream);

/* ---- training the geometry head: backward of [conv3x3, GroupNorm(, GELU)], of the bilinear x2 and of the transposed convolution
 * (csrc/conv_gn_bwd.hip).  The forward-shaped convolutions (the training forward and dx = conv3x3(dz, W')) are
 * gdrnpp_conv_bias_act_f32 below, whose two-level fp32 sums meet the gradient tests' bar at a depth of 2304.
 * All tensors NHWC fp32.  No atomics: every sum over pixels goes through workspace slots whose count depends on the shape alone
 * and is added in slot order in fp64, so two calls give equal bits.  An output given as NULL is not computed, the launches only
 * it needs are left out and the other outputs keep their bits.  Argument errors return GDRNPP_EINVAL / GDRNPP_ELIMIT with
 * gdrnpp_last_error text and launch nothing; every *_workspace_bytes query returns 0 for a shape its kernel does not take.
 *  groupnorm_stats_nhwc : the statistics pass of gdrnpp_groupnorm_act_nhwc alone: gn_partials f64[N, P, G, 2] with P =
 *                 gdrnpp_groupnorm_workspace_bytes(N, HW, G) / (16 N G); follow with gdrnpp_groupnorm_apply_nhwc.  The training
 *                 forward keeps z and these partials for the backward.
 *  groupnorm_act_backward : for y = act(gamma xhat + beta), xhat = (z - mean) rstd over the groups of GroupNorm(G, C, eps), act
 *                 the exact GELU (act_gelu != 0) or nothing, and grad_y = dL/dy: dz f32[N,HW,C], dgamma, dbeta f32[C] (each may be
 *                 NULL, not all).  z is the normalised layer's INPUT and gn_partials / P the forward's partial sums as
 *                 gdrnpp_groupnorm_apply_nhwc takes them: mean and rstd are rebuilt by that kernel's expression, so xhat has the
 *                 forward's bits; neither y nor the pre-activation is kept.  dA = grad_y gelu'(a), gelu'(x) = Phi(x) + x phi(x);
 *                 dbeta = sum dA, dgamma = sum dA xhat, dz = rstd (gamma dA - (s1 + xhat s2) / m) with s1 / s2 the group's sums of
 *                 gamma dA / gamma dA xhat and m = HW C / G.  Shapes of gdrnpp_groupnorm_act_nhwc: C % 4 == 0, (C / G) % 4 == 0,
 *                 C / 4 divides 256, G <= 64, N <= 65535.
 *  conv3x3_wgrad_f32 : dW[co][ci][ky][kx] = sum_{n,y,x} dz[n,y,x,co] x[n,y+ky-1,x+kx-1,ci] (zero outside the image), dW
 *                 f32[Cout,Cin,3,3] contiguous, for dz f32[N,H,W,Cout] and x f32[N,H,W,Cin]; Cin % 128 == 0, Cout % 128 == 0.
 *                 An implicit TN GEMM on the exact-f32 matrix instruction with gdrnpp_gemm_tn_f32's sums: rows are the N H W
 *                 pixels in 512-row chunks dealt to at most min(64, 512 / (9 Cin Cout / 128^2)) slots, fp32 chains of at most
 *                 128 rows carried in fp64, slots added in index order, one rounding.
 *  upsample_bilinear2x_backward_nhwc : the adjoint of gdrnpp_upsample_bilinear2x_nhwc: dx f32[N,H,W,C] from grad_y
 *                 f32[N,2H,2W,C], every input pixel summing the output pixels that read it with the forward's own fp32 index and
 *                 lambda arithmetic, in (row, column) order, in fp64, rounded once.  C % 4 == 0.
 *  deconv_im2col_nhwc : the adjoint of gdrnpp_deconv_col2im_nhwc: dcols f32[N,H,W,KS*KS,C] with dcols[n,h,w,ky,kx,c] =
 *                 dy[n, h stride - pad + ky, w stride - pad + kx, c] or 0 outside dy f32[N,OH,OW,C] (values copied, nothing
 *                 summed).  The transposed convolution's gradients are then two existing products: dx = gdrnpp_linear_f32_exact(dcols,
 *                 Wmat) with Wmat f32[KS*KS*C, Cin], rows (ky, kx, co), and dW = gdrnpp_gemm_tn_f32(x, dcols).  C % 4 == 0. */
int gdrnpp_groupnorm_stats_nhwc(const float* x, double* gn_partials, int N, int HW, int C, int G, void* stream);
size_t gdrnpp_groupnorm_act_backward_workspace_bytes(int N, int HW, int C, int G);
int gdrnpp_groupnorm_act_backward(const float* z, const double* gn_partials, int P, const float* gamma, const float* beta,
                                  const float* grad_y, float* dz, float* dgamma, float* dbeta, int N, int HW, int C, int G,
                                  float eps, int act_gelu, void* workspace, size_t workspace_bytes, void* stream);
size_t gdrnpp_conv3x3_wgrad_f32_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int gdrnpp_conv3x3_wgrad_f32(const float* dz, const float* x, float* dW, int N, int H, int W, int Cin, int Cout, void* workspace,
                             size_t workspace_bytes, void* stream);
int gdrnpp_upsample_bilinear2x_backward_nhwc(const float* grad_y, float* dx, int N, int H, int W, int C, void* stream);
int gdrnpp_deconv_im2col_nhwc(const float* dy, float* dcols, int N, int H, int W, int C, int KS, int stride, int pad, int out_pad,
                              void* stream);

/* ---- training Patch-PnP (ConvPnPNet): backward of the 3x3 / stride 2 / pad 1 convolutions, the NCHW flatten and the two pose heads
 * (csrc/pnp_bwd.hip).  The rules of the section above hold: NHWC fp32, no atomics, fixed summation orders (two calls give equal
 * bits), a NULL output is not computed and its launches are left out, argument errors return GDRNPP_EINVAL / GDRNPP_ELIMIT with
 * gdrnpp_last_error text and launch nothing, a workspace query returns 0 for a shape outside its kernel.  The forward convolution is
 * gdrnpp_conv_bias_act_f32 with ks = 3, stride = 2.
 *  conv3x3s2_wgrad_f32 : dW[co][ci][ky][kx] = sum_{n,oy,ox} dz[n,oy,ox,co] x[n,2oy+ky-1,2ox+kx-1,ci] (zero outside the image), dW
 *                 f32[Cout,Cin,3,3] contiguous, dz f32[N,H/2,W/2,Cout], x = channels [0, Cin) of f32[N,H,W,ldx].  H and W even,
 *                 Cout % 128 == 0; Cin % 128 == 0 with ldx == Cin, or any Cin <= ldx with ldx % 32 == 0 (the channels are padded
 *                 with zeros to a multiple of 128 inside the kernel, whatever x holds beyond Cin, and only the Cin real ones are
 *                 stored).  The sums of gdrnpp_conv3x3_wgrad_f32 with the N H/2 W/2 output pixels as rows; workspace slots x 9 x
 *                 Cin' x Cout doubles, Cin' = Cin rounded up to 128.
 *  conv3x3s2_dinput_f32 : dx[n,y,x,ci] = sum dz[n,oy,ox,co] W[co,ci,ky,kx] over 2oy+ky-1 = y, 2ox+kx-1 = x, by the parity class of
 *                 (y, x): 1, 2, 2 or 4 taps, none for oy = H/2 or ox = W/2.  w f32[9 Cout, ldw], row (ky 3 + kx) Cout + co, column
 *                 ci (ldw % 4 == 0, >= Cin; columns from Cin on are ignored).  dx: channels [0, Cin) of rows of lddx channels, the
 *                 channels [Cin, lddx) written 0; Cin / lddx as Cin / ldx above.  Exact-f32 matrix instruction, the depth in (ky,
 *                 kx, co) order in fp32 chains of 128 carried in fp64, one rounding; the order does not depend on N.
 *  nhwc_flatten_nchw : dst f32[B, C HW] = src f32[B, HW, C] transposed per image (x.flatten(1) of an NCHW tensor held NHWC);
 *                 inverse != 0: dst f32[B, HW, C] from src f32[B, C HW].  Values are copied.
 *  pnp_fc_heads_backward : for rot = feat w_r^T + b_r, t = feat w_t^T + b_t (gdrnpp_pnp_fc_heads) and g_r f32[B,rot_dim], g_t
 *                 f32[B,3] (either may be NULL: no gradient from that head): dfeat f32[B,K] = g_r w_r + g_t w_t, dW_r
 *                 f32[rot_dim,K] = g_r^T feat, dW_t f32[3,K], db_r, db_t the column sums of g; sums over B in index order in fp64,
 *                 one rounding.  Every output may be NULL; the outputs of a head whose source is NULL are written 0.  K <= 1024,
 *                 rot_dim <= 9. */
size_t gdrnpp_conv3x3s2_wgrad_f32_workspace_bytes(int N, int H, int W, int Cin, int ldx, int Cout);
int gdrnpp_conv3x3s2_wgrad_f32(const float* dz, const float* x, int ldx, float* dW, int N, int H, int W, int Cin, int Cout,
                               void* workspace, size_t workspace_bytes, void* stream);
int gdrnpp_conv3x3s2_dinput_f32(const float* dz, const float* w, int ldw, float* dx, int lddx, int N, int H, int W, int Cin, int Cout,
                                void* stream);
int gdrnpp_nhwc_flatten_nchw(const float* src, float* dst, int B, int HW, int C, int inverse, void* stream);
int gdrnpp_pnp_fc_heads_backward(const float* g_r, const float* g_t, const float* feat, const float* w_r, const float* w_t, float* dfeat,
                                 float* dW_r, float* dW_t, float* db_r, float* db_t, int B, int K, int rot_dim, void* stream);

/* ---- three-product form of the split GEMM ("fp16x2"): what hip_layers uses by default for large launches (a3) ----------------
 * Every fp32 operand is written as h + l with h = rn_f16(x), l = rn_f16(x - h): 22 significant bits; the products h*l, l*h, h*h
 * go through v_mfma_f32_32x32x16_f16 with fp32 accumulation — half the matrix work of the six-product form above.  The operand
 * representation costs 1.3e-7 .. 2.2e-7 of the output scale, below the fp32 accumulation error all three engines share on
 * realistic operands: against an fp64 product at K = 128 .. 4096 three products 3.9e-7 .. 3.0e-6, six products 4.8e-7 .. 3.0e-6,
 * hipBLASLt fp32 6.2e-7 .. 3.9e-6 (profiles/r03y_split2_accuracy.txt).  Weights are scaled into the fp16 range by an exact power
 * of two when they are packed
 * (gdrnpp_pack_weight_f16x2: W f32[N][K] -> fp16 [N/128][K/16][2][2][128][8] + a 16-byte trailer holding the scale,
 * gdrnpp_pack_weight_f16x2_bytes(N, K) bytes; conv weights reordered to [Cout][ky][kx][Cin] first, as for bf16x3), activations
 * are split as they are.  Both sides of the fp16 range are checked by every launch and reported in its RANGE WORD (range_flag
 * argument, or the library's own word behind gdrnpp_split2_range_word):
 *   GDRNPP_SPLIT2_NONFINITE   an activation beyond 65504 (or a non-finite input): a stored value or an A element was inf / NaN;
 *   GDRNPP_SPLIT2_SMALL_ROWS  an A row that is not all zero has rms below 2^-4 over its K elements: the low halves fall into the
 *                             fp16 subnormal spacing (absolute operand error 2^-25), i.e. more than 2^-21 of that row's output.
 * On either bit the caller repeats the work in the six-product form (engine.inference_step does, and keeps the flagged layer
 * there).  gdrnpp_pack_weight_f16x2 applies the small-rows test to the scaled weight rows and leaves the verdict in the trailer
 * (word 3 of the 16 bytes behind the tiles: 1 = some non-zero row is below range; such a weight belongs on the six-product form).
 * gdrnpp_linear_f32_split2: as gdrnpp_linear_f32_split (N % 128 == 0, K % 32 == 0, any M, M*K*4 < 4 GiB).
 * gdrnpp_conv3x3_f32_split2: 3x3 / stride 1 / pad 1 convolution over NHWC (Cin % 32 == 0, Cout % 128 == 0), epilogue 0 / 1
 * (bias / bias + GELU); gn_partials != NULL additionally writes the GroupNorm partials of gdrnpp_conv3x3_f32_split_gnstats
 * (epilogue 0, H*W % 256 == 0, Cout == 8 * groups). */
size_t gdrnpp_pack_weight_f16x2_bytes(int N, int K);
int gdrnpp_pack_weight_f16x2(const float* W, void* packed, int N, int K, void* stream);
int gdrnpp_linear_f32_split2(const float* A, const void* W_packed, const float* bias, const float* gamma, const float* resid,
                             float* C, int M, int N, int K, int epilogue, int* range_flag, void* stream);
/* "f16x2 rows": an activation tensor f32[M,K] in which every aligned group of 8 consecutive elements of a row has been replaced,
 * in the same 32 bytes, by its 8 fp16 h halves followed by its 8 fp16 l halves (h = rn_f16(x), l = rn_f16(x - h): the operand
 * split of the three-product kernels).  Same shape, strides and size as the fp32 tensor; only a consumer with the flag can read it.
 * A consumer takes its MFMA operands straight from it instead of splitting every k-tile again for every 128-column tile of the
 * output (K = 512, N = 2048: 16 times per element); a producer pays ~3 VALU operations per element once.  Results are bit-identical
 * to the fp32 hand-over (same conversions), range words unchanged (the consumer still sums the squares of the h halves per row).
 * rows: GDRNPP_A_F16X2_ROWS = A is one (epilogue 1 / 2: the two ConvNeXt MLP layers), GDRNPP_C_F16X2_ROWS = write C as one
 * (epilogue 0 / 1; N % 8 == 0 holds by N % 128 == 0).  Producers: this function, gdrnpp_dwconv7x7_ln_nhwc_rows. */
#define GDRNPP_A_F16X2_ROWS 1
#define GDRNPP_C_F16X2_ROWS 2
int gdrnpp_linear_f32_split2_rows(const float* A, const void* W_packed, const float* bias, const float* gamma, const float* resid,
                                  float* C, int M, int N, int K, int epilogue, int rows, int* range_flag, void* stream);
int gdrnpp_conv3x3_f32_split2(const float* x_nhwc, const void* W_packed, const float* bias, float* y_nhwc, double* gn_partials,
                              int n_img, int H, int W, int Cin, int Cout, int groups, int epilogue, int* range_flag,
                              void* stream);
/* any KH x KW / stride / zero-pad convolution with at most 32 taps (ConvNeXt's 2x2/2 downsamples, Patch-PnP's 3x3/2), epilogue 0 / 1 */
int gdrnpp_conv2d_f32_split2(const float* x_nhwc, const void* W_packed, const float* bias, float* y_nhwc, int n_img, int H, int W,
                             int Cin, int Cout, int KH, int KW, int stride, int pad, int epilogue, int* range_flag,
                             void* stream);
/* ConvNeXt block tail  y = resid + gamma * fc2(gelu(fc1(x)))  (timm ConvNeXtBlock.forward behind conv_dw + norm; the reference's
 * backbone module, core/utils/timm_utils.py:34) for the two shallow stages (C = 128, hidden = 512 and C = 256, hidden = 1024) in ONE
 * launch, three-product form:
 * the hidden tensor never reaches HBM (csrc/gemm_mlp_fused.hip: everything computed transposed, x rows split once and held in
 * registers, the GELU'd accumulator tile IS the second GEMM's operand, weights streamed through LDS once per 256 pixels).
 * W_packed: gdrnpp_pack_mlp_fused_f16x2(fc1.weight f32[hidden,C], fc2.weight f32[C,hidden]) — gdrnpp_pack_mlp_fused_f16x2_bytes(C,
 * hidden) bytes (0 = shape not supported); 32-byte trailer behind the tiles {amax1, 2^-e1, 2^e1, rows1, amax2, 2^-e2, 2^e2, rows2}
 * (rows* = 1: a non-zero weight row of that layer is below the range, the layer belongs on the six-product form).
 * x, resid, y f32[M,C] row-major (NHWC pixels); b1 f32[hidden], b2 / gamma f32[C].  range_flag_fc1 / _fc2: the range words of the
 * two layers, both required (x rows are judged into the first, hidden rows and stored values into the second).  Results equal
 * gdrnpp_linear_f32_split2(gelu) + gdrnpp_linear_f32_split2(scale_res) to fp32 rounding (other k order), not bit for bit. */
size_t gdrnpp_pack_mlp_fused_f16x2_bytes(int C, int hidden);
int gdrnpp_pack_mlp_fused_f16x2(const float* W1, const float* W2, void* packed, int C, int hidden, void* stream);
int gdrnpp_convnext_mlp_f32_fused(const float* x, const void* W_packed, const float* b1, const float* b2, const float* gamma,
                                  const float* resid, float* y, int M, int C, int hidden, int* range_flag_fc1, int* range_flag_fc2,
                                  void* stream);
/* range_flag: device int the launch ORs its range word into (the caller owns, zeroes and reads it — one per layer and stream
 * tells the caller WHICH layer left the range and keeps concurrent users apart); NULL = the library's own word, read (*word) and
 * optionally reset by gdrnpp_split2_range_word (synchronises the stream). */
#define GDRNPP_SPLIT2_NONFINITE 1
#define GDRNPP_SPLIT2_SMALL_ROWS 2
int gdrnpp_split2_range_word(int* word, int reset, void* stream);

/* ---- depth-to-flow (SURVEY §8b boundary "flow") — replaces the flow_cuda torch extension,
 * core/csrc/flow/src/flow_cuda.cpp:30-47 (kernel flow_cuda_kernel.cu:33-64).
 * depth_src, depth_tgt f32[B,1,H,W]; KT f32[B,3,4] = K [R|t] (source -> target); Kinv f32[B,3,3]
 * -> flow f32[B,2,H,W] (channel 0 = dh, 1 = dw), valid f32[B,1,H,W]; both fully written. */
int gdrnpp_flow_forward(const float* depth_src, const float* depth_tgt, const float* KT, const float* Kinv,
                        float* flow, float* valid, int B, int H, int W, void* stream);

/* ---- YOLOX detection post-processing — det/yolox/utils/boxes.py:34-74 (`postprocess`):
 * (cx,cy,w,h) -> corners, class max / first argmax, obj*class_conf >= conf_thre, then torchvision.ops.batched_nms
 * (class_agnostic = 0: boxes offset by class * (max_coordinate + 1)) or nms (class_agnostic = 1), restated.
 * det_preds f32[B,A,5+C] (read only; the reference overwrites its first four columns in place)
 * -> out_dets f32[B,max_det,7] = (x1,y1,x2,y2,obj_conf,class_conf,class) in keep order (descending score, ties by
 * anchor index), out_count i32[B] = number kept (may exceed max_det: only the first max_det rows are written).
 * A <= 16384.  workspace: gdrnpp_yolox_postprocess_workspace_bytes(B, A) bytes of device memory. */
size_t gdrnpp_yolox_postprocess_workspace_bytes(int B, int A);
int gdrnpp_yolox_postprocess(const float* det_preds, int B, int A, int C, float conf_thre, float nms_thre,
                             int class_agnostic, float* out_dets, int* out_count, int max_det,
                             void* workspace, size_t workspace_bytes, void* stream);

/* ---- YOLOX detector forward (det/yolox/models: CSPDarknet + PAFPN + decoupled head), csrc/yolox_net.hip.  All tensors NHWC fp32;
 * a "slice" is `n` channels starting at channel `off` of a buffer whose pixel rows are `ld` channels long.  No atomics, no split
 * over K: every launch is bit-reproducible.
 *
 * gdrnpp_conv_bias_act_f32: c = act(conv(a, w) + bias) + res — implicit GEMM on v_mfma_f32_32x32x2_f32, fp32 accumulation in
 * a fixed two-level order per output (partial sums of about sqrt(K) products, then their sum).  Kernel ks x ks with ks in {1, 3}, stride in {1, 2}, padding (ks - 1) / 2, so
 * OH = (H + 2 pad - ks) / stride + 1 (OW alike).
 *   a    f32[B,H,W,lda], channels a_off .. a_off + cin; cin, lda and a_off multiples of 4.
 *   w    f32[ks*ks*cin, ldw]: row (ky * ks + kx) * cin + ci, column = output channel; ldw a multiple of 4, >= cout (columns
 *        beyond cout are not read into a result).  BatchNorm is folded by the caller.  Any cout: the last N tile may be partial.
 *   bias f32[cout] or NULL.
 *   res  NULL or f32[B,OH,OW,ldr], channels r_off .. r_off + cout, added AFTER the activation; may be the output slice itself.
 *   c    channels c_off .. c_off + cout of rows of ldc channels.  c_img_rows = 0: c is f32[B,OH,OW,ldc] (c_row0 must be 0).
 *        Otherwise c is f32[B,c_img_rows,ldc] and output pixel (oy, ox) of image b is row c_row0 + oy * OW + ox of that image
 *        (a prediction layer writing at its level's anchor offset of det_preds).  Nothing outside the slice is written.
 *        a must not overlap the output slice.
 *   act  GDRNPP_ACT_*.  GDRNPP_ACT_YOLOX_BOX (cout = 4, no res): channel 0 -> (v + ox) * dec_stride, 1 -> (v + oy) * dec_stride,
 *        2 and 3 -> exp(v) * dec_stride (the reference head's decode_outputs on the box columns).
 * Argument errors return GDRNPP_EINVAL / GDRNPP_ELIMIT with gdrnpp_last_error text and launch nothing. */
#define GDRNPP_ACT_NONE 0
#define GDRNPP_ACT_SILU 1
#define GDRNPP_ACT_SIGMOID 2
#define GDRNPP_ACT_YOLOX_BOX 3
int gdrnpp_conv_bias_act_f32(const float* a, int lda, int a_off, const float* w, int ldw, const float* bias, const float* res, int ldr,
                             int r_off, float* c, int ldc, int c_off, long c_img_rows, long c_row0, int B, int H, int W, int cin,
                             int cout, int ks, int stride, int act, float dec_stride, void* stream);
/* Focus stem: x f32[B,3,H,W] (NCHW, H and W even) -> 12 channels at y_off of y f32[B,H/2,W/2,ldy]; channel 3 q + c holds colour c
 * of the 2x2 cell's pixel q = top-left, bottom-left, top-right, bottom-right (the reference's concatenation order). */
int gdrnpp_yolox_focus(const float* x_nchw, float* y, int ldy, int y_off, int B, int H, int W, void* stream);
/* SPP: buf f32[B,H,W,ld]; reads channels off .. off + C and writes their stride-1 max pools with windows 5, 9 and 13 (borders
 * padded with -inf, as nn.MaxPool2d) into channels off + C .., off + 2 C .., off + 3 C ..; off + 4 C <= ld.  One launch, exact. */
int gdrnpp_spp_maxpool_5_9_13(float* buf, int ld, int off, int C, int B, int H, int W, void* stream);
/* Nearest-neighbour x2 upsample of a slice into a slice: x f32[B,h,w,ldx] -> y f32[B,2h,2w,ldy]; C, offsets and row lengths
 * multiples of 4. */
int gdrnpp_upsample_nearest2x_slice(const float* x, int ldx, int x_off, float* y, int ldy, int y_off, int B, int h, int w, int C,
                                    void* stream);

/* ---- the detector's two ends (csrc/yolox_pre.hip) ----
 * gdrnpp_yolox_letterbox: `preproc` of det/yolox/data/data_augment.py:161-177 as ValTransform(legacy=False) uses it.
 * images_u8 u8[B,H,W,3] (BGR, rows of 3 W bytes, no alignment assumed) -> cv2.resize(INTER_LINEAR) to rh x rw placed top-left
 * on a canvas of 114, as float.  rh = int(H r), rw = int(W r) with r = min(Ht / H, Wt / W) are the CALLER's arithmetic (Python
 * floats in the reference); the kernel derives no size.  The resize restates OpenCV's 8-bit path (11-bit coefficients, int
 * horizontal pass, the vertical pass's shifts and rounding, border clamps; rh x rw == H x W is a copy, an exact 2:1 reduction in
 * both axes the area mean).  focus = 0: out f32[B,3,Ht,Wt] (ldy, y_off ignored).  focus = 1: out f32[B,Ht/2,Wt/2,ldy], the 12
 * channels from y_off on exactly as gdrnpp_yolox_focus of the NCHW form writes them (y_off, ldy multiples of 4).
 * Ht, Wt positive multiples of 32, or GDRNPP_EINVAL and no launch. */
int gdrnpp_yolox_letterbox(const unsigned char* images_u8, int B, int H, int W, int rh, int rw, float* out, int Ht, int Wt, int focus,
                           int ldy, int y_off, void* stream);

/* gdrnpp_rois_from_dets: gdrnpp_yolox_postprocess output -> the per-ROI table of the pose path, compacted over the batch.
 * dets f32[B,max_det,7], count i32[B] (values above max_det are clamped), max_det <= 1024.  A detection is dropped when
 * obj_conf * class_conf < score_thr or its class lies outside [0, num_classes); with top_k_per_obj > 0 only the top_k_per_obj
 * highest scores per (image, class) stay (ties: the earlier row) and an image's ROIs come in class order, then descending
 * score; with 0 they keep their order.  Boxes are divided by `ratio` in float, then centre, (bw, bh) clamped to >= 1,
 * scale = min(max(bw, bh) * dzi_pad_scale, max(H, W)) and resize_ratio = out_res / scale in double.  cam f32[3,3]
 * (cam_per_image = 0) or f32[B,3,3]; extents f32[num_classes,3].  Every column of `table` holds `cap` rows; ROIs beyond cap are
 * dropped from the tail.  n_rois i32[1] = rows written, per_image i32[B] = rows of every image; roi_id = the row's index.
 * The struct itself is host memory, its members are device pointers. */
typedef struct gdrnpp_roi_table {
  double* center64;    /* [cap,2] */
  double* scale64;     /* [cap] */
  int* im_idx;         /* [cap] */
  long long* roi_cls;  /* [cap] */
  float* roi_cam;      /* [cap,3,3] */
  float* roi_center;   /* [cap,2] */
  float* roi_wh;       /* [cap,2] */
  float* scale;        /* [cap] */
  float* resize_ratio; /* [cap] */
  float* roi_extent;   /* [cap,3] */
  float* score;        /* [cap] */
  int* roi_id;         /* [cap] */
} gdrnpp_roi_table;
size_t gdrnpp_rois_from_dets_workspace_bytes(int B, int max_det);
int gdrnpp_rois_from_dets(const float* dets, const int* count, int B, int max_det, int num_classes, float ratio, int H, int W,
                          double dzi_pad_scale, int out_res, const float* cam, int cam_per_image, const float* extents,
                          double score_thr, int top_k_per_obj, int cap, const gdrnpp_roi_table* table, int* n_rois, int* per_image,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- instance masks for SAVE_RESULTS_ONLY — gdrn_evaluator.py:914-945:
 * detectron2 paste_masks_in_image(mask_probs, boxes, (im_H, im_W), threshold) + the uncompressed COCO run-length
 * encoding of lib/utils/mask_utils.py:96-109, fused: the full-size masks are never materialised.
 * mask_probs f32[B,mask_h,mask_w]; boxes_xyxy f32[B,4] (x0,y0,x1,y1 = roi_center -/+ scale/2)
 * -> counts u32[B,max_runs] (column-major runs, the first run counts zeros), n_runs i32[B] (> max_runs = overflow:
 * re-run with a larger max_runs; im_H*im_W+1 always suffices). */
int gdrnpp_paste_masks_rle(const float* mask_probs, const float* boxes_xyxy, int B, int mask_h, int mask_w,
                           int im_H, int im_W, float threshold, unsigned* counts, int* n_runs, int max_runs,
                           void* stream);

/* ---- pose record packing for the RCCL all-gather (a13) -------------------
 * rec f32[b,16] = R(9) | t(3) | score | obj_id | roi_id | valid(1) */
int gdrnpp_pack_pose_records(const float* R, const double* t_refined,
                             const float* t_net, const float* score,
                             const int* obj_id, const int* roi_id, float* rec,
                             int b, void* stream);

/* ---- GDRN's training losses (csrc/gdrn_loss.hip) — gdrn_loss of core/gdrn_modeling/models/GDRN_double_mask.py:287-536 ----
 * gdrnpp_gdrn_dense_losses: the terms over the geometry head's maps, one pass.  All maps contiguous NCHW float:
 * out_x / out_y / out_z f32[B,Cx,o,o] (Cx = 1 with xyz_type 0 = L1, 2 <= Cx <= 256 with xyz_type 1 = CE_coor; all three or none),
 * out_mask, out_mask_full f32[B,1,o,o], out_region f32[B,Cr,o,o] (Cr >= 2); a null map = its term is absent (its sum is 0).
 * gt_xyz f32[B,3,o,o] (L1) or gt_xyz_bin u8[B,3,o,o] (CE_coor), gt_region i32[B,o,o], the masks f32[B,o,o] of 0 / 1 (a mask that
 * no selector names may be null).  xyz_mask, mask_gt, region_mask: 0 trunc, 1 visib, 2 obj, 3 full; mask_type, full_type: 0 = L1,
 * 1 = BCE with logits; the full-mask term is always taken against mask_full.
 * sums f64[8] = the numerators of x, y, z, mask, full mask, region, then the pixel counts of the xyz and the region mask:
 *   xyz L1      sum |out m - gt m|                      xyz CE_coor / region   sum of CE(out m, target (long) m) over ALL pixels
 *   mask L1     sum |out - gt|                          mask BCE               sum of max(x,0) - x z + log(1 + exp(-|x|))
 * Per-pixel terms in fp32, accumulation in fp64; per-workgroup partials go to the workspace and are added in workgroup order (no
 * floating-point atomics: equal bits on every run).  A pixel whose mask is 0 contributes log C (its logits are out * 0) and its
 * maps are not read.  bad_targets i32[1] receives the number of (pixel, term) pairs whose masked target lies outside [0, C): such a
 * pixel is left out of the sum.  Argument errors return GDRNPP_EINVAL / GDRNPP_ELIMIT and launch nothing. */
size_t gdrnpp_gdrn_dense_losses_workspace_bytes(int B, int o);
int gdrnpp_gdrn_dense_losses(const float* out_x, const float* out_y, const float* out_z, int Cx, const float* out_mask,
                             const float* out_mask_full, const float* out_region, int Cr, const float* gt_xyz,
                             const unsigned char* gt_xyz_bin, const int* gt_region, const float* mask_trunc, const float* mask_visib,
                             const float* mask_obj, const float* mask_full, int xyz_type, int xyz_mask, int mask_type, int mask_gt,
                             int full_type, int region_mask, int B, int o, double* sums, int* bad_targets, void* workspace,
                             size_t workspace_bytes, void* stream);

/* gdrnpp_gdrn_dense_losses_backward: recomputes from the inputs of the forward and writes, for every non-null grad_*, the gradient of
 *   scale[0..2] x, y, z numerators / max(sums[6], 1) + scale[3] mask / (B o o) + scale[4] full mask / (B o o) + scale[5] region / max(sums[7], 1)
 * with respect to that map (same shape).  sums f64[8]: the forward's result, scale f32[6]: both read on the device.
 * L1: sign(out m - gt m) m s with sign(0) = 0; CE: (softmax - onehot) m s, 0 at a pixel with a target outside [0, C);
 * BCE: (sigmoid(x) - z) s; mask L1: sign(out - gt) s. */
int gdrnpp_gdrn_dense_losses_backward(const float* out_x, const float* out_y, const float* out_z, int Cx, const float* out_mask,
                                      const float* out_mask_full, const float* out_region, int Cr, const float* gt_xyz,
                                      const unsigned char* gt_xyz_bin, const int* gt_region, const float* mask_trunc,
                                      const float* mask_visib, const float* mask_obj, const float* mask_full, int xyz_type, int xyz_mask,
                                      int mask_type, int mask_gt, int full_type, int region_mask, int B, int o, const double* sums,
                                      const float* scale, float* grad_x, float* grad_y, float* grad_z, float* grad_mask,
                                      float* grad_mask_full, float* grad_region, void* stream);

/* gdrnpp_gdrn_pose_losses: the per-ROI terms, one workgroup per ROI, fp64 inside.  R_pred, R_gt f32[B,9]; t_pred, t_gt f32[B,3]
 * (needed with r_only = 0); obj i32[B] into points f32[n_obj,P,3], extents f32[n_obj,3] (null: no PM_NORM_BY_EXTENT) and sym_off
 * i32[n_obj+1] into sym_rots f64[n_sym_total,9] (an empty range: an asymmetric object); pred_t_, gt_trans_ratio, gt_trans f32[B,3]
 * (pred_t_ null: no centroid / z term).  symmetric: R_gt of a ROI is replaced by R_gt S_k of the symmetry with the smallest
 * re(R_pred, R_gt S_k); R_gt itself is the first candidate, the comparison is a strict <, the earliest candidate wins.
 * pm_type 0 L1, 1 Smooth_L1(beta), 2 MSE; z_type 0 REL (gt_trans_ratio[:,2]), 1 ABS (gt_trans[:,2]).
 * sums f64[3] = sum over ROI, point, axis of loss(w (R_pred p [+ t_pred]) - w (R_gt' p [+ t_gt])) with w = 1 / max(extent) or 1,
 * sum |pred_t_[:, :2] - gt_trans_ratio[:, :2]|, sum |pred_t_[:, 2] - gt_z|: per-ROI partials (workspace) added in ROI order.
 * R_gt_sel f32[B,9] (may be null) = R_gt'; dR_pred f32[B,9], dt_pred f32[B,3] = d sums[0] / d R_pred, t_pred (dt_pred 0 with r_only);
 * dpred_t_ f32[B,3] = d sums[1] / d pred_t_[:, :2] and d sums[2] / d pred_t_[:, 2].  A ROI whose obj lies outside [0, n_obj) makes
 * sums[0] NaN and reads nothing. */
size_t gdrnpp_gdrn_pose_losses_workspace_bytes(int B);
int gdrnpp_gdrn_pose_losses(const float* R_pred, const float* R_gt, const float* t_pred, const float* t_gt, const int* obj,
                            const float* points, int n_obj, int P, const double* sym_rots, const int* sym_off, int n_sym_total,
                            const float* extents, const float* pred_t_, const float* gt_trans_ratio, const float* gt_trans, int symmetric,
                            int r_only, int z_type, int pm_type, double beta, int B, double* sums, float* R_gt_sel, float* dR_pred,
                            float* dt_pred, float* dpred_t_, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Ranger optimiser step over every tensor of an optimiser (csrc/ranger.hip) — step() of lib/torch_utils/solver/ranger.py:111-200 ----
 * One launch updates all tensors (a second, earlier launch forms the row means of centralised rows longer than a tile).  Three DEVICE
 * tables, built by the caller:
 *   tensors    one entry per tensor with a gradient: the five f32 arrays of numel elements (slow is touched only with LOOKAHEAD), row_len
 *              = numel / shape[0] where the gradient is centralised (mean over all dimensions but the first subtracted), 0 where not,
 *              and the step's coefficients as fp32: wd_lr = -weight_decay * lr (0 = no decay), step_lr = -step_size * lr.
 *   work       the tensors cut into items of at most GDRNPP_RANGER_TILE elements, one workgroup each.  An item of a centralised tensor
 *              with row_len <= GDRNPP_RANGER_TILE covers whole rows (start and count multiples of row_len) and has mean_slot -1; a longer
 *              row is cut into items that lie inside it, with mean_slot = the row's index in long_rows.  Other tensors: mean_slot -1.
 *   long_rows  the rows longer than a tile; long_means f32[n_long_rows] is scratch for their means.
 * Per element, in fp32 with every product and sum rounded on its own:
 *   g  = nan_to_num(g, 0, 1e5, -1e5) with NAN_TO_NUM, written back to the gradient;  g -= row mean (sum in fp64, fixed order)
 *   v  = v beta2 + ((1 - beta2) g) g;   m = m beta1 + (1 - beta1) g;   p += wd_lr p  (wd_lr != 0)
 *   p += step_lr (m / (sqrt(v) + eps)) with RECTIFIED, p += step_lr m without;   LOOKAHEAD: slow += alpha (p - slow), p = slow.
 * The tables are not validated (they live on the device): an item must lie inside its tensor.  A count above the tile is cut to it. */
#define GDRNPP_RANGER_TILE 12288
#define GDRNPP_RANGER_RECTIFIED 1
#define GDRNPP_RANGER_LOOKAHEAD 2
#define GDRNPP_RANGER_NAN_TO_NUM 4
typedef struct gdrnpp_ranger_tensor {
  float* p;
  float* g;
  float* m;
  float* v;
  float* slow;
  long long numel;
  int row_len;
  int flags;
  float beta1, beta2, one_minus_beta1, one_minus_beta2, eps, alpha, wd_lr, step_lr;
  int reserved[2];
} gdrnpp_ranger_tensor; /* 96 bytes */
typedef struct gdrnpp_ranger_work {
  long long start;
  int tensor;
  int count;
  int mean_slot;
  int reserved;
} gdrnpp_ranger_work; /* 24 bytes */
typedef struct gdrnpp_ranger_long_row {
  long long row;
  int tensor;
  int reserved;
} gdrnpp_ranger_long_row; /* 16 bytes */
int gdrnpp_ranger_step(const gdrnpp_ranger_tensor* tensors, int n_tensors, const gdrnpp_ranger_work* work, int n_work,
                       const gdrnpp_ranger_long_row* long_rows, int n_long_rows, float* long_means, void* stream);

/* ---- ModelEMA update over every floating-point tensor of a model (csrc/model_ema.hip) — update() of det/yolox/utils/ema.py:50-60 and
 * lib/torch_utils/torch_utils.py:247-258 ----
 * One launch updates all (EMA tensor, model tensor) pairs.  Two DEVICE tables, built by the caller once per model; their records are
 * plain little-endian words without padding (csrc/model_ema.hip asserts the layout, hip_lib/net.py builds it):
 *   tensors    24 bytes per pair: float* ema at 0 (the EMA's f32 array, read and written), const float* model at 8 (the model's, read
 *              only), long long numel at 16 (elements of each).
 *   work       16 bytes per item: long long start at 0, int tensor at 8, int count at 12 — the tensors cut into pieces, one workgroup
 *              each.  Pieces of 8192 elements (the kernel's tile, a multiple of 4) take its straight-line path; any count is correct.
 * Per element, in fp32 with every product and the sum rounded on its own (no fused multiply-add):
 *   ema = fadd(fmul(ema, decay), fmul(one_minus_decay, model))
 * which is torch's `v *= d; v += (1.0 - d) * m` on fp32 tensors bit for bit when decay = (float)d and one_minus_decay = (float)(1.0 - d),
 * the subtraction done in double.  The coefficients are arguments: they change with every update, the tables do not.
 * 16-byte accesses where ema + start and model + start are both 16-byte aligned, dword accesses otherwise.
 * The tables are not validated (they live on the device), but nothing outside an EMA tensor is written whatever they say: an item
 * whose tensor index is outside [0, n_tensors) or whose start is outside [0, numel) is skipped, and its count is cut to the tensor's
 * end.  n_work == 0 is a success without a launch. */
int gdrnpp_model_ema_update(const void* tensors, int n_tensors, const void* work, int n_work, float decay, float one_minus_decay,
                            void* stream);

/* ---- YOLOX training (csrc/yolox_loss.hip) — get_losses / get_assignments / get_in_boxes_info / dynamic_k_matching of
 * det/yolox/models/yolo_head.py:256-627 and IOUloss of det/yolox/models/losses.py, for the whole batch with no host round trip ----
 * raw f32[B,A,5+C]: the head's undecoded rows (reg 4, objectness logit, C class logits), levels concatenated in level order, each
 * level row-major.  anchors f32[A,3] = (x_shift, y_shift, stride).  labels f32[B,G,5] = (class, cx, cy, w, h); the gts of an image
 * are its first num_gt rows, num_gt = the number of rows whose five values sum to more than 0 (the reference's rule).
 *
 * gdrnpp_yolox_assign (no gradient): decode xy = (raw + shift) stride, wh = exp(raw) stride; candidates = anchors whose cell centre
 * lies inside any gt box or any gt's 2.5-stride centre square; per (gt, candidate) the IoU of bboxes_iou(xyxy=False) and
 *   cost = sum_c BCE(sqrt(sigmoid(cls_c) sigmoid(obj)), onehot) [logs clamped at -100] + 3 (-log(iou + 1e-8)) + 1e5 [not (in box and in centre)]
 * all in fp32, every product and sum rounded on its own.  Per gt dynamic_k = max(1, int(sum of the 10 largest IoUs)) and the dynamic_k
 * lowest-cost candidates are chosen; an anchor chosen by several gts goes to the argmin of the cost over ALL gts of the image; ties
 * go to the lowest index.  -> matched_gt i32[B,A] (-1 = background), matched_iou f32[B,A] (0 on background), num_fg i32[B],
 * num_gt i32[B].  A gt without any candidate anchor gets no foreground (the reference raises there); a class outside [0, C) has no
 * positive class term (the reference's one_hot raises there).  workspace: gdrnpp_yolox_assign_workspace_bytes(B, A) bytes. */
size_t gdrnpp_yolox_assign_workspace_bytes(int B, int A);
int gdrnpp_yolox_assign(const float* raw, const float* anchors, const float* labels, int B, int A, int C, int G, int* matched_gt,
                        float* matched_iou, int* num_fg, int* num_gt, void* workspace, size_t workspace_bytes, void* stream);

/* gdrnpp_yolox_losses: out f64[6] = loss_iou, loss_conf, loss_l1, loss_cls, num_fg = max(sum of num_fg[b], 1), sum of num_gt[b] with
 *   loss_iou  = 5 sum_fg IOUloss(decoded box, gt box) / num_fg     iou_type 0: 1 - iou^2 (1e-16 in the denominator), 1: giou with its clamps
 *   loss_conf = sum over all anchors of BCEWithLogits(obj, [foreground]) / num_fg
 *   loss_cls  = sum_fg,c BCEWithLogits(cls_c, onehot_c iou of the match) / num_fg     cls_type 1: fvcore's sigmoid_focal_loss(fl_alpha, fl_gamma)
 *   loss_l1   = sum_fg |raw reg - (gt_xy / stride - shift, log(gt_wh / stride + 1e-8))| / num_fg with use_l1, else 0
 * Per-anchor terms in fp64 from the fp32 inputs (the decode and the match's IoU included), per-workgroup partials (workspace) added in
 * a fixed tree and then in workgroup order: equal bits on every run.
 * gdrnpp_yolox_losses_backward: recomputes from the same inputs and writes grad_raw f32[B,A,5+C] = the gradient of
 * scale[0] loss_iou + scale[1] loss_conf + scale[2] loss_l1 + scale[3] loss_cls by raw, the decode's chain rule inside; the match, its
 * IoU and num_fg are constants.  out: the forward's result; scale f32[4]; both read on the device. */
size_t gdrnpp_yolox_losses_workspace_bytes(int B, int A);
int gdrnpp_yolox_losses(const float* raw, const float* anchors, const float* labels, const int* matched_gt, const int* num_fg,
                        const int* num_gt, int B, int A, int C, int G, int iou_type, int cls_type, float fl_alpha, float fl_gamma, int use_l1,
                        double* out, void* workspace, size_t workspace_bytes, void* stream);
int gdrnpp_yolox_losses_backward(const float* raw, const float* anchors, const float* labels, const int* matched_gt, const double* out,
                                 const float* scale, int B, int A, int C, int G, int iou_type, int cls_type, float fl_alpha, float fl_gamma,
                                 int use_l1, float* grad_raw, void* stream);

/* ---- training YOLOX's BaseConv: convolution, BatchNorm2d with batch statistics, SiLU (csrc/conv_bn_bwd.hip) ----
 * The rules of the training sections above hold: NHWC fp32, no atomics, every sum over pixels through workspace slots whose count
 * depends on the shape alone, added in slot order in fp64 and rounded once (two calls give equal bits), a NULL output is not computed
 * and its launches are left out, argument errors return GDRNPP_EINVAL / GDRNPP_ELIMIT with gdrnpp_last_error text and launch
 * nothing, a workspace query returns 0 for a shape outside its kernel.  The forward convolution (act = none, no bias) and the
 * stride-1 data gradient (the flipped, transposed weight) are gdrnpp_conv_bias_act_f32; a convolution bias gradient is
 * gdrnpp_colsum_f32.  M = N OH OW is the number of pixels, C % 4 == 0, C <= 4096.
 *  bn_train_stats_nhwc : mean f32[C] and invstd f32[C] = 1 / sqrt(var + eps) of z f32[M, C] per channel, M >= 2 (M = 1 is an argument
 *                 error, as in PyTorch); the mean and the biased variance are summed in fp64.  running_mean / running_var (each
 *                 may be NULL) are updated in place: r = (1 - momentum) r + momentum (mean | var M / (M - 1)).
 *  bn_silu_apply_nhwc : y = silu(a), a = gamma (z - mean) invstd + beta, a evaluated in fp64 and rounded once.
 *  bn_silu_backward : for grad_y = dL/dy: dA = grad_y silu'(a), silu'(a) = s (1 + a (1 - s)), s = sigmoid(a), with a rebuilt from z by
 *                 the apply kernel's own expression (the forward's bits; neither y nor a is kept); dbeta = sum dA, dgamma = sum dA
 *                 xhat, dz = gamma invstd (dA - dbeta / M - xhat dgamma / M).  dz, dgamma, dbeta may each be NULL, not all.
 *  conv_wgrad_f32 : dW[co][ci][ky][kx] = sum_{n,oy,ox} dz[n,oy,ox,co] x[n, stride oy + ky - pad, stride ox + kx - pad, ci] (zero
 *                 outside the image), dW f32[Cout,Cin,ks,ks] contiguous, dz f32[N,OH,OW,Cout], x f32[N,H,W,Cin]; ks in {1, 3},
 *                 stride in {1, 2}, pad = (ks - 1) / 2, H and W even at stride 2, ANY Cin % 4 == 0 and Cout % 4 == 0.  The sums of
 *                 gdrnpp_conv3x3_wgrad_f32 with the N OH OW output pixels as rows; both channel counts are padded to 128 with zeros
 *                 inside the kernel and only the real elements are stored: workspace slots x ks ks x Cin x Cout doubles, 512-row
 *                 chunks dealt to at most min(64, 512 / (ks ks ceil(Cin / 128) ceil(Cout / 128))) slots.
 *  conv3x3s2_dinput_any_f32 : gdrnpp_conv3x3s2_dinput_f32 for any Cin % 4 == 0, Cout % 4 == 0 and a contiguous dx f32[N,H,W,Cin];
 *                 w f32[9 Cout, Cin], row (ky 3 + kx) Cout + co.  The depth in (ky, kx, co) order, a tap's channels padded to a
 *                 multiple of 32 with zeros, in fp32 chains of 128 carried in fp64, one rounding; the order does not depend on N. */
size_t gdrnpp_bn_train_stats_workspace_bytes(long M, int C);
int gdrnpp_bn_train_stats_nhwc(const float* z, float* mean, float* invstd, float* running_mean, float* running_var, long M, int C,
                               double eps, double momentum, void* workspace, size_t workspace_bytes, void* stream);
int gdrnpp_bn_silu_apply_nhwc(const float* z, const float* mean, const float* invstd, const float* gamma, const float* beta, float* y,
                              long M, int C, void* stream);
size_t gdrnpp_bn_silu_backward_workspace_bytes(long M, int C);
int gdrnpp_bn_silu_backward(const float* grad_y, const float* z, const float* mean, const float* invstd, const float* gamma,
                            const float* beta, float* dz, float* dgamma, float* dbeta, long M, int C, void* workspace,
                            size_t workspace_bytes, void* stream);
size_t gdrnpp_conv_wgrad_f32_workspace_bytes(int N, int H, int W, int Cin, int Cout, int ks, int stride);
int gdrnpp_conv_wgrad_f32(const float* dz, const float* x, float* dW, int N, int H, int W, int Cin, int Cout, int ks, int stride,
                          void* workspace, size_t workspace_bytes, void* stream);
int gdrnpp_conv3x3s2_dinput_any_f32(const float* dz, const float* w, float* dx, int N, int H, int W, int Cin, int Cout, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* GDRNPP_HIP_H_ */
