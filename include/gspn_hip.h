/*
 * gspn_hip.h -- C ABI of libgspn_hip.so: the MI355X (gfx950) implementation of the GSPN /
 * PointNet++ set-abstraction hot path.
 *
 * Drop-in boundary.  Every entry point below replaces one C launcher (or CPU loop) that the
 * reference's TensorFlow OpKernels call; the scalar and pointer order is the reference
 * launcher's, followed by one extra `void* stream` (a hipStream_t; NULL = the null stream).
 * The reference launchers go to the legacy default stream and return void
 * (tf_ops/sampling/tf_sampling_g.cu:194-211); here every call is stream-ordered and returns
 *      0                      success
 *      GSPN_ERR_ARG  (-1)     a size/attribute the reference OP_REQUIRES would reject
 *      GSPN_ERR_UNSUPPORTED   (-2)  valid input outside what this build supports
 *      > 0                    a hipError_t from the launch
 * Nothing throws across the ABI.  No entry point allocates or frees device memory: the caller
 * owns every buffer (as TF's allocate_output/allocate_temp do in the reference).  Gradient
 * entry points zero their output themselves (stream-ordered), replacing the reference's
 * cudaMemset calls (tf_sampling.cpp:174, tf_grouping.cpp:234,307, tf_nndistance_g.cu:153-154).
 * All pointers are device pointers; tensors are dense row-major float32 / int32.
 * Thread safety: the library holds no mutable global state (its tuning hooks only READ the environment).
 */
#ifndef GSPN_HIP_H
#define GSPN_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define GSPN_ERR_ARG (-1)
#define GSPN_ERR_UNSUPPORTED (-2)

/* Build facts: squared-distance contraction policy (see oracle/gspn_oracle.c header) and ABI rev.
 * GSPN_ABI_VERSION is bumped whenever an entry point is added, removed or changes its argument list or workspace layout; a binder
 * compares it with gspn_abi_version() of the library it loaded (gspn_amd/_lib.py raises on a mismatch: a stale .so fails loudly).
 *   1: round 1.   2: round 2 (gspn_fps_background removed, ~30 entry points added, finalize / workspace layouts changed).
 *   3: round 3 (gspn_sa_rel_shift, gspn_bn_apply, gspn_mlp_gemm_*, status word of the multi-CU FPS checked).
 *   4: round 3 (gspn_mlp_bwd_fused, gspn_mlp_bwd_fused_work_bytes).   5: round 3 (gspn_dense_rsum; the fused launch's pooled form).
 *   6: round 3 (gspn_fps_cells_prepass_order, gspn_bn_colsum / gspn_bn_apply_grad of tf_util's stand-alone batch norm).
 *   8: round 4 (gspn_pool32_select_groups).
 *   7: round 4 (gspn_nmdistance_grad_csr, gspn_bn_finalize_parts_pivot, gspn_mlp_bwd_fused_coef, gspn_dot, gspn_queryballpoint_ws; gspn_queryballpoint now launches a prefix scan + a continuation kernel -- same output).
 *   9: round 6 (the *_ws drop-in gradient launchers, gspn_fp_concat_grad_csr_split).   10: gspn_threenn_nested.
 *  11: gspn_deconv_fwd / gspn_deconv_bwd_input / gspn_deconv_bwd_kernel (+ _work_bytes).
 *  12: gspn_box_shrink / gspn_points_bbox / gspn_spn_target_gen.
 *  13: gspn_nms3d / gspn_box_point_count / gspn_sample_points_in_boxes / gspn_detection_target_select / gspn_crop_gather_grad.
 *  14: gspn_class_nms3d / gspn_nearest_in_sets.
 *  15: gspn_crop_linear_fwd / gspn_crop_linear_bwd_side (+ _part_floats).
 *  16: gspn_crop_mean.
 *  17: gspn_tile_add / gspn_tile_sum (+ _part_floats).
 *  18: gspn_fps_segments (+ _ws_bytes).
 *  19: gspn_scene_confidence / gspn_scene_rank / gspn_sem_iou_counts.
 *  20: gspn_batch_assemble / gspn_adam_tf_flat / gspn_momentum_flat / gspn_scalars_accumulate. */
/* Additive at 20: gspn_instance_overlaps / gspn_instance_match.  Nothing that was there changed, so the number stayed; a binder that wants
 * the two and finds an older library fails at the symbol lookup.
 *  21: gspn_dw_args / gspn_rsum_args; one gspn_mlp_bwd_data (gspn_mlp_bwd_data_cols / _dw / _dw2 / _ex removed); gspn_mlp_bwd_dw and
 *      gspn_mlp_bwd_data_pooltop take the two structs. */
/* Additive at 21: gspn_segment_labels (+ _ws_bytes).  Nothing that was there changed, so the number stayed; a binder that wants the two and
 * finds an older library fails at the symbol lookup.
 * Additive at 21: gspn_sample_points_in_boxes_seeds (a seed per scene; gspn_sample_points_in_boxes keeps its draws bit for bit).
 * Additive at 21: gspn_lift_masks (+ gspn_lift_part_doubles): predictions on a scan's own vertices.
 * Additive at 21: gspn_nearest_point (+ gspn_nearest_point_ws_bytes): exact one-nearest search over a cell grid in global memory.
 * Additive at 21: gspn_segment_vote, gspn_segment_label_vote (+ their _ws_bytes): masks and labels snapped to a scan's segments.
 * Additive at 21: gspn_mask_overlaps, gspn_mask_nms (+ their _ws_bytes): duplicate instance masks suppressed by pairwise IoU.
 * Additive at 21: gspn_mask_components, gspn_mask_component_filter (+ their _ws_bytes): fragments cut off on the mesh dropped from masks.
 * Additive at 21: gspn_mask_hole_fill (+ gspn_mask_hole_fill_ws_bytes): the gaps a mask encloses on the mesh are filled. */
#define GSPN_ABI_VERSION 21
int gspn_dist_policy(void);
int gspn_abi_version(void);
/* Additive at 21: gspn_grid_blocks.  The number of workgroups this build launches for a grid-stride kernel over `total` items in blocks of
 * `block` threads (the capped grid every elementwise and gather / scatter launcher uses); GSPN_ERR_ARG for total < 0 or block < 1. */
long gspn_grid_blocks(long total, int block);

/* ---------------- tf_ops/sampling ---------------------------------------------------- */

/* farthestpointsamplingLauncher(b,n,m,inp,temp,out)  tf_sampling.cpp:94, tf_sampling_g.cu:203-205.
 * inp (b,n,3) f32 -> out (b,m) i32.  temp: the reference's scratch, (32,n) f32 = 128*n bytes (tf_sampling.cpp:111-115).  It is
 * the workspace of the cell kernels below (n >= 8192); required for n > GSPN_FPS_RESIDENT_MAX, may be NULL below that (the plain
 * on-chip kernel then runs: same output, about half the speed at n = 32768). */
#define GSPN_FPS_RESIDENT_MAX 32768
int gspn_farthestpointsampling(int b, int n, int m, const float* inp, float* temp, int* out, void* stream);

/* Same result as gspn_farthestpointsampling, several times fewer serial rounds: FPS on a scene that the caller has sorted into
 * 16 spatial cells (csz = ceil(n/16) points each, Morton order; inside a cell by the reference tie rank (k mod 512, k)):
 *   sxyz (b,n,3) = inp gathered by perm;  perm (b,n) i32: sorted position -> original index;  inp0 (b,3) = original point 0.
 * One wave per cell; exact wave culling by bounding box and several provably-sequential picks per barrier
 * (gspn_amd/csrc/sampling.hip: fps_cell_kernel).  Requires csz <= 2048 (n <= 32768). */
int gspn_fps_cells(int b, int n, int m, int csz, const float* sxyz, const int* perm, const float* inp0, int* out, void* stream);
/* Drop-in for gspn_farthestpointsampling with identical output (n <= 32768): runs the spatial pre-pass (voxel counting sort +
 * per-cell rank sort, two small kernels) and the cell kernel on `stream`.  ws: gspn_fps_cells_ws_bytes(b,n) bytes of scratch. */
long gspn_fps_cells_ws_bytes(int b, int n);
int gspn_farthestpointsampling_cells(int b, int n, int m, const float* inp, void* ws, int* out, void* stream);
/* The two halves of gspn_farthestpointsampling_cells on the same workspace: the spatial pre-pass (counting sort into 16 cells + rank
 * sort inside each cell) and the sampling kernel proper.  Calling them one after the other on one stream equals the combined call.
 * The counting sort places the points of one 16^3 voxel with LDS atomics, so which of them fall on which side of a cell boundary is
 * arbitrary: perm (the first b*n words of ws: sorted position -> original index) is a permutation of 0..n-1 per scene that may differ
 * from call to call between points of one voxel.  `out` does not depend on it (the sampling kernel is exact for every assignment). */
int gspn_fps_cells_prepass(int b, int n, const float* inp, void* ws, void* stream);
/* the same, also leaving the scene's points in 16^3-voxel Morton order in vorder (b, n) int32 (original indices; arbitrary order inside
 * a voxel): a finer spatial order than the 16 cells of ws, for gspn_threenn_ordered. */
int gspn_fps_cells_prepass_order(int b, int n, const float* inp, void* ws, int* vorder, void* stream);
int gspn_fps_cells_sample(int b, int n, int m, const float* inp, const void* ws, int* out, void* stream);

/* Scenes that do not fit one CU (n > 32768; tf_sampling_g.cu:137-141 is the reference's any-n path, data_prep.py:64-83 its caller
 * at n ~ 1e5, m = 30000): the same cell scheme on G workgroups (CUs) per scene, 16*G cells, candidates exchanged between the CUs
 * once per round (gspn_amd/csrc/sampling_multi.hip).  Output identical to gspn_farthestpointsampling.  G = 0 picks the
 * workgroup count measured fastest for the scene size (ceil(n/16384) up to 10, ceil(n/24576) up to 32, ceil(n/32768) beyond); the caller
 * may ask for more (<= 32: smaller cells, but every workgroup lengthens a round's exchange), never for fewer than hold the scene.  Works for any
 * n >= 1 (also below 32768, e.g. one large scene spread over several CUs).  ws: gspn_fps_multi_ws_bytes(b,n) bytes.
 * prepass + sample = the combined call, as for the single-CU cell kernel.  gspn_fps_multi_status synchronises the stream and returns
 * 0, or 1 if a bounded inter-workgroup wait expired (the workgroups of a scene were not co-resident; output invalid). */
long gspn_fps_multi_ws_bytes(int b, int n);
int gspn_fps_multi_prepass(int b, int n, int G, const float* inp, void* ws, void* stream);
int gspn_fps_multi_sample(int b, int n, int m, int G, const float* inp, void* ws, int* out, void* stream);
int gspn_farthestpointsampling_multi(int b, int n, int m, int G, const float* inp, void* ws, int* out, void* stream);
int gspn_fps_multi_status(const void* ws, int b, int n, void* stream);
/* A launch is capped at 128 co-resident workgroups (fewer than 8 scenes per launch beyond G = 16).  The sampling call zeroes `out`
 * before it launches, so after an expired wait every entry is still a valid index (0); the status word -- one int32 at byte offset
 * gspn_fps_multi_status_offset(b, n) of ws -- is then 1.  A caller MUST look at it before trusting `out`: synchronously with
 * gspn_fps_multi_status, or by copying the word asynchronously and checking it at its next synchronisation point (what
 * gspn_amd/tf_sampling.py does: a non-zero word raises GspnHipError there). */
long gspn_fps_multi_status_offset(int b, int n);

/* gatherpointLauncher(b,n,m,inp,idx,out)  tf_sampling.cpp:125, tf_sampling_g.cu:206-208 */
int gspn_gatherpoint(int b, int n, int m, const float* inp, const int* idx, float* out, void* stream);

/* scatteraddpointLauncher(b,n,m,out_g,idx,inp_g)  tf_sampling.cpp:150, tf_sampling_g.cu:209-211.
 * inp_g (b,n,3) is zeroed here first. */
int gspn_scatteraddpoint(int b, int n, int m, const float* out_g, const int* idx, float* inp_g, void* stream);

/* probsampleLauncher(b,n,m,inp_p,inp_r,temp,out)  tf_sampling.cpp:65, tf_sampling_g.cu:198-201.
 * temp: (b,n) floats (the cumulative sums). */
int gspn_probsample(int b, int n, int m, const float* inp_p, const float* inp_r, float* temp, int* out, void* stream);

/* Segmented farthest point sampling: dataset.py:107-118, the resampling of EVERY instance of every scene to m = npoint_ins points, in one
 * fixed set of launches with one workgroup per (scene, group) (gspn_amd/csrc/sampling_segments.hip).  The reference runs
 * farthestpointsamplingKernel once per instance, at b = 1, on the host-compacted cloud curpc[curgroup == j].
 *   pc (b,n,3); order (b,n), offsets (b,g+1) = gspn_inverse_lists of the scenes' group labels over g targets (members of a group in
 *   ascending point index; labels outside [0,g) dropped) -> idx_out (b,g,m) i32 scene indices, pts_out (b,g,m,3) = pc[idx_out],
 *   count_out (b,g) i32 = the group sizes.
 * For group j of scene s with c = offsets[j+1] - offsets[j] members L[k] = order[offsets[j] + k]:
 *   j == 0 (background, :108-109) or c == 0:  idx_out = -1, pts_out = 0
 *   c > m:   the picks of farthestpointsamplingKernel (tf_sampling_g.cu:105-170) on the cloud pc[L[0..c)]: the first pick is k = 0, equal
 *            distances go to the lowest (k mod 512, k) of the COMPACTED position k; idx_out = L[pick]
 *   c == m:  L in order (:114-115)
 *   c < m:   L in order, then draw t = 0..m-c-1 is L[(uint64(gspn_roi_rand32(seed, s, j, t)) * c) >> 32] (:116-118; the reference draws with
 *            np.random.choice, so this stream is this library's own; seed is read from seed_dev as in the ROI stage below)
 * n <= 32768 (GSPN_ERR_UNSUPPORTED beyond; the reference's scans hold at most 30000 points, data_prep.py:65), m >= 1, g >= 1, b * g < 2^31.
 * No host synchronisation and static shapes: the call captures in a graph.  ws: gspn_fps_segments_ws_bytes(b,n,g) bytes, which is 0 in this
 * build (the kernels read an instance through order while they load it; ws may then be NULL). */
long gspn_fps_segments_ws_bytes(int b, int n, int g);
int gspn_fps_segments(int b, int n, int g, int m, const long long* seed_dev, const float* pc, const int* order, const int* offsets, void* ws,
                      int* idx_out, float* pts_out, int* count_out, void* stream);

/* ---------------- tf_ops/grouping ---------------------------------------------------- */

/* queryBallPointLauncher(b,n,m,radius,nsample,xyz1,xyz2,idx,pts_cnt)  tf_grouping.cpp:96,
 * tf_grouping_g.cu:186-189.  Rows without any hit are zero-filled (uninitialised in the reference). */
int gspn_queryballpoint(int b, int n, int m, float radius, int nsample, const float* xyz1, const float* xyz2,
                        int* idx, int* pts_cnt, void* stream);
/* the same with a workspace (gspn_ball_ws_bytes(b, n, m) bytes, 16-byte aligned): on sparse clouds -- a ball holds few points, the
 * reference's scan reads the whole cloud -- the queries are answered through a cell grid over the data points (all hits of the 3 x 3 x 3
 * block around the query's cell, sorted by index); dense clouds and crowded balls take the scan.  Identical output. */
long gspn_ball_ws_bytes(int b, int n, int m);
int gspn_queryballpoint_ws(int b, int n, int m, float radius, int nsample, const float* xyz1, const float* xyz2, void* ws,
                           int* idx, int* pts_cnt, void* stream);

/* Host helper (no GPU work): the squared-distance threshold T the ball-query kernel compares against,
 * i.e. the smallest float with sqrtf(T) >= radius, so that  s < T  <=>  max(sqrtf(s),1e-20f) < radius
 * (tf_grouping_g.cu:27-28) bit-exactly; 0 when radius <= 1e-20f. */
float gspn_ball_threshold(float radius);

/* selectionSortLauncher(b,n,m,k,dist,outi,out)  tf_grouping.cpp:138, tf_grouping_g.cu:190-193 */
int gspn_selectionsort(int b, int n, int m, int k, const float* dist, int* outi, float* out, void* stream);

/* knn_point(k, xyz1, xyz2) of tf_grouping.py:71-96 as ONE call, for 3-D points: the reference composes it in TensorFlow from a dense
 * (b,m,n) squared-distance tensor (:85-87), selectionSortLauncher and a slice (:88-92).  Same val (b,m,k) / idx (b,m,k), ties
 * included, without the matrix (gspn_amd/csrc/knn.hip).  k <= 32 here (GSPN_ERR_UNSUPPORTED beyond: use gspn_selectionsort);
 * k > n is rejected like the slice would be. */
int gspn_knn_point(int b, int n, int m, int k, const float* xyz1, const float* xyz2, float* val, int* idx, void* stream);

/* knn_point (tf_grouping.py:71-96) is composed on the host side exactly as the reference does:
 * dense squared-distance matrix + gspn_selectionsort + slice (see gspn_amd/tf_grouping.py). */

/* groupPointLauncher(b,n,c,m,nsample,points,idx,out)  tf_grouping.cpp:172, tf_grouping_g.cu:194-197 */
int gspn_grouppoint(int b, int n, int c, int m, int nsample, const float* points, const int* idx, float* out, void* stream);

/* groupPointGradLauncher(b,n,c,m,nsample,grad_out,idx,grad_points)  tf_grouping.cpp:203,
 * tf_grouping_g.cu:198-202.  grad_points (b,n,c) is zeroed here first. */
int gspn_grouppoint_grad(int b, int n, int c, int m, int nsample, const float* grad_out, const int* idx, float* grad_points, void* stream);

/* groupMaxpoolLauncher / groupMaxpoolGradLauncher  tf_grouping.cpp:241,277, tf_grouping_g.cu:203-210 */
int gspn_groupmaxpool(int b, int n, int c, int m, int nsample, const float* points, const int* idx, float* out, int* max_idx, void* stream);
int gspn_groupmaxpool_grad(int b, int n, int c, int m, const float* grad_out, const int* max_idx, float* grad_points, void* stream);

/* ---------------- tf_ops/3d_interpolation (CPU-only in the reference) ----------------- */

/* threenn_cpu(b,n,m,xyz1,xyz2,dist,idx)  tf_interpolate.cpp:60-103 */
int gspn_threenn(int b, int n, int m, const float* xyz1, const float* xyz2, float* dist, int* idx, void* stream);
/* the same, with the unknown points handed to the threads in the given order: order (b,n) int32, a permutation of 0..n-1 per scene
 * (e.g. the first b*n words of the workspace gspn_fps_cells_prepass filled for xyz1).  Identical output for every order; a spatially
 * coherent one makes the exact re-evaluations of a wave coincide (8 x 32768 <- 2048: 171 us in the given order, 108 us in the FPS
 * pre-pass order, 81 us in an 8^3 voxel order). */
int gspn_threenn_ordered(int b, int n, int m, const float* xyz1, const float* xyz2, const int* order, float* dist, int* idx, void* stream);
/* three_nn of one query set against L <= 8 subsets of one known cloud in a single scan (ABI 10; gspn_amd/csrc/threenn_nested.hip):
 *   xyz1 (b,n,3), xyz2 (b,m,3), local (L,b,m) i32: the index of known point k inside level l, or -1 if k is not in that level;
 *   order (b,n) i32 or NULL as in gspn_threenn_ordered;  dist (L,b,n,3) f32, idx (L,b,n,3) i32 in each level's own indexing.
 * For every level bit-identical to gspn_threenn(b, n, m_l, xyz1, <the points of level l in local order>, ...), ties included.
 * GSPN_ERR_ARG for L < 1 or negative sizes, GSPN_ERR_UNSUPPORTED for L > 8 or sizes whose grid / row counts overflow an int. */
int gspn_threenn_nested(int b, int n, int m, int L, const float* xyz1, const float* xyz2, const int* local, const int* order, float* dist, int* idx,
                        void* stream);
/* threeinterpolate_cpu(b,m,c,n,points,idx,weight,out)  tf_interpolate.cpp:107-127 */
int gspn_threeinterpolate(int b, int m, int c, int n, const float* points, const int* idx, const float* weight, float* out, void* stream);
/* threeinterpolate_grad_cpu(b,n,c,m,grad_out,idx,weight,grad_points)  tf_interpolate.cpp:131-153;
 * grad_points (b,m,c) is zeroed here first. */
int gspn_threeinterpolate_grad(int b, int n, int c, int m, const float* grad_out, const int* idx, const float* weight, float* grad_points, void* stream);

/* Input matrix of a feature-propagation MLP in one pass -- three_interpolate + tf.concat of utils/pointnet_util.py:161-166
 * (interpolated features FIRST, then points1), written with row pitch ld >= c2+c1 (pad columns zero):
 *   out (b*n, ld);  points2 (b,m,c2), idx/weight (b,n,3), points1 (b,n,c1) or NULL when c1 == 0.
 * gspn_fp_concat_grad: grad_out (b*n, ld) -> grad_points2 (b,m,c2) (zeroed here, then scatter-added: tf_interpolate.cpp:131-153)
 * and grad_points1 (b,n,c1); either output may be NULL. */
int gspn_fp_concat(int b, int n, int m, int c2, int c1, const float* points2, const int* idx, const float* weight,
                   const float* points1, int ld, float* out, void* stream);
int gspn_fp_concat_grad(int b, int n, int m, int c2, int c1, int ld, const float* grad_out, const int* idx, const float* weight,
                        float* grad_points2, float* grad_points1, void* stream);
/* The same gradient without atomics, in the reference's summation order (bit-identical to its sequential loop): `order` (b, 3n) holds the
 * positions p = 3*i + t of the flattened idx array sorted by idx[p] (ties in ascending p), `offsets` (b, m+1) the range of each sparse
 * point in it -- coordinate-only data a caller builds once per batch (gspn_amd/geometry.py: fp_geometry). */
int gspn_fp_concat_grad_csr(int b, int n, int m, int c2, int c1, int ld, const float* grad_out, const int* order, const int* offsets,
                            const float* weight, float* grad_points2, float* grad_points1, void* stream);
/* The same sums with lists longer than split_t entries shared out over the sixteen rows of a workgroup (ABI 9): a fixed order -- run-to-run identical bits -- that
 * DIFFERS from the reference loop's for those lists, so not for three_interpolate's gradient; for internal gathers whose order is this library's own (the transposed
 * aggregation of a pre-aggregated first layer).  On clustered clouds one sparse point is the nearest neighbour of > 1000 dense points.  split_t = 0: as above. */
int gspn_fp_concat_grad_csr_split(int b, int n, int m, int c2, int c1, int ld, const float* grad_out, const int* order, const int* offsets,
                                  const float* weight, float* grad_points2, float* grad_points1, int split_t, void* stream);

/* ---------------- tf_ops/nn_distance -------------------------------------------------- */

/* NmDistanceKernelLauncher(b,n,xyz,m,xyz2,result,result_i,result2,result2_i)  tf_nndistance.cpp:168,
 * tf_nndistance_g.cu:128-131 */
int gspn_nmdistance(int b, int n, const float* xyz, int m, const float* xyz2, float* result, int* result_i,
                    float* result2, int* result2_i, void* stream);
/* NmDistanceGradKernelLauncher(...)  tf_nndistance.cpp:208, tf_nndistance_g.cu:152-157;
 * both gradients are zeroed here first. */
int gspn_nmdistance_grad(int b, int n, const float* xyz1, int m, const float* xyz2, const float* grad_dist1, const int* idx1,
                         const float* grad_dist2, const int* idx2, float* grad_xyz1, float* grad_xyz2, void* stream);
/* The same gradient as a gather through inverse lists (gspn_inverse_lists of idx1 over cloud 2's m points: order1 (b,n), offsets1 (b,m+1);
 * of idx2 over cloud 1's n points: order2 (b,m), offsets2 (b,n+1)): terms added in the order of the reference's sequential CPU twin
 * (tf_nndistance.cpp:126-163) -- bit-identical to it, no memset, no atomics.  Any cloud size. */
int gspn_nmdistance_grad_csr(int b, int n, const float* xyz1, int m, const float* xyz2, const float* grad_dist1, const int* idx1,
                             const float* grad_dist2, const int* idx2, const int* order1, const int* offsets1, const int* order2,
                             const int* offsets2, float* grad_xyz1, float* grad_xyz2, void* stream);

/* ---------------- the four gradient launchers again, WITH a workspace (ABI 9) ----------------
 * The reference's gradient launchers are scatter-adds whose signatures have no slot for scratch memory, so the symbols above that keep those
 * signatures exactly can only scatter with hardware atomics (unordered sums, every gradient row read through an atomic).  The same launchers with
 * ONE more argument before the stream -- `void* ws`, gspn_<op>_ws_bytes(...) bytes, 16-byte aligned (an OpKernel's allocate_temp) -- build the
 * inverse lists of the index tensor in ws (gspn_inverse_lists) and GATHER: every gradient row is read once, sums are formed in a fixed order
 * (ascending position of the flattened index tensor), no atomics, no memset.  Both steps run on the caller's stream; nothing is cached.
 *   gspn_threeinterpolate_grad_ws : bit-identical to the reference's sequential loop (tf_interpolate.cpp:131-153) as compiled by g++
 *   gspn_nmdistance_grad_ws       : terms in the order of the sequential CPU twin (tf_nndistance.cpp:126-163), any cloud size
 *   gspn_grouppoint_grad_ws, gspn_scatteraddpoint_ws : one fixed order where the reference (atomicAdd, tf_grouping_g.cu:66-83,
 *       tf_sampling_g.cu:183-192) defines none.  Rows narrower than 16 floats (coordinates, colours) are FASTER through the atomic symbols;
 *       these are for callers that need run-to-run identical bits.
 * Measured against the plain symbols: profiles/r06_dropin_ws.txt; INTEGRATION.md section B shows the OpKernel side. */
long gspn_grouppoint_grad_ws_bytes(int b, int n, int c, int m, int nsample);
int gspn_grouppoint_grad_ws(int b, int n, int c, int m, int nsample, const float* grad_out, const int* idx, float* grad_points, void* ws, void* stream);
long gspn_scatteraddpoint_ws_bytes(int b, int n, int m);
int gspn_scatteraddpoint_ws(int b, int n, int m, const float* out_g, const int* idx, float* inp_g, void* ws, void* stream);
long gspn_threeinterpolate_grad_ws_bytes(int b, int n, int c, int m);
int gspn_threeinterpolate_grad_ws(int b, int n, int c, int m, const float* grad_out, const int* idx, const float* weight, float* grad_points, void* ws,
                                  void* stream);
long gspn_nmdistance_grad_ws_bytes(int b, int n, int m);
int gspn_nmdistance_grad_ws(int b, int n, const float* xyz1, int m, const float* xyz2, const float* grad_dist1, const int* idx1, const float* grad_dist2,
                            const int* idx2, float* grad_xyz1, float* grad_xyz2, void* ws, void* stream);

/* ---------------- utils/tf_util.py conv2d_transpose (tf.layers.conv2d_transpose, VALID, NHWC) -------------------------------
 * The reference's decoder (model_rpointnet.py:274-322) upsamples with tf_util.conv2d_transpose (tf_util.py:188-267), which runs
 * tf.layers.conv2d_transpose; TensorFlow supplies its arithmetic.  Here (gspn_amd/csrc/deconv.hip) it is three implicit GEMMs on the FP32
 * MFMA, with no im2col buffer:
 *   Ho = hi*sh + max(kh - sh, 0)   (wo alike)
 *   Y[n, oy, ox, co] = bias[co] + sum over (iy, ix, ky, kx) with iy*sh + ky == oy and ix*sw + kx == ox of X[n, iy, ix, ci] * K[ky, kx, co, ci]
 * X (n, hi, wi, cin), K (kh, kw, cout, cin) -- no kernel flip --, bias (cout) or NULL, Y (n, Ho, Wo, cout).  Output pixels that no tap
 * reaches (k < s) hold bias only.  Any sizes >= 1 (GSPN_ERR_ARG below that; GSPN_ERR_UNSUPPORTED when n*Ho*Wo or kh*kw*cin*cout exceeds
 * 2^30, or sh*sw / kh*kw exceeds 65535).  No atomics: every sum has a fixed order, two identical calls give identical bits. */
int gspn_deconv_fwd(int n, int hi, int wi, int cin, int cout, int kh, int kw, int sh, int sw, const float* X, const float* K,
                    const float* bias, float* Y, void* stream);
/* dX (n, hi, wi, cin) = the gradient of Y with respect to X for the upstream gradient dY (n, Ho, Wo, cout); dX is overwritten. */
int gspn_deconv_bwd_input(int n, int hi, int wi, int cin, int cout, int kh, int kw, int sh, int sw, const float* dY, const float* K,
                          float* dX, void* stream);
/* dK (kh, kw, cout, cin) and dbias (cout), both overwritten; either may be NULL (not both).  ws: gspn_deconv_bwd_kernel_work_bytes(...)
 * bytes of scratch (a function of the shape alone; 0 for arguments the launcher rejects) for the split reduction's partial tiles. */
long gspn_deconv_bwd_kernel_work_bytes(int n, int hi, int wi, int cin, int cout, int kh, int kw, int sh, int sw);
int gspn_deconv_bwd_kernel(int n, int hi, int wi, int cin, int cout, int kh, int kw, int sh, int sw, const float* dY, const float* X,
                           float* dK, float* dbias, void* ws, void* stream);

/* ---------------- models/model_rpointnet.py box arithmetic of the shape proposal stage (gspn_amd/csrc/spn_boxes.hip) -------
 * Boxes are (centre x, y, z, size l, w, h).  fp32, no atomics, no workspace; every expression is evaluated as written (no contraction). */

/* box_shrink (:529-551).  box (b,s,6), pc (b,n,3) -> out (b,s,6).  A point is inside a box when pc >= c - size/2 and pc <= c + size/2 on
 * all three axes.  With hi / lo the per-axis max / min over the inside points: out = [(hi + lo)/2, hi - lo + 1e-3] if hi - lo > 0 on all
 * three axes, else six zeros (no point inside, or the inside points flat on an axis).  Equal to the reference's gamma = 1e4 formulation
 * while |coordinate| < 5e3. */
int gspn_box_shrink(int b, int s, int n, const float* box, const float* pc, float* out, void* stream);

/* Per-row bounding box: out[r] = [(hi + lo)/2, hi - lo], hi / lo the max / min over the m points of pts[r] + offset[r].
 * pts (rows,m,3), offset (rows,3) or NULL, out (rows,6).  bbox_ins_pred (:406-408, offset = the seed) and pc_ins_center (:358). */
int gspn_points_bbox(int rows, int m, const float* pts, const float* offset, float* out, void* stream);

/* spn_target_gen (:599-644) for a whole batch, one workgroup per scene.  proposals (b,s,6), seed_cls (b,s) f32 (1 = foreground seed),
 * gt_cls (b,g) f32 (rows with gt_cls <= 0 are padding and skipped in place), gt_boxes (b,g,6) -> spn_match (b,s) i32:
 *   +1  largest IoU >= 0.5 and foreground seed, or the foreground-seed proposal of largest IoU (> 0; ties: lowest index) of a valid box
 *   -1  largest IoU < 0.5 and not positive (every proposal of a scene without a valid box)
 *    0  otherwise.
 * IoU = intersection / (vol_a + vol_b - intersection + 1e-8). */
int gspn_spn_target_gen(int b, int s, int g, const float* proposals, const float* seed_cls, const float* gt_cls, const float* gt_boxes,
                        int* spn_match, void* stream);

/* ---------------- models/model_rpointnet.py ROI stage: from shape proposals to the inputs of the heads (gspn_amd/csrc/roi.hip; gspn_nms3d: nms3d.hip) -------
 * Same rules as the box arithmetic above: fp32, no atomics, no workspace, no host synchronisation, nothing contracted.
 *
 * Random numbers.  A stateless counter-based generator; with 64-bit unsigned arithmetic modulo 2^64 and
 *   mix(z):  z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *   gspn_roi_rand32(seed, scene, a, b) = (uint32)(mix(mix(seed + 0x9E3779B97F4A7C15 * (scene + 1)) ^ ((uint64)a << 32 | b)) >> 32)
 * (the finaliser of splitmix64, twice).  seed is read from ONE int64 on the device (seed_dev), so a captured launch draws afresh on every
 * replay once the caller has added to that word.  A uniform rank below count is (uint64(rand32) * count) >> 32. */

/* nms_3d (:436-466) for a whole batch, one workgroup per scene.  boxes (b,n,6), scores (b,n) -> selected (b,max_output_size) i32, -1 padded.
 * Candidates in descending score, the lower index first among equal scores (the reference's argsort leaves that order open); the first
 * pre_nms_limit of them (all when <= 0) whose score is > score_threshold.  Greedy: the first live candidate is written out, then every live
 * candidate -- the pick included -- with iou > iou_threshold leaves, iou = inter / (((vol_cand + vol_pick) - inter) + 1e-8f), bounds
 * c - s/2 and c + s/2, volume (l*w)*h.  A pick whose own iou does not exceed the threshold (zero volume) is picked again, as in the
 * reference.  n <= 4096. */
int gspn_nms3d(int b, int n, int pre_nms_limit, int max_output_size, float iou_threshold, float score_threshold, const float* boxes,
               const float* scores, int* selected, void* stream);

/* count (b,s) i32: the points of pc (b,n,3) with pc >= (c - s/2) - margin && pc <= (c + s/2) + margin on all axes, per box of boxes (b,s,6)
 * (:673-676 with margin 0, :764-766 with margin 1e-3f). */
int gspn_box_point_count(int b, int s, int n, float margin, const float* boxes, const float* pc, int* count, void* stream);

/* sample_points_within_box (:584-597) from the boxes themselves: idx_out (b,r,nsmp) i32, draw j of box (scene, roi) is the inside point
 * (same test as gspn_box_point_count) of ascending rank (uint64(gspn_roi_rand32(seed, scene, roi, j)) * count) >> 32.  A box without an
 * inside point and an all-zero box give a row of zeros.  n <= 32768. */
int gspn_sample_points_in_boxes(int b, int r, int n, int nsmp, float margin, const long long* seed_dev, const float* boxes, const float* pc,
                                int* idx_out, void* stream);
/* The same with a seed per scene: seeds (b) i64 on the device, and draw j of box (scene, roi) uses gspn_roi_rand32(seeds[scene], 0, roi, j).
 * Row `scene` is therefore what gspn_sample_points_in_boxes gives for that scene alone (b = 1) with the one seed seeds[scene]: a scene's
 * draws do not depend on the batch it is run in or on its slot there (gspn_amd/tester.py batches test scenes on this).  Same kernel, same
 * argument checks and limits. */
int gspn_sample_points_in_boxes_seeds(int b, int r, int n, int nsmp, float margin, const long long* seeds, const float* boxes, const float* pc,
                                      int* idx_out, void* stream);

/* The decisions of detection_target_gen (:662-720) for a whole batch, one workgroup per scene.  proposals (b,s,6), count (b,s) i32 (of
 * gspn_box_point_count, margin 0), gt_cls (b,g) f32 (not read: the reference trims its ground truth by all-zero boxes alone, :664; the
 * caller gathers the class by roi_gt), gt_boxes (b,g,6) -> roi_src, roi_gt (b,rois_per_image) i32.
 * A proposal takes part when it is not an all-zero row and count > 0; a ground-truth box when it is not an all-zero row.  Positive: the
 * largest IoU (as gspn_spn_target_gen) >= 0.5; negative: < 0.5, all of them when no ground-truth box takes part.  Candidate i has the key
 * gspn_roi_rand32(seed, scene, i, 0xFFFFFFFF); the npos = min(P, max_positive) positives of smallest (key, index) fill rows 0..npos-1 in
 * that order, then the min(N, (int)(inv_ratio * (float)npos) - npos) negatives of smallest (key, index), the product in fp32.  roi_src: the
 * proposal of each row, -1 for padding; roi_gt: the ground-truth box of largest IoU (lowest index on ties, untrimmed numbering), -1 for
 * negatives and padding.  Rows past rois_per_image are dropped.  s <= 1024. */
int gspn_detection_target_select(int b, int s, int g, int rois_per_image, int max_positive, float inv_ratio, const long long* seed_dev,
                                 const float* proposals, const int* count, const float* gt_cls, const float* gt_boxes, int* roi_src,
                                 int* roi_gt, void* stream);

/* The gradient of points_cropping's gathers (:801-803): grad_points (b,n,c) = the sum of grad_out (b,len,c) over the positions whose idx
 * (b,len) names the point, through the inverse lists order / offsets of idx (gspn_inverse_lists).  The result is the one of
 * gspn_sa_group_concat_grad_csr up to the grouping of the sum: the sorted positions are cut into chunks of 64, summed per chunk, and the
 * partial sums of a list that crosses chunks are added in chunk order -- a fixed order, so the bits repeat, and a list of any length (the
 * rows of zeros of negative and padding ROIs all name point 0) is spread over the chip.  part: gspn_crop_gather_grad_part_floats floats. */
long gspn_crop_gather_grad_part_floats(int b, int len, int c);
int gspn_crop_gather_grad(int b, int n, int c, int len, const int* idx, const int* order, const int* offsets, const float* grad_out,
                          float* part, float* grad_points, void* stream);

/* ---------------- models/model_rpointnet.py detection output stage: behind the two heads (gspn_amd/csrc/detect.hip; gspn_class_nms3d: nms3d.hip) ---
 * Same rules as the ROI stage: fp32, no atomics, no workspace, no host synchronisation, nothing contracted. */

/* The per-class NMS of refine_detections (:855-901) for a whole batch, one workgroup per scene.  boxes (b,n,6), scores (b,n), class_ids
 * (b,n) i32 -> selected (b,max_output_size) i32, -1 padded.  A row is a candidate when class_ids > 0 (the caller folds its confidence filter
 * in by zeroing the class id).  Within one class the picks are those of gspn_nms3d with pre_nms_limit -1 and score_threshold -inf on the
 * rows of that class -- descending score, the lower index first among equal scores, iou = inter / (((vol_cand + vol_pick) - inter) + 1e-8f),
 * a candidate leaves when iou > iou_threshold -- with max_per_class picks at most; a pick that survives its own test is picked again until
 * the class is full (zero volume; at a threshold of 0.1 any volume below about 1.1e-9), and the repeated picks count as one row (:893).
 * Classes do not suppress each other.  selected: the picked rows of all classes in descending score, the lower index first among equal
 * scores, the first max_output_size of them (:897-901).  n <= 4096. */
int gspn_class_nms3d(int b, int n, int max_per_class, int max_output_size, float iou_threshold, const float* boxes, const float* scores,
                     const int* class_ids, int* selected, void* stream);

/* The nearest point of r sets per scene for every query point, behind a box test (unmold_segmentation, :1032-1044, without its (B,R,N,P)
 * distance tensor).  query (b,n,3), sets (b,r,p,3), boxes (b,r,6) or NULL -> idx (b,r,n) i32: the position j that minimises
 * (dx*dx + dy*dy) + dz*dz, d = query[s,i] - sets[s,k,j], the smallest j among equal distances (tf.argmin).  With boxes, a query that is
 * not inside box k -- q >= c - s/2 && q <= c + s/2 on all axes -- gets -1 and is not searched.  p <= 4096, n <= 32768. */
int gspn_nearest_in_sets(int b, int r, int n, int p, const float* query, const float* sets, const float* boxes, int* idx, void* stream);

/* ---------------- models/model_rpointnet.py heads: the first layer over the crop (gspn_amd/csrc/heads.hip) ----------------------------
 * classification_head (:915) and segmentation_head (:946) start with a 1x1 convolution of the crop points_cropping (:785-816) builds,
 * concat(pc_fea[idx] (C), center_n (3), coord_n (3)) with center_n = (center[idx] - roi centre) / size, coord_n = (pc[idx] - roi centre) /
 * size.  The layer is linear and per point, so with T (b*n, ldt >= cout) = pc_fea . W[:C] (one gspn_mlp_fwd launch over the b*n points)
 *     Y[row, :] = T[scene*n + idx[row], :cout] + center_n[row] . Wside[0:3] + coord_n[row] . Wside[3:6] + bias,   row over (b, r, p)
 * and the (b, r, p, C + 6) crop is never written.  idx (b,r,p) i32 scene-local (a value outside [0, n) is clamped), pc, center (b,n,3),
 * rois (b,r,6) zero padded, Wside (6,cout) = rows C..C+5 of the layer's weights, bias (cout).  size is 1 when normalize == 0; otherwise
 * rois[.., 3:6], with 1 added when the row's six values sum to 0 (:812; the centre is read before that, as in the reference).
 * fp32, no atomics, no host synchronisation.  cout a multiple of 4 and <= 256, ldt a multiple of 4, T / Wside / bias / Y / dY /
 * dcenter_rows 16-byte aligned: GSPN_ERR_UNSUPPORTED otherwise, before anything is launched. */
int gspn_crop_linear_fwd(int b, int n, int r, int p, int cout, const float* T, int ldt, const int* idx, const float* pc, const float* center,
                         const float* rois, int normalize, const float* Wside, const float* bias, float* Y, void* stream);

/* The gradients of the above that are not gathers: dWside (6,cout) = side^T . dY and dbias (cout) = colsum(dY) over the b*r*p rows of dY
 * (rows, cout), and dcenter_rows (rows, 4) = ((dY[row] . Wside[k]) / size[k], k = 0..2; 0): the gradient of the centre coordinates each row
 * read.  Every workgroup writes one partial (7, cout) into part (gspn_crop_linear_part_floats floats; 0 for sizes the launcher does not
 * take) and a second kernel adds the partials in workgroup order in double: a fixed order, the same bits on every call.  The gradients of
 * the two gathers -- dT from dY at width cout, dcenter from dcenter_rows at width 4 -- are gspn_crop_gather_grad through the inverse
 * lists of idx.  pc and rois get no gradient. */
long gspn_crop_linear_part_floats(int b, int r, int p, int cout);
int gspn_crop_linear_bwd_side(int b, int n, int r, int p, int cout, const float* dY, const int* idx, const float* pc, const float* center,
                              const float* rois, int normalize, const float* Wside, float* part, float* dWside, float* dbias,
                              float* dcenter_rows, void* stream);

/* The per-ROI mean of a few gathered columns (gspn_amd/csrc/crop_mean.hip): what the inference path keeps of the fb_prob and sem_prob
 * columns it crops with the features (:1144-1150), without widening the crop.  table (b,n,c) f32, idx (b,r,p) i32 scene-local (a value
 * outside [0, n) is clamped, as in gspn_crop_linear_fwd) -> out (b,r,c) f32:
 *     out[s, k, :] = (1/p) * sum_j table[s, idx[s, k, j], :]
 * The all-zero index rows of padding ROIs average point 0 p times, as the reference does: there is no masking.  One workgroup per
 * (scene, ROI); the sum is taken in double in an order that depends on the shape alone, divided by p in double and rounded to float once
 * (no atomics: the same bits on every call, and a row that names one point p times returns that point's values exactly).
 * 1 <= c <= 64 (GSPN_ERR_UNSUPPORTED beyond, before anything is launched), p >= 1, b * r < 2^31; no alignment beyond 4 bytes. */
int gspn_crop_mean(int b, int n, int r, int p, int c, const float* table, const int* idx, float* out, void* stream);

/* ---------------- a linear layer over concat(tile(global), local), split (gspn_amd/csrc/tile_linear.hip) -------------------------------
 * segmentation_head's conv_post_0 (:966-970) reads concat(tile(global (groups, cg), p), local (groups*p, cl)).  It is linear, so
 *     y[g*p + j, :] = local[g*p + j, :] . W[cg:]  +  (global[g, :] . W[:cg] + bias)
 * two gspn_mlp_fwd launches and the broadcast add below; the concatenation is never written, and the gradient of the global product is the
 * per-group sum of dY.  A, Y, dY (groups*p, c), G, dG (groups, c), all contiguous with row pitch c.
 * c a multiple of 4 and <= GSPN_MLP_MAX_CHANNELS, groups * p < 2^31, every pointer 16-byte aligned: GSPN_ERR_UNSUPPORTED otherwise, before
 * anything is launched.  fp32, no atomics, no host synchronisation. */

/* Y[g*p + j, :] = A[g*p + j, :] + G[g, :]: one fp32 add per element, the bits of the broadcast add.  Y == A is allowed. */
int gspn_tile_add(long groups, int p, int c, const float* A, const float* G, float* Y, void* stream);

/* dG[g, :] = sum_j dY[g*p + j, :], summed in double in an order that depends on the shape alone and rounded to float once: the same bits on
 * every call, and p equal rows return p * row exactly when p is a power of two.  With few groups the rows of a group are spread over
 * several workgroups, which write double partials into part (gspn_tile_sum_part_floats floats, 16-byte aligned; 0 -- part may then be
 * NULL -- when the shape needs none or is not taken); a second kernel adds them in workgroup order in double. */
long gspn_tile_sum_part_floats(long groups, int p, int c);
int gspn_tile_sum(long groups, int p, int c, const float* dY, float* part, float* dG, void* stream);

/* ---------------- utils/pointnet_util.py composition helpers --------------------------- */

/* (rows, c) -> (rows, ld >= c), the extra columns zero: the 16-byte feature rows gspn_mlp_fwd_gather reads */
int gspn_pad_rows(long rows, int c, int ld, const float* src, float* dst, void* stream);

/* sample_and_group's tail in one pass (pointnet_util.py:41-52): out (b,m,ns,cx+c) where the cx=3
 * xyz channels are xyz[idx]-new_xyz (:41-42) and the c feature channels are points[idx] (:46);
 * xyz_first=1 gives concat([grouped_xyz, grouped_points]) (:48), 0 gives the features-first order
 * of models/model_rpointnet.py:61.  points may be NULL (c=0).  ld_out >= 3+c is the row pitch
 * of out in floats (rows may be padded for the MLP kernels; pad columns are written as 0). */
int gspn_sa_group_concat(int b, int n, int c, int m, int nsample, const float* xyz, const float* new_xyz, const float* points,
                         const int* idx, int xyz_first, int ld_out, float* out, void* stream);
/* gradient of the above w.r.t. points: grad_points (b,n,c) += grad_out[..., feature channels];
 * zeroed here first. */
int gspn_sa_group_concat_grad(int b, int n, int c, int m, int nsample, const int* idx, int xyz_first, int ld_out,
                              const float* grad_out, float* grad_points, void* stream);
/* The same gradient as a gather (no atomics, fixed summation order): `order` (b, m*nsample) = positions of the flattened idx rows
 * sorted by data-point index (ties ascending), `offsets` (b, n+1) = each data point's range in it. */
int gspn_sa_group_concat_grad_csr(int b, int n, int c, int m, int nsample, const int* order, const int* offsets, int xyz_first, int ld_out,
                                  const float* grad_out, float* grad_points, void* stream);

/* ---------------- utils/tf_util.py conv2d 1x1 (+bias +BN +ReLU) : the shared MLP ------- */
/* The reference delegates this arithmetic to TensorFlow (tf_util.py:120-185, 515-534):
 *      y = x.W + bias ;  z = relu(gamma*(y-mean)*rsqrt(var+eps)+beta)
 * per layer over `rows` = b*m*nsample rows (NHWC, 1x1 kernel == a row-major GEMM).  Here each
 * layer is an fp32-MFMA GEMM (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulate) with the
 * element-wise work fused into the operand staging (prologue) / accumulator store (epilogue), so an
 * activation tensor is written once (pre-BN) and read once by its consumer.
 *
 * gspn_mlp_fwd:  Y(rows,ldy)[:, :cout] = act(X)(rows,ldx)[:, :cin] . W(cin,cout) + bias
 *   act(X) = X                           if in_scale == NULL
 *          = relu(X*in_scale+in_shift)   otherwise (per input channel: the previous layer's BN+ReLU)
 *   stats (may be NULL; gspn_mlp_fwd_stats_bytes(rows,cout) bytes, need not be zeroed): every row-block writes its own
 *   partial column sums of Y and Y^2 (no hot-spot atomics); gspn_bn_finalize adds the partials in double.
 * Limits of this build: cin, cout <= GSPN_MLP_MAX_CHANNELS (GSPN_ERR_UNSUPPORTED beyond; the widest layer of the reference's
 * networks has 768 input channels, model_rpointnet.py:109,181), rows < 2^31.
 */
#define GSPN_MLP_MAX_CHANNELS 1024
int gspn_mlp_fwd(long rows, int cin, int cout, const float* X, int ldx, const float* in_scale, const float* in_shift,
                 const float* W, const float* bias, float* Y, int ldy, float* stats, void* stream);
/* gspn_mlp_fwd + the first half of a max-pool over groups of 32 consecutive rows (pointnet_util.py:123-124, nsample = 32): per group
 * and channel the largest raw output and its row offset, taken from the accumulators (vmax, amax: each (rows/32, cout)).  BN+ReLU is
 * increasing in y for scale >= 0, so gspn_pool32_select finishes the pool from these once scale/shift exist:
 * out = relu(scale*vmax + shift), arg = amax -- the (rows, cout) tensor is not read again, except for channels with a negative scale
 * (their group minimum is taken from Y by the select kernel, which also stores it back: on return vmax holds y at the arg row for every
 * channel -- what gspn_pool_rsum needs in backward, so that pass need not gather from Y either). */
int gspn_mlp_fwd_pool32(long rows, int cin, int cout, const float* X, int ldx, const float* in_scale, const float* in_shift,
                        const float* W, const float* bias, float* Y, int ldy, float* stats, float* vmax, int* amax, void* stream);
int gspn_pool32_select(long groups, int c, float* vmax, const int* amax, const float* Y, int ldy,
                       const float* scale, const float* shift, float* out, int* arg, void* stream);
/* The same for groups of ns = 32 * sub rows (model_rpointnet.py:68: max over 256 / 512 grouped rows): vmax / amax (groups * sub, c) as
 * gspn_mlp_fwd_pool32 left them (not modified); out, arg (row offset inside the group, 0 .. ns-1), yarg (y at the arg row) are (groups, c).
 * c a multiple of 4, 16-byte aligned arrays (GSPN_ERR_UNSUPPORTED otherwise: the caller then runs gspn_bnrelu_maxpool over Y). */
int gspn_pool32_select_groups(long groups, int sub, int c, const float* vmax, const int* amax, const float* Y, int ldy,
                              const float* scale, const float* shift, float* out, int* arg, float* yarg, void* stream);
/* bytes of the `stats` workspace for a (rows, cout) layer */
long gspn_mlp_fwd_stats_bytes(long rows, int cout);

/* BN finalize (tf.contrib.layers.batch_norm, tf_util.py:529-534): from stats = (sum, sumsq) over
 * `rows` rows produce the batch mean / biased variance (saved for backward), scale = gamma*rsqrt(var+eps),
 * shift = beta - mean*scale, and update the moving averages in place
 * (moving = moving*decay + batch*(1-decay)).  `stats` is the workspace gspn_mlp_fwd filled for the same (rows, c).  is_training==0: scale/shift come from the moving
 * statistics, mean/var are set to them and nothing is updated (stats may be NULL). */
int gspn_bn_finalize(long rows, int c, const float* stats, const float* gamma, const float* beta, float eps, float decay,
                     int is_training, float* moving_mean, float* moving_var, float* mean, float* var,
                     float* scale, float* shift, void* stream);
/* the same on nparts partial rows [nparts][2][c] of column sums from any producer (e.g. gspn_preagg_fwd) */
int gspn_bn_finalize_parts(long rows, int c, const float* stats, int nparts, const float* gamma, const float* beta, float eps, float decay,
                           int is_training, float* moving_mean, float* moving_var, float* mean, float* var, float* scale, float* shift,
                           void* stream);
/* the same with the partial sums taken about a pivot row (gspn_bn_colsum(dZ = NULL, mean = pivot)): mean = pivot + sum/rows; pivot may be NULL */
int gspn_bn_finalize_parts_pivot(long rows, int c, const float* stats, int nparts, const float* gamma, const float* beta, float eps, float decay,
                                 int is_training, float* moving_mean, float* moving_var, float* mean, float* var, float* scale, float* shift,
                                 const float* pivot, void* stream);

/* out(groups,c) = max over the ns rows of each group of relu(Y*scale+shift)   (tf.reduce_max,
 * pointnet_util.py:123-124); arg (groups,c) gets the row offset (0..ns-1) of the first maximum. */
int gspn_bnrelu_maxpool(long groups, int ns, int c, const float* Y, int ldy, const float* scale, const float* shift,
                        float* out, int* arg, void* stream);
/* out = relu(Y*scale+shift) materialised (last layer of an FP module) */
int gspn_bnrelu_apply(long rows, int c, const float* Y, int ldy, const float* scale, const float* shift, float* out, int ldo, void* stream);

/* ---- stand-alone batch normalisation over the rows of a (rows, c) matrix (gspn_amd/csrc/batchnorm.hip): the device side of
 * tf_util.batch_norm_for_fc / _conv1d / _conv2d (utils/tf_util.py:515-580: tf.contrib.layers.batch_norm over all leading axes).
 *   forward : gspn_bn_colsum(dZ = NULL) -> gspn_bn_finalize_parts -> gspn_bn_apply(relu = 0)
 *   backward: gspn_bn_colsum(dZ)        -> gspn_mlp_bwd_coef      -> gspn_bn_backward_apply
 * gspn_bn_colsum leaves *nparts_out partial rows [2][c] in part (gspn_bn_colsum_part_floats(rows, c) floats): column sums of
 * (x, x^2) when dZ is NULL, of (dz, dz * xhat) with xhat = (x - mean) * rsqrt(var + eps) otherwise. */
long gspn_bn_colsum_part_floats(long rows, int c);
int gspn_bn_colsum(long rows, int c, const float* X, int ldx, const float* dZ, int ldz, const float* mean, const float* var, float eps,
                   float* part, int* nparts_out, void* stream);
/* out = x*scale + shift (two roundings: tf.nn.batch_normalization, tf_util.py:511), through a ReLU when relu != 0 */
int gspn_bn_apply(long rows, int c, const float* X, int ldx, const float* scale, const float* shift, int relu, float* out, int ldo, void* stream);
/* dX = cA*dZ + cB*X + cC per column (training mode: the coefficients of gspn_mlp_bwd_coef; inference: cA = scale, cB = cC = 0) */
int gspn_bn_backward_apply(long rows, int c, const float* dZ, int ldz, const float* X, int ldx, const float* cA, const float* cB, const float* cC,
                           float* dX, int lddx, void* stream);

/* ---- backward of one layer -------------------------------------------------------------
 * With z = relu(s*y+t) and upstream gradient dz (dense, or the scatter of a pooled gradient to its
 * arg-max rows), the gradient w.r.t. the pre-BN output is
 *      dyh = dz * [s*y+t > 0]
 *      dY  = cA*dyh + cB*y + cC                     (per output channel coefficients)
 * which covers BN-training (cA=gamma*rstd, cB/cC from the two batch reductions), BN-inference
 * (cA=scale, cB=cC=0) and no-BN (cA=1).  dY is never materialised. */
typedef struct gspn_dy_args {
    const float* Y;        /* (rows, ldy) pre-BN output saved by the forward pass */
    int ldy;
    const float* dZ;       /* dense upstream gradient (rows, ldz), or NULL when pooled */
    int ldz;
    const float* dPool;    /* pooled upstream gradient (rows/ns, c), or NULL */
    const int* pool_arg;   /* (rows/ns, c) arg-max row offsets from gspn_bnrelu_maxpool */
    int ns;
    const float* scale;    /* c : forward scale/shift (relu mask) */
    const float* shift;
    const float* cA;       /* c each: coefficients written by gspn_mlp_bwd_wgrad (read by gspn_mlp_bwd_data only) */
    const float* cB;
    const float* cC;
} gspn_dy_args;
/* The dW reduction a pass A called with dW = NULL left undone: the final sum over the partial tiles in `work`, as a kernel of its own
 * (gspn_mlp_bwd_dw) or in spare workgroups of pass B. */
typedef struct gspn_dw_args {
    const float* X;        /* the layer's input and its pitch as that pass A got them, so that the workspace layout is found again */
    int ldx;               /* (in pass B X may be NULL, and only a non-NULL X needs ldx >= cin; gspn_mlp_bwd_dw needs ldx >= cin) */
    const float* var;      /* cout: the statistics pass A normalised with (required under use_bn) */
    const float* gamma;    /* cout, or NULL */
    float eps;
    int use_bn;            /* as in that pass A; 0 after gspn_mlp_bwd_wgrad_known (the partial tiles are dW's own: a plain sum) */
    int is_training;
    const float* work;     /* the gspn_mlp_bwd_work_bytes(rows, cin, cout) buffer pass A filled */
    float* dW;             /* (cin, cout) */
    /* a second, plain reduction riding along in gspn_mlp_bwd_data (no other entry point reads these four; cin2 == 0: none): dW2 (cin2, cout) =
     * the sum of nslots2 partial tiles at part2 ([slot][2][cin2*cout], first half) -- the side-column weight gradient of gspn_preagg_bwd_dy */
    const float* part2;
    int cin2;
    int nslots2;
    float* dW2;
} gspn_dw_args;
/* The previous layer's BN reductions out of pass B's epilogue: this launch's dX is that layer's dz, and the sums r0 = sum(dyh), r1 = sum(dyh*xhat)
 * it needs for early coefficients (below) are taken from the finished tiles.  Every field is required. */
typedef struct gspn_rsum_args {
    const float* Yp;       /* (rows, ldyp >= cin) that layer's pre-BN output = this layer's input before activation */
    int ldyp;
    const float* scale;    /* cin each: its forward scale / shift (relu mask) */
    const float* shift;
    const float* mean;     /* cin each: its batch statistics */
    const float* var;
    float eps;
    float* part;           /* gspn_rsum_part_floats(rows, cin) floats: partial rows [*nparts_out][2][cin] for gspn_mlp_bwd_coef */
    int* nparts_out;
} gspn_rsum_args;

/* Pass A -- ONE read of (X, Y, dz):  the BN reductions r0 = sum(dyh), r1 = sum(dyh*xhat) and the raw
 * weight-gradient products G1 = act(X)^T.dyh, Gx = act(X)^T.xhat, g3 = act(X)^T.1 are accumulated into
 * per-row-chunk partials in `work` (gspn_mlp_bwd_work_bytes(rows,cin,cout) bytes; no hot-spot atomics, deterministic
 * second-stage sum in double), then finalised on the device into
 *   dW(cin,cout) = cA (.) (G1 - r0/R g3 1^T - r1/R (.) Gx)            (training-mode BN)
 *                = cA (.) G1                                           (BN on moving statistics, or no BN)
 *   cA=gamma*rstd (1 without BN), cB=-gamma*rstd^2*r1/R, cC=-gamma*rstd*(r0/R - mean*rstd*r1/R)   (0 outside training)
 *   dgamma=r1, dbeta=r0 (under BN), dbias=sum(dY).
 * mean/var are the statistics the forward pass normalised with (batch, or moving when !is_training).
 * Any of cA..dbias may be NULL.  dW may be NULL too: the final sum over the partial tiles is then left to
 * gspn_mlp_bwd_dw (same rows/cin/cout/a/X/ldx, same `work`), which nothing downstream of the layer waits for -- a caller can
 * put it on another stream, ordered after this call, and overlap it with the next layer's kernels. */
int gspn_mlp_bwd_wgrad(long rows, int cin, int cout, const gspn_dy_args* a, const float* X, int ldx,
                       const float* in_scale, const float* in_shift, const float* mean, const float* var, const float* gamma,
                       float eps, int use_bn, int is_training, float* work, float* cA, float* cB, float* cC,
                       float* dgamma, float* dbeta, float* dbias, float* dW, void* stream);
long gspn_mlp_bwd_work_bytes(long rows, int cin, int cout);
int gspn_mlp_bwd_dw(long rows, int cin, int cout, const gspn_dy_args* a, const gspn_dw_args* dw, void* stream);
/* Pass B -- dX(rows,ldx)[:, col0 : col0+ncols] = dY . W^T with dY = cA*dyh + cB*y + cC rebuilt on the fly (the whole row: col0 = 0,
 * ncols = cin).  The other columns of dX are left untouched: for inputs whose leading or trailing channels need no gradient -- the xyz
 * columns of a set-abstraction input, the raw colours of the last FP level.
 *   dw (NULL: no dW job rides): gspn_mlp_bwd_dw in the same launch, in spare workgroups of pass B instead of a kernel of its own; dW is
 *       the same sum taken over 16 instead of 64 slot slices per output.
 *   rs (NULL: no BN reductions): the previous layer's BN reductions from the epilogue.  They need the whole row.
 * dX is bit-identical in all four forms.  One set of argument checks, run before anything is launched.  GSPN_ERR_ARG: rows < 0, cin or
 * cout <= 0, ldx < cin, `a` NULL or without Y / scale / shift / cA / cB / cC or an upstream gradient, a column range outside [0, cin);
 * with dw or rs also rows == 0 (the plain form returns 0 for it: nothing to do); dw without work or dW, with use_bn and no var, with
 * cin2 > 0 and no part2 / dW2 / nslots2, or with a non-NULL X and ldx < cin (the entry points this one replaces disagreed on a NULL X
 * with ldx < cin: accepted, as by the one gspn_amd/mlp.py called); rs with a NULL field, ldyp < cin, or anything but the whole row.
 * GSPN_ERR_UNSUPPORTED: cin or cout > GSPN_MLP_MAX_CHANNELS, rows >= 2^31. */
int gspn_mlp_bwd_data(long rows, int cin, int cout, const gspn_dy_args* a, const float* W, int col0, int ncols, float* dX, int ldx,
                      const gspn_dw_args* dw /* NULL: no dW job rides */, const gspn_rsum_args* rs /* NULL: no BN reductions */, void* stream);
/* Pass B of a POOLED TOP layer (pool groups of 32 rows) as a streaming GEMM on the layer's input: with dY = cA*dyh + cB*y + cC and
 * y = xhat.W + b,   dX = xhat.(W diag(cB) W^T) + S.W^T + const,   S = cA*dyh (one non-zero per pool group and channel) -- the layer's own
 * (rows, cout) output is not read.  a: the layer's gspn_dy_args (dPool, pool_arg, ns = 32, cA/cB/cC); pooled: the (rows/32, cout) pooled
 * output of the forward pass; scratch: gspn_pooltop_scratch_floats(rows, cin, cout) floats.  The layer's dW reduction rides in the small
 * launch that prepares the operands; the previous layer's BN reductions come out of the epilogue (dw and rs as gspn_mlp_bwd_data takes
 * them, both required).
 * GSPN_ERR_UNSUPPORTED outside cin <= 64, cout <= 128 (multiples of 4), ns = 32, 16-byte aligned rows: call gspn_mlp_bwd_data then. */
long gspn_pooltop_scratch_floats(long rows, int cin, int cout);
int gspn_mlp_bwd_data_pooltop(long rows, int cin, int cout, const gspn_dy_args* a, const float* W, const float* bias, const float* pooled,
                              float* scratch, float* dX, int ldx, const gspn_dw_args* dw, const gspn_rsum_args* rs, void* stream);

/* ---- early coefficients: pass A as ONE GEMM ------------------------------------------------------------------------------------
 * Training-mode BN's backward needs r0 = sum(dyh) and r1 = sum(dyh*xhat) over all rows before dY exists; gspn_mlp_bwd_wgrad side-steps
 * that with a second product (Gx) inside the GEMM -- twice the matrix work.  When the two sums are taken BEFORE pass A, the coefficients
 * cA/cB/cC are final and gspn_mlp_bwd_wgrad_known runs one GEMM dW = act(X)^T . dY (g: optional gspn_gather_args of a fused first layer,
 * defined below; dW may be NULL, the sum over partial tiles then rides in gspn_mlp_bwd_data / gspn_mlp_bwd_dw called with use_bn = 0):
 *   - top layer of a pooled stack: gspn_pool_rsum takes the sums from (dPool, pool_arg, Y) -- (groups x c) work; ldy == 0 says Y is
 *     already the (groups, c) tensor of y at the arg row (vmax after gspn_pool32_select): no gather from the (rows, c) output;
 *   - any other layer l: its dz is the dX of layer l+1's pass B, whose epilogue takes them (gspn_mlp_bwd_data with rs, Yp = Y of layer l);
 *   - gspn_mlp_bwd_coef(rows, c, nparts, part, ...) sums the partial rows [nparts][2][c] in double and writes cA, cB, cC, dgamma, dbeta,
 *     dbias (the same formulas as gspn_mlp_bwd_wgrad's).  part: gspn_rsum_part_floats(rows, c) floats. */
struct gspn_gather_args;
long gspn_rsum_part_floats(long rows, int c);
int gspn_pool_rsum(long groups, int ns, int c, const float* dPool, const int* arg, const float* Y, int ldy, const float* scale,
                   const float* shift, const float* mean, const float* var, float eps, float* part, int* nparts_out, void* stream);
/* the same sums for the top layer of a stack with a DENSE upstream gradient dZ (rows, ldz): one streaming pass over (dZ, Y).
 * c a multiple of 4, c <= 1024, 16-byte aligned pitches (GSPN_ERR_UNSUPPORTED otherwise: use gspn_mlp_bwd_wgrad's two-product form). */
int gspn_dense_rsum(long rows, int c, const float* dZ, int ldz, const float* Y, int ldy, const float* scale, const float* shift,
                    const float* mean, const float* var, float eps, float* part, int* nparts_out, void* stream);
int gspn_mlp_bwd_coef(long rows, int c, int nparts, const float* part, const float* mean, const float* var, const float* gamma, float eps,
                      float* cA, float* cB, float* cC, float* dgamma, float* dbeta, float* dbias, void* stream);
int gspn_mlp_bwd_wgrad_known(long rows, int cin, int cout, const gspn_dy_args* a, const float* X, int ldx, const float* in_scale,
                             const float* in_shift, const struct gspn_gather_args* g, float* work, float* dW, void* stream);
/* Pass A and pass B of one layer in ONE launch (r03).  With known coefficients (a->cA/cB/cC final) and either a dense upstream gradient
 * (a->dZ) or the gradient of a max-pool over groups of 32 rows (a->dZ NULL, a->dPool / a->pool_arg, a->ns == 32),
 *     dW (cin, cout)        = relu(Xp*in_scale + in_shift)^T . dY
 *     dX (rows, ldx >= cin) = dY . W^T
 * come from the same staged dY tile.  Xp (rows, ldxp) is the previous layer's raw output, in_scale / in_shift its forward scale / shift.
 * part (optional, with that layer's mean_p / var_p): its BN reductions, exactly what gspn_mlp_bwd_data leaves with rs (*nparts_out rows for
 * gspn_mlp_bwd_coef).  work: the gspn_mlp_bwd_work_bytes(rows, cin, cout) buffer.
 * GSPN_ERR_UNSUPPORTED outside cin in {32, 64}, cout in {32, 64, 128}, rows >= 65536 a multiple of 128, 16-byte aligned pitches:
 * run gspn_mlp_bwd_wgrad_known + gspn_mlp_bwd_data then. */
long gspn_mlp_bwd_fused_work_bytes(long rows, int cin, int cout);
int gspn_mlp_bwd_fused(long rows, int cin, int cout, const gspn_dy_args* a, const float* W, const float* Xp, int ldxp, const float* in_scale,
                       const float* in_shift, float* dX, int ldx, float* work, float* dW, const float* mean_p, const float* var_p,
                       float eps_p, float* part, int* nparts_out, void* stream);
/* gspn_mlp_bwd_fused + gspn_mlp_bwd_coef of the PREVIOUS layer (cin channels; gamma_p and the outputs as gspn_mlp_bwd_coef takes them) with this
 * layer's dW reduction riding in the coefficient launch: two launches instead of three (r04).  part / nparts_out / mean_p / var_p required. */
int gspn_mlp_bwd_fused_coef(long rows, int cin, int cout, const gspn_dy_args* a, const float* W, const float* Xp, int ldxp, const float* in_scale,
                            const float* in_shift, float* dX, int ldx, float* work, float* dW, const float* mean_p, const float* var_p,
                            float eps_p, float* part, int* nparts_out, const float* gamma_p, float* cA_p, float* cB_p, float* cC_p,
                            float* dgamma_p, float* dbeta_p, float* dbias_p, void* stream);

/* Pre-aggregated first layer of an SA / FP module (gspn_amd/csrc/mlp.hip, "Pre-aggregated first layer"): the layer is linear, so its
 * feature part is multiplied on the SOURCE points (F = feat.W_feat, a small GEMM through gspn_mlp_fwd) and the grouped / interpolated
 * rows are then formed from F:   Y[r] = sum_t w[r,t] * F[idx[r,t]] + side[r,:side_n] . Wside + bias,   T = 1 (grouping, w = NULL) or 3
 * (3-NN interpolation).  idx are global source rows, or scene-local ones when per_scene_rows > 0 (output rows / source rows per scene);
 * with global idx (per_scene_rows == 0) per_scene_src is the total number of source rows of F (0: not given, taken as <= rows).
 * stats: the column sums of Y, gspn_preagg_fwd_parts(rows, cout) partial rows for gspn_bn_finalize_parts, or NULL.
 * cout must be 4 * 2^k (gspn_preagg_ok); F, Y 16-byte aligned.  Same result as the GEMM over materialised rows up to fp32 rounding
 * (a different order of additions). */
int gspn_preagg_ok(int cout);
long gspn_preagg_fwd_parts(long rows, int cout);     /* partial rows [parts][2][cout] gspn_preagg_fwd writes into stats */
int gspn_preagg_fwd(long rows, int cout, int T, const float* F, const int* idx, const float* w, int per_scene_rows, int per_scene_src,
                    const float* side, int side_ld, int side_n, const float* Wside, const float* bias, float* Y, float* stats, void* stream);
/* backward half that touches the (rows, cout) tensors: dY = cA*relu'(y*scale+shift)*dz + cB*y + cC written to dY (rows, cout), and
 * dWside (side_n, cout) = side^T . dY (per-workgroup partials in part, gspn_preagg_part_floats(cout, side_n) floats, summed in double in a
 * fixed order).  The rest of the layer's backward runs on source rows: G = transpose-gather of dY (gspn_sa_group_concat_grad_csr /
 * gspn_fp_concat_grad_csr on dY), dW_feat = feat^T . G, d(feat) = G . W_feat^T (gspn_mlp_bwd_wgrad / gspn_mlp_bwd_data, no BN). */
long gspn_preagg_part_floats(int cout, int side_n);
int gspn_preagg_bwd_dy(long rows, int cout, const gspn_dy_args* a, const float* side, int side_ld, int side_n, float* dY, float* part,
                       float* dWside, int* nslots_out, void* stream);
/* (dWside == NULL: the partial tiles stay at part, *nslots_out of them, for gspn_mlp_bwd_data to sum as its second job (part2) in a launch that exists anyway) */

/* ---- fused set-abstraction front end: sample_and_group's concat (pointnet_util.py:36-52) + the first conv2d (:109-113)
 * without the grouped (b, npoint, nsample, 3+c) tensor.  gspn_sa_rel writes, per grouped row r = ((i*m + j)*ns + k), its centred
 * coordinates rel[r] = (xyz[i, idx[r]] - new_xyz[i, j], 0) and its source row gidx[r] = i*n + idx[r] (20 bytes per row).  The first
 * layer then reads VIRTUAL input rows [ feat[gidx[r]][0..ldf) | rel[r][0..4) ] -- the LDS-DMA of the streaming kernels takes each quad
 * from where it lives -- and W's rows are picked to match: xyz_first = 1 for W = [xyz(3); features(c)] (sample_and_group, :48),
 * 0 for W = [features(c); xyz(3)] (multi_encoding_net, model_rpointnet.py:61).
 *   feat: (b*n, ldf) rows, ldf % 4 == 0, ldf >= c (columns >= c are ignored), 16-byte aligned.
 * gspn_mlp_fwd_gather / gspn_mlp_bwd_wgrad_gather are gspn_mlp_fwd / gspn_mlp_bwd_wgrad for such a first layer (no input activation);
 * they return GSPN_ERR_UNSUPPORTED for shapes the streaming kernels do not take (the caller then materialises the rows with
 * gspn_sa_group_concat).  Workspace of the backward call: gspn_mlp_bwd_work_bytes(rows, gspn_mlp_gather_cin(g), cout).
 * Pass B of that layer is the ordinary gspn_mlp_bwd_data over the feature columns (it does not read the layer's input). */
typedef struct gspn_gather_args {
    const float* feat;
    int ldf;
    int c;
    const int* gidx;
    const float* rel;
    int xyz_first;
} gspn_gather_args;
int gspn_sa_rel(int b, int n, int m, int ns, const float* xyz, const float* new_xyz, const int* idx, float* rel, int* gidx, void* stream);
/* the same with the per-seed shift of multi_encoding_net (model_rpointnet.py:56-57, called with a stop_gradient shift at :377):
 * rel[r] = ((xyz[i, idx[r]] - new_xyz[i, j]) - shift[i, j], 0); shift (b, m, 3) or NULL (= gspn_sa_rel) */
int gspn_sa_rel_shift(int b, int n, int m, int ns, const float* xyz, const float* new_xyz, const float* shift, const int* idx,
                      float* rel, int* gidx, void* stream);
int gspn_mlp_gather_cin(const gspn_gather_args* g);
int gspn_mlp_fwd_gather(long rows, const gspn_gather_args* g, int cout, const float* W, const float* bias, float* Y, int ldy,
                        float* stats, void* stream);
int gspn_mlp_bwd_wgrad_gather(long rows, const gspn_gather_args* g, int cout, const gspn_dy_args* a, const float* mean, const float* var,
                              const float* gamma, float eps, int use_bn, int is_training, float* work, float* cA, float* cB, float* cC,
                              float* dgamma, float* dbeta, float* dbias, float* dW, void* stream);

/* Inverse lists (CSR) of an index tensor -- what the gather-form gradients walk.  idx (b,L) int32 with values in [0,n):
 * order (b,L) = positions 0..L-1 grouped by value, ascending inside a group; offsets (b,n+1) = start of every group (offsets[n] = L).
 * Same result as a stable sort of idx + searchsorted.  work: gspn_inverse_lists_work_ints(b,L,n) ints.  Positions with a value
 * outside [0,n) are dropped: offsets[s][n] is then the number of positions of scene s that were kept, smaller than L, and the tail
 * order[s][offsets[s][n] .. L) is NOT WRITTEN -- it keeps what the caller's buffer held.  Every consumer in this library walks order
 * through offsets alone and never reads the tail; a caller that looks at it must fill it first.
 * (Extension: the reference scatters with atomicAdd -- tf_grouping_g.cu:78-86, tf_interpolate.cpp:119-143 -- and needs no such lists.) */
long gspn_inverse_lists_work_ints(int b, int L, int n);
int gspn_inverse_lists(int b, int L, int n, const int* idx, int* work, int* order, int* offsets, void* stream);

/* ---------------- the prediction export stage: the arithmetic of test.py:155-205 (gspn_amd/csrc/predict.hip, ABI 19) -------------- */

/* test.py:163-189 and :204 for every detection of every scene, one workgroup per (scene, detection).  idx (b,r,n) i32: the position in
 * detection k's crop of the crop point nearest to scene point j, -1 where j is outside k's box (gspn_nearest_in_sets with the boxes);
 * masks (b,r,p) f32; class_ids (b,r) i32; sem_prob (b,n,c) f32; point_fb (b,n) f32.  With g[j] = idx[j] >= 0 ? masks[idx[j]] : 0, in double
 * (every float product widened first, so every term is exact):
 *   S0 = sum g,  S1 = sum g * sem_prob[j, class],  S2 = sum g * point_fb[j];  sem_conf = S1 / (1e-8 + S0),  fb_conf = S2 / (1e-8 + S0)
 *   mask[j] = (double)g[j] > mask_th  (u8, 0 or 1);  mask_points = the number of set bytes of the row.
 * The order of the additions depends on the shape alone (no atomics): the same bits on every call.  A row whose class is outside
 * [1, c) writes zeros to all four outputs.  A point outside the box reads neither masks nor the tables; an index >= p is clamped.
 * sem_conf, fb_conf (b,r) f64; mask (b,r,n) u8; mask_points (b,r) i32. */
int gspn_scene_confidence(int b, int r, int n, int p, int c, const int* idx, const float* masks, const int* class_ids, const float* sem_prob,
                          const float* point_fb, double mask_th, double* sem_conf, double* fb_conf, unsigned char* mask, int* mask_points,
                          void* stream);

/* test.py:159-161 and :191-205, one workgroup per scene, r <= GSPN_SCENE_RANK_MAX_R (GSPN_ERR_UNSUPPORTED above).  det_score (b,r) f32,
 * class_ids (b,r) i32, sem_conf, fb_conf (b,r) f64, label_map (c,) i32.  score = ((double)det_score * sem_conf) * fb_conf.
 * Group 0: class in [1, c), sem_conf > sem_th and fb_conf > fb_th;  group 1: class in [1, c) otherwise;  group 2: the other rows, which
 * the reference drops (their score is 0).  A row's output position is its rank by (group ascending, score descending, row ascending),
 * found by counting; a NaN score ranks as -infinity.  In output order: order (b,r) i32: the row at each position; label_ids (b,r) i32:
 * label_map[class], 0 in group 2; confidence (b,r) f32: 1, 0.97, 0 by group; score (b,r) f64.  count (b,) i32: rows of groups 0 and 1. */
#define GSPN_SCENE_RANK_MAX_R 1024
int gspn_scene_rank(int b, int r, int c, const float* det_score, const int* class_ids, const double* sem_conf, const double* fb_conf,
                    double sem_th, double fb_th, const int* label_map, int* order, int* count, int* label_ids, float* confidence,
                    double* score, void* stream);

/* train.py:365-368, 385-386 on the device.  logits (rows,c) f32, labels (rows,) i32; pred = the FIRST column of the row's maximum
 * (np.argmax; a NaN never wins).  For s = 1..c-1: inter[s-1] += #(pred == s and label == s), uni[s-1] += #(pred == s or label == s),
 * ADDED to the caller's (c-1,) int64 accumulators (per-workgroup LDS counters, then one 64-bit integer atomic per class and workgroup:
 * exact in any order).  A label outside [1, c) counts for no class.  2 <= c <= GSPN_SEM_IOU_MAX_C. */
#define GSPN_SEM_IOU_MAX_C 256
int gspn_sem_iou_counts(long rows, int c, const float* logits, const int* labels, long long* inter, long long* uni, void* stream);

/* ---------------- instance AP evaluation: overlap counts and matching (gspn_amd/csrc/evaluate.hip, additive at ABI 20) ---- */

/* The counts the metric needs, one workgroup per (scene, row) and one per scene.  masks (b,r,n) u8, a byte that is not 0 is a set point;
 * pred_class (b,r) i32; seg_label, group_label (b,n) i32.  A point is VOID when its seg label is outside [1, c) or its group label is
 * outside [0, g).  For a row k of class s in [1, c):
 *   inter[k, j]   = the set points of k with seg == s and group == j          (b,r,g) i32
 *   void_count[k] = its set points that are void,  pred_count[k] = its set points          (b,r) i32
 * A row whose class is outside [1, c) writes zeros to all three.  gt_count[s, j] = the points of the scene that are not void and have
 * seg == s and group == j, (b,c,g) i32; its row s = 0 is zero.  The mask is read 16 bytes per lane between the first and the last 16-byte
 * boundary of a row and byte-wise outside, so masks needs no alignment; the label arrays are read at set bytes only.
 * g <= GSPN_INSTANCE_MAX_G, c * g <= GSPN_INSTANCE_MAX_CG, b * r < 2^31 (GSPN_ERR_UNSUPPORTED beyond, before anything is launched). */
#define GSPN_INSTANCE_MAX_G 4096
#define GSPN_INSTANCE_MAX_CG 8192
int gspn_instance_overlaps(int b, int r, int n, int c, int g, const unsigned char* masks, const int* pred_class, const int* seg_label,
                           const int* group_label, int* inter, int* void_count, int* pred_count, int* gt_count, void* stream);

/* The matching of DESIGN.md 4.18, one wave per (scene, threshold, class).  inter, void_count, pred_count, gt_count: gspn_instance_overlaps';
 * pred_class (b,r) i32; confidence (b,r) f32; count (b,) i32: the rows k < count are the scene's predictions; thresholds (t,) f64.
 * A row is valid when k < count, its class is in [1, c) and pred_count >= min_region; a gt (s, j) is eligible when gt_count >= min_region.
 * iou = (double)inter / (double)(gt_count + pred_count - inter), compared by a strict > with the threshold.
 *   n_true, n_false (b,t,r) i32: the records (true = 1 / true = 0, confidence[k]) row k contributes at that threshold
 *   hard_fn (b,t,c) i32: the eligible gts of the class without an event;  n_gt, n_pred (b,c) i32: its eligible gts and its valid rows.
 * r <= GSPN_INSTANCE_MATCH_MAX_R, min_region >= 1, b * t * c < 2^31 (GSPN_ERR_UNSUPPORTED beyond, before anything is launched). */
#define GSPN_INSTANCE_MATCH_MAX_R 1024
int gspn_instance_match(int b, int r, int c, int g, int t, int min_region, const int* inter, const int* void_count, const int* pred_count,
                        const int* pred_class, const float* confidence, const int* count, const int* gt_count, const double* thresholds,
                        int* n_true, int* n_false, int* hard_fn, int* n_gt, int* n_pred, void* stream);

/* ---------------- data_prep.py: segments to instance labels (gspn_amd/csrc/data_prep.hip, additive at ABI 21) ------------ */

/* collect_label's double loop (data_prep.py:25-40) as a table and a gather.  seg_indices (n,) i32: the segment of every vertex;
 * pair_segment, pair_object (p,) i32: the (segment, objectId) pairs of segGroups flattened in file order, group by group and segment by
 * segment; s: one more than the largest segment id of seg_indices.
 *   out_label[v]   = the objectId of the LAST pair whose segment is seg_indices[v], or -1 when there is none          (n,) i32
 *   *out_conflicts = the number of times the reference prints Error!: the sum, over the segments that have a vertex, of (pairs naming the
 *                    segment - 1), a repeat inside one group included                                                  one i32
 * A pair whose segment no vertex has -- one that is negative or >= s included -- does nothing and is no conflict.  A vertex whose entry is
 * negative or >= s gets -1.  p == 0 is legal (every label -1; the two pair pointers must still be non-null).  Integer max and sums only:
 * the same result in any thread order.  ws: gspn_segment_labels_ws_bytes(s) bytes (three words per segment), 4-byte aligned; the call
 * initialises it.  No array needs more than its element's alignment.  GSPN_ERR_ARG for a null pointer, n < 1, s < 1 or p < 0;
 * GSPN_ERR_UNSUPPORTED for n > GSPN_SEGMENT_LABELS_MAX_N or s > GSPN_SEGMENT_LABELS_MAX_S, all before anything is launched.  No host
 * synchronisation and static shapes: the call captures in a graph. */
#define GSPN_SEGMENT_LABELS_MAX_N (1 << 24)
#define GSPN_SEGMENT_LABELS_MAX_S (1 << 26)
int gspn_segment_labels(int n, int p, int s, const int* seg_indices, const int* pair_segment, const int* pair_object, void* ws, int* out_label,
                        int* out_conflicts, void* stream);
long gspn_segment_labels_ws_bytes(int s);

/* ---------------- predictions on a scan's own vertices (gspn_amd/csrc/lift.hip, additive at ABI 21) ---------------------- */

/* test.py:163-189 and :204 with a vertex of the scan in the place of a scene point, for ONE scan: gspn_nearest_in_sets behind the boxes and
 * gspn_scene_confidence in one pass that never writes the (r,v) index tensor.  verts (v,3) f32; crops (r,p,3) f32: the crop points of each
 * detection; boxes (r,6) f32 (centre, size); masks (r,p) f32; class_ids (r) i32; src (v) i32: the scene point each vertex takes its
 * semantic row from, a value outside [0, n) clamped into it; sem_prob (n,c) f32; vert_fb (v) f32; mask_th a double.
 * For detection k and vertex i:  g = masks[k][j], j the crop point of k nearest to the vertex by the unfused fp32 (dx*dx + dy*dy) + dz*dz,
 * the smallest j among equal distances, if the vertex is inside box k (x >= c - s/2 && x <= c + s/2 on every axis, bounds included; a NaN
 * coordinate is inside nothing); g = 0 otherwise.  In double, every float operand widened before the product:
 *   S0 = sum g,  S1 = sum g * sem_prob[src[i], class_k],  S2 = sum g * vert_fb[i];  sem_conf = S1 / (1e-8 + S0),  fb_conf = S2 / (1e-8 + S0)
 *   mask[k][i] = (double)g > mask_th  (u8, 0 or 1; every byte is written);  mask_points = the number of set bytes of the row.
 * A row whose class is outside [1, c) writes zeros to all four outputs.  A vertex outside the box reads neither masks nor the tables.
 * One workgroup per (detection, tile of 256 or 1024 vertices -- 1024 once r * ceil(v / 1024) >= 512) leaves (S0, S1, S2, set bytes) in its
 * own slot of part; one wave per detection adds the slots in ascending order.  The order of the additions depends on (r, v) alone (no
 * atomics): the same bits on every call.  part: gspn_lift_part_doubles(r, v) doubles (0 for sizes the call declines), 8-byte aligned; it
 * need not be initialised and nothing is read from it that this call did not write.  sem_conf, fb_conf (r) f64; mask (r,v) u8;
 * mask_points (r) i32.  Row offsets are 64-bit: r * v may exceed 2^31.  GSPN_ERR_ARG for a size <= 0, a null pointer or a NaN threshold;
 * GSPN_ERR_UNSUPPORTED for p > GSPN_LIFT_MAX_P, r > 65535 or v > GSPN_LIFT_MAX_V, all before anything is launched.  No host
 * synchronisation, nothing allocated, static shapes. */
#define GSPN_LIFT_MAX_P 4096
#define GSPN_LIFT_MAX_V (1 << 24)
long gspn_lift_part_doubles(int r, int v);
int gspn_lift_masks(int r, int v, int p, int n, int c, const float* verts, const float* crops, const float* boxes, const float* masks,
                    const int* class_ids, const int* src, const float* sem_prob, const float* vert_fb, double mask_th, double* part,
                    double* sem_conf, double* fb_conf, unsigned char* mask, int* mask_points, void* stream);

/* ---------------- one nearest neighbour over a global cell grid (gspn_amd/csrc/nearest.hip, additive at ABI 21) -------------- */

/* For every query of xyz1 (b,n,3) the nearest of the known points xyz2 (b,m,3) of its scene: dist (b,n) f32, idx (b,n) i32.  The pair is
 * the FIRST COLUMN OF gspn_threenn on the same inputs, bit for bit: the distance is the unfused fp32 (dx*dx + dy*dy) + dz*dz
 * (tf_interpolate.cpp:71-74), squared; among equal distances the lowest index wins; a pair whose distance is NaN or +inf never wins; a
 * query with no winner gets (+inf, 0), what the reference's 1e40 initialisation leaves.  Exact, not approximate, and the same bits on every
 * call: the known points are sorted into a grid of cells in ws (bounding box, histogram, exclusive scan, scatter; integer atomics only, no
 * float atomics), about 4 per cell and at most 2^16 cells per scene, with cells per axis that follow the box's extents; a query scans the
 * 3 x 3 x 3 block of cells around its own, accepts when its best distance is below the shrunk distance to every face of the block that has
 * cells behind it, and otherwise goes on over every cell its ball touches (with an empty block: over blocks of twice the reach until one
 * holds a point or every cell was read), comparing (distance, index) pairs so that the order of the points inside a cell does not matter; a
 * cell that lies farther from the query than the best pair found is not read.  A query far outside the box of the known points, or in a
 * hollow of the cloud, degrades towards a scan of all of them and stays correct.
 * ws: gspn_nearest_point_ws_bytes(b, m) bytes (0 for sizes the call declines), 16-byte aligned; it need not be initialised, the call resets
 * its own counters and reads nothing from it that it did not write.  Row offsets are 64-bit: b * n may exceed 2^31.  GSPN_ERR_ARG for a
 * negative size, m == 0 with n > 0, or a null pointer; GSPN_ERR_UNSUPPORTED for m > GSPN_NEAREST_MAX_M, a ws that is not 16-byte aligned or
 * b * ceil(n / 256) >= 2^31, all before anything is launched; b == 0 or n == 0 returns 0.  No host synchronisation, nothing allocated,
 * static shapes: the call captures in a graph. */
#define GSPN_NEAREST_MAX_M (1 << 24)
long gspn_nearest_point_ws_bytes(int b, int m);
int gspn_nearest_point(int b, int n, int m, const float* xyz1, const float* xyz2, void* ws, float* dist, int* idx, void* stream);

/* ---------------- segment voting (gspn_amd/csrc/segments.hip, additive at ABI 21) ------------------------------------------- */

/* One scan of v vertices.  seg (v) i32: the segment of every vertex; a vertex whose entry is outside [0, s) is UNSEGMENTED: it never votes,
 * keeps its own value, and its entry indexes nothing.
 *
 * gspn_segment_vote: masks (r,v) u8, any nonzero byte set.  size[g] = the vertices of segment g, cnt[k][g] = those whose byte of row k is
 * set; segment g is set in row k iff (double)cnt[k][g] > vote_th * (double)size[g], one IEEE double multiply and a strict compare.
 *   out[k][i] = the bit of seg[i] in row k for a segmented vertex, masks[k][i] != 0 for an unsegmented one   (r,v) u8, 0 or 1, every byte written
 *   mask_points[k] = the number of set bytes of out[k]                                                       (r) i32
 * out may be masks itself.  vote_th a double in [0, 1).
 * gspn_segment_label_vote: labels (v) i32, c classes.  The winner of a segment is the label in [0, c) that most of its vertices hold, the
 * lowest among equal counts; a label outside [0, c) does not vote.  out[i] (v) i32 = the winner of seg[i] for a segmented vertex whose
 * segment had a voter, labels[i] otherwise.  out may be labels itself.
 *
 * Integer atomics only (no float atomics): the same bits on every call.  Row offsets are 64-bit: r * v may exceed 2^31.  ws:
 * gspn_segment_vote_ws_bytes(r, v, s) -- (r + 1) * s i32 counters, then r * ceil(s / 64) decision words -- or
 * gspn_segment_label_vote_ws_bytes(v, s, c) -- s * c counters, s winners -- bytes (0 for sizes the call declines, and for r == 0 or
 * v == 0), 16-byte aligned; it need not be initialised and nothing is read from it that the call did not write.
 * GSPN_ERR_ARG for a negative size, a null pointer (ws included), vote_th NaN or outside [0, 1), or c < 1; GSPN_ERR_UNSUPPORTED for
 * v > GSPN_SEGMENT_VOTE_MAX_V, r > 65535, s > GSPN_SEGMENT_VOTE_MAX_S, (r + 1) * s or s * c > GSPN_SEGMENT_VOTE_MAX_COUNTERS, or a ws that
 * is not 16-byte aligned, all before anything is launched; r == 0 or v == 0 then returns 0.  No host synchronisation, nothing allocated,
 * static shapes: a call with a caller-held ws captures in a graph. */
#define GSPN_SEGMENT_VOTE_MAX_V (1 << 24)
#define GSPN_SEGMENT_VOTE_MAX_S (1 << 24)
#define GSPN_SEGMENT_VOTE_MAX_COUNTERS (1 << 28)
long gspn_segment_vote_ws_bytes(int r, int v, int s);
int gspn_segment_vote(int r, int v, int s, const unsigned char* masks, const int* seg, double vote_th, void* ws, unsigned char* out,
                      int* mask_points, void* stream);
long gspn_segment_label_vote_ws_bytes(int v, int s, int c);
int gspn_segment_label_vote(int v, int s, int c, const int* labels, const int* seg, void* ws, int* out, void* stream);

/* ---------------- mask NMS (gspn_amd/csrc/mask_nms.hip, additive at ABI 21) -------------------------------------------------- */

/* b scenes, each r mask rows of v bytes in PRIORITY ORDER (row 0 the best), any nonzero byte set.  size[k] = the set bytes of row k,
 * inter[i][j] = the vertices set in both rows i and j.
 *
 * gspn_mask_overlaps: masks (b,r,v) u8 -> sizes (b,r) i32, inter (b,r,r) i32, symmetric, sizes on the diagonal.
 * gspn_mask_nms: count (b) i32 ON THE DEVICE, live = clamp(count, 0, r) leading rows; labels (b,r) i32 or null; iou_th a double in [0, 1).
 * Walk k = 0 .. live-1: row k is SUPPRESSED iff some earlier KEPT row i < k has (labels null or label[i] == label[k]) and
 *   (double)inter[i][k] > iou_th * (double)(size[i] + size[k] - inter[i][k]),    one IEEE double multiply and a strict compare.
 * A suppressed row suppresses nobody; an IoU exactly at the threshold does not suppress; an empty row neither suppresses nor is suppressed.
 *   keep[k] (b,r) u8        = 1 for a kept live row, 0 for a suppressed row and for a row at or beyond live
 *   out[k] (b,r,v) u8       = all zero for a suppressed row, the input as 0 / 1 for every other row (the rows beyond live too); every byte written
 *   mask_points[k] (b,r) i32 = the set bytes of out[k]
 * out may be masks itself.
 *
 * Integer atomics only (no float atomics): the same bits on every call.  Row offsets are 64-bit: b * r * v may exceed 2^31.  ws:
 * gspn_mask_overlaps_ws_bytes(b, r, v) -- b * r * ceil(v / 64) 64-bit words -- or gspn_mask_nms_ws_bytes(b, r, v) -- the same, then, each
 * 16-byte aligned, b * r and b * r * r i32 -- bytes (0 for sizes the call declines, and for b, r or v == 0), 16-byte aligned; it need not
 * be initialised and nothing is read from it that the call did not write.
 * GSPN_ERR_ARG for a negative size, a null pointer other than labels (ws included), iou_th NaN or outside [0, 1); GSPN_ERR_UNSUPPORTED for
 * r > GSPN_MASK_NMS_MAX_R, v > GSPN_MASK_NMS_MAX_V, b > GSPN_MASK_NMS_MAX_B (a grid dimension) or a ws that is not 16-byte aligned, all
 * before anything is launched; b, r or v == 0 then returns 0.  No host synchronisation (count is read on the device), nothing allocated,
 * static shapes: a call with a caller-held ws captures in a graph. */
#define GSPN_MASK_NMS_MAX_R 1024
#define GSPN_MASK_NMS_MAX_V (1 << 24)
#define GSPN_MASK_NMS_MAX_B 65535
long gspn_mask_overlaps_ws_bytes(int b, int r, int v);
int gspn_mask_overlaps(int b, int r, int v, const unsigned char* masks, void* ws, int* sizes, int* inter, void* stream);
long gspn_mask_nms_ws_bytes(int b, int r, int v);
int gspn_mask_nms(int b, int r, int v, const unsigned char* masks, const int* count, const int* labels, double iou_th, void* ws,
                  unsigned char* out, unsigned char* keep, int* mask_points, void* stream);

/* ---------------- mask components (gspn_amd/csrc/components.hip, additive at ABI 21) ----------------------------------------- */

/* One scan: r mask rows of v bytes, any nonzero byte set, and f triangles faces (f,3) i32.  The edges of a face (a, b, c) are {a,b}, {b,c},
 * {a,c}; an edge with an end outside [0, v) is ignored, duplicate and degenerate faces are harmless.  The components of row k are the
 * connected components of its set vertices under the edges whose two ends are both set in row k; rows are independent.
 *
 * gspn_mask_components:
 *   comp[k][x] (r,v) i32 = the smallest vertex of x's component in row k, -1 where x is not set
 *   ncomp[k] (r) i32     = the number of components of row k
 *   largest[k] (r) i32   = the vertex count of its largest component, 0 for an empty row
 * gspn_mask_component_filter: a component of s vertices is KEPT iff s >= min_vertices and (double)s >= min_share * (double)largest[k], one
 * IEEE double multiply and a non-strict compare.  min_vertices >= 1, min_share a double in [0, 1]; 1 keeps the largest component(s) alone,
 * ties included; (1, 0) is the identity up to the normalisation of a nonzero byte to 1.
 *   out[k][x] (r,v) u8     = 1 iff x is set and its component is kept, else 0; every byte written
 *   mask_points[k] (r) i32 = the set bytes of out[k]
 *   ncomp[k], nkept[k] (r) i32 = the components of row k, and those kept
 * out may be masks itself.
 *
 * A lock-free union-find whose loops all carry the bound v; ncomp[k] = -1 marks a row in which a loop reached it, which a correct build
 * never does.  Integer atomics only: the same bits on every call.  Row offsets are 64-bit: r * v may exceed 2^31.  ws:
 * gspn_mask_components_ws_bytes(r, v, f) -- v * ceil(r / 64) 64-bit words, then, each 16-byte aligned, r * v and r i32 -- or
 * gspn_mask_component_filter_ws_bytes(r, v, f) -- the same, then r * v and r i32 more -- bytes (0 for sizes the call declines, and for r or
 * v == 0), 16-byte aligned; it need not be initialised and nothing is read from it that the call did not write.
 * GSPN_ERR_ARG for a negative size, a null pointer (ws included; faces may be null when f == 0), min_vertices < 1, min_share NaN or outside
 * [0, 1]; GSPN_ERR_UNSUPPORTED for r > GSPN_MASK_COMPONENTS_MAX_R, v > GSPN_MASK_COMPONENTS_MAX_V, f > GSPN_MASK_COMPONENTS_MAX_F or a ws
 * that is not 16-byte aligned, all before anything is launched; r or v == 0 then returns 0, and with f == 0 every set vertex is its own
 * component.  No host synchronisation, nothing allocated, static shapes: a call with a caller-held ws captures in a graph. */
#define GSPN_MASK_COMPONENTS_MAX_R 1024
#define GSPN_MASK_COMPONENTS_MAX_V (1 << 24)
#define GSPN_MASK_COMPONENTS_MAX_F (1 << 26)
long gspn_mask_components_ws_bytes(int r, int v, int f);
int gspn_mask_components(int r, int v, int f, const unsigned char* masks, const int* faces, void* ws, int* comp, int* ncomp, int* largest,
                         void* stream);
long gspn_mask_component_filter_ws_bytes(int r, int v, int f);
int gspn_mask_component_filter(int r, int v, int f, const unsigned char* masks, const int* faces, int min_vertices, double min_share, void* ws,
                               unsigned char* out, int* mask_points, int* ncomp, int* nkept, void* stream);

/* ---------------- mask holes (gspn_amd/csrc/components.hip, additive at ABI 21) ---------------------------------------------- */

/* One scan as above, with the vertices xyz (v,3) f32.  Rows are independent.  For row k, points_in[k] is the number of set vertices; the BOX
 * is the closed axis-aligned box over the set vertices whose three coordinates are all finite (none: no box, no candidate); a vertex is
 * INSIDE iff lo <= c && c <= hi on all three axes as IEEE float compares, so -0.0 and +0.0 are one place and a vertex with a NaN coordinate
 * is never inside.  A CANDIDATE is an unset vertex inside the box; the candidate components are those of the candidates under the edges
 * whose two ends are both candidates of row k.  A candidate component is OPEN iff an edge joins it to an unset vertex that is no candidate
 * (an unset vertex outside the box), and TOUCHES iff an edge joins it to a set vertex.  A candidate component of s vertices is a HOLE iff
 * it is not open, it touches, s <= max_vertices and (double)s <= max_share * (double)points_in[k], one IEEE double multiply and a
 * non-strict compare.  max_vertices >= 0, max_share a double in [0, 1]; max_vertices = 0 is the identity up to the normalisation of a
 * nonzero byte to 1.
 *   out[k][x] (r,v) u8     = 1 iff x is set or lies in a hole, else 0; every byte written
 *   mask_points[k] (r) i32 = points_in[k] + nfilled[k], the set bytes of out[k]
 *   nholes[k], nfilled[k] (r) i32 = the holes filled in row k, and their vertices
 *   label[k][x] (r,v) i32, or null = -2 where x is set, -1 where it is unset and no candidate, else the smallest vertex of its candidate
 *                            component
 * out may be masks itself.
 *
 * The union-find of the components on the candidates, then one pass over the faces that marks what each component borders; every loop
 * carries the bound v, and nholes[k] = -1 marks a row in which one reached it, which a correct build never does.  Integer atomics only:
 * the same bits on every call.  Row offsets are 64-bit.  ws: gspn_mask_hole_fill_ws_bytes(r, v, f) bytes -- two tables of
 * v * ceil(r / 64) 64-bit words (candidates, set), then, each 16-byte aligned, r * v, r, 6 * r, r and r * v i32 (sizes with the flags of a
 * root, marks, box keys, points_in, and the parents, which live in label instead when there is one) -- (0 for sizes the call declines, and
 * for r or v == 0), 16-byte aligned; it need not be initialised and nothing is read from it that the call did not write.
 * GSPN_ERR_ARG for a negative size, a null pointer (ws included; faces may be null when f == 0, label may always be null),
 * max_vertices < 0, max_share NaN or outside [0, 1]; GSPN_ERR_UNSUPPORTED for r > GSPN_MASK_HOLE_FILL_MAX_R, v > GSPN_MASK_HOLE_FILL_MAX_V,
 * f > GSPN_MASK_HOLE_FILL_MAX_F or a ws that is not 16-byte aligned, all before anything is launched, an argument error first; r or
 * v == 0 then returns 0 and writes nothing, and with f == 0 there are no holes.  No host synchronisation, nothing allocated, static
 * shapes: a call with a caller-held ws captures in a graph. */
#define GSPN_MASK_HOLE_FILL_MAX_R 1024
#define GSPN_MASK_HOLE_FILL_MAX_V (1 << 24)
#define GSPN_MASK_HOLE_FILL_MAX_F (1 << 26)
long gspn_mask_hole_fill_ws_bytes(int r, int v, int f);
int gspn_mask_hole_fill(int r, int v, int f, const unsigned char* masks, const int* faces, const float* xyz, int max_vertices,
                        double max_share, void* ws, unsigned char* out, int* mask_points, int* nholes, int* nfilled, int* label, void* stream);

/* ---------------- train.py: the per-step batch, the reference's optimisers, the running loss sums (gspn_amd/csrc/train.hip, ABI 20) -------
 *
 * gspn_batch_assemble: get_batch (train.py:221-240) over dataset.py:143-190 for b batch slots from a cache of nscene scenes on the device.
 *   cache:   pc_all, color_all (nscene,n,3) f32; group_all, seg_all (nscene,n) i32; pc_ins_all (nscene,g,m,3) f32, zero rows beyond a
 *            scene's groups; ngroup_all (nscene) i32; scene_idx (b) i32 ON THE DEVICE (clamped to [0, nscene)); seed_dev: one int64.
 *   outputs: pc, color (b,n,3); group_label, seg_label (b,n) i32; pc_ins (b,g,m,3); group_indicator (b,g) i32; bbox_ins (b,g,6);
 *            smpw (b,n) = 1; rotation (b,3,3) f64 and translation (b,3) f64, as drawn.
 * Slot s takes scene k = scene_idx[s].  Nothing is read back and there is no workspace: the call captures.  n <= 2^31.
 *
 * Permutation (dataset.py:156-160): out[s, i] = in[k, gspn_batch_perm(seed, s, n, i)] for pc, color and both label rows; permute = 0: the
 * identity (:162-166).  gspn_batch_perm is a stateless bijection of [0, n), a function of (seed, s) only.  With h = the smallest integer
 * in 1..16 with 4^h >= n, mask = 2^h - 1 and the round keys key[r] = gspn_roi_rand32(seed, s, GSPN_PERM_STREAM, r), r = 0..3:
 *   fmix32(x):  x ^= x >> 16;  x *= 0x85EBCA6B;  x ^= x >> 13;  x *= 0xC2B2AE35;  x ^= x >> 16          (uint32, modulo 2^32)
 *   E(x):       l = x >> h, r = x & mask;  four times, for key[0..3]:  (l, r) = (r, l ^ (fmix32(r ^ key) >> (32 - h)));  E = l << h | r
 *   gspn_batch_perm(seed, s, n, i) = the first of E(i), E(E(i)), ... that is < n
 * (a balanced Feistel network over 2h bits, cycle-walked: E permutes [0, 4^h), so the walk ends and distinct i end on distinct values).
 *
 * Augmentation (:174-183), augment = 1, with draw(t) = gspn_roi_rand32(seed, s, GSPN_AUGMENT_STREAM, t) and float64 throughout:
 *   angle = (6.283185307179586 * draw(0)) / 2^32;  c = cos(angle), sn = sin(angle);  R = [[c, sn, 0], [-sn, c, 0], [0, 0, 1]]
 *   Box-Muller, pair p = 0, 1:  u1 = (draw(1 + 2p) + 1) / 2^32,  u2 = draw(2 + 2p) / 2^32,  rad = sqrt(-2 log(u1)),
 *                               z[2p] = rad * cos(6.283185307179586 * u2),  z[2p + 1] = rad * sin(6.283185307179586 * u2);   t = z[0..2]
 *   every row x of pc and of pc_ins (the all-zero padding rows included) becomes, for a = 0..2,
 *       (float)(((x0 * R[0][a] + x1 * R[1][a]) + x2 * R[2][a]) + t[a]),   nothing fused.
 * R and t are drawn once, by a one-wave launch, into the rotation / translation outputs; the launches that transform pc and pc_ins read
 * them from there.  augment = 0: R = identity, t = 0 and the coordinates are copied, not passed through the transform.
 * Padding (:168-172): group_indicator[s, j] = j < ngroup_all[k].  Boxes (:185-188): bbox_ins = gspn_points_bbox of the output pc_ins. */
#define GSPN_PERM_STREAM 0xFFFFFFFDu    /* `a` of the round keys: no group, no ROI, nor the scene stream 0xFFFFFFFE of gspn_amd/dataset.py */
#define GSPN_AUGMENT_STREAM 0xFFFFFFFCu /* `a` of the draws of R and t */
int gspn_batch_assemble(int nscene, int b, long n, int g, int m, const float* pc_all, const float* color_all, const int* group_all,
                        const int* seg_all, const float* pc_ins_all, const int* ngroup_all, const int* scene_idx,
                        const long long* seed_dev, int permute, int augment, float* pc, float* color, int* group_label, int* seg_label,
                        float* pc_ins, int* group_indicator, float* bbox_ins, float* smpw, double* rotation, double* translation,
                        void* stream);

/* tf.train.AdamOptimizer's rule (train.py:156) over one flat fp32 buffer, gspn_adam_flat's arguments without weight_decay:
 *   m += (g - m) * (1 - b1);  v += (g * g - v) * (1 - b2);  lr_t = lr * sqrt(1 - b2^step) / (1 - b1^step);  p -= (m * lr_t) / (sqrt(v) + eps)
 * with g multiplied by grad_scale first and lr_t computed on the host in double.  It parts from gspn_adam_flat where sqrt(v) is not
 * large against eps: there eps is added to the bias-corrected root. */
int gspn_adam_tf_flat(long n, float* p, const float* g, float* m, float* v, float lr, float b1, float b2, float eps, float grad_scale,
                      long step, void* stream);

/* tf.train.MomentumOptimizer (train.py:154; torch.optim.SGD(momentum=, dampening=0) is the same rule):
 *   accum = momentum * accum + g * grad_scale;  p -= lr * accum */
int gspn_momentum_flat(long n, float* p, const float* g, float* accum, float lr, float momentum, float grad_scale, void* stream);

/* sums[i] += *ptrs[i] for i < k <= GSPN_SCALARS_MAX, count[0] += 1: the running loss sums of train.py:288-297 without the per-step
 * read-back.  ptrs: k pointers to fp32 scalars ON THE DEVICE, the array itself in HOST memory (it is passed to the kernel by value);
 * sums (k) f64 and count (1) i64 on the device.  One wave. */
#define GSPN_SCALARS_MAX 16
int gspn_scalars_accumulate(int k, const float* const* ptrs, double* sums, long long* count, void* stream);

/* utils/pointnet_util.py:157-160 in one kernel: dist (total,3) squared distances of three_nn -> weight (total,3):
 * d = max(d, 1e-10); weight_k = (1/d_k) / ((1/d_0 + 1/d_1) + 1/d_2) */
int gspn_three_nn_weights(long total, const float* dist, float* weight, void* stream);

/* n device-to-device copies (src[i] -> dst[i], bytes[i] bytes; the three arrays live on the HOST) in one launch per 40 segments:
 * refills the persistent buffers a captured step reads (extension: scheduling helper, no reference counterpart). */
int gspn_multi_copy(int n, const void* const* src, void* const* dst, const long* bytes, void* stream);

/* Adam (torch.optim.Adam's rule; the reference trains with tf.train.AdamOptimizer) over one flat fp32 buffer of n parameters:
 * p, g (gradients), m, v (moments) all flat; g is multiplied by grad_scale first (1/world after a SUM all-reduce); step >= 1 = number of
 * this update.  One launch for the whole model. */
int gspn_adam_flat(long n, float* p, const float* g, float* m, float* v, float lr, float b1, float b2, float eps, float weight_decay,
                   float grad_scale, long step, void* stream);

/* The same update with the step number kept on the DEVICE: state = two 8-byte words, zero-initialised once by the caller (state[0] = updates done so far,
 * state[1] = scratch).  No argument changes from step to step, so the launch can be a node of a captured hipGraph (ABI 9). */
int gspn_adam_flat_dev(long n, float* p, const float* g, float* m, float* v, float lr, float b1, float b2, float eps, float weight_decay,
                       float grad_scale, unsigned long long* state, void* stream);

/* out[0] = <a, b> over n floats, deterministic (1024 per-workgroup partials added in index order, in double).  work: gspn_dot_work_floats() floats. */
long gspn_dot_work_floats(void);
int gspn_dot(long n, const float* a, const float* b, float* work, float* out, void* stream);

int gspn_fill_zero(void* ptr, long bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
