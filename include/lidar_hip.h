/*
 * lidar_hip.h — C ABI of liblidar_hip.so (hand-written gfx950 / CDNA4 kernels).
 *
 * This is the drop-in boundary for the reference's per-frame hot path.  Every entry point takes
 * raw DEVICE pointers (unless a parameter says "host"), explicit sizes and a hipStream_t passed as
 * void*; nothing allocates, frees or synchronises inside (scratch comes from a caller-provided
 * workspace whose size is returned by the matching *_workspace_bytes query), so every call is
 * capturable into a hipGraph.  Return value: 0 = ok, <0 = error (LIDAR_ERR_*), never exit().
 *
 * Each declaration cites the reference interface it replaces (paths under /root/reference/).
 * The Python-side binding a maintainer adds is shown in INTEGRATION.md.
 *
 * This text is also read by a program: lidardetection_amd/_lib.py derives its ctypes table and its LIDAR_* limits from it, and
 * csrc/common.h includes it, so every definition is compiled against its declaration.  Keep to what that parser maps without
 * guessing: parameters and returns of type void, int, float, double, size_t, long long (or a fixed-width / unsigned integer) by
 * value, pointers to them of any depth and constness; no struct by value, array, function-pointer or variadic parameter; an
 * object-like `#define LIDAR_<NAME>` is an integer expression of literals, parentheses, unary minus, <<, * and +.
 */
#ifndef LIDAR_HIP_H
#define LIDAR_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LIDAR_OK 0
#define LIDAR_ERR_ARG (-1)
#define LIDAR_ERR_LAUNCH (-2)
#define LIDAR_ERR_WORKSPACE (-3)
#define LIDAR_ERR_UNSUPPORTED (-4) /* an optional library-backed path is not available: keep the other path */

/* ------------------------------------------------------------------ voxelisation
 * Replaces spconv.utils.VoxelGeneratorV2.generate (external, un-vendored; call site
 * pcdet/datasets/processor/data_processor.py:48-80) for a whole batch, and the voxel part of
 * DatasetTemplate.collate_batch (pcdet/datasets/dataset.py:153-185: concatenation + batch index
 * column).  Results are identical to running the sequential scan frame by frame.
 *
 *   points        (sum N_f, C) f32, frames concatenated
 *   point_offsets (batch+1) i32 DEVICE, exclusive prefix of N_f
 *   n_max         host upper bound of max_f N_f (sizes the launch and the workspace)
 *   range6/voxel_size3/grid3  HOST arrays: [x0,y0,z0,x1,y1,z1], [vx,vy,vz], [nx,ny,nz]
 *   compact       1: frame f's rows start at sum_{g<f} V_g (the collate_batch layout)
 *                 0: frame f's rows start at f*max_voxels
 *   algo          0: auto (3 when it applies, else 2); 3 (1 is accepted as an alias): LDS-binned, 2 launches — bin + zero-fill
 *                 roles in one launch, then emit; a frame's points are hash-partitioned by pillar into n_max / 1280 bins, one
 *                 workgroup each (a bin with more than 3072 points — zero-padded clouds — is handled exactly by a streaming
 *                 variant); needs n_max <= 32768, max_points < 16384 and an x / y grid below 2^24 cells; no global atomics
 *                 on the data path; more distinct voxels (4096) / list cells (3072) in ONE hash bin than its LDS holds
 *                 (adversarial input only) sets the sticky flag read by lidar_voxelize_error_flag / mirrored to the host by
 *                 lidar_voxelize_set_error_mirror; 2: global hash table (any n_max);
 *                 4: as 3 with a RESIDENT output buffer (compact layout): the caller passes the SAME voxels / num_points
 *                 buffers call after call and does not write to them in between; the zero padding then survives from call
 *                 to call and only the slots the previous call filled are re-zeroed (~30 MB of HBM traffic per 16 KITTI
 *                 frames instead of 150 MB), results unchanged.  The workspace remembers the buffer addresses: another
 *                 buffer (or the first call) is cleared in full, so only an in-place modification by the caller between
 *                 calls can break the contract
 *   voxels        (batch*max_voxels, max_points, C) f32; rows [0, total) fully written (zero padded)
 *   coords        (batch*max_voxels, 4) i32 [b, z, y, x]
 *   num_points    (batch*max_voxels) i32
 *   voxel_offsets (batch+1) i32: first row of each frame; [batch] = total rows (compact) */
size_t lidar_voxelize_workspace_bytes(int batch, int n_max, int max_voxels);
/* call once after allocating the workspace (and again after any failed call) */
int lidar_voxelize_workspace_init(void *ws, size_t ws_bytes, int batch, int n_max, int max_voxels, void *stream);
int lidar_voxelize(const float *points, const int *point_offsets, int batch, int n_max, int num_features,
                   const float *range6, const float *voxel_size3, const int *grid3, int max_points,
                   int max_voxels, int compact, int algo, float *voxels, int *coords, int *num_points,
                   int *voxel_offsets, void *ws, size_t ws_bytes, void *stream);
/* lidar_voxelize for a caller that also knows the frame offsets on the HOST — the reference's collate_batch does
 * (pcdet/datasets/dataset.py:153-185 builds the batch index from the per-sample lengths): host_offsets = batch + 1 ints in host
 * memory with the same contents as point_offsets (nullptr = none).  Up to 64 frames they travel as kernel arguments, and the
 * LDS-binned launches (algo 3 / 4) issue their first point read without a dependent load of the offsets; results identical. */
int lidar_voxelize_hostoff(const float *points, const int *point_offsets, const int *host_offsets, int batch, int n_max,
                           int num_features, const float *range6, const float *voxel_size3, const int *grid3, int max_points,
                           int max_voxels, int compact, int algo, float *voxels, int *coords, int *num_points,
                           int *voxel_offsets, void *ws, size_t ws_bytes, void *stream);
/* Measurement only: a timer = four HIP events carried by the launches themselves (hipExtLaunchKernel's start / stop events):
 * the time from the start of the call's first kernel to the end of its last one, as a kernel trace would report it, without the
 * marker / queue overhead of a hipEventRecord bracket around the call.  lidar_voxelize_time_next arms `timer` for the calling
 * thread's next lidar_voxelize(_hostoff) call: the LDS-binned path records into it, any other path (or an argument error)
 * disarms it unrecorded.  lidar_timer_elapsed_ms waits for the stop event (< 0: nothing was recorded);
 * lidar_timer_parts_ms splits the same span into {first launch, gap between the launches, last launch}. */
void *lidar_timer_create(void);
void lidar_timer_destroy(void *timer);
void lidar_voxelize_time_next(void *timer);
float lidar_timer_elapsed_ms(void *timer);
int lidar_timer_parts_ms(void *timer, float *out3);
/* optional: a device-visible HOST int (pinned + mapped memory) that receives the same error bits, so the caller can poll
 * the flag without a copy or a synchronisation (nullptr unregisters).  Cleared by the caller. */
int lidar_voxelize_set_error_mirror(void *ws, size_t ws_bytes, int batch, int n_max, int max_voxels, int *host_flag,
                                    void *stream);
/* host-synchronous read of the sticky overflow flag of algo 3 / 4 (0 = fine); not for use inside captures */
int lidar_voxelize_error_flag(void *ws, size_t ws_bytes, int batch, int n_max, int max_voxels);

/* HOST voxel generator: spconv.utils.VoxelGeneratorV2.generate for ONE frame on a CPU core, for the reference's real call
 * site — DataProcessor.transform_points_to_voxels inside forked DataLoader workers (pcdet/datasets/processor/
 * data_processor.py:48-80, pcdet/datasets/__init__.py:73), which must not touch the GPU.  Touches no HIP state.
 *   points (n, C) f32 HOST; voxels (max_voxels, max_points, C), coords_zyx (max_voxels, 3) [z, y, x], num_points (max_voxels)
 *   caller-allocated and UNinitialised: rows [0, return value) are fully written (zero padded), the rest is left alone.
 *   scratch: lidar_voxelize_cpu_scratch_bytes(n) bytes.  Returns the voxel count (>= 0) or a negative LIDAR_ERR_*. */
size_t lidar_voxelize_cpu_scratch_bytes(int n);
int lidar_voxelize_cpu(const float *points, int n, int num_features, const float *range6, const float *voxel_size3,
                       const int *grid3, int max_points, int max_voxels, float *voxels, int *coords_zyx, int *num_points,
                       void *scratch, size_t scratch_bytes);

/* ------------------------------------------------------------------ PillarVFE (one PFN layer, eval)
 * Replaces PillarVFE.forward + PFNLayer.forward (pcdet/models/backbones_3d/vfe/pillar_vfe.py:94-123,
 * :29-49) with BatchNorm1d(eps=1e-3) in eval mode folded by the caller:
 *   scale = gamma / sqrt(var + eps), shift = beta - mean*scale  (both (cout)); no-norm: scale=1, shift=bias.
 *   weight (cout, C+6[+1]) row-major = nn.Linear.weight; feature order [point C | xyz-mean | xyz-centre | dist]
 *   coords/num_points may be the f32 tensors the reference's load_data_to_gpu produces
 *   (pcdet/models/__init__.py:22) — set *_are_float — or the i32 outputs of lidar_voxelize.
 *   num_voxels_dev optional device int (e.g. &voxel_offsets[batch]); rows >= it are skipped. */
int lidar_pillar_vfe(const float *voxels, const void *num_points, const void *coords, int num_voxels,
                     const int *num_voxels_dev, int max_points, int num_features, const float *weight,
                     const float *scale, const float *shift, int cout, const float *voxel_size3,
                     const float *range6, int with_distance, int coords_are_float, int num_are_float,
                     float *out, void *stream);

/* MeanVFE.forward (pcdet/models/backbones_3d/vfe/mean_vfe.py:14-31): out (V, C) */
int lidar_mean_vfe(const float *voxels, const void *num_points, int num_voxels, int max_points,
                   int num_features, int num_are_float, float *out, void *stream);

/* PointPillarScatter.forward (pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py:14-37), nz == 1:
 * canvas (batch, channels, ny, nx) f32, every element written exactly once. channels in {32,64,128}.
 * A pillar with b outside [0, batch), x outside [0, nx) or a row outside [0, ny) lies outside the canvas and is left out
 * (x == nx is not the first cell of the next row).
 * channels_last = 1 writes the same logical tensor with NHWC strides (torch.channels_last), which MIOpen's fp32
 * convolutions consume without layout transposes. */
/* Resident-canvas variant: ONE persistent channels-last canvas (B, ny, nx, C); a call clears the cells the previous call wrote
 * (prev_cells / prev_count: caller-owned state, num_voxels ints + 1 int; start with a zero canvas and *prev_count = 0) and
 * writes the new pillars -- ~2*V*C*4 bytes instead of the whole canvas; the canvas equals a fresh PointPillarScatter output. */
int lidar_pillar_scatter_update(const float *pillar_features, const void *coords, int coords_are_float, int num_voxels,
                                const int *num_voxels_dev, int channels, int batch, int nx, int ny, float *canvas,
                                int *prev_cells, int *prev_count, void *stream);
/* The backbone's first convolution straight from the pillars (PointPillarScatter pointpillar_scatter.py:14-37 + the first
 * ZeroPad2d / Conv2d / BatchNorm / ReLU of BaseBEVBackbone, base_bev_backbone.py:34-45, fused): the k x k / stride / pad
 * convolution's neighbour table over ALL output pixels in NHWC map order, nbr[(b * OH + oy) * OW + ox][ky * k + kx] = pillar row
 * at input cell (oy * stride - pad + ky, ox * stride - pad + kx) or -1.  lidar_spconv_implicit_gemm_sorted over this table with
 * weight (k * k, Cin, Cout), the folded shift as bias and ReLU writes the layer's dense NHWC output (rows without taps get
 * act(bias)); the > 90 %-zero canvas is never built.  ws: lidar_pillar_conv_table_workspace_bytes (inverse cell -> pillar map). */
size_t lidar_pillar_conv_table_workspace_bytes(int batch, int nx, int ny);
int lidar_pillar_conv_table(const void *coords, int coords_are_float, int num_voxels, const int *num_voxels_dev, int batch, int nx,
                            int ny, int k, int stride, int pad, int *nbr, void *ws, size_t ws_bytes, void *stream);
size_t lidar_pillar_scatter_workspace_bytes(int batch, int nx, int ny);
int lidar_pillar_scatter(const float *pillar_features, const void *coords, int coords_are_float, int num_voxels,
                         const int *num_voxels_dev, int channels, int batch, int nx, int ny, int channels_last,
                         float *canvas, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ PillarVFE + one PFNLayer, TRAIN mode (csrc/pfn_train.hip)
 * pillar_vfe.py:29-49, :94-123 with BatchNorm1d(eps) in train mode: batch statistics over all num_voxels_dev * max_points rows
 * (padded slots included), no (V, P, cout) tensor.  Same inputs and support as lidar_pillar_vfe (num_features 3..8,
 * max_points <= 64, cout <= 64), plus gamma / beta (cout) of the norm.  Forward writes out (V, cout) (rows past the device count
 * zero) and what the backward reads: zsel (V, cout) f32 and slot (V, cout) u8 (the selected row of every pillar and channel),
 * stats (272 doubles: the moment sums, mean, inverse std, N), scale_shift (2 * cout) and batch_stats (3 * cout: batch mean, biased
 * variance, unbiased variance -- the caller applies the running-statistics update).  Backward: grad_out (V, cout) -> d_weight
 * (cout, nf), d_gamma, d_beta (cout).  No float atomics: both are bitwise reproducible.  ws: lidar_pfn_train_workspace_bytes. */
#define LIDAR_PFN_TRAIN_STATS_DOUBLES 272
size_t lidar_pfn_train_workspace_bytes(int num_voxels, int num_features, int cout, int with_distance);
int lidar_pfn_train_forward(const float *voxels, const void *num_points, const void *coords, int num_voxels, const int *num_voxels_dev,
                            int max_points, int num_features, const float *weight, const float *gamma, const float *beta, int cout,
                            float eps, const float *voxel_size3, const float *range6, int with_distance, int coords_are_float,
                            int num_are_float, float *out, float *zsel, unsigned char *slot, double *stats, float *scale_shift,
                            float *batch_stats, void *ws, size_t ws_bytes, void *stream);
int lidar_pfn_train_backward(const float *voxels, const void *num_points, const void *coords, int num_voxels, const int *num_voxels_dev,
                             int max_points, int num_features, const float *weight, const float *gamma, int cout,
                             const float *voxel_size3, const float *range6, int with_distance, int coords_are_float, int num_are_float,
                             const float *grad_out, const float *zsel, const unsigned char *slot, const double *stats,
                             const float *scale_shift, float *d_weight, float *d_gamma, float *d_beta, void *ws, size_t ws_bytes,
                             void *stream);
/* PointPillarScatter backward: grad_features (V, channels) = grad_canvas at each pillar's cell (lidar_pillar_scatter's cell
 * rule), zero for rows past num_voxels_dev and pillars outside the canvas (b outside [0, batch), x outside [0, nx), row outside
 * [0, ny)).  channels in {32, 64, 128}; channels_last: grad_canvas has NHWC strides. */
int lidar_pillar_scatter_backward(const float *grad_canvas, const void *coords, int coords_are_float, int num_voxels,
                                  const int *num_voxels_dev, int channels, int batch, int nx, int ny, int channels_last,
                                  float *grad_features, void *stream);

/* ------------------------------------------------------------------ BatchNorm2d + ReLU, TRAIN mode (csrc/bn_train.hip)
 * Replaces the train-mode BatchNorm2d -> ReLU pairs of BaseBEVBackbone and the concat of its deblocks
 * (pcdet/models/backbones_2d/base_bev_backbone.py:31-69, 103) on channels-last fp32 maps.  A map is `rows` = B * H * W rows of
 * channels at row stride ld (floats), starting at channel offset off.  One call takes nseg (1..4) input maps as one concatenated
 * channel space (segment i owns channels [sum seg_C[:i], + seg_C[i]) of gamma, beta, y and every per-channel output); x, x_ld,
 * x_off, seg_C and dx are HOST arrays of nseg entries (x / dx hold device pointers).  Supported: seg_C % 4 == 0, 4 <= seg_C <= 1024,
 * ld % 4 == 0, off % 4 == 0, off + C <= ld, 16-byte aligned pointers, rows >= 2 (torch refuses one value per channel).
 * Forward: batch statistics over the rows (fp64 sums, fixed-order reduction), y = max(z * gamma / sigma + beta - mu gamma / sigma, 0)
 * into channels [y_off, y_off + sum seg_C) of the (rows, y_ld) output; stats (2 * ctot doubles: mean, 1 / sigma), scale_shift
 * (2 * ctot floats) for the backward; batch_stats (3 * ctot floats: mean, biased variance, unbiased variance -- the caller applies
 * the running-statistics update).  Backward: grad_y read at (g_ld, g_off), the ReLU mask recomputed from z; dz written to dx[i] at
 * x_ld[i] / x_off[i] (the layout of its z), d_gamma / d_beta (ctot).  No float atomics, no host read: bitwise reproducible and
 * graph-capturable.  ws: lidar_bn_relu_train_workspace_bytes(rows, ctot) (pure host; 0 for rows < 1 or channels < 1). */
size_t lidar_bn_relu_train_workspace_bytes(long long rows, int channels);
int lidar_bn_relu_train_forward(int nseg, void *const *x, const int *x_ld, const int *x_off, const int *seg_C, long long rows,
                                const float *gamma, const float *beta, float eps, float *y, int y_ld, int y_off, double *stats,
                                float *scale_shift, float *batch_stats, void *ws, size_t ws_bytes, void *stream);
int lidar_bn_relu_train_backward(int nseg, void *const *x, const int *x_ld, const int *x_off, const int *seg_C, long long rows,
                                 const float *grad_y, int g_ld, int g_off, const float *gamma, const double *stats,
                                 const float *scale_shift, void *const *dx, float *d_gamma, float *d_beta, void *ws, size_t ws_bytes,
                                 void *stream);
/* The residual form, y = max(BN(z) + r, 0), for SparseBasicBlock's bn2 -> += identity -> relu on one (rows, channels) map (the
 * reference's pcdet/models/backbones_3d/spconv_backbone.py:57-62): z / dz at row stride x_ld, the residual r at r_ld, d_r at dr_ld,
 * y at y_ld, grad_y at g_ld (floats; every stride % 4 == 0 and >= channels; no channel offsets).  The same kernels, statistics
 * and fixed-order fp64 reductions as above, with r added before the ReLU; the backward recomputes the mask from
 * z * scale + shift + r > 0, writes d_r = the masked gradient, and dz / d_gamma / d_beta as above.  Supported: channels % 4 == 0,
 * 4 <= channels <= 1024, rows >= 2, 16-byte aligned pointers.  stats / scale_shift / batch_stats / ws as above
 * (lidar_bn_relu_train_workspace_bytes(rows, channels)).  No float atomics, no host read: bitwise reproducible. */
int lidar_bn_add_relu_train_forward(const float *x, int x_ld, const float *r, int r_ld, int channels, long long rows,
                                    const float *gamma, const float *beta, float eps, float *y, int y_ld, double *stats,
                                    float *scale_shift, float *batch_stats, void *ws, size_t ws_bytes, void *stream);
int lidar_bn_add_relu_train_backward(const float *x, int x_ld, const float *r, int r_ld, int channels, long long rows,
                                     const float *grad_y, int g_ld, const float *gamma, const double *stats, const float *scale_shift,
                                     float *dx, float *d_r, int dr_ld, float *d_gamma, float *d_beta, void *ws, size_t ws_bytes,
                                     void *stream);

/* ------------------------------------------------------------------ iou3d_nms
 * boxes are (N,7) f32 [x, y, z, dx, dy, dz, heading].
 * mode 0 = boxes_overlap_bev_gpu (pcdet/ops/iou3d_nms/src/iou3d_nms.cpp:49-68, kernel.cu:236-249)
 * mode 1 = boxes_iou_bev_gpu     (iou3d_nms.cpp:70-88, kernel.cu:251-265);  out (n_a, n_b) f32 */
size_t lidar_iou_workspace_bytes(int n_a, int n_b);
int lidar_boxes_pairwise_bev(const float *boxes_a, int n_a, const float *boxes_b, int n_b, int mode, float *out,
                             void *ws, size_t ws_bytes, void *stream);

/* nms_gpu (iou3d_nms.cpp:90-136) / nms_normal_gpu (:139-186), batched, greedy reduce on the device.
 *   boxes (batch, n_max, 7) already sorted by descending score; counts (batch) i32 device or NULL
 *   keep (batch, n_max) i64 device: positions of kept boxes, ascending; num_keep (batch) i32 device */
size_t lidar_nms_workspace_bytes(int batch, int n_max);
int lidar_nms_batch(const float *boxes, const int *counts, int batch, int n_max, float thresh, int normal,
                    long long *keep, int *num_keep, void *ws, size_t ws_bytes, void *stream);
/* same, but only the first max_keep survivors of each frame are wanted (the caller truncates to NMS_POST_MAXSIZE anyway,
 * pcdet/models/model_utils/model_nms_utils.py:19-21): the greedy pass stops early; num_keep <= max_keep */
int lidar_nms_batch_limited(const float *boxes, const int *counts, int batch, int n_max, float thresh, int normal,
                            int max_keep, long long *keep, int *num_keep, void *ws, size_t ws_bytes, void *stream);
/* test hook: device pointer to the (batch, n_max, ceil(n_max/64)) u64 suppression mask inside ws */
const void *lidar_nms_mask_ptr(void *ws, int batch, int n_max);

/* ------------------------------------------------------------------ pointnet2_stack (stacked-batch layout)
 * Every *_batch_cnt is a (B) i32 DEVICE array of per-sample counts.  Index outputs are i32. */
/* ball_query_wrapper_stack (pcdet/ops/pointnet2/pointnet2_stack/src/ball_query.cpp:31-47, ball_query_gpu.cu:16-66):
 * idx (M, nsample) zero-filled by the caller; an empty ball gets idx[.,0] = -1 */
int lidar_ball_query_stack(int B, int M, float radius, int nsample, const float *new_xyz, const int *new_xyz_batch_cnt,
                           const float *xyz, const int *xyz_batch_cnt, int *idx, void *stream);
/* two radii over the same centres / candidates in one pass (the scales of one StackSAModuleMSG): each idx_x equals what
 * lidar_ball_query_stack returns for (radius_x, nsample_x); every squared distance is computed once */
int lidar_ball_query_stack2(int B, int M, float radius_a, int nsample_a, float radius_b, int nsample_b, const float *new_xyz,
                            const int *new_xyz_batch_cnt, const float *xyz, const int *xyz_batch_cnt, int *idx_a, int *idx_b,
                            void *stream);
/* The same lists through a cell grid over the candidates (csrc/pointnet2.hip: one binning pass per batch element, then three cell
 * rows per centre instead of every candidate; hits are put back into index order at the end).  N = rows of xyz; idx_b == NULL or
 * radius_b <= 0: one radius; nsample <= 64.  ws: lidar_ball_query_grid_workspace_bytes(B, N), uninitialised. */
size_t lidar_ball_query_grid_workspace_bytes(int B, int N);
int lidar_ball_query_stack_grid(int B, int M, int N, float radius_a, int nsample_a, float radius_b, int nsample_b,
                                const float *new_xyz, const int *new_xyz_batch_cnt, const float *xyz, const int *xyz_batch_cnt,
                                int *idx_a, int *idx_b, void *ws, size_t ws_bytes, void *stream);
/* group_points_wrapper_stack (group_points.cpp:31-69 fwd, group_points_gpu.cu:71-102): out (M, C, nsample) */
int lidar_group_points_stack(int B, int M, int C, int nsample, const float *features, const int *features_batch_cnt,
                             const int *idx, const int *idx_batch_cnt, float *out, void *stream);
/* group_points_grad_wrapper_stack (group_points_gpu.cu:15-45): grad_features (N, C) zero-filled by the caller */
/* Row-major grouping for the inference path of StackSAModuleMSG (pointnet2_stack/pointnet2_modules.py:58-92): out (M, nsample,
 * stride) with row (m, s) = [xyz[idx] - new_xyz[m] if use_xyz | features[idx] | zeros up to stride]; idx is the RAW result of
 * lidar_ball_query_stack (-1 in column 0 = empty ball -> zero rows, as QueryAndGroup zeroes them, pointnet2_utils.py:146-152). */
int lidar_group_rows_stack(int B, int M, int C, int nsample, int use_xyz, int stride, const float *xyz, const float *new_xyz,
                           const float *features, const int *features_batch_cnt, const int *idx, const int *idx_batch_cnt,
                           float *out, void *stream);
/* The same layer with the first linear map moved in front of the gather (it commutes with it): table (N, H) =
 * [xyz | features] @ W + b per SOURCE point, query_term (M, H) = new_xyz @ W_xyz per query (or null), and
 * out (M, nsample, H) = relu(table[idx] - query_term[m]); an empty ball gives empty_row (H) = relu(b).  H % 4 == 0. */
int lidar_group_rows_affine_stack(int B, int M, int H, int nsample, const float *table, const float *query_term,
                                  const float *empty_row, const int *features_batch_cnt, const int *idx, const int *idx_batch_cnt,
                                  float *out, void *stream);
/* A two-layer scale in one kernel: the gather above, the second layer on the matrix cores (W2 (H1, H2) row-major, b2) and the max
 * over the samples — out (M, H2) = max_s relu(relu(table[idx] - query_term[m]) @ W2 + b2).  H1 in {16, 32, 64}, 1 <= H2 <= 128,
 * nsample in {8, 16, 32} (lidar_sa_layer2_max_supported); query_term may be null; an empty ball (idx[m][0] < 0) gives
 * relu(empty_row @ W2 + b2).  Dynamic LDS per launch: (H1 * NT * 32 + 4 * 32 * (H1 + 1)) * 4 bytes with NT = ceil(H2 / 32), from
 * 4 224 (H1 16, NT 1) to 66 048 bytes (H1 64, NT 4: 96 < H2 <= 128); the launch requests what exceeds 64 KiB itself
 * (hipFuncAttributeMaxDynamicSharedMemorySize), so every declared shape runs. */
int lidar_sa_layer2_max_supported(int H1, int H2, int nsample);
int lidar_sa_layer2_max_stack(int B, int M, int H1, int H2, int nsample, const float *table, const float *query_term,
                              const float *empty_row, const float *W2, const float *b2, const int *features_batch_cnt,
                              const int *idx, const int *idx_batch_cnt, float *out, void *stream);
int lidar_group_points_grad_stack(int B, int M, int C, int N, int nsample, const float *grad_out, const int *idx,
                                  const int *idx_batch_cnt, const int *features_batch_cnt, float *grad_features,
                                  void *stream);
/* ---- set abstraction, TRAIN mode (csrc/sa_train.hip): StackSAModuleMSG.forward in grad mode
 * (pointnet2_stack/pointnet2_modules.py:58-92: QueryAndGroup -> 1x1 Conv2d / BatchNorm2d / ReLU -> max_pool2d over the samples) on
 * row-major (M * nsample, H) fp32 matrices, row (m, s) at "pair number" m * nsample + s; idx is the RAW ball-query result as for
 * lidar_group_rows_affine_stack (idx[m][0] < 0: empty ball).  Supported (lidar_sa_train_supported, pure host): H % 4 == 0,
 * 4 <= H <= 128, 1 <= nsample <= 64; further M >= 0, N >= 0 (a zero size: no launch, success), M * nsample < 2^31, 16-byte aligned
 * pointers, any per-frame count may be 0.  Anything else: LIDAR_ERR_ARG before any launch.  No float atomics, no host read: bitwise
 * reproducible. */
int lidar_sa_train_supported(int H, int nsample);
/* The first layer in front of the gather, without bias and ReLU (BatchNorm follows): z (M * nsample, H) with row (m, s) =
 * table[start_b + idx[m][s]] - query_term[m] (query_term may be null); the rows of an empty ball are exactly 0 and take part in the
 * batch statistics, as new_features[empty_ball_mask] = 0 feeds the bias-free conv in the reference (pointnet2_utils.py:146-152).
 * N = rows of table. */
int lidar_sa_gather_train_forward(int B, int M, int N, int H, int nsample, const float *table, const float *query_term,
                                  const int *features_batch_cnt, const int *idx, const int *idx_batch_cnt, float *z, void *stream);
/* The inverse index of that gather, in place of the float atomicAdd per element of group_points_grad_kernel_stack
 * (group_points_gpu.cu:15-45): keys (M * nsample) i32 = each pair's global source row, N for the pairs of empty balls (left out).
 * The caller sorts (key, pair number) stably by key -- `pairs` is the sorted pair numbers -- and lidar_sa_row_start turns the sorted
 * keys into row_start (N + 1): source row n is read by pairs[row_start[n] .. row_start[n + 1]), ascending pair numbers, duplicates
 * kept (a ball padded with its first hit lists that source several times).  Entries of `pairs` from row_start[N] on are the
 * left-out pairs. */
int lidar_sa_pair_keys(int B, int M, int N, int nsample, const int *features_batch_cnt, const int *idx, const int *idx_batch_cnt,
                       int *keys, void *stream);
int lidar_sa_row_start(long long num_pairs, int N, const int *sorted_keys, int *row_start, void *stream);
/* d_table (N, H)[n] = sum of dz over n's list in list order (every row written, 0 for an empty list); d_query (M, H)[m] =
 * -sum_s dz[m, s] in ascending s, 0 for an empty ball (d_query may be null).  fp64 accumulators, rounded once. */
int lidar_sa_gather_train_backward(int M, int N, int H, int nsample, const float *dz, const int *idx, const int *row_start,
                                   const int *pairs, float *d_table, float *d_query, void *stream);
/* The last layer's BatchNorm2d (batch statistics over all M * nsample rows) + ReLU + max_pool2d over the samples
 * (pointnet2_modules.py:84-90), fused: out (M, H) = max_s relu(z * scale + shift), arg (M, H) u8 = the lowest s among equal maxima
 * (gamma of either sign); stats / scale_shift / batch_stats as lidar_bn_relu_train_forward lays them out (the caller applies the
 * running-statistics update).  Backward: the gradient of y is grad_out[m, c] at row (m, arg[m, c]) where z * scale + shift > 0
 * (recomputed) and 0 elsewhere; dz (M * nsample, H) is the full BatchNorm backward of it, d_gamma / d_beta (H).  The post-activation
 * (M * nsample, H) tensor is never written.  M * nsample >= 2.  ws: lidar_bn_relu_max_train_workspace_bytes (pure host; 0 outside
 * the support). */
size_t lidar_bn_relu_max_train_workspace_bytes(int M, int nsample, int H);
int lidar_bn_relu_max_train_forward(const float *z, int M, int nsample, int H, const float *gamma, const float *beta, float eps,
                                    float *out, unsigned char *arg, double *stats, float *scale_shift, float *batch_stats, void *ws,
                                    size_t ws_bytes, void *stream);
int lidar_bn_relu_max_train_backward(const float *z, int M, int nsample, int H, const float *grad_out, const unsigned char *arg,
                                     const float *gamma, const double *stats, const float *scale_shift, float *dz, float *d_gamma,
                                     float *d_beta, void *ws, size_t ws_bytes, void *stream);
/* furthest_point_sampling_wrapper (sampling.cpp, sampling_gpu.cu:24-140; same kernel in pointnet2_batch):
 * points (b, n, 3), temp (b, n) = 1e10 on entry, idx (b, m) */
int lidar_furthest_point_sampling(int b, int n, int m, const float *points, float *temp, int *idx, void *stream);
/* three_nn_wrapper_stack (interpolate_gpu.cu:16-75): dist2 (N,3) squared distances, idx (N,3) global indices */
int lidar_three_nn_stack(int B, int N, const float *unknown, const int *unknown_batch_cnt, const float *known,
                         const int *known_batch_cnt, float *dist2, int *idx, void *stream);
/* three_interpolate_wrapper_stack (:107-126) / _grad_ (:151-172): features (M, C), out (N, C) */
int lidar_three_interpolate_stack(int N, int C, const float *features, const int *idx, const float *weight, float *out,
                                  void *stream);
int lidar_three_interpolate_grad_stack(int N, int C, const float *grad_out, const int *idx, const float *weight,
                                       float *grad_features, void *stream);

/* ------------------------------------------------------------------ pointnet2_batch (dense, channel-major)
 * pcdet/ops/pointnet2/pointnet2_batch/src/pointnet2_api.cpp:10-24 */
int lidar_ball_query_batch(int b, int n, int m, float radius, int nsample, const float *new_xyz, const float *xyz,
                           int *idx, void *stream);                       /* ball_query_gpu.cu:15-51 */
int lidar_group_points_batch(int b, int c, int n, int npoints, int nsample, const float *points, const int *idx,
                             float *out, void *stream);                   /* group_points_gpu.cu:53-72 */
int lidar_group_points_grad_batch(int b, int c, int n, int npoints, int nsample, const float *grad_out, const int *idx,
                                  float *grad_points, void *stream);      /* group_points_gpu.cu:14-31 */
int lidar_gather_points_batch(int b, int c, int n, int npoints, const float *points, const int *idx, float *out,
                              void *stream);                              /* sampling_gpu.cu:15-31 */
int lidar_gather_points_grad_batch(int b, int c, int n, int npoints, const float *grad_out, const int *idx,
                                   float *grad_points, void *stream);     /* sampling_gpu.cu:53-70 */
int lidar_three_nn_batch(int b, int n, int m, const float *unknown, const float *known, float *dist2, int *idx,
                         void *stream);                                   /* interpolate_gpu.cu:16-59 */
int lidar_three_interpolate_batch(int b, int c, int m, int n, const float *points, const int *idx, const float *weight,
                                  float *out, void *stream);              /* interpolate_gpu.cu:84-104 */
int lidar_three_interpolate_grad_batch(int b, int c, int n, int m, const float *grad_out, const int *idx,
                                       const float *weight, float *grad_points, void *stream);  /* :127-149 */

/* ------------------------------------------------------------------ roiaware_pool3d / roipoint_pool3d
 * roiaware_pool3d_gpu (pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:29-66): argmax (R,x,y,z,C) i32,
 * pts_idx_of_voxels (R,x,y,z,max_pts) i32 (slot 0 = count) and pooled (R,x,y,z,C) f32 zero-filled by the
 * caller; pool_method 0 = max, 1 = avg; 1 <= out_x/y/z <= 255, max_pts >= 2, channels >= 1.  No (boxes x points) scratch matrix
 * is needed. */
int lidar_roiaware_pool3d_forward(int boxes_num, int pts_num, int channels, int max_pts_each_voxel, int out_x, int out_y,
                                  int out_z, const float *rois, const float *pts, const float *pts_feature, int *argmax,
                                  int *pts_idx_of_voxels, float *pooled_features, int pool_method, void *stream);
/* roiaware_pool3d_gpu_backward (roiaware_pool3d.cpp:68-96): grad_in (P, C) zero-filled by the caller */
int lidar_roiaware_pool3d_backward(int boxes_num, int out_x, int out_y, int out_z, int channels, int max_pts_each_voxel,
                                   const int *pts_idx_of_voxels, const int *argmax, const float *grad_out,
                                   float *grad_in, int pool_method, void *stream);
/* points_in_boxes_gpu (roiaware_pool3d.cpp:98-118): boxes (B,T,7), pts (B,P,3), box_idx_of_points (B,P) pre-filled -1 */
int lidar_points_in_boxes(int batch, int boxes_num, int pts_num, const float *boxes, const float *pts,
                          int *box_idx_of_points, void *stream);
/* roipool3d_gpu (pcdet/ops/roipoint_pool3d/src/roipoint_pool3d.cpp:23-54): xyz (B,N,3), boxes3d (B,M,7) already
 * enlarged, pts_feature (B,N,C) -> pooled (B,M,S,3+C), empty_flag (B,M); both zero-filled by the caller; S <= 1024 */
int lidar_roipoint_pool3d_forward(int batch, int pts_num, int boxes_num, int feature_len, int sampled_pts_num,
                                  const float *xyz, const float *boxes3d, const float *pts_feature,
                                  float *pooled_features, int *pooled_empty_flag, void *stream);

/* ------------------------------------------------------------------ sparse 3D convolution (spconv v1.x semantics)
 * Replaces the external, un-vendored `spconv` package (docs/INSTALL.md:9,28-29; call sites
 * pcdet/models/backbones_3d/spconv_backbone.py:3-26,76-116, spconv_unet.py, roi_heads/partA2_head.py).
 * indices are (N,4) i32 [b,z,y,x]; spatial shape (D,H,W); kernel offsets enumerate (kz,ky,kx) row-major.
 * Rulebooks are neighbour tables nbr (N_out, K) i32: nbr[j][k] = input row feeding output row j through
 * offset k, or -1 (spconv.ops.get_indice_pairs gives the same relation as per-offset pair lists). */
size_t lidar_spconv_hash_capacity(int n);            /* slots; table memory = capacity * 12 bytes */
int lidar_spconv_build_hash(const int *indices, int n, int D, int H, int W, void *table, size_t capacity, void *stream);
/* SubMConv3d rulebook: outputs == inputs (same row order) */
int lidar_spconv_subm_table(const int *indices, int n, int D, int H, int W, int kD, int kH, int kW, const void *table,
                            size_t capacity, int *nbr, void *stream);
/* SparseConv3d rulebook in two phases (the caller reads *num_out in between to size nbr):
 *   phase 1 -> out_indices (out_cap >= n*prod ceil(k/s) rows, 4), *num_out; output rows in first-touch order
 *   phase 2 -> nbr (num_out, K) and nbr_t (n, K) = transposed table (inverse conv / input gradient)
 * Refused with LIDAR_ERR_ARG before any launch, by phase 1 (lidar_spconv_conv_outputs) and by the grid builder's entry points
 * below alike: a kernel size, stride, batch or extent <= 0, and a padded input thinner than the kernel along an axis (D + 2 pD <
 * kD, ...: such a level has no output site; even kernels, mixed strides, stride > kernel and an extent of 1 with padding are all
 * fine).  Phase 2 (lidar_spconv_conv_tables) takes no extents: it checks kernel, stride and counts only and relies on the
 * workspace phase 1 filled.  lidar_spconv_build_hash refuses a capacity that is not a power of two or is below 2 n.
 * Duplicated input coordinates: the LOWEST row is the one the forward tables (nbr, SubM table) name; in nbr_t every row of the
 * coordinate, the losing ones included, holds the output rows its coordinate reaches (both builders). */
size_t lidar_spconv_conv_table_workspace_bytes(int n, int kD, int kH, int kW, int sD, int sH, int sW);
int lidar_spconv_conv_outputs(const int *indices, int n, int batch, int D, int H, int W, int kD, int kH, int kW, int sD,
                              int sH, int sW, int pD, int pH, int pW, int *out_indices, int out_cap, int *num_out,
                              void *ws, size_t ws_bytes, void *stream);
int lidar_spconv_conv_tables(int n, int kD, int kH, int kW, int sD, int sH, int sW, int num_out, int *nbr, int *nbr_t,
                             void *ws, size_t ws_bytes, void *stream);
/* The same rulebooks through DENSE index grids (csrc/rulebook_grid.hip): one persistent (batch, D, H, W) int32 grid per resolution
 * level, owned by the caller, every cell "empty" (0x7FFFFFFF) between uses; a coordinate lookup is one load instead of a hash probe
 * sequence, and nothing is built or cleared per table.  Tables and output numbering are identical to the hash builder's.
 *   lidar_spconv_grid_init     once per grid
 *   lidar_spconv_grid_rows     mode 0: rows of a tensor -> grid (atomicMin: duplicates keep the lowest row); 1: the same cells
 *                              back to empty; 2: plain store (output rows after lidar_spconv_grid_outputs); n_dev optional
 *   lidar_spconv_grid_table    nbr (n_out, K): SubM (stride 1, padding k / 2, out_indices = the input rows) or regular forward
 *   lidar_spconv_grid_table_t  nbr_t (n, K) of a regular convolution, from the OUTPUT level's grid
 *   lidar_spconv_grid_outputs  unique output sites in first-touch order -> out_indices, *num_out (device); grid_out (empty on
 *                              entry) is left holding candidate ids: follow with lidar_spconv_grid_rows(out_indices, mode 2)
 * Capacity-sized tensors (no host read-back of *num_out): a row whose batch index is negative is a PADDING row — no neighbours
 * (tables hold -1), reaches no output, never scattered.  lidar_spconv_grid_pad_rows turns rows [min(*num_dev, cap), cap) of
 * out_indices into padding rows; `limit` of the table builders = row count of the tensor the looked-up grid holds (grid values
 * >= limit read as "no row"; <= 0: no limit), so a capacity that turns out too small yields wrong tables, never wild row ids.
 * `batch` = frames the grids were allocated for: a row whose batch index lies outside [0, batch) is treated like a padding row
 * (skipped), never an out-of-bounds access.
 *   lidar_spconv_transpose_table  nbr_t (n_in, K), pre-filled with -1 by the caller, from nbr (n_out, K) alone:
 *                              nbr[j][k] == i  <=>  nbr_t[i][k] == j (equals grid_table_t when input coordinates are unique) */
int lidar_spconv_grid_init(int *grid, size_t cells, void *stream);
int lidar_spconv_grid_rows(const int *indices, int n, const int *n_dev, int batch, int D, int H, int W, int *grid, int mode, void *stream);
int lidar_spconv_grid_table(const int *out_indices, int n_out, int batch, int D, int H, int W, int kD, int kH, int kW, int sD, int sH, int sW,
                            int pD, int pH, int pW, const int *grid_in, int limit, int *nbr, void *stream);
int lidar_spconv_grid_table_t(const int *indices, int n, int batch, int D, int H, int W, int kD, int kH, int kW, int sD, int sH, int sW, int pD,
                              int pH, int pW, const int *grid_out, int limit, int *nbr_t, void *stream);
int lidar_spconv_grid_pad_rows(int *out_indices, const int *num_dev, int cap, void *stream);
int lidar_spconv_transpose_table(const int *nbr, int n_out, int K, int n_in, int *nbr_t, void *stream);
size_t lidar_spconv_grid_outputs_workspace_bytes(int n, int K);
int lidar_spconv_grid_outputs(const int *indices, int n, int batch, int D, int H, int W, int kD, int kH, int kW, int sD, int sH, int sW, int pD,
                              int pH, int pW, int *grid_out, int *out_indices, int *num_out, void *ws, size_t ws_bytes,
                              void *stream);
/* indice_conv forward (and input gradient with the transposed table + transposed weights):
 * out (n_out, Cout) = sum_k in[nbr[., k]] @ weight[k] (+ bias); weight (K, Cin, Cout); fp32 MFMA; 1 <= Cin, Cout <= 128, any K > 0,
 * n_out >= 0 (0: nothing is launched); everything else is LIDAR_ERR_ARG before any launch.
 *
 * Limits on K of the mask-ordered route, in one place:
 *   lidar_spconv_row_masks                  K <= 32   one bit per offset in an int32; offset 31 is the SIGN bit of the mask
 *   lidar_spconv_sorted_gemm_supported      K <= 32   and Cin in {16, 32, 64, 128}, Cout % 4 == 0, 1 <= Cout <= 128; the sorted entry points
 *   lidar_spconv_packed_floats (!= 0)                 take both row_mask and order or (n_out == 0) neither, and refuse any other shape
 *   lidar_spconv_mask_group                 K <= 31   its bin key holds K - popcount(mask) in 5 bits
 *   spconv/ops.py sorted_gemm_supported     K <= 31   (it orders rows with lidar_spconv_mask_group)
 * K = 32 on the mask-ordered route is therefore reached with lidar_spconv_row_masks + any sort of the (signed) masks, not through
 * ops.mask_order; tests/test_gpu_spconv_kernel_support.py runs it. */
int lidar_spconv_implicit_gemm(const float *in_features, const int *nbr, int n_out, int K, int Cin, int Cout,
                               const float *weight, const float *bias, float *out_features, void *stream);
/* the same GEMM with the inference epilogue of the reference's SubMConv3d/SparseConv3d + BatchNorm1d + ReLU triplets
 * (pcdet/models/backbones_3d/spconv_backbone.py:20-26; BN scale folded into `weight`, shift passed as `bias`) and of
 * SparseBasicBlock (spconv_backbone.py:49-63): out = act(gemm + bias + residual); residual (n_out, Cout) or NULL */
int lidar_spconv_implicit_gemm_fused(const float *in_features, const int *nbr, int n_out, int K, int Cin, int Cout,
                                     const float *weight, const float *bias, const float *residual, int relu,
                                     float *out_features, void *stream);
/* Mask-sorted execution of the same GEMM: on LiDAR occupancy a site has 3-13 of its 27 neighbours, so in table order most
 * MFMA rows of a 32-row tile are padding.  lidar_spconv_row_masks gives each row's offset bit mask (K <= 32); the caller
 * argsorts the masks (any device sort) and passes the order: workgroup row i computes table / output row order[i], so
 * rows with equal masks share MFMA tiles and offsets unused by a whole workgroup are skipped entirely.  Every output
 * still sums the same products in the same (offset) order: results are bit-identical to the table-order call. */
int lidar_spconv_row_masks(const int *nbr, int n_out, int K, int *masks, void *stream);
/* Row order for lidar_spconv_implicit_gemm_sorted WITHOUT a sort: every row finds its mask's group in an open-addressing table
 * (a table holds only a few thousand distinct masks) and takes a rank in it; groups are laid out by their top 12 mask bits (measured:
 * as good for the GEMM as a full sort), a row's position = first position of its group + its rank.  masks (n_out): bit k =
 * nbr[row][k] >= 0; order (n_out): table row visited i-th — equal masks contiguous, groups ascending in their top 12 bits.
 * 3 launches, no host sync.  The workspace keeps the table, which must be empty when a call starts (lidar_spconv_mask_group_init
 * once per buffer; every call leaves it empty) and whose layout depends on the buffer size only: always pass the same (ws,
 * ws_bytes) pair, sized for the largest table, and do not share one workspace between streams.  K <= 31. */
size_t lidar_spconv_mask_group_workspace_bytes(int n_out);
int lidar_spconv_mask_group_init(void *ws, size_t ws_bytes, void *stream);
int lidar_spconv_mask_group(const int *nbr, int n_out, int K, int *masks, int *order, void *ws, size_t ws_bytes, void *stream);
int lidar_spconv_sorted_gemm_supported(int K, int Cin, int Cout);
int lidar_spconv_implicit_gemm_sorted(const float *in_features, const int *nbr, const int *row_mask, const int *order,
                                      int n_out, int K, int Cin, int Cout, const float *weight, const float *bias,
                                      const float *residual, int relu, float *out_features, void *stream);
/* The same GEMM reading the weights in PACKED form: lidar_spconv_pack_weights lays the folded (K, Cin, Cout) weights out in the
 * order the MFMA lanes consume them (once per weight update; lidar_spconv_packed_floats floats, 0 = shape not supported:
 * Cin in {16, 32, 64, 128}, Cout % 4 == 0, K <= 32), so that a stage goes global -> LDS by LDS-DMA and the B operands of four
 * MFMA steps are one 128-bit LDS read.  Same products in the same order: bit-identical to lidar_spconv_implicit_gemm_sorted. */
size_t lidar_spconv_packed_floats(int K, int Cin, int Cout);
int lidar_spconv_pack_weights(const float *weight, int K, int Cin, int Cout, float *packed, void *stream);
int lidar_spconv_implicit_gemm_sorted_packed(const float *in_features, const int *nbr, const int *row_mask, const int *order,
                                             int n_out, int K, int Cin, int Cout, const float *packed, const float *bias,
                                             const float *residual, int relu, float *out_features, void *stream);
/* weight gradient: grad_weight (K, Cin, Cout) += sum_j in[nbr[j][k]]^T (x) grad_out[j]; zero-filled by the caller */
int lidar_spconv_wgrad(const float *in_features, const float *grad_out, const int *nbr, int n_out, int K, int Cin, int Cout,
                       float *grad_weight, void *stream);
/* weight gradient on the matrix cores: same contraction as lidar_spconv_wgrad, grad_weight overwritten (no zero fill),
 * deterministic (per-chunk partials in `ws`, summed in order); order = mask order of nbr's rows (lidar_spconv_row_masks +
 * argsort) or NULL; Cin, Cout in {16, 32, 64, 128} (lidar_spconv_wgrad_mfma_supported). */
int lidar_spconv_wgrad_mfma_supported(int K, int Cin, int Cout);
size_t lidar_spconv_wgrad_workspace_bytes(int n_out, int K, int Cin, int Cout);
int lidar_spconv_wgrad_mfma(const float *in_features, const float *grad_out, const int *nbr, const int *order, int n_out, int K,
                            int Cin, int Cout, float *grad_weight, void *ws, size_t ws_bytes, void *stream);
/* SparseConvTensor.dense(): (N, C) rows at (N,4) indices -> (B, C, D, H, W), every element written once */
size_t lidar_sparse_to_dense_workspace_bytes(int batch, int D, int H, int W);
int lidar_sparse_to_dense(const float *features, const int *indices, int n, int channels, int batch, int D, int H, int W,
                          float *out, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ dense BEV backbone epilogue
 * Eval-mode BatchNorm2d + ReLU after every Conv2d / ConvTranspose2d of BaseBEVBackbone
 * (pcdet/models/backbones_2d/base_bev_backbone.py:34-45,51-57) with the BN scale folded into the weights: one pass
 * out[pix][out_off + c] = act(in[pix][c] + bias[c]) over NHWC rows; out may alias in (out_C == C, out_off == 0) or be
 * the channel slice of the concatenated map (base_bev_backbone.py:103).  C, out_C, out_off multiples of 4. */
int lidar_bias_act_nhwc(const float *in, const float *bias, long long n_pix, int C, int relu, float *out, int out_C,
                        int out_off, void *stream);
/* Same epilogue for a ConvTranspose2d with kernel == stride == s (base_bev_backbone.py:51-55) evaluated as a GEMM:
 * in (batch*h*w, s*s*C) with column order (ky, kx, c); out[b][s*y+ky][s*x+kx][out_off + c] = act(in + bias[c]). */
int lidar_bias_act_upsample_nhwc(const float *in, const float *bias, int batch, int h, int w, int s, int C, int relu,
                                 float *out, int out_C, int out_off, void *stream);
/* A ConvTranspose2d / Conv2d with kernel == stride == 1 (the first deblock, base_bev_backbone.py:58-77) + folded BatchNorm +
 * ReLU as ONE library GEMM (hipBLASLt, RELU_BIAS epilogue) writing with a leading dimension:
 * D[m][0..N) = act(A (M, K) @ W (K, N) + bias (N)), row m of D at D + m * ldd — i.e. straight into the layer's channel slice
 * of the concatenated NHWC map (base_bev_backbone.py:103).  ws: scratch for the library (may be null / 0).  Returns
 * LIDAR_ERR_UNSUPPORTED when the library is not loadable or has no kernel for the problem. */
int lidar_dense_gemm_bias_act(const float *A, long long M, int K, const float *W, int N, const float *bias, int relu,
                              float *D, int ldd, void *ws, size_t ws_bytes, void *stream);
/* The library offers several kernels per shape and the wrapper keeps the one that timed fastest at the first call.  For N ranks
 * to run the SAME kernel (the reference's DDP ranks all run cuDNN's deterministic heuristic pick: pcdet/utils/common_utils.py:170-184
 * launches identical processes), rank 0's picks are exported — 7 ints per shape — and imported by the others before their first
 * call.  export returns the number of plans (writes at most cap). */
int lidar_dense_gemm_export_choices(int *out7, int cap);
int lidar_dense_gemm_import_choices(const int *in7, int n);

/* 3x3 / stride 1 / padding 1 fp32 convolution + folded BatchNorm shift + ReLU on NHWC maps — the LAYER_NUMS stride-1 layers of
 * every BaseBEVBackbone block (pcdet/models/backbones_2d/base_bev_backbone.py:34-45) — as Winograd F(2x2, 3x3) on the fp32 matrix
 * cores (csrc/wino_conv.hip): 2.25x fewer MFMA cycles than the direct form, |error| ~ 1e-6 of the output scale.
 * lidar_wino_pack_weights: w (Cout, Cin, 3, 3) contiguous (BatchNorm scale already folded in) -> `packed`, lidar_wino_packed_floats
 * (Cin, Cout) floats (0: shape not supported — Cin % 8 == 0, Cin >= 16 and Cout % 32 == 0 are); once per weight update.
 * lidar_wino_conv3x3_nhwc: out[b][y][x][out_off + co] = act(conv(in, w)[b][y][x][co] + bias[co]), `in` (B, H, W, Cin), `out`
 * (B, H, W, out_C) — out_off / out_C as in lidar_bias_act_nhwc (a slice of the concatenated map); bias may be null. */
size_t lidar_wino_packed_floats(int Cin, int Cout);
int lidar_wino_supported(int Cin, int Cout);
int lidar_wino_pack_weights(const float *w, int Cin, int Cout, float *packed, void *stream);
int lidar_wino_conv3x3_nhwc(const float *in, int B, int H, int W, int Cin, const float *packed, const float *bias, int relu, int Cout,
                            float *out, int out_C, int out_off, void *stream);
/* Grouped form — n_groups independent 3x3 convolutions in one launch: group g reads input channels [g * group_cin, (g + 1) *
 * group_cin) of the (B, H, W, in_C) map and writes output channels [32 g, 32 g + 32) (fewer real outputs: zero-padded filters) — the
 * second-layer branch convolutions of AnchorHeadMulti's SEPARATE_MULTIHEAD heads (pcdet/models/dense_heads/anchor_head_multi.py:60-110).
 * packed = lidar_wino_pack_weights of the stacked (32 n_groups, group_cin, 3, 3) filters; bias: 32 n_groups values or null. */
int lidar_wino_conv3x3_grouped_nhwc(const float *in, int B, int H, int W, int in_C, int group_cin, int n_groups, const float *packed,
                                    const float *bias, int relu, float *out, int out_C, int out_off, void *stream);
/* ... with a COMPACT output: group g keeps its grp_cout[g] (<= 32) real channels at [out_off + grp_ooff[g], + grp_cout[g]) of the
 * (B, H, W, out_C) map (device int arrays; ranges must fit and not overlap); the padded channels never reach memory. */
int lidar_wino_conv3x3_grouped_compact_nhwc(const float *in, int B, int H, int W, int in_C, int group_cin, int n_groups,
                                            const float *packed, const float *bias, int relu, const int *grp_cout, const int *grp_ooff,
                                            float *out, int out_C, int out_off, void *stream);

/* The same stride-1 3x3 layers as Winograd F(4x4, 3x3) (csrc/wino43_conv.hip): 4x fewer MFMA cycles than the direct form (F(2x2):
 * 2.25x), interpolation points {0, 1, -1, 1/2, -2, inf}, filter transform in fp64; |error| ~ 1e-5 of the output scale (asserted at
 * 1e-4 against the fp64 convolution).  Supported: Cin % 16 == 0, Cin >= 32, Cout % 64 == 0 (lidar_wino43_packed_floats = 36 Cin Cout,
 * 0 = unsupported).  `in` is (B, H, W, in_C) and the layer reads channels [0, Cin); the input and output maps stay below 2^31 bytes each.  Replaces the same reference
 * layers as lidar_wino_conv3x3_nhwc (pcdet/models/backbones_2d/base_bev_backbone.py:34-45). */
size_t lidar_wino43_packed_floats(int Cin, int Cout);
int lidar_wino43_supported(int Cin, int Cout);
int lidar_wino43_pack_weights(const float *w, int Cin, int Cout, float *packed, void *stream);
int lidar_wino43_conv3x3_nhwc(const float *in, int B, int H, int W, int Cin, int in_C, const float *packed, const float *bias, int relu,
                              int Cout, float *out, int out_C, int out_off, void *stream);
/* The same kernel in its shared-transform workgroup shape (one tile group x four blocks of 32 output channels: the input transform
 * and the region DMA of a tile group run once per 128 output channels instead of once per 64).  Bit-identical results; supported:
 * Cin % 16 == 0, Cin >= 32, Cout % 128 == 0.  The waves walk the 36 positions in another order, so the filters have their OWN packed
 * layout: `packed` of lidar_wino43s_conv3x3_nhwc comes from lidar_wino43s_pack_weights (lidar_wino43s_packed_floats = 36 Cin Cout
 * floats, 0 = unsupported), never from lidar_wino43_pack_weights, and the other way round.  Everything else as above. */
size_t lidar_wino43s_packed_floats(int Cin, int Cout);
int lidar_wino43s_supported(int Cin, int Cout);
int lidar_wino43s_pack_weights(const float *w, int Cin, int Cout, float *packed, void *stream);
int lidar_wino43s_conv3x3_nhwc(const float *in, int B, int H, int W, int Cin, int in_C, const float *packed, const float *bias, int relu,
                               int Cout, float *out, int out_C, int out_off, void *stream);

/* The WEIGHT GRADIENT of the same layers (training; torch hands it to MIOpen) as Winograd F(3x3, 4x4) on the fp32 matrix cores
 * (csrc/wino43_wgrad.hip): dw[co][ci][a][b] = sum_{n,h,w} g[n][h][w][co] x[n][h + a - 1][w + b - 1][ci] with zero padding, 36
 * multiplications per 4 x 4 tile and (ci, co) where the direct sum needs 144.  x: (B, H, W) pixels of x_ld floats, channels [0, Cin);
 * g (the output gradient): (B, H, W) pixels of g_ld floats, channels [0, Cout); any H, W >= 1; each map below 2^31 - 1 bytes.
 * dw: contiguous (Cout, Cin, 3, 3), OVERWRITTEN.  Supported: Cin, Cout multiples of 32 in [32, 512].  fp32 MFMA accumulation over
 * at most 512 tiles, partial sums in ws (plain stores; its previous contents do not matter), summed in fixed order in fp64 together
 * with the output transform, one rounding to fp32: no float atomics, bitwise reproducible, no host read, graph-capturable.
 * ws: lidar_wino43_wgrad_workspace_bytes (pure host; 0 for unsupported or empty shapes), 16-byte aligned. */
int lidar_wino43_wgrad_supported(int Cin, int Cout);
size_t lidar_wino43_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout);
int lidar_wino43_wgrad_nhwc(const float *x, int x_ld, const float *g, int g_ld, int B, int H, int W, int Cin, int Cout, float *dw,
                            void *ws, size_t ws_bytes, void *stream);

/* ConvTranspose2d with kernel == stride == s (the deblocks of BaseBEVBackbone, base_bev_backbone.py:51-57) + folded BatchNorm shift
 * + ReLU + the write into the layer's channel slice of the concatenated map (base_bev_backbone.py:103) as ONE fp32-MFMA kernel
 * (csrc/deconv_gemm.hip): out[b][s y + ky][s x + kx][out_off + c] = act(sum_k in[b][y][x][k] W[k][(ky, kx, c)] + bias[c]).
 * W: (K, s * s * C_up) row-major, columns ordered (ky, kx, c); packed once per weight update (lidar_deconv_pack_weights,
 * lidar_deconv_packed_floats floats; 0 = unsupported: K % 8 == 0, K >= 16, C_up % 128 == 0 and s * s * C_up % 512 == 0 are supported). */
size_t lidar_deconv_packed_floats(int K, int N);
int lidar_deconv_supported(int K, int s, int C_up);
int lidar_deconv_pack_weights(const float *W, int K, int N, float *packed, void *stream);
int lidar_deconv_gemm_nhwc(const float *in, int B, int h, int w, int K, const float *packed, const float *bias, int relu, int s, int C_up,
                           float *out, int out_C, int out_off, void *stream);

/* The two GRADIENTS of the same layer without bias (training; torch hands them to MIOpen) as fp32-MFMA GEMMs on the NHWC maps
 * (csrc/deconv_train.hip).  p = (b, y, x) runs over the P = B h w input pixels; W is the module's weight in torch's own layout
 * (K, C_up, s, s), contiguous; g (the gradient of the layer's output): (B, s h, s w) pixels of g_ld floats, channels [0, C_up).
 *   lidar_deconv_dgrad_nhwc:  dx[p][k] = sum_{ky,kx,c} g[b][s y + ky][s x + kx][c] W[k][c][ky][kx], written at the row stride
 *     dx_ld >= K (columns [K, dx_ld) are not touched); the reduction (s^2 C_up long) is not split: bitwise reproducible.
 *   lidar_deconv_wgrad_nhwc:  dw[k][c][ky][kx] = sum_p x[p][k] g[b][s y + ky][s x + kx][c]; x: P pixels of x_ld floats, channels
 *     [0, K); dw: contiguous (K, C_up, s, s), OVERWRITTEN (never read).  fp32 MFMA accumulation over at most 4096 pixels, partial sums
 *     in ws (plain stores; its previous contents do not matter), summed in fixed order in fp64, one rounding to fp32: no float
 *     atomics, bitwise reproducible, no host read, graph-capturable.  ws: lidar_deconv_wgrad_workspace_bytes (pure host; 0 for
 *     unsupported or empty shapes), 16-byte aligned; LIDAR_ERR_WORKSPACE when it is missing or short.
 * Supported (lidar_deconv_train_supported, pure host; everything else is refused with LIDAR_ERR_ARG): s in {1, 2, 4}, K % 8 == 0 in
 * [LIDAR_DECONV_TRAIN_MIN_K, LIDAR_DECONV_TRAIN_MAX_C], C_up % 32 == 0 in [LIDAR_DECONV_TRAIN_MIN_CUP, LIDAR_DECONV_TRAIN_MAX_C].
 * x and g are 16-byte aligned with x_ld % 4 == 0 and g_ld % 4 == 0; each map (x, g, dx at their row strides) stays below 2^31 - 1
 * bytes.  Every argument is checked before any launch. */
#define LIDAR_DECONV_TRAIN_MIN_K 16
#define LIDAR_DECONV_TRAIN_MIN_CUP 32
#define LIDAR_DECONV_TRAIN_MAX_C 512
int lidar_deconv_train_supported(int K, int s, int C_up);
size_t lidar_deconv_wgrad_workspace_bytes(int B, int h, int w, int K, int s, int C_up);
int lidar_deconv_dgrad_nhwc(const float *g, int g_ld, const float *W, int B, int h, int w, int K, int s, int C_up, float *dx, int dx_ld,
                            void *stream);
int lidar_deconv_wgrad_nhwc(const float *x, int x_ld, const float *g, int g_ld, int B, int h, int w, int K, int s, int C_up, float *dw,
                            void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ anchor-head post-processing feeding NMS (8f rank 1)
 * head: (n_loc = B*H*W, row_stride) rows of the merged head output [cls | box | dir] as the 1x1 heads emit it
 * (pcdet/models/dense_heads/anchor_head_single.py:45-55).  Anchor index = loc * anchors_per_loc + a, class logit
 * channel = cls_off + a * num_class + c (the view(batch, num_anchors, -1) of anchor_head_template.py:247-250).
 * lidar_anchor_scores: scores[i] = max_c sigmoid(logit) if >= score_thresh else -1, labels[i] = argmax_c
 *   (detector3d_template.py:205-230 + model_nms_utils.py:6-10).
 * lidar_decode_topk: boxes (batch, k, 7) = ResidualCoder.decode_torch (box_coder_utils.py:45-77) + direction-bin
 *   correction (anchor_head_template.py:253-266) of the anchors picked by top_idx (batch, k) int64 (per-frame anchor ids);
 *   anchors (n_anchor_per_frame, 7). */
int lidar_anchor_scores(const float *head, long long n_loc, int row_stride, int cls_off, int anchors_per_loc, int num_class,
                        float score_thresh, float *scores, unsigned char *labels, void *stream);
int lidar_decode_topk(const float *head, int batch, long long locs_per_frame, int row_stride, int box_off, int dir_off,
                      int anchors_per_loc, int num_dir_bins, const long long *top_idx, int k, const float *anchors,
                      float dir_offset, float dir_limit_offset, float period, float *boxes, void *stream);
/* The box / direction heads at the selected anchors only (csrc/head_rows.hip, csrc/anchor_post.hip).  The reference computes
 * conv_box and conv_dir_cls on the whole map (pcdet/models/dense_heads/anchor_head_single.py:45-55) and class_agnostic_nms then
 * gathers box_preds at the top-k indices (pcdet/models/model_utils/model_nms_utils.py:6-25); here the 1x1 product itself runs for
 * those anchors only.
 *   lidar_head_rows_supported  C % 4 == 0, 4 <= C <= LIDAR_HEAD_ROWS_MAX_C, anchors_per_loc in [1, 8], num_dir_bins in [0, 4], a part
 *                              map of part_bytes < 2^31 - 1 bytes.  Host only.
 *   lidar_head_rows            part0 / part1: n_parts (1 or 2) NHWC maps of frames_per_part frames x locs_per_frame rows x C floats
 *                              (16-byte aligned); frame f lives in part f / frames_per_part.  head_wt (C, ldw) row-major and head_b
 *                              (ldw) are the merged head's weight and bias; anchor a of a location reads columns box_off + 7 a .. + 7
 *                              and dir_off + num_dir_bins a .. + num_dir_bins.  idx: (batch, k) int64 per-frame anchor ids
 *                              (loc * anchors_per_loc + a, inside [0, locs_per_frame * anchors_per_loc): the caller's duty), or NULL
 *                              = every anchor in order (k must be locs_per_frame * anchors_per_loc).
 *                              -> out (batch, k, 7 + num_dir_bins) logits [7 box residuals | direction logits].  A value depends
 *                              only on its row and its weight column (fixed summation order, no atomics): the same anchor gives the
 *                              same bits at any list position, frame, part and in either mode.  batch == 0 or k == 0: nothing written.
 *   lidar_decode_topk_rows     lidar_decode_topk reading such compact logits (batch, k, 7 + num_dir_bins) instead of the head map:
 *                              the same device function, bit-equal boxes for bit-equal logits. */
#define LIDAR_HEAD_ROWS_MAX_C 1024
#define LIDAR_HEAD_ROWS_MAX_ANCHORS 8
#define LIDAR_HEAD_ROWS_MAX_DIR_BINS 4
int lidar_head_rows_supported(int C, int anchors_per_loc, int num_dir_bins, long long part_bytes);
int lidar_head_rows(const float *part0, const float *part1, int n_parts, int frames_per_part, long long locs_per_frame, int C,
                    const float *head_wt, int ldw, const float *head_b, int box_off, int dir_off, int anchors_per_loc, int num_dir_bins,
                    const long long *idx, int batch, long long k, float *out, void *stream);
int lidar_decode_topk_rows(const float *logits, int batch, int k, int num_dir_bins, const long long *top_idx, const float *anchors,
                           float dir_offset, float dir_limit_offset, float period, float *boxes, void *stream);
/* Exact top-k of the masked scores that feed NMS (reference: torch.topk(box_scores, k = min(NMS_PRE_MAXSIZE, n)) in
 * class_agnostic_nms, pcdet/models/model_utils/model_nms_utils.py:9-11) for a whole batch, deterministic — descending score, ties by
 * ascending anchor index (torch.topk leaves ties unspecified) — in 3 launches, no host synchronisation (csrc/topk.hip).
 *   lidar_topk_workspace_bytes / _init   workspace for (batch, n) scores; init once per buffer (histograms start at zero)
 *   lidar_anchor_scores_hist             = lidar_anchor_scores on (batch, locs_per_frame, row_stride) head rows, and counts every score
 *                                        >= score_thresh into the workspace's per-frame histogram (launch 1 of the 3)
 *   lidar_topk_desc                      scores (batch, n) f32, n % 4 == 0, rows 16-B aligned; k <= 4096; candidates = scores >=
 *                                        valid_min (> 0); hist_ready: the histogram was filled by lidar_anchor_scores_hist with
 *                                        score_thresh == valid_min (scores <= score_max); else one more pass builds it.
 *                                        -> top_scores (batch, k), top_idx (batch, k) i64, counts (batch) i32 = candidates kept;
 *                                        slots past counts[b] hold (-1, 0) */
size_t lidar_topk_workspace_bytes(int batch, long long n);
int lidar_topk_workspace_init(void *ws, size_t ws_bytes, int batch, long long n, void *stream);
int lidar_anchor_scores_hist(const float *head, int batch, long long locs_per_frame, int row_stride, int cls_off, int anchors_per_loc,
                             int num_class, float score_thresh, float *scores, unsigned char *labels, void *ws, size_t ws_bytes,
                             void *stream);
int lidar_topk_desc(const float *scores, int batch, long long n, int k, float valid_min, float score_max, int hist_ready,
                    float *top_scores, long long *top_idx, int *counts, void *ws, size_t ws_bytes, void *stream);
/* Everything between the NMS keep lists and the detector's output, batched, one launch (reference, per sample:
 * selected = keep[:NMS_POST_MAXSIZE]; final boxes / scores / labels by index chains — pcdet/models/model_utils/
 * model_nms_utils.py:19-25, pcdet/models/detectors/detector3d_template.py:236-262).  boxes (batch, k, 7), top_scores (batch, k),
 * top_idx (batch, k) i64 anchor ids, labels (batch, n) u8 class ids, keep (batch, keep_stride) i64 candidate positions, num_keep
 * (batch) -> out_boxes (batch, post, 7), out_scores (batch, post), out_labels (batch, post) i64 = class + 1, out_num (batch) =
 * min(num_keep, post); slots past out_num repeat candidate 0. */
int lidar_post_nms_gather(const float *boxes, const float *top_scores, const long long *top_idx, const unsigned char *labels,
                          const long long *keep, const int *num_keep, int batch, int k, long long n, int keep_stride, int post,
                          float *out_boxes, float *out_scores, long long *out_labels, int *out_num, void *stream);

/* ------------------------------------------------------------------ anchor target assignment (training)
 * AxisAlignedTargetAssigner.assign_targets (pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py:37-129,
 * assign_targets_single :131-210; built in anchor_head_template.py:55-72, called from :90-101) on its deterministic path
 * (POS_FRACTION < 0, MATCH_HEIGHT False) for a whole batch and every anchor class, no host synchronisation (csrc/anchor_assign.hip).
 * Matching: nearest-BEV IoU (pcdet/utils/box_utils.py:238-287, limit_period pcdet/utils/common_utils.py:52-55); targets:
 * ResidualCoder.encode_torch (pcdet/utils/box_coder_utils.py:13-42).
 *   anchors, counts, per_loc, out_off, matched, unmatched, remap   HOST arrays of num_classes (<= 16) entries, passed by value in
 *       the kernel arguments: DEVICE pointer to the class's contiguous (counts[k], anchor_dim) anchors, anchors per output location,
 *       output offset, thresholds, and the SEPERATE_MULTIHEAD label id (> 0) or 0 = the gt's own class id.  Anchor i of class k goes
 *       to output anchor (i / per_loc[k]) * a_total + out_off[k] + i % per_loc[k] (single head: the view(*fmap, -1) + cat(dim=-1)
 *       of :102-115; multihead: per_loc = counts, out_off = running sum, :92-100).
 *   class_of_id   HOST (128) int8: entry id + 64, for gt class ids -64..63 -> anchor class index or -1 (class_names[id - 1] ==
 *                 anchor class name with numpy's wrap, :61-66; ids past the name list, where the reference raises, match none)
 *   gt (batch, max_gt, gt_cols) f32 [box (gt_cols - 1) | class id]; gt_enlarged: same shape or NULL (its boxes are encoded)
 *   code_size == 6 + (sincos ? 2 : 1) + min(anchor_dim, gt_cols - 1) - 7
 *   -> labels (batch, n_total) i32, targets (batch, n_total, code_size) f32, weights (batch, n_total) f32; n_total = sum counts.
 *   targets are encoded for the reference's fg_inds (forced or >= matched, class > 0, before its background pass, :176), so with
 *   matched < unmatched a label-0 anchor may carry targets; weights follow the final labels.
 *   norm_by_num_examples: weights of labels > 0 are 1 / max(#labels >= 0 of the (frame, class), 1) (:201-205); one more launch. */
size_t lidar_anchor_assign_workspace_bytes(int batch, int max_gt, int num_classes);
int lidar_anchor_assign(const float *const *anchors, const long long *counts, const long long *per_loc, const long long *out_off,
                        const float *matched, const float *unmatched, const int *remap, int num_classes, int anchor_dim,
                        long long a_total, const signed char *class_of_id, const float *gt, const float *gt_enlarged, int batch,
                        int max_gt, int gt_cols, int code_size, int sincos, int norm_by_num_examples, int *labels, float *targets,
                        float *weights, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ ATSS anchor target assignment (training)
 * ATSSTargetAssigner.assign_targets (pcdet/models/dense_heads/target_assigner/atss_target_assigner.py:16-141) for a whole batch and
 * every anchor set in one call on the caller's stream: no host read, no float atomics, bitwise reproducible, graph-capturable (three
 * kernels in a line; csrc/atss_assign.hip).
 *   anchors, counts   HOST arrays of num_sets entries: DEVICE pointer to the set's contiguous (counts[k], anchor_dim) anchors in
 *                     output order (use_multihead: already permuted (3, 4, 0, 1, 2, 5)), and its anchor count
 *   gt (batch, max_gt, gt_cols) f32 [box (gt_cols - 1) | class id].  Per frame the rows after the last one whose box columns do
 *   not sum to 0 (fp32, left to right) are trimmed, row 0 always stays (:41-44); every kept gt meets every set (no class mask).
 *   Per (frame, set, gt): the topk anchors by ascending (centre distance, anchor index) are candidates; threshold = mean + unbiased
 *   std of their IoUs + 1e-6 (rotated BEV IoU, or 3D IoU with match_height; csrc/iou3d_dev.h); a candidate is positive when
 *   iou >= threshold and its centre, rotated by -heading, has |x| <= dy / 2 and |y| <= dx / 2 (the reference's column swap, :109).
 *   An anchor positive for several gts takes the largest IoU (then the lowest gt).  Each gt then forces the anchor of largest IoU
 *   over the set (lowest index; anchor 0 when nothing overlaps) to itself; of several gts forcing one anchor the highest wins.
 *   code_size == 6 + (sincos ? 2 : 1) + min(anchor_dim, gt_cols - 1) - 7
 *   -> labels (batch, n_total) i32 = matched gt's class id (may be <= 0) or 0, targets (batch, n_total, code_size) f32 =
 *   ResidualCoder.encode_torch where label > 0 else 0, weights (batch, n_total) f32 = 1 where label > 0 else 0; n_total = sum
 *   counts, the sets one after the other.  Every output element is written by the call.
 *   ws: lidar_atss_assign_workspace_bytes(batch, max_gt, num_sets, topk) bytes, 256-byte aligned: (batch, num_sets, max_gt,
 *   topk + 1) i32 anchor indices, then the same shape of u64 priorities.
 * Supported (lidar_atss_assign_supported, pure host; everything else is refused with LIDAR_ERR_ARG before any launch):
 * 1 <= num_sets <= 16, anchor_dim >= 7, gt_cols >= 8, code_size <= 16, sincos and match_height in {0, 1}, 2 <= topk <= 32,
 * topk <= counts[k] <= 2^30 for every set, 1 <= max_gt <= 256; batch >= 0 (0: nothing is launched), batch * num_sets * max_gt < 2^31. */
int lidar_atss_assign_supported(const long long *counts, int num_sets, int anchor_dim, int gt_cols, int code_size, int sincos,
                                int topk, int max_gt, int match_height);
size_t lidar_atss_assign_workspace_bytes(int batch, int max_gt, int num_sets, int topk);
int lidar_atss_assign(const float *const *anchors, const long long *counts, int num_sets, int anchor_dim, const float *gt, int batch,
                      int max_gt, int gt_cols, int code_size, int sincos, int topk, int match_height, int *labels, float *targets,
                      float *weights, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ second-stage RoI target assignment (training)
 * ProposalTargetLayer.forward (pcdet/models/roi_heads/target_assigner/proposal_target_layer.py:13-238) and the canonical transform
 * of RoIHeadTemplate.assign_targets (pcdet/models/roi_heads/roi_head_template.py:101-131) for a whole batch in ONE launch on the
 * caller's stream: no host read, no float atomics, bitwise reproducible, graph-capturable, no workspace (csrc/proposal_target.hip).
 *   rois (batch, num_rois, box_dim) f32, roi_scores (batch, num_rois) f32, roi_labels (batch, num_rois) i64,
 *   gt_boxes (batch, max_gt, box_dim + 1) f32 [box | class id]; gt_boxes_enlarged: the same shape or NULL.  Per frame the trailing
 *   rows whose fp32 left-to-right sum (class id included) is 0 are trimmed, row 0 always stays (:94-97); trim, IoU and gt labels
 *   come from gt_boxes_enlarged when given (:93), gt_of_rois from gt_boxes (:116-117).  3D IoU: boxes_iou3d_gpu
 *   (pcdet/ops/iou3d_nms/iou3d_nms_utils.py:48-81) on the polygon clipper of csrc/iou3d_dev.h.
 *   by_class: SAMPLE_ROI_BY_EACH_CLASS (:204-238: only gts whose label equals the roi's; none -> overlap 0, assignment 0).
 *   fg_rois_per_image = int(np.round(FG_RATIO * ROI_PER_IMAGE)); hard_quota HOST (roi_per_image + 1) ints, hard_quota[n] =
 *   int(n * HARD_BG_RATIO) in [0, n] (Python double arithmetic, :177); cls_fg_minus_bg = CLS_FG_THRESH - CLS_BG_THRESH in double,
 *   rounded once.  cls_score_type 0: 'cls' (1 / 0 / -1), 1: 'roi_iou'.
 *   Randomness (the kernel draws nothing): fg_keys (batch, num_rois) f32, draws (batch, roi_per_image) f32 in [0, 1).  The
 *   without-replacement fg choice (:144-145) takes the fg candidates with the smallest (key, roi index), in that order; every
 *   with-replacement pick for output slot s is candidates[min(floor(draws[b][s] * n), n - 1)], product in fp32, candidates in
 *   ascending roi index.  Slot order: fg, hard bg, easy bg.
 *   -> out_rois (batch, P, box_dim), out_gt_of_rois (batch, P, box_dim + 1) after the canonical transform, out_gt_of_rois_src (the
 *   same rows before it), out_iou, out_scores, out_cls_labels (batch, P) f32, out_labels, out_reg_valid (batch, P) i64,
 *   out_sampled (batch, P) i32 roi indices, P = roi_per_image; max_overlaps (batch, num_rois) f32 and gt_assignment (batch,
 *   num_rois) i32 of every roi; frame_status (batch) i32: 0, or 1 for a frame with neither fg nor bg (NaN overlaps; the reference
 *   raises NotImplementedError, :166-169), whose sampled outputs are zeros.
 * Supported (lidar_proposal_target_supported, pure host; everything else is refused with LIDAR_ERR_ARG before any launch):
 * 1 <= num_rois <= 1024, 1 <= max_gt <= 512, 1 <= roi_per_image <= 512, 7 <= box_dim <= 16; batch >= 0 (0: nothing is launched). */
#define LIDAR_PROPOSAL_TARGET_MAX_ROIS 1024
#define LIDAR_PROPOSAL_TARGET_MAX_GT 512
#define LIDAR_PROPOSAL_TARGET_MAX_SAMPLES 512
#define LIDAR_PROPOSAL_TARGET_MAX_DIM 16
int lidar_proposal_target_supported(int num_rois, int max_gt, int roi_per_image, int box_dim);
int lidar_proposal_target(const float *rois, const float *roi_scores, const long long *roi_labels, const float *gt_boxes,
                          const float *gt_boxes_enlarged, int batch, int num_rois, int max_gt, int box_dim, int roi_per_image,
                          int fg_rois_per_image, const int *hard_quota, int by_class, int cls_score_type, float reg_fg_thresh,
                          float cls_fg_thresh, float cls_bg_thresh, float cls_bg_thresh_lo, float cls_fg_minus_bg,
                          const float *fg_keys, const float *draws, float *out_rois, float *out_gt_of_rois,
                          float *out_gt_of_rois_src, float *out_iou, float *out_scores, long long *out_labels,
                          long long *out_reg_valid, float *out_cls_labels, int *out_sampled, int *frame_status,
                          float *max_overlaps, int *gt_assignment, void *stream);

/* ------------------------------------------------------------------ train-time augmentation (GT sampling, world transforms, range)
 * Everything the reference does per frame in DataLoader workers between "raw cloud + annotations" and "points the voxeliser sees",
 * for a whole batch in ONE call on the caller's stream (csrc/augment.hip, five launches): no host read, no float atomics, bitwise
 * reproducible, graph-capturable.  The kernels draw nothing: which database objects are candidates, the flips, angles and scales
 * come from the caller.  Reference: pcdet/datasets/augmentor/database_sampler.py (__call__ :181-232, add_sampled_boxes_to_scene
 * :118-179), augmentor_utils.py :6-109, data_augmentor.py:108-134, pcdet/datasets/processor/data_processor.py:19-34.
 *   points (n_points, C) f32, point_offsets (batch + 1) i32 DEVICE; gt_boxes (batch, max_gt, 8) f32 [box | class id], gt_counts
 *   (batch) i32: real rows per frame.  A row inside the count with class id 0 is an annotated object of a class that is not trained:
 *   it takes part in the collision test and is dropped from the output (gt_boxes_mask + keep_arrays_by_name of the reference).
 *   Database: db_points (db_rows, C) f32 object-local points (relative to the box centre), db_offsets (n_obj + 1) i32, db_boxes
 *   (n_obj, 7) f32, db_cls (n_obj) i32 1-based class ids.  cand (batch, groups, per_group) i32 database indices in SAMPLE_GROUPS
 *   order, -1 = no candidate (an index outside [0, n_obj) counts as -1).
 *   Per frame, DEVICE: flip_x, flip_y (batch) i32 0/1; rot (batch) f32 and rot_cs (batch, 2) f32 = [cos, sin] of it, taken in double on
 *   the host and rounded once; scale (batch) f32 or NULL (scaling skipped: the reference's `< 1e-3` range test is a host decision);
 *   sample_rot (batch, groups, per_group) f32 or NULL (SAMPLE_ROT_ANGLE); plane (batch, 4) f32 or NULL (USE_ROAD_PLANE): the lidar
 *   height of the road under (x, y, z) is plane . [x, y, z, 1] (put_boxes_on_road_planes is affine in the box centre).
 *   HOST: remove_extra_width[3] (REMOVE_EXTRA_WIDTH), collide_extra_width[3] or NULL (REMOVE_SAMPLE_BOXES_EXTRA_WIDTH), pc_range[6],
 *   remove_outside_boxes, min_num_corners (0..8).
 * Per frame, in the reference's order:
 *   1. collision test (:194-227): groups in order; a candidate is valid iff its rotated BEV IoU (boxes_iou_bev_cpu's expression on the
 *      clipper of csrc/iou3d_dev.h) is exactly 0 against every existing box (all real input rows + the valid samples of earlier
 *      groups) and against every OTHER candidate of its group, valid or not; both boxes' dims + collide_extra_width when given;
 *   2. road plane: mv = z - dz / 2 - plane . [x, y, z, 1], z -= mv; heading += sample_rot (both after the collision test);
 *   3. paste and carve: a scene point inside any valid sample's box enlarged by remove_extra_width is removed, with the semantics of
 *      points_in_boxes_cpu (xy margin 1e-2, fabsf(z - cz) > dz / 2 is outside); object points are rotated by sample_rot about the
 *      object's origin, translated to the database box centre, z -= mv;
 *   4. world flip x (y, heading negated), flip y (x negated, heading = -(heading + pi)), rotation about z (rotate_points_along_z's
 *      matrix; heading += rot), scaling of columns 0..5 / points 0..2, then limit_period(heading, 0.5, 2 pi);
 *   5. range mask: points kept iff x and y lie in [min, max], both ends closed (z is not tested); with remove_outside_boxes a box is
 *      kept iff at least min_num_corners of its 8 corners lie inside the closed 3-D range;
 *   6. stable compaction.
 * -> out_points (cap, C): per frame the valid pasted objects' points in (group, candidate) order, then the surviving scene points in
 *    input order (rows at and past out_offsets[batch] are not written); out_offsets (batch + 1) i32; out_gt_boxes (batch, max_gt +
 *    groups * per_group, 8) zero-padded, the trained input rows first in input order, then the valid samples; out_gt_counts (batch);
 *    sample_valid (batch, groups, per_group) i32.
 * cap: rows of out_points.  obj_rows_bound: the caller's sum of the point counts of every candidate's object; a call with
 * cap < n_points + obj_rows_bound is refused on the host, and no row at or past cap is ever written.
 * Supported (lidar_augment_supported, pure host; everything else is refused with LIDAR_ERR_ARG before any launch): 3 <= C <= 8,
 * 1 <= groups <= 8, 0 <= per_group <= 64, max_gt + groups * per_group <= 512; batch >= 0 (0 launches nothing); frames of 0 points
 * and frames with gt_counts 0 are valid.  With C == 4 the point arrays, and always out_gt_boxes, must be 16-byte aligned.
 * NOT built: velocity columns (boxes are 7 wide).
 *
 * lidar_augment_mf: the same call with the multi-frame extras of the reference carried along (database_sampler.py:165-177,
 * augmentor_utils.py:24-28, :51-55, :80-84, :105-107, data_processor.py:29-32, dataset.py:139-142): every gt has a pose in each of
 * the S = stack_frames stacked sweeps.  The same kernels run; the thread of aug_frame_kernel that owns a box row also owns its S poses
 * and writes them at the box's compacted rank.  points, point_offsets, gt_boxes, gt_counts and sample_valid come out bitwise as from
 * lidar_augment.  All DEVICE f32, 4-byte aligned:
 *   gt_locations (batch, max_gt, S, 3), gt_rotations_y (batch, max_gt, S): rows past gt_counts are ignored; db_locations (n_obj, S, 3),
 *   db_rotations_y (n_obj, S): the database objects' poses in the absolute frame of db_boxes.
 *   -> out_locations (batch, max_gt + groups * per_group, S, 3), out_rotations_y (batch, max_gt + groups * per_group, S): row r is
 *   the pose of row r of out_gt_boxes; every element is written, rows at and past out_gt_counts[b] are zero.
 * Per row and sweep, fp32 in the reference's order.  A pasted sample: z -= mv (the road-plane shift of its box); with sample_rot a:
 * rotations_y += a, location -= centre, turned by a with the [cos, sin] the object's points get, += centre (centre: the sample's box
 * xyz after the road plane).  Every kept row: the world flips (flip x: y and rotations_y negated; flip y: x negated, rotations_y =
 * -(rotations_y + pi)), the world rotation's matrix and rotations_y += rot, scaling of the location.  rotations_y is NOT folded by
 * limit_period (the reference folds the boxes' heading only).  A pose row is kept iff its box is: the poses are not range-tested.
 * Declared divergence: a class-id-0 row is dropped from the boxes AND from both pose arrays.  The reference masks gt_boxes with
 * gt_boxes_mask but concatenates the samples' poses onto its unmasked `locations` (add_sampled_boxes_to_scene) and masks only boxes
 * and names in DataAugmentor.forward, after which its pose rows no longer line up with its box rows; that defect is not reproduced.
 * Supported (lidar_augment_mf_supported): what lidar_augment_supported accepts and 1 <= stack_frames <= 8; NULL or misaligned pose
 * arrays are refused with LIDAR_ERR_ARG before any launch; batch == 0 launches nothing.  The workspace is lidar_augment's. */
#define LIDAR_AUGMENT_MAX_FEATURES 8
#define LIDAR_AUGMENT_MAX_GROUPS 8
#define LIDAR_AUGMENT_MAX_PER_GROUP 64
#define LIDAR_AUGMENT_MAX_BOXES 512
int lidar_augment_supported(int num_features, int max_gt, int groups, int per_group);
size_t lidar_augment_workspace_bytes(int batch, int groups, int per_group, int cap);
int lidar_augment(const float *points, const int *point_offsets, int n_points, int num_features, const float *gt_boxes,
                  const int *gt_counts, int batch, int max_gt, const float *db_points, const int *db_offsets, const float *db_boxes,
                  const int *db_cls, int n_obj, int db_rows, const int *cand, int groups, int per_group, const int *flip_x,
                  const int *flip_y, const float *rot, const float *rot_cs, const float *scale, const float *sample_rot,
                  const float *plane, const float *remove_extra_width, const float *collide_extra_width, const float *pc_range,
                  int remove_outside_boxes, int min_num_corners, long long obj_rows_bound, int cap, float *out_points,
                  int *out_offsets, float *out_gt_boxes, int *out_gt_counts, int *sample_valid, void *ws, size_t ws_bytes,
                  void *stream);
#define LIDAR_AUGMENT_MF_MAX_FRAMES 8
int lidar_augment_mf_supported(int num_features, int max_gt, int groups, int per_group, int stack_frames);
int lidar_augment_mf(const float *points, const int *point_offsets, int n_points, int num_features, const float *gt_boxes,
                     const int *gt_counts, int batch, int max_gt, const float *db_points, const int *db_offsets, const float *db_boxes,
                     const int *db_cls, int n_obj, int db_rows, const int *cand, int groups, int per_group, const int *flip_x,
                     const int *flip_y, const float *rot, const float *rot_cs, const float *scale, const float *sample_rot,
                     const float *plane, const float *remove_extra_width, const float *collide_extra_width, const float *pc_range,
                     int remove_outside_boxes, int min_num_corners, long long obj_rows_bound, int cap, const float *gt_locations,
                     const float *gt_rotations_y, const float *db_locations, const float *db_rotations_y, int stack_frames,
                     float *out_points, int *out_offsets, float *out_gt_boxes, int *out_gt_counts, int *sample_valid,
                     float *out_locations, float *out_rotations_y, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ anchor-head RPN loss (training), forward + backward
 * AnchorHeadTemplate.get_loss / AnchorHeadMulti.get_loss for a whole batch and every head, no host synchronisation, no float atomics
 * (csrc/anchor_loss.hip).  Reference: pcdet/models/dense_heads/anchor_head_template.py:102-224 (get_cls_layer_loss,
 * add_sin_difference, get_direction_target, get_box_reg_layer_loss, get_loss), anchor_head_multi.py:245-370, pcdet/utils/loss_utils.py
 * (SigmoidFocalClassificationLoss :9-72, WeightedSmoothL1Loss :75-136, WeightedL1Loss :139-178, WeightedCrossEntropyLoss :181-205).
 *   cls, box, dir, counts, cols, col_off   HOST arrays of num_heads (<= 16) entries, passed by value in the kernel arguments: DEVICE
 *       pointers to head k's contiguous (batch, counts[k], cols[k]) class logits, (batch, counts[k], code_size) box encodings and
 *       (batch, counts[k], num_dir_bins) direction logits (dir NULL without a direction classifier); head k owns anchors
 *       sum(counts[<k]) .. + counts[k] of the frame, and compares its cols[k] (<= 16) logits with one-hot columns col_off[k] ..
 *       (SEPARATE_MULTIHEAD; otherwise 0 and cols == num_class).  sum(counts) == n_total.
 *   labels (batch, n_total) i32, targets (batch, n_total, code_size) f32 (the assigner's box_cls_labels / box_reg_targets),
 *   anchors (n_total, anchor_dim) f32, shared by every frame (only column 6 is read, for the direction target); code_size 7..16,
 *   num_dir_bins 1..8
 *   code_weights HOST (code_size); weights HOST (7): cls_weight, loc_weight, dir_weight, pos_cls_weight, neg_cls_weight,
 *       DIR_OFFSET, 2 pi / NUM_DIR_BINS
 *   flags: 1 add_sin_difference on column 6, 2 WeightedL1Loss (else WeightedSmoothL1Loss, beta 1/9), 4 direction classifier
 *   forward -> losses (3) DEVICE f32: cls, loc, dir terms (each weighted and divided by batch, as the reference returns them); the
 *       per-frame positive counts stay in the workspace for backward, which must get the same workspace and inputs.
 *   backward: grad_losses (3) DEVICE f32 -> d_cls / d_box / d_dir HOST arrays of num_heads DEVICE pointers in the layouts of the
 *       inputs (an array or an entry NULL: not written). */
size_t lidar_anchor_loss_workspace_bytes(int batch, const long long *counts, int num_heads);
int lidar_anchor_loss_forward(const float *const *cls, const float *const *box, const float *const *dir, const long long *counts,
                              const int *cols, const int *col_off, int num_heads, const int *labels, const float *targets,
                              const float *anchors, int anchor_dim, int batch, long long n_total, int num_class, int code_size,
                              int num_dir_bins, const float *code_weights, const float *weights, int flags, float *losses, void *ws,
                              size_t ws_bytes, void *stream);
int lidar_anchor_loss_backward(const float *const *cls, const float *const *box, const float *const *dir, const long long *counts,
                               const int *cols, const int *col_off, int num_heads, const int *labels, const float *targets,
                               const float *anchors, int anchor_dim, int batch, long long n_total, int num_class, int code_size,
                               int num_dir_bins, const float *code_weights, const float *weights, int flags,
                               const float *grad_losses, float *const *d_cls, float *const *d_box, float *const *d_dir, void *ws,
                               size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ RoI-head loss (training), forward + backward
 * RoIHeadTemplate.get_loss (pcdet/models/roi_heads/roi_head_template.py:133-233: get_box_cls_layer_loss with CLS_LOSS
 * BinaryCrossEntropy, get_box_reg_layer_loss with REG_LOSS smooth-l1 and CORNER_LOSS_REGULARIZATION) on what the target layer
 * writes, for all n = batch * roi_per_image rows: ONE forward launch on the caller's stream, no host read, no allocation, no atomics,
 * bitwise reproducible, graph-capturable (csrc/roi_loss.hip).
 *   rcnn_cls (n, 1) f32 logits, rcnn_reg (n, 7) f32, rois (batch, P, 7) f32, gt_of_rois (batch, P, 8) f32 in the roi's canonical
 *   frame, gt_of_rois_src (batch, P, 8) f32 before the transform, reg_valid_mask (batch, P) i64, rcnn_cls_labels (batch, P) f32
 *   (soft labels in [0, 1] or 1 / 0 / -1; a row is valid when its label is >= 0).  Inputs are never written.
 *   weights HOST (3): rcnn_cls_weight, rcnn_reg_weight, rcnn_corner_weight; code_weights HOST (7); flags: 1 corner regulariser.
 *   cls    = sum_valid bce(x, t) / max(n_valid, 1) * w_cls, bce in the stable form max(x, 0) - x t + log1p(exp(-|x|)) (equal to the
 *            reference's binary_cross_entropy(sigmoid(x), t) for |x| < 27.6, where its clamps do not engage; continued beyond)
 *   reg    = sum_fg sum_7 smoothL1((pred - target) * code_w, beta 1/9) / max(fg_sum, 1) * w_reg, fg = reg_valid_mask > 0, target =
 *            ResidualCoder.encode_torch(gt_of_rois[:7], roi with centre and heading zeroed), sizes clamped at 1e-5, a NaN target
 *            takes the prediction; non-fg rows are skipped
 *   corner = mean_fg mean_8 smoothL1(min(|p - g|, |p - g_flip|), beta 1) * w_corner on the corners of the decoded prediction and
 *            of gt_of_rois_src[:7] (get_corner_loss_lidar); 0 without fg rows or without the flag
 *   forward -> out (5) DEVICE f32: cls, reg, corner, fg_sum, n_valid.  The rows' gradient pieces and the two counts stay in the
 *       workspace; backward takes the same workspace, weights and flags.  batch 0: no kernel, out is zeroed.
 *   backward: grad_out (3) DEVICE f32 (upstream gradients of cls, reg, corner) -> d_rcnn_cls (n, 1), d_rcnn_reg (n, 7); either may
 *       be NULL (not written).
 * Supported (lidar_roi_loss_supported, pure host; everything else is refused with LIDAR_ERR_ARG before any launch): roi_dim 7,
 * gt_dim 8, reg_dim 7, cls_dim 1 (ResidualCoder without sin/cos, class-agnostic regression, no tracking info), batch >= 0,
 * 1 <= roi_per_image <= 512, batch * roi_per_image <= 65536. */
#define LIDAR_ROI_LOSS_MAX_SAMPLES 512
#define LIDAR_ROI_LOSS_MAX_ROWS 65536
int lidar_roi_loss_supported(int batch, int roi_per_image, int roi_dim, int gt_dim, int reg_dim, int cls_dim);
size_t lidar_roi_loss_workspace_bytes(int batch, int roi_per_image);
int lidar_roi_loss_forward(const float *rcnn_cls, const float *rcnn_reg, const float *rois, const float *gt_of_rois,
                           const float *gt_of_rois_src, const long long *reg_valid_mask, const float *rcnn_cls_labels, int batch,
                           int roi_per_image, const float *weights, const float *code_weights, int flags, float *out, void *ws,
                           size_t ws_bytes, void *stream);
int lidar_roi_loss_backward(int batch, int roi_per_image, const float *weights, const float *code_weights, int flags,
                            const float *grad_out, float *d_rcnn_cls, float *d_rcnn_reg, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ point-head targets and loss (training)
 * PointHeadTemplate.assign_stack_targets with set_ignore_flag=True and get_cls / box / part_layer_loss
 * (pcdet/models/dense_heads/point_head_template.py:49-191) for a stacked point set: ONE launch for the targets, two for the loss
 * forward, ONE for its backward, all on the caller's stream; no host read, no allocation, no atomics, bitwise reproducible
 * (csrc/point_head.hip).
 *   points (n, 4) f32 [bs_idx, x, y, z] in any frame order (a bs_idx outside [0, batch) keeps label 0 and zero targets);
 *   gt_boxes (batch, m, 8) f32 [box7 | class], zero rows as padding (they take part, enlarged too, as in the reference);
 *   extra_width HOST (3); flags: 1 box labels, 2 part labels; mean_size HOST (n_mean, 3) or NULL with n_mean 0
 *   (PointResidualCoder use_mean_size; class id c reads row c - 1, class 0 the last row, classes beyond n_mean wrap).
 *   targets -> point_cls_labels (n) i64: fg (inside the first containing gt row = owner) 1 if num_class == 1 else (long)class,
 *       -1 for fg XOR inside any enlarged row, else 0; point_box_labels (n, 8) f32 PointResidualCoder.encode_torch on fg rows, 0
 *       elsewhere; point_part_labels (n, 3) f32 rotate_z(p - centre, -rz) / dims + 0.5 on fg rows, 0 elsewhere; point_box_idx (n)
 *       i32 owner row or -1.  Every element is written.
 *   loss: point_cls_preds (n, num_class), point_box_preds (n, 8), point_part_preds (n, 3) f32, each may be NULL (term skipped,
 *       record entry 0); weights HOST (3): point_cls_weight, point_box_weight, point_part_weight; code_weights HOST (8).
 *       cls  = sum_{label >= 0} focal(x, onehot(label)) / max(npos, 1) * w_cls (alpha 0.25, gamma 2), npos = #(label > 0)
 *       box  = sum_{label > 0} sum_8 smoothL1((pred - label) * code_w, beta 1/9) / max(npos, 1) * w_box, a NaN label takes the pred
 *       part = sum_{label > 0} sum_3 bce_logits(x, t) / (3 max(npos, 1)) * w_part, bce in the stable logits form
 *   forward -> out (4) DEVICE f32: cls, box, part, npos; the workspace (lidar_point_loss_ws_bytes(n)) keeps the tile partials and
 *       the count for backward.  n 0: no kernel, out is zeroed.
 *   backward: the same inputs and workspace, grad_out (3) DEVICE f32 -> d_cls_preds, d_box_preds, d_part_preds; any may be NULL.
 * Supported (lidar_point_head_supported, pure host; everything else is refused with LIDAR_ERR_ARG before any launch):
 * 0 <= n <= 2^20, 1 <= batch <= 64, 0 <= m <= 128, gt_dim 8, 1 <= num_class <= 8, 0 <= n_mean <= 8. */
#define LIDAR_POINT_HEAD_MAX_POINTS (1 << 20)
#define LIDAR_POINT_HEAD_MAX_BATCH 64
#define LIDAR_POINT_HEAD_MAX_GT 128
#define LIDAR_POINT_HEAD_MAX_CLASS 8
#define LIDAR_POINT_HEAD_MAX_MEAN 8
int lidar_point_head_supported(long long n, int batch, int m, int gt_dim, int num_class, int n_mean);
int lidar_point_targets(const float *points, long long n, const float *gt_boxes, int batch, int m, int gt_dim,
                        const float *extra_width, int num_class, int flags, const float *mean_size, int n_mean,
                        long long *point_cls_labels, float *point_box_labels, float *point_part_labels, int *point_box_idx,
                        void *stream);
size_t lidar_point_loss_ws_bytes(long long n);
int lidar_point_loss_forward(const float *point_cls_preds, const float *point_box_preds, const float *point_part_preds,
                             const long long *point_cls_labels, const float *point_box_labels, const float *point_part_labels,
                             long long n, int num_class, const float *weights, const float *code_weights, float *out, void *ws,
                             size_t ws_bytes, void *stream);
int lidar_point_loss_backward(const float *point_cls_preds, const float *point_box_preds, const float *point_part_preds,
                              const long long *point_cls_labels, const float *point_box_labels, const float *point_part_labels,
                              long long n, int num_class, const float *weights, const float *code_weights, const float *grad_out,
                              float *d_cls_preds, float *d_box_preds, float *d_part_preds, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ multi-frame point head and union gt boxes (training)
 * The multi-frame supervision of tools/cfgs/livox_models/pv_rcnn_multiframe.yaml (STACK_FRAME_SIZE S stacked sweeps): every gt
 * carries its pose in each sweep, locations (batch, m, S, 3) f32 and rotations_y (batch, m, S) f32, next to gt_boxes (batch, m, 8)
 * f32 [box7 | class].  PointHeadSimpleMultiFrame.assign_targets / get_cls_layer_loss
 * (pcdet/models/dense_heads/point_head_simple_multiframe.py:23-90) and the USE_MULTIFRAME_ENLARGED_GT_BOXES block of
 * AnchorHeadSingle.forward (pcdet/models/dense_heads/anchor_head_single.py:61-89), all on the caller's stream; no host read, no
 * allocation, no atomics, bitwise reproducible (csrc/point_head_mf.hip).
 *   targets (ONE launch) -> point_cls_labels (n, S) i64, frame index fastest: column s is exactly what lidar_point_targets writes
 *       for gt_boxes with columns 0:3 := locations[:, :, s] and column 6 := rotations_y[:, :, s] (fg = inside the first containing
 *       row: 1 if num_class == 1 else (long)class; -1 for fg XOR inside any row enlarged by extra_width HOST (3); else 0; zero
 *       padding rows take part, enlarged too; a bs_idx outside [0, batch) gives 0 in every column); point_box_idx (n, S) i32, the
 *       owner row per frame or -1, may be NULL.  Every element is written.
 *   loss: point_cls_preds (n, S * num_class) f32, column s * num_class + c; L = point_cls_labels (n, S).  npos = #(L > 0) over all
 *       frames, norm = max(npos, 1), w_n = sum_s ([L_ns >= 0] / norm) (each term divided first, added in fp32 in frame order),
 *       target t[n, s * num_class + c] = [L_ns == c + 1],
 *       cls = point_cls_weight * sum_{n, j} focal(x_nj, t_nj; alpha 0.25, gamma 2) * w_n over ALL S * num_class columns: as in the
 *       reference, a frame column whose label is -1 is still a negative target, weighted by the other frames' share of w_n; a
 *       point ignored in every frame weighs 0.
 *   forward (two launches) -> out (2) DEVICE f32: cls, npos; the workspace (lidar_point_loss_mf_ws_bytes(n)) keeps the tile
 *       partials and the count for backward.  n 0: no kernel, out is zeroed.
 *   backward (ONE launch): the same inputs and workspace, grad_out (1) DEVICE f32 -> d_cls_preds (n, S * num_class).
 *   lidar_multiframe_enlarged_boxes (ONE launch, one thread per gt row) -> gt_boxes_enlarged (batch, m, 8): the reference as it
 *       runs.  Its line 78 writes rotations_y into the LAST column, for 8-column boxes the class, which boxes_to_corners_3d never
 *       reads: every frame's corners use the gt's own heading, rotations_y has no effect and is no argument here.  Columns 0:3 and
 *       5:8 are the gt's; column 3 (4) is the extent in x (y) of all 8 S corners in the gt's local frame (corners, minus the gt
 *       centre, rotated by -gt[6], max - min).  gt_dim must be 8: with more columns the reference's [:, -2] is not the heading.
 * Supported (lidar_point_head_mf_supported, pure host; everything else is refused with LIDAR_ERR_ARG before any launch):
 * 0 <= n <= 2^20, 1 <= batch <= 64, 0 <= m <= 128, 1 <= S <= 8, 1 <= num_class <= 4 (at most 32 logit columns).
 * The poses these take come out of lidar_augment_mf during training (same layout: zero rows past the count).
 * NOT built: REG_TRACKING_INFO of ProposalTargetLayer and the RoI loss. */
#define LIDAR_POINT_HEAD_MF_MAX_FRAMES 8
#define LIDAR_POINT_HEAD_MF_MAX_CLASS 4
int lidar_point_head_mf_supported(long long n, int batch, int m, int stack_frames, int num_class);
int lidar_point_targets_mf(const float *points, long long n, const float *gt_boxes, const float *locations, const float *rotations_y,
                           int batch, int m, int stack_frames, const float *extra_width, int num_class,
                           long long *point_cls_labels, int *point_box_idx, void *stream);
size_t lidar_point_loss_mf_ws_bytes(long long n);
int lidar_point_loss_mf_forward(const float *point_cls_preds, const long long *point_cls_labels, long long n, int stack_frames,
                                int num_class, float point_cls_weight, float *out, void *ws, size_t ws_bytes, void *stream);
int lidar_point_loss_mf_backward(const float *point_cls_preds, const long long *point_cls_labels, long long n, int stack_frames,
                                 int num_class, float point_cls_weight, const float *grad_out, float *d_cls_preds, void *ws,
                                 size_t ws_bytes, void *stream);
int lidar_multiframe_enlarged_boxes(const float *gt_boxes, const float *locations, int batch, int m, int gt_dim, int stack_frames,
                                    float *gt_boxes_enlarged, void *stream);

/* ------------------------------------------------------------------ fused optimiser step (training)
 * What follows loss.backward() in the reference's loop (tools/train_utils/train_utils.py:36-42) for OPTIMIZER: adam_onecycle:
 * clip_grad_norm_(model.parameters(), GRAD_NORM_CLIP), then OptimWrapper.step (tools/train_utils/optimization/fastai_optim.py:
 * 132-149, built by tools/train_utils/optimization/__init__.py:19-32): p.data.mul_(1 - wd * lr) over every parameter with
 * requires_grad, then torch.optim.Adam with betas (mom, 0.99).  Here: three launches over all tensors at once, on the caller's
 * stream; no host read, no allocation, no float atomics, bitwise reproducible; fp32 only (csrc/optim_step.hip).
 *   table DEVICE (n_tensors, LIDAR_OPTIM_ENTRY) 64-bit words per tensor: param, grad, exp_avg, exp_avg_sq addresses (contiguous
 *       f32, 4-byte aligned; 16-byte aligned tensors move as 16-byte vectors), numel, step lag (steps of the optimiser this tensor
 *       sat out: its bias corrections use t - lag).  A NULL grad is a parameter without a gradient this step: it takes no part
 *       in the norm and gets the decay only, its state is not touched.  Parameters that do not require a gradient are not listed.
 *   chunk map DEVICE: chunk c covers elements [chunk_index[c] * LIDAR_OPTIM_CHUNK, + LIDAR_OPTIM_CHUNK) of tensor chunk_tensor[c].
 *       lidar_optim_plan (pure HOST, host pointers) writes the map of a list of numel values, tensor by tensor, and returns the
 *       number of chunks (at most `capacity` are written; chunk_tensor / chunk_index may be NULL to count only; < 0: error).
 *   lidar_optim_grad_norm -> norm_out DEVICE (2) f32: total_norm = sqrt(sum g^2) (squares and sums in fp64, one rounding to fp32)
 *       and the clip coefficient min(1, max_norm / (total_norm + 1e-6)), torch.nn.utils.clip_grad_norm_'s with norm_type 2.
 *       ws: lidar_optim_workspace_bytes(n_chunks) bytes, 8-byte aligned.  n_chunks 0: total_norm 0.
 *   lidar_optim_adam_step: per element, g = norm_out[1] * grad, p *= (float)decay (the caller passes the double 1 - wd * lr),
 *       m += (1 - beta1) * (g - m), v = beta2 * v + (1 - beta2) * g * g, denom = sqrt(v) / sqrt(1 - beta2^t) + eps,
 *       p -= lr / (1 - beta1^t) * m / denom: torch's single-tensor Adam, the CURRENT beta1 in the bias correction as torch has it
 *       when betas change between steps.  t >= 1: the optimiser's step count after this step.
 *       flags: LIDAR_OPTIM_WRITE_CLIPPED stores g back (what clip_grad_norm_ leaves), LIDAR_OPTIM_ZERO_GRAD stores zeros, 0 leaves
 *       the gradient as it is.  Non-finite norms propagate as in the reference. */
#define LIDAR_OPTIM_CHUNK 1024
#define LIDAR_OPTIM_ENTRY 6
#define LIDAR_OPTIM_WRITE_CLIPPED 1
#define LIDAR_OPTIM_ZERO_GRAD 2
long long lidar_optim_plan(const long long *numel, int n_tensors, int *chunk_tensor, int *chunk_index, long long capacity);
size_t lidar_optim_workspace_bytes(long long n_chunks);
int lidar_optim_grad_norm(const long long *table, int n_tensors, const int *chunk_tensor, const int *chunk_index,
                          long long n_chunks, float max_norm, float *norm_out, void *ws, size_t ws_bytes, void *stream);
int lidar_optim_adam_step(const long long *table, int n_tensors, const int *chunk_tensor, const int *chunk_index,
                          long long n_chunks, const float *norm_out, double lr, double beta1, double beta2, double eps,
                          double decay, long long t, int flags, void *stream);

/* HeightCompression in one pass (pcdet/models/backbones_2d/map_to_bev/height_compression.py:21-24): the (N, C*D, H, W) BEV
 * map of a sparse tensor written directly channels-last: out[b][h][w][c*D + d]; D <= 4, channels % 4 == 0; same workspace
 * as lidar_sparse_to_dense. */
int lidar_sparse_to_bev_nhwc(const float *features, const int *indices, int n, int channels, int batch, int D, int H, int W,
                             float *out, void *ws, size_t ws_bytes, void *stream);
/* Its backward (csrc/sparse_train.hip): d_features (n, channels) with d_features[row][c] = grad_out[b][y][x][c * D + z] for the
 * row's indices [b, z, y, x] (the ones the forward took).  grad_out is the gradient of the channels-last (batch, H, W, channels * D)
 * map or a channel slice of a wider one: g_ld floats per pixel, the slice starting at channel g_off (g_off >= 0,
 * g_off + channels * D <= g_ld).  A pure gather: no atomics, no workspace, every output element written once; a row the forward
 * skips (b outside [0, batch), z / y / x outside the volume) gets an exactly zero gradient.  Supported (the forward's range):
 * channels % 4 == 0, 1 <= D <= 4, n >= 0 (0: success, nothing is launched); indices and d_features 16-byte aligned; 16-byte reads
 * when grad_out is 16-byte aligned and g_ld % 4 == g_off % 4 == 0, scalar reads otherwise.  LIDAR_ERR_ARG outside that range. */
int lidar_sparse_to_bev_nhwc_backward(const float *grad_out, int g_ld, int g_off, const int *indices, int n, int channels, int batch,
                                      int D, int H, int W, float *d_features, void *stream);

/* ------------------------------------------------------------------ KITTI-eval rotated BEV IoU (8f rank 4)
 * rotate_iou_gpu_eval (pcdet/datasets/kitti/kitti_object_eval_python/rotate_iou.py:290-330; numba.cuda in the reference):
 * boxes (n, 5) / query_boxes (k, 5) as (x, y, w, l, angle) -> iou (n, k); criterion -1: IoU, 0: inter / area(query),
 * 1: inter / area(box), 2: intersection area. */
int lidar_rotate_iou_eval(const float *boxes, int n, const float *query_boxes, int k, int criterion, float *iou, void *stream);

/* ------------------------------------------------------------------ KITTI AP evaluation
 * What get_official_eval_result runs around the rotated IoU (pcdet/datasets/kitti/kitti_object_eval_python/eval.py: clean_data :30-83,
 * image_box_overlap :86-113, d3_box_overlap :121-154, compute_statistics_jit :157-275, get_thresholds :9-27, eval_class :448-553;
 * numba in the reference) for a whole evaluation set, on the caller's stream, without a host read, an allocation or a float atomic:
 * two runs give the same bits (csrc/kitti_eval.hip).
 *   Rows.  The set is packed once: every frame's boxes stacked, frame f owning rows [off[f], off[f + 1]) of
 *     gt (total_gt, LIDAR_KITTI_EVAL_GT_COLS) f64: bbox 0..3, location 4..6, dimensions 7..9, rotation_y 10, alpha 11, occluded 12,
 *         truncated 13;  dt (total_dt, LIDAR_KITTI_EVAL_DT_COLS) f64: the same first twelve columns, score 12 (finite);
 *     gt_cls / dt_cls i32: 0 car, 1 pedestrian, 2 cyclist, 3 van, 4 person_sitting, 5 truck (lower-cased names, as clean_data
 *         compares them), LIDAR_KITTI_EVAL_CLS_DONTCARE for the exact name "DontCare", LIDAR_KITTI_EVAL_CLS_OTHER for the rest;
 *     gt_off, dt_off (frames + 1) i32 and ov_off (frames + 1) i64, ov_off[f + 1] - ov_off[f] = dt_f * gt_f, all DEVICE.
 *     max_gt / max_dt: the caller's bound on the rows of one frame.  A frame whose offsets break it, or leave total_gt / total_dt /
 *     ov_total, takes no part (it counts as empty); nothing outside the arrays is touched whatever the offsets hold.
 *   lidar_kitti_eval_overlaps -> overlaps (ov_total) f64: frame f's (dt_f, gt_f) block, dt-major, at ov_off[f] (same-frame pairs
 *     only: the reference computes all pairs of 100 frames and discards the rest).  metric 0: image_box_overlap in fp64 (boxes = dt,
 *     query = gt); 1: the rotated BEV IoU of lidar_rotate_iou_eval on (x, z, dx, dz, ry) rounded to fp32; 2: d3_box_overlap: the
 *     criterion-2 intersection area ROUNDED TO FP32, d3_box_overlap_kernel's arithmetic in fp64, the result rounded to fp32 again
 *     (the reference works in place on the fp32 array before its cast to float64).  criterion as in the reference (-1 IoU, 0 over
 *     the dt box, 1 over the gt box, else the intersection); the matcher takes -1, and for metric 0 a second block set with
 *     criterion 0 whose DontCare columns are compute_statistics_jit's overlaps_dt_dc.
 *   lidar_kitti_eval_class: eval_class for one metric.  classes HOST (num_class) ids 0..5, difficulties HOST (num_diff) 0..2,
 *     min_overlaps HOST (num_overlap, num_class) f64 (min_overlaps[:, metric, :]).  A configuration is (class slot m, difficulty
 *     slot l, overlap row k), index c = (m * num_diff + l) * num_overlap + k.  dc_overlaps: metric 0 only (else NULL).  Outputs, DEVICE:
 *       matched (n_cfg, total_gt) f64   pass 1 (compute_fp False, thresh 0): the score a gt row's match emitted, -inf for none.
 *                                       Gts in row order take the unassigned det with overlap > min_overlap and the highest score;
 *                                       the comparisons are strict, so the lowest row wins a tie
 *       num_valid_gt (num_class * num_diff) i32
 *       thresholds (n_cfg, 41) f64, num_thresholds (n_cfg) i32   get_thresholds' sequential scan in fp64 over the scores sorted
 *                                       descending; no matched score: no thresholds, and the curves stay zero
 *       counts (n_cfg, 41, 3) i64       tp, fp, fn of pass 2 (compute_fp True) summed over frames, 0 past num_thresholds.  Pass 2
 *                                       skips dets below the threshold; among the eligible dets with ignored_det 0 the largest overlap
 *                                       wins (lowest row on a tie), otherwise the first eligible one with ignored_det 1; for metric 0
 *                                       an unmatched det with overlap > min_overlap over a DontCare box is not a false positive
 *       curves (3, n_cfg, 41) f64       precision, recall, orientation: per threshold, then the running maximum from the right over
 *                                       the first num_thresholds entries; zero beyond (orientation all zero without compute_aos).
 *                                       The similarity sum(1 + cos(gt alpha - dt alpha)) / 2 is written per frame and added over
 *                                       frames in frame order in fp64
 *     ws: lidar_kitti_eval_workspace_bytes(...) bytes, 256-byte aligned.
 * Supported (lidar_kitti_eval_supported, pure host): 0 <= frames <= 2^20, total_gt <= 2^20, total_dt <= 2^22, max_gt and max_dt
 * <= 1024, 1..8 classes, 1..3 difficulties, 1..16 overlap rows; frames with no gt, no dt or neither are valid, and so is an empty
 * set.  Negative sizes, a metric outside 0..2, ids outside their ranges and missing pointers are LIDAR_ERR_ARG, sizes beyond the
 * support LIDAR_ERR_UNSUPPORTED, a short workspace LIDAR_ERR_WORKSPACE, all before any launch. */
#define LIDAR_KITTI_EVAL_GT_COLS 14
#define LIDAR_KITTI_EVAL_DT_COLS 13
#define LIDAR_KITTI_EVAL_CLS_DONTCARE 6
#define LIDAR_KITTI_EVAL_CLS_OTHER 7
#define LIDAR_KITTI_EVAL_MAX_GT 1024
#define LIDAR_KITTI_EVAL_MAX_DT 1024
#define LIDAR_KITTI_EVAL_MAX_FRAMES (1 << 20)
#define LIDAR_KITTI_EVAL_MAX_TOTAL_GT (1ll << 20)
#define LIDAR_KITTI_EVAL_MAX_TOTAL_DT (1ll << 22)
#define LIDAR_KITTI_EVAL_MAX_CLASS 8
#define LIDAR_KITTI_EVAL_MAX_DIFF 3
#define LIDAR_KITTI_EVAL_MAX_OVERLAP 16
#define LIDAR_KITTI_EVAL_PTS 41
int lidar_kitti_eval_supported(int frames, long long total_gt, long long total_dt, int max_gt, int max_dt, int num_class,
                               int num_diff, int num_overlap);
size_t lidar_kitti_eval_workspace_bytes(int frames, long long total_gt, long long total_dt, int max_gt, int max_dt, int num_class,
                                        int num_diff, int num_overlap);
int lidar_kitti_eval_overlaps(int metric, int criterion, const double *gt, const double *dt, const int *gt_off, const int *dt_off,
                              const long long *ov_off, int frames, long long total_gt, long long total_dt, long long ov_total,
                              int max_gt, int max_dt, double *overlaps, void *stream);
int lidar_kitti_eval_class(int metric, const double *gt, const double *dt, const int *gt_cls, const int *dt_cls, const int *gt_off,
                           const int *dt_off, const long long *ov_off, const double *overlaps, const double *dc_overlaps, int frames,
                           long long total_gt, long long total_dt, long long ov_total, int max_gt, int max_dt, const int *classes,
                           int num_class, const int *difficulties, int num_diff, const double *min_overlaps, int num_overlap,
                           int compute_aos, double *matched, int *num_valid_gt, double *thresholds, int *num_thresholds,
                           long long *counts, double *curves, void *ws, size_t ws_bytes, void *stream);

/* ------------------------------------------------------------------ CPU entry points (HOST pointers, no GPU touched)
 * Called by the reference from DataLoader workers (augmentation / database creation). */
/* boxes_iou_bev_cpu (pcdet/ops/iou3d_nms/src/iou3d_cpu.cpp:232-252): out (n_a, n_b) rotated BEV IoU */
int lidar_boxes_iou_bev_cpu(const float *boxes_a, int n_a, const float *boxes_b, int n_b, float *out);
/* points_in_boxes_cpu (pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:143-168): out (n_boxes, n_pts) 0/1, margin 1e-2 */
int lidar_points_in_boxes_cpu(const float *boxes, int n_boxes, const float *pts, int n_pts, int *out);

#ifdef __cplusplus
}
#endif
#endif /* LIDAR_HIP_H */
