// The multi-frame point head (PointHeadSimpleMultiFrame of tools/cfgs/livox_models/pv_rcnn_multiframe.yaml) and the multi-frame
// union gt boxes of AnchorHeadSingle, for a whole stacked batch.  Each gt carries its pose in every one of the S stacked sweeps:
// locations (B, M, S, 3), rotations_y (B, M, S).  Reference: pcdet/models/dense_heads/point_head_simple_multiframe.py
// (assign_targets :23-56, get_cls_layer_loss :58-90), pcdet/models/dense_heads/anchor_head_single.py:61-89,
// pcdet/utils/box_utils.py (boxes_to_corners_3d, enlarge_box3d), pcdet/utils/common_utils.py (rotate_points_along_z).
//
//   targets   ONE launch in place of the reference's loop over S frames x B batch entries.  One thread per point, 256 per
//             workgroup; the workgroup walks the batch entries its points name as point_head.hip does, stages the S poses of that
//             entry's gt rows once in LDS (cos / sin of -rotations_y once per (gt, s)), and each point walks the rows once per s.
//             Column s of the result is what point_head.hip's kernel writes for gt_boxes with columns 0:3 := locations[:, :, s] and
//             column 6 := rotations_y[:, :, s]: the staged row and the in-box test are the same functions (point_head_dev.h,
//             pt_in_box_dev.h).  The (n, S) labels and owners leave through LDS, so that a workgroup's stores are contiguous.
//   loss fwd  two launches.  The reference's per-point weight is w_n = sum_s [L_ns >= 0] / norm, every term divided first and the
//             terms added in float32 in frame order; it takes one of S values, selected by k_n = #{s: L_ns >= 0}.  Tiles of 256
//             rows write the unnormalised focal sums of their rows separately per k (and #positives), so that norm, which needs
//             the whole batch, enters only in the one-workgroup finalize: it adds the tiles in float64 in a fixed order, forms
//             w(k) as the reference does and writes {cls, npos}.  No atomics: two calls are bit-equal.
//   loss bwd  ONE launch, one row per thread, recomputed from the logits, the labels and the count in the workspace.
//   The quirk kept (point_head_simple_multiframe.py:64-79): a frame column whose label is -1 is still a negative target, weighted by
//   the OTHER frames' share of w_n; a point ignored in every frame weighs 0 and gets exact zero gradients.
//
//   enlarged  ONE launch, one thread per gt row: anchor_head_single.py:67-88 as it runs.  Line 78 writes rotations_y into the LAST
//             column, which for 8-column boxes is the class and is never read by boxes_to_corners_3d, so every frame's corners are
//             turned by the gt's own heading and rotations_y has no effect.  Operation order of the reference: corners (dims *
//             template, rotate by heading, + locations[s]), - gt centre, rotate by -heading, max - min over the 8 S corners.
//
// Declared support (lidar_point_head_mf_supported): 0 <= N <= 2^20, 1 <= B <= 64, 0 <= M <= 128, 1 <= S <= 8, 1 <= num_class <= 4
// (at most 32 logit columns), gt rows of exactly 8 columns [box7 | class].
#include "common.h"
#include "loss_dev.h"
#include "point_head_dev.h"
#include <math.h>

#define PHMF_MAX_S LIDAR_POINT_HEAD_MF_MAX_FRAMES
#define PHMF_MAX_C LIDAR_POINT_HEAD_MF_MAX_CLASS
#define PHMF_MAX_W (PHMF_MAX_S * PHMF_MAX_C)

struct PHMFTargetParams {
    float extra[3];
    int n, batch, m, frames, num_class;
};

// dynamic LDS: max(m * S staged rows, the workgroup's (256, S) labels and owners as ints)
static inline size_t phmf_target_lds(int m, int frames) {
    const size_t stage = sizeof(PHGt) * (size_t)m * frames, outs = sizeof(int) * 2 * PH_THREADS * (size_t)frames;
    return stage > outs ? stage : outs;
}

__global__ __launch_bounds__(PH_THREADS) void point_targets_mf_kernel(PHMFTargetParams p, const float *__restrict__ points,
                                                                      const float *__restrict__ gt, const float *__restrict__ loc,
                                                                      const float *__restrict__ rot, long long *__restrict__ labels,
                                                                      int *__restrict__ owner_out) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ int s_lo[PH_THREADS / 64], s_hi[PH_THREADS / 64];
    PHGt *s_gt = (PHGt *)s_dyn;                       // [s][k]
    const int t = threadIdx.x, S = p.frames;
    const long long row0 = (long long)blockIdx.x * PH_THREADS;
    const long long i = row0 + t;
    float x = 0.f, y = 0.f, z = 0.f;
    int frame = -1;                                   // -1: past the end, or a bs_idx that names no batch entry (labels stay 0)
    if (i < p.n) {
        const float *q = points + (size_t)i * 4;
        x = q[1]; y = q[2]; z = q[3];
        frame = ph_frame_of(q[0], p.batch);
    }
    int lo, hi;
    ph_frame_range(frame, p.batch, s_lo, s_hi, lo, hi);

    int lab[PHMF_MAX_S], own[PHMF_MAX_S];
#pragma unroll
    for (int s = 0; s < PHMF_MAX_S; ++s) { lab[s] = 0; own[s] = -1; }
    for (int f = lo; f <= hi; ++f) {                  // uniform over the workgroup
        if (!__syncthreads_or(frame == f)) continue;  // also: everyone is done with the previous entry's rows
        for (int e = t; e < p.m * S; e += PH_THREADS) {          // e = k * S + s: locations and rotations_y are read contiguously
            const int k = e / S, s = e - k * S;
            const float *g = gt + ((size_t)f * p.m + k) * 8;
            const float *l = loc + ((size_t)f * p.m * S + e) * 3;
            const float row[8] = {l[0], l[1], l[2], g[3], g[4], g[5], rot[(size_t)f * p.m * S + e], g[7]};
            s_gt[s * p.m + k] = ph_stage_gt(row, p.extra);
        }
        __syncthreads();
        if (frame == f) {
#pragma unroll
            for (int s = 0; s < PHMF_MAX_S; ++s) {
                if (s >= S) break;
                const PHGt *rows = s_gt + s * p.m;
                int owner = -1, cls = 0;
                bool ext = false;
                for (int k = 0; k < p.m; ++k) {
                    const PHGt &r = rows[k];
                    float ax, ay;
                    if (owner < 0 && pt_in_box(r.b, x, y, z, ax, ay)) { owner = k; cls = (int)r.cls; }      // .long() truncates
                    if (!ext) ext = pt_in_box(ph_enlarged(r), x, y, z, ax, ay);
                    if (owner >= 0 && ext) break;
                }
                const bool fg = owner >= 0;
                lab[s] = fg ? (p.num_class == 1 ? 1 : cls) : (fg != ext ? -1 : 0);
                own[s] = owner;
            }
        }
    }
    __syncthreads();                                  // the staged rows are dead: their LDS carries the results out
    int *s_lab = (int *)s_dyn, *s_own = s_lab + PH_THREADS * S;
#pragma unroll
    for (int s = 0; s < PHMF_MAX_S; ++s) {
        if (s >= S) break;
        s_lab[t * S + s] = lab[s];
        s_own[t * S + s] = own[s];
    }
    __syncthreads();
    const int cnt = (int)min((long long)PH_THREADS, (long long)p.n - row0) * S;
    for (int e = t; e < cnt; e += PH_THREADS) {
        labels[row0 * S + e] = (long long)s_lab[e];
        if (owner_out) owner_out[row0 * S + e] = s_own[e];
    }
}

// ---------------------------------------------------------------- loss
struct PHMFLossParams {
    float w_cls;
    int n, frames, num_class, tiles;
};

struct PHMFWs {
    float *partial;      // (tiles, PHMF_MAX_S): unnormalised focal sums of each tile's rows with k frames not ignored, at [k - 1]
    int *npos;           // (tiles)
    int *count;          // #(label > 0) over the batch and all frames
};

static inline size_t phmf_ws_layout(int tiles, PHMFWs *w, char *base) {
    WsCarve c{base};
    char *p;
    p = c.take(sizeof(float) * PHMF_MAX_S * (size_t)tiles); if (w) w->partial = (float *)p;
    p = c.take(sizeof(int) * (size_t)tiles);                if (w) w->npos = (int *)p;
    p = c.take(sizeof(int));                                if (w) w->count = (int *)p;
    return c.off;
}

// w(k): k terms 1 / norm added in float32 one after the other (the other S - k terms are zeros and change nothing)
__device__ __forceinline__ float phmf_weight(int k, float inv_norm) {
    float w = 0.0f;
    for (int q = 0; q < k; ++q) w += inv_norm;
    return w;
}

__global__ __launch_bounds__(PH_THREADS) void point_loss_mf_tile_kernel(PHMFLossParams p, const float *__restrict__ cls_preds,
                                                                        const long long *__restrict__ labels, PHMFWs w) {
    __shared__ float s_buf[PH_THREADS * PHMF_MAX_W];
    __shared__ BlockSumLds<PH_THREADS / 64, PHMF_MAX_S, 1> s_red;
    const int t = threadIdx.x, S = p.frames, C = p.num_class, W = S * C;
    const long long row0 = (long long)blockIdx.x * PH_THREADS;
    const long long i = row0 + t;
    ph_tile_load(s_buf, cls_preds, row0, p.n, W);
    __syncthreads();
    float v = 0.0f;
    int k = 0, npos = 0;
    if (i < p.n) {
        const long long *L = labels + i * S;
        for (int s = 0; s < S; ++s) { k += L[s] >= 0; npos += L[s] > 0; }
        if (k > 0)
            for (int s = 0; s < S; ++s) {
                const long long lab = L[s];
                for (int c = 0; c < C; ++c) v += sigmoid_focal(s_buf[t * W + s * C + c], lab == c + 1 ? 1.0f : 0.0f, nullptr);
            }
    }
    float sum[PHMF_MAX_S];
#pragma unroll
    for (int q = 0; q < PHMF_MAX_S; ++q) sum[q] = q == k - 1 ? v : 0.0f;
    int cnt[1] = {npos};
    block_sum(sum, cnt, s_red);
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < PHMF_MAX_S; ++q) w.partial[(size_t)blockIdx.x * PHMF_MAX_S + q] = sum[q];
        w.npos[blockIdx.x] = cnt[0];
    }
}

__global__ __launch_bounds__(PH_THREADS) void point_loss_mf_finalize_kernel(PHMFLossParams p, PHMFWs w, float *__restrict__ out) {
    __shared__ double s_sum[PH_THREADS];
    __shared__ int s_cnt[PH_THREADS];
    const int t = threadIdx.x;
    double acc[PHMF_MAX_S];
#pragma unroll
    for (int q = 0; q < PHMF_MAX_S; ++q) acc[q] = 0.0;
    int npos = 0;
    for (int k = t; k < p.tiles; k += PH_THREADS) {      // thread t takes tiles t, t + 256, ... in order
#pragma unroll
        for (int q = 0; q < PHMF_MAX_S; ++q) acc[q] += (double)w.partial[(size_t)k * PHMF_MAX_S + q];
        npos += w.npos[k];
    }
    s_cnt[t] = npos;
    __syncthreads();
    for (int h = PH_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) s_cnt[t] += s_cnt[t + h];
        __syncthreads();
    }
    npos = s_cnt[0];
    const float inv = 1.0f / fmaxf((float)npos, 1.0f);
    double v = 0.0;
#pragma unroll
    for (int q = 0; q < PHMF_MAX_S; ++q) v += (double)phmf_weight(q + 1, inv) * acc[q];      // acc[q] is 0 for q >= S
    s_sum[t] = v;
    __syncthreads();
    for (int h = PH_THREADS / 2; h > 0; h >>= 1) {       // the fixed tree of ordered_reduce.h
        if (t < h) s_sum[t] += s_sum[t + h];
        __syncthreads();
    }
    if (t == 0) {
        out[0] = (float)s_sum[0] * p.w_cls;
        out[1] = (float)npos;
        *w.count = npos;
    }
}

__global__ __launch_bounds__(PH_THREADS) void point_loss_mf_bwd_kernel(PHMFLossParams p, const float *__restrict__ cls_preds,
                                                                       const long long *__restrict__ labels, PHMFWs w,
                                                                       const float *__restrict__ grad, float *__restrict__ d_cls) {
    __shared__ float s_buf[PH_THREADS * PHMF_MAX_W];
    const int t = threadIdx.x, S = p.frames, C = p.num_class, W = S * C;
    const long long row0 = (long long)blockIdx.x * PH_THREADS;
    const long long i = row0 + t;
    const float inv = 1.0f / fmaxf((float)*w.count, 1.0f);
    ph_tile_load(s_buf, cls_preds, row0, p.n, W);
    __syncthreads();
    if (i < p.n) {
        const long long *L = labels + i * S;
        int k = 0;
        for (int s = 0; s < S; ++s) k += L[s] >= 0;
        const float sc = grad[0] * p.w_cls * phmf_weight(k, inv);
        for (int s = 0; s < S; ++s) {
            const long long lab = L[s];
            for (int c = 0; c < C; ++c) {
                float dx = 0.0f;
                if (k > 0) sigmoid_focal(s_buf[t * W + s * C + c], lab == c + 1 ? 1.0f : 0.0f, &dx);
                s_buf[t * W + s * C + c] = k > 0 ? sc * dx : 0.0f;      // each thread rewrites only its own row
            }
        }
    }
    __syncthreads();
    ph_tile_store(s_buf, d_cls, row0, p.n, W);
}

// ---------------------------------------------------------------- multi-frame union boxes
__global__ __launch_bounds__(PH_THREADS) void multiframe_enlarged_boxes_kernel(int rows, int frames, const float *__restrict__ gt,
                                                                               const float *__restrict__ loc, float *__restrict__ out) {
    const int r = blockIdx.x * PH_THREADS + threadIdx.x;
    if (r >= rows) return;
    float g[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) g[q] = gt[(size_t)r * 8 + q];
    // cos / sin correctly rounded to fp32 via double, as make_boxcs forms them
    const float ca = (float)cos((double)g[6]), sa = (float)sin((double)g[6]);
    const float cb = (float)cos((double)-g[6]), sb = (float)sin((double)-g[6]);
    float xlo = INFINITY, xhi = -INFINITY, ylo = INFINITY, yhi = -INFINITY;
    for (int s = 0; s < frames; ++s) {
        const float *l = loc + ((size_t)r * frames + s) * 3;
#pragma unroll
        for (int c = 0; c < 4; ++c) {      // the template's (x, y) signs; its z does not reach the x / y extents
            const float tx = (c == 0 || c == 1) ? 0.5f : -0.5f, ty = (c == 0 || c == 3) ? 0.5f : -0.5f;
            const float px = g[3] * tx, py = g[4] * ty;
            // points @ [[cos, sin, 0], [-sin, cos, 0], [0, 0, 1]], + the frame's location, - the gt centre
            const float wx = (px * ca + py * (-sa)) + l[0] - g[0], wy = (px * sa + py * ca) + l[1] - g[1];
            const float lx = wx * cb + wy * (-sb), ly = wx * sb + wy * cb;
            xlo = fminf(xlo, lx); xhi = fmaxf(xhi, lx);
            ylo = fminf(ylo, ly); yhi = fmaxf(yhi, ly);
        }
    }
    g[3] = xhi - xlo;
    g[4] = yhi - ylo;
#pragma unroll
    for (int q = 0; q < 8; ++q) out[(size_t)r * 8 + q] = g[q];
}

// ---------------------------------------------------------------- host side
LIDAR_EXPORT int lidar_point_head_mf_supported(long long n, int batch, int m, int stack_frames, int num_class) {
    return n >= 0 && n <= PH_MAX_N && batch >= 1 && batch <= PH_MAX_B && m >= 0 && m <= PH_MAX_M && stack_frames >= 1 &&
           stack_frames <= PHMF_MAX_S && num_class >= 1 && num_class <= PHMF_MAX_C;
}

LIDAR_EXPORT int lidar_point_targets_mf(const float *points, long long n, const float *gt_boxes, const float *locations,
                                        const float *rotations_y, int batch, int m, int stack_frames, const float *extra_width,
                                        int num_class, long long *point_cls_labels, int *point_box_idx, void *stream) {
    if (!lidar_point_head_mf_supported(n, batch, m, stack_frames, num_class) || !extra_width) return LIDAR_ERR_ARG;
    if (n == 0) return LIDAR_OK;
    if (!points || (m > 0 && (!gt_boxes || !locations || !rotations_y)) || !point_cls_labels) return LIDAR_ERR_ARG;
    PHMFTargetParams p = {};
    for (int q = 0; q < 3; ++q) p.extra[q] = extra_width[q];
    p.n = (int)n; p.batch = batch; p.m = m; p.frames = stack_frames; p.num_class = num_class;
    hipLaunchKernelGGL(point_targets_mf_kernel, dim3((unsigned)divup(n, PH_THREADS)), dim3(PH_THREADS),
                       phmf_target_lds(m, stack_frames), (hipStream_t)stream, p, points, gt_boxes, locations, rotations_y,
                       point_cls_labels, point_box_idx);
    return lidar_check_launch("lidar_point_targets_mf");
}

LIDAR_EXPORT size_t lidar_point_loss_mf_ws_bytes(long long n) {
    if (n < 0 || n > PH_MAX_N) return 0;
    return phmf_ws_layout(divup(n, PH_THREADS), nullptr, nullptr);
}

static int phmf_loss_params(PHMFLossParams &p, long long n, int stack_frames, int num_class, float point_cls_weight) {
    if (!lidar_point_head_mf_supported(n, 1, 0, stack_frames, num_class)) return LIDAR_ERR_ARG;
    p = PHMFLossParams{};
    p.w_cls = point_cls_weight;
    p.n = (int)n; p.frames = stack_frames; p.num_class = num_class; p.tiles = divup(n, PH_THREADS);
    return LIDAR_OK;
}

LIDAR_EXPORT int lidar_point_loss_mf_forward(const float *point_cls_preds, const long long *point_cls_labels, long long n,
                                             int stack_frames, int num_class, float point_cls_weight, float *out, void *ws,
                                             size_t ws_bytes, void *stream) {
    PHMFLossParams p;
    const int st = phmf_loss_params(p, n, stack_frames, num_class, point_cls_weight);
    if (st != LIDAR_OK) return st;
    if (!out) return LIDAR_ERR_ARG;
    if (n == 0) {      // nothing to launch: zero loss, zero positives
        if (hipMemsetAsync(out, 0, 2 * sizeof(float), (hipStream_t)stream) != hipSuccess) return LIDAR_ERR_LAUNCH;
        return LIDAR_OK;
    }
    if (!point_cls_preds || !point_cls_labels || !ws) return LIDAR_ERR_ARG;
    PHMFWs w;
    if (ws_bytes < phmf_ws_layout(p.tiles, &w, (char *)ws)) return LIDAR_ERR_WORKSPACE;
    hipLaunchKernelGGL(point_loss_mf_tile_kernel, dim3((unsigned)p.tiles), dim3(PH_THREADS), 0, (hipStream_t)stream, p,
                       point_cls_preds, point_cls_labels, w);
    hipLaunchKernelGGL(point_loss_mf_finalize_kernel, dim3(1), dim3(PH_THREADS), 0, (hipStream_t)stream, p, w, out);
    return lidar_check_launch("lidar_point_loss_mf_forward");
}

LIDAR_EXPORT int lidar_point_loss_mf_backward(const float *point_cls_preds, const long long *point_cls_labels, long long n,
                                              int stack_frames, int num_class, float point_cls_weight, const float *grad_out,
                                              float *d_cls_preds, void *ws, size_t ws_bytes, void *stream) {
    PHMFLossParams p;
    const int st = phmf_loss_params(p, n, stack_frames, num_class, point_cls_weight);
    if (st != LIDAR_OK) return st;
    if (n == 0) return LIDAR_OK;
    if (!point_cls_preds || !point_cls_labels || !grad_out || !d_cls_preds || !ws) return LIDAR_ERR_ARG;
    PHMFWs w;
    if (ws_bytes < phmf_ws_layout(p.tiles, &w, (char *)ws)) return LIDAR_ERR_WORKSPACE;
    hipLaunchKernelGGL(point_loss_mf_bwd_kernel, dim3((unsigned)p.tiles), dim3(PH_THREADS), 0, (hipStream_t)stream, p,
                       point_cls_preds, point_cls_labels, w, grad_out, d_cls_preds);
    return lidar_check_launch("lidar_point_loss_mf_backward");
}

LIDAR_EXPORT int lidar_multiframe_enlarged_boxes(const float *gt_boxes, const float *locations, int batch, int m, int gt_dim,
                                                 int stack_frames, float *gt_boxes_enlarged, void *stream) {
    if (!lidar_point_head_mf_supported(0, batch, m, stack_frames, 1) || gt_dim != 8) return LIDAR_ERR_ARG;
    if (m == 0) return LIDAR_OK;
    if (!gt_boxes || !locations || !gt_boxes_enlarged) return LIDAR_ERR_ARG;
    const int rows = batch * m;
    hipLaunchKernelGGL(multiframe_enlarged_boxes_kernel, dim3((unsigned)divup(rows, PH_THREADS)), dim3(PH_THREADS), 0,
                       (hipStream_t)stream, rows, stack_frames, gt_boxes, locations, gt_boxes_enlarged);
    return lidar_check_launch("lidar_multiframe_enlarged_boxes");
}
