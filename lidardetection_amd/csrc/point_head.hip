// Point-head targets and loss (PointHeadSimple / PointHeadBox / PointIntraPartOffsetHead) for a whole stacked batch.  Reference:
// pcdet/models/dense_heads/point_head_template.py (assign_stack_targets :49-129 with set_ignore_flag=True, get_cls_layer_loss
// :131-155, get_part_layer_loss :157-170, get_box_layer_loss :172-191), pcdet/utils/box_coder_utils.py:153-187
// (PointResidualCoder.encode_torch), pcdet/utils/box_utils.py (enlarge_box3d), pcdet/utils/loss_utils.py:9-136
// (SigmoidFocalClassificationLoss, WeightedSmoothL1Loss), pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:23-36, 313-336.
//
//   targets   ONE launch, one thread per point, 256 per workgroup.  Rows come in any frame order, so a workgroup walks the frames
//             its points name (smallest to largest bs_idx, frames without a point of the workgroup skipped by a workgroup-wide
//             vote), stages that frame's gt rows once in LDS (centre, dims, cos / sin of -rz, enlarged dims, heading, class) and
//             each of its points walks them: owner = the first row whose box holds the point, ignore = fg XOR (any enlarged box
//             holds it).  Padding rows take part like any other row, enlarged as well, as in the reference.  Every output
//             element is written: labels int64, box labels (N, 8), part labels (N, 3), owner int32.
//   loss fwd  two launches: tiles of 256 rows write unnormalised partials {cls, box, part, #positives} (wave shuffles, then the
//             four waves in order), a one-workgroup finalize sums the tiles in tile order (thread t takes tiles t, t + 256, ...,
//             then lanes by shuffle and waves in order), divides, applies the weights and writes the record {cls, box, part,
//             pos_num}.  No atomics: two calls are bit-equal.  The workspace keeps the partials and the count.
//   loss bwd  ONE launch, one row per thread, recomputed from the inputs and the count in the workspace; the upstream triple is
//             read from device memory.  Rows without a contribution get exact zeros.
// The (N, C) logits and all three gradient outputs go through LDS so that global accesses are contiguous over the tile; box and
// part rows are read by the positive rows only (a few per cent of the points), directly.
//
// The element math is loss_dev.h's, the ordered sums common.h's block_sum; the staged gt row, the frame walk's range and the tile
// copies are point_head_dev.h's, shared with point_head_mf.hip.
// cls: sigmoid_focal; the one-hot column of label c > 0 is c - 1; rows with label -1 weigh 0.
// box: smooth_l1 over the 8 codes, positives only.
// part: bce_logits, positives only (the deviation from binary_cross_entropy that roi_loss.hip documents for its cls term).
//
// Declared support (lidar_point_head_supported): 0 <= N <= 2^20, 1 <= B <= 64, 0 <= M <= 128, 1 <= num_class <= 8,
// 0 <= n_mean <= 8, gt rows of exactly 8 columns [box7 | class].
#include "common.h"
#include "loss_dev.h"
#include "point_head_dev.h"
#include <math.h>

#define PH_MAX_C LIDAR_POINT_HEAD_MAX_CLASS
#define PH_MAX_MEAN LIDAR_POINT_HEAD_MAX_MEAN

struct PHTargetParams {
    float extra[3];
    float mean[PH_MAX_MEAN * 3];
    int n, batch, m, num_class, n_mean, ret_box, ret_part;
};

__global__ __launch_bounds__(PH_THREADS) void point_targets_kernel(PHTargetParams p, const float *__restrict__ points,
                                                                   const float *__restrict__ gt,
                                                                   long long *__restrict__ labels, float *__restrict__ box_labels,
                                                                   float *__restrict__ part_labels, int *__restrict__ owner_out) {
    __shared__ PHGt s_gt[PH_MAX_M];
    __shared__ int s_lo[PH_THREADS / 64], s_hi[PH_THREADS / 64];
    __shared__ float s_mean[PH_MAX_MEAN * 3];         // indexed per point: LDS, so that the by-value table never goes to scratch
    const int t = threadIdx.x;
    const int i = blockIdx.x * PH_THREADS + t;
    if (t < PH_MAX_MEAN * 3) s_mean[t] = p.mean[t];   // made visible by the barrier below
    float x = 0.f, y = 0.f, z = 0.f;
    int frame = -1;                                   // -1: past the end, or a bs_idx that names no frame (the row keeps label 0)
    if (i < p.n) {
        const float *q = points + (size_t)i * 4;
        x = q[1]; y = q[2]; z = q[3];
        frame = ph_frame_of(q[0], p.batch);
    }
    // the range of frames this workgroup has to visit
    int lo, hi;
    ph_frame_range(frame, p.batch, s_lo, s_hi, lo, hi);

    int owner = -1;
    bool ext = false;
    float lx = 0.f, ly = 0.f;                         // the point in the owner's frame
    float g[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};      // the owner's gt row
    for (int f = lo; f <= hi; ++f) {                  // uniform over the workgroup
        if (!__syncthreads_or(frame == f)) continue;  // also: everyone is done with the previous frame's rows
        for (int k = t; k < p.m; k += PH_THREADS) s_gt[k] = ph_stage_gt(gt + ((size_t)f * p.m + k) * 8, p.extra);
        __syncthreads();
        if (frame == f) {
            for (int k = 0; k < p.m; ++k) {
                const PHGt &r = s_gt[k];
                float ax, ay;
                if (owner < 0 && pt_in_box(r.b, x, y, z, ax, ay)) {
                    owner = k; lx = ax; ly = ay;
                    g[0] = r.b.cx; g[1] = r.b.cy; g[2] = r.b.cz; g[3] = r.b.dx; g[4] = r.b.dy; g[5] = r.b.dz; g[6] = r.rz; g[7] = r.cls;
                }
                if (!ext) ext = pt_in_box(ph_enlarged(r), x, y, z, ax, ay);
                if (owner >= 0 && ext) break;
            }
        }
    }
    if (i >= p.n) return;
    const bool fg = owner >= 0;
    const bool ignore = fg != ext;
    const int cls = fg ? (int)g[7] : 0;               // .long() truncates
    labels[i] = fg ? (p.num_class == 1 ? 1ll : (long long)cls) : (ignore ? -1ll : 0ll);
    owner_out[i] = owner;
    if (p.ret_box) {
        float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (fg) {
            // PointResidualCoder.encode_torch; clamp_min keeps a NaN
            const float dxg = g[3] < 1e-5f ? 1e-5f : g[3], dyg = g[4] < 1e-5f ? 1e-5f : g[4], dzg = g[5] < 1e-5f ? 1e-5f : g[5];
            if (p.n_mean > 0) {
                // mean_size[class - 1] with torch's negative indexing: class 0 (a padding row's) takes the last row.  A class
                // beyond n_mean is an error in the reference; here it wraps, so that the index stays inside the table.
                int mi = (cls - 1) % p.n_mean;
                if (mi < 0) mi += p.n_mean;
                const float dxa = s_mean[mi * 3], dya = s_mean[mi * 3 + 1], dza = s_mean[mi * 3 + 2];
                const float diag = sqrtf(dxa * dxa + dya * dya);
                o[0] = (g[0] - x) / diag; o[1] = (g[1] - y) / diag; o[2] = (g[2] - z) / dza;
                o[3] = logf(dxg / dxa); o[4] = logf(dyg / dya); o[5] = logf(dzg / dza);
            } else {
                o[0] = g[0] - x; o[1] = g[1] - y; o[2] = g[2] - z;
                o[3] = logf(dxg); o[4] = logf(dyg); o[5] = logf(dzg);
            }
            o[6] = cosf(g[6]); o[7] = sinf(g[6]);
        }
#pragma unroll
        for (int q = 0; q < 8; ++q) box_labels[(size_t)i * 8 + q] = o[q];
    }
    if (p.ret_part) {
        // rotate_points_along_z(p - centre, -rz) / dims + 0.5: lx, ly are that rotation's x and y.  The dims are not clamped,
        // unless box labels are made as well: the reference's encode_torch clamps the rows it is handed in place at 1e-5, and the
        // part labels are formed from the same rows afterwards
        float o[3] = {0.f, 0.f, 0.f};
        if (fg) {
            const float dx = (p.ret_box && g[3] < 1e-5f) ? 1e-5f : g[3], dy = (p.ret_box && g[4] < 1e-5f) ? 1e-5f : g[4];
            const float dz = (p.ret_box && g[5] < 1e-5f) ? 1e-5f : g[5];
            o[0] = lx / dx + 0.5f; o[1] = ly / dy + 0.5f; o[2] = (z - g[2]) / dz + 0.5f;
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) part_labels[(size_t)i * 3 + q] = o[q];
    }
}

// ---------------------------------------------------------------- loss
struct PHLossParams {
    float code_w[8];
    float w_cls, w_box, w_part;
    int n, num_class, tiles;
};

struct PHWs {
    float *partial;      // (tiles, 3): unnormalised cls, box, part sums of each tile
    int *npos;           // (tiles)
    int *count;          // #(label > 0) over the batch
};

static inline size_t ph_ws_layout(int tiles, PHWs *w, char *base) {
    WsCarve c{base};
    char *p;
    p = c.take(sizeof(float) * 3 * (size_t)tiles); if (w) w->partial = (float *)p;
    p = c.take(sizeof(int) * (size_t)tiles);       if (w) w->npos = (int *)p;
    p = c.take(sizeof(int));                       if (w) w->count = (int *)p;
    return c.off;
}

__global__ __launch_bounds__(PH_THREADS) void point_loss_tile_kernel(PHLossParams p, const float *__restrict__ cls_preds,
                                                                     const float *__restrict__ box_preds,
                                                                     const float *__restrict__ part_preds,
                                                                     const long long *__restrict__ labels,
                                                                     const float *__restrict__ box_labels,
                                                                     const float *__restrict__ part_labels, PHWs w) {
    __shared__ float s_buf[PH_THREADS * PH_MAX_C];
    __shared__ BlockSumLds<PH_THREADS / 64, 3, 1> s_red;
    const int t = threadIdx.x, C = p.num_class;
    const long long row0 = (long long)blockIdx.x * PH_THREADS;
    const long long i = row0 + t;
    if (cls_preds) ph_tile_load(s_buf, cls_preds, row0, p.n, C);
    __syncthreads();
    float cls = 0.0f, box = 0.0f, part = 0.0f;
    int npos = 0;
    if (i < p.n) {
        const long long lab = labels[i];
        if (cls_preds && lab >= 0)
            for (int j = 0; j < C; ++j) cls += sigmoid_focal(s_buf[t * C + j], lab == j + 1 ? 1.0f : 0.0f, nullptr);
        if (lab > 0) {
            npos = 1;
            if (box_preds) {
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    box += smooth_l1(box_preds[(size_t)i * 8 + q], box_labels[(size_t)i * 8 + q], p.code_w[q], nullptr);
            }
            if (part_preds) {
#pragma unroll
                for (int q = 0; q < 3; ++q)
                    part += bce_logits(part_preds[(size_t)i * 3 + q], part_labels[(size_t)i * 3 + q], nullptr);
            }
        }
    }
    float sum[3] = {cls, box, part};
    int cnt[1] = {npos};
    block_sum(sum, cnt, s_red);
    if (t == 0) {
#pragma unroll
        for (int q = 0; q < 3; ++q) w.partial[(size_t)blockIdx.x * 3 + q] = sum[q];
        w.npos[blockIdx.x] = cnt[0];
    }
}

__global__ __launch_bounds__(PH_THREADS) void point_loss_finalize_kernel(PHLossParams p, PHWs w, float *__restrict__ out) {
    __shared__ BlockSumLds<PH_THREADS / 64, 3, 1> s_red;
    const int t = threadIdx.x;
    float sum[3] = {0.0f, 0.0f, 0.0f};      // cls, box, part
    int npos[1] = {0};
    for (int k = t; k < p.tiles; k += PH_THREADS) {
#pragma unroll
        for (int q = 0; q < 3; ++q) sum[q] += w.partial[(size_t)k * 3 + q];
        npos[0] += w.npos[k];
    }
    block_sum(sum, npos, s_red);
    if (t == 0) {
        const float nf = fmaxf((float)npos[0], 1.0f);
        out[0] = sum[0] / nf * p.w_cls;
        out[1] = sum[1] / nf * p.w_box;
        out[2] = sum[2] / (3.0f * nf) * p.w_part;
        out[3] = (float)npos[0];
        *w.count = npos[0];
    }
}

__global__ __launch_bounds__(PH_THREADS) void point_loss_bwd_kernel(PHLossParams p, const float *__restrict__ cls_preds,
                                                                    const float *__restrict__ box_preds,
                                                                    const float *__restrict__ part_preds,
                                                                    const long long *__restrict__ labels,
                                                                    const float *__restrict__ box_labels,
                                                                    const float *__restrict__ part_labels, PHWs w,
                                                                    const float *__restrict__ grad, float *__restrict__ d_cls,
                                                                    float *__restrict__ d_box, float *__restrict__ d_part) {
    __shared__ float s_buf[PH_THREADS * PH_MAX_C];
    const int t = threadIdx.x, C = p.num_class;
    const long long row0 = (long long)blockIdx.x * PH_THREADS;
    const long long i = row0 + t;
    const float nf = fmaxf((float)*w.count, 1.0f);
    const long long lab = i < p.n ? labels[i] : -1;
    if (d_cls) {
        ph_tile_load(s_buf, cls_preds, row0, p.n, C);
        __syncthreads();
        if (i < p.n) {
            const float sc = grad[0] * p.w_cls / nf;
            for (int j = 0; j < C; ++j) {
                float dx = 0.0f;
                if (lab >= 0) sigmoid_focal(s_buf[t * C + j], lab == j + 1 ? 1.0f : 0.0f, &dx);
                s_buf[t * C + j] = lab >= 0 ? sc * dx : 0.0f;      // each thread rewrites only its own row
            }
        }
        __syncthreads();
        ph_tile_store(s_buf, d_cls, row0, p.n, C);
        __syncthreads();
    }
    if (d_box) {
        if (i < p.n) {
            const float sc = grad[1] * p.w_box / nf;
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                float dx = 0.0f;
                if (lab > 0) smooth_l1(box_preds[(size_t)i * 8 + q], box_labels[(size_t)i * 8 + q], p.code_w[q], &dx);
                s_buf[t * 8 + q] = lab > 0 ? sc * dx : 0.0f;
            }
        }
        __syncthreads();
        ph_tile_store(s_buf, d_box, row0, p.n, 8);
        __syncthreads();
    }
    if (d_part) {
        if (i < p.n) {
            const float sc = grad[2] * p.w_part / (3.0f * nf);
#pragma unroll
            for (int q = 0; q < 3; ++q) {
                float dx = 0.0f;
                if (lab > 0) bce_logits(part_preds[(size_t)i * 3 + q], part_labels[(size_t)i * 3 + q], &dx);
                s_buf[t * 3 + q] = lab > 0 ? sc * dx : 0.0f;
            }
        }
        __syncthreads();
        ph_tile_store(s_buf, d_part, row0, p.n, 3);
    }
}

// ---------------------------------------------------------------- host side
LIDAR_EXPORT int lidar_point_head_supported(long long n, int batch, int m, int gt_dim, int num_class, int n_mean) {
    return n >= 0 && n <= PH_MAX_N && batch >= 1 && batch <= PH_MAX_B && m >= 0 && m <= PH_MAX_M && gt_dim == 8 && num_class >= 1 &&
           num_class <= PH_MAX_C && n_mean >= 0 && n_mean <= PH_MAX_MEAN;
}

LIDAR_EXPORT int lidar_point_targets(const float *points, long long n, const float *gt_boxes, int batch, int m, int gt_dim,
                                     const float *extra_width, int num_class, int flags, const float *mean_size, int n_mean,
                                     long long *point_cls_labels, float *point_box_labels, float *point_part_labels,
                                     int *point_box_idx, void *stream) {
    if (!lidar_point_head_supported(n, batch, m, gt_dim, num_class, n_mean) || !extra_width || (flags & ~3) || (n_mean > 0 && !mean_size))
        return LIDAR_ERR_ARG;
    if (n == 0) return LIDAR_OK;
    if (!points || (m > 0 && !gt_boxes) || !point_cls_labels || !point_box_idx || ((flags & 1) && !point_box_labels) ||
        ((flags & 2) && !point_part_labels))
        return LIDAR_ERR_ARG;
    PHTargetParams p = {};
    for (int q = 0; q < 3; ++q) p.extra[q] = extra_width[q];
    for (int q = 0; q < n_mean * 3; ++q) p.mean[q] = mean_size[q];
    p.n = (int)n; p.batch = batch; p.m = m; p.num_class = num_class; p.n_mean = n_mean;
    p.ret_box = flags & 1; p.ret_part = (flags & 2) ? 1 : 0;
    hipLaunchKernelGGL(point_targets_kernel, dim3((unsigned)divup(n, PH_THREADS)), dim3(PH_THREADS), 0, (hipStream_t)stream, p,
                       points, gt_boxes, point_cls_labels, point_box_labels, point_part_labels, point_box_idx);
    return lidar_check_launch("lidar_point_targets");
}

LIDAR_EXPORT size_t lidar_point_loss_ws_bytes(long long n) {
    if (n < 0 || n > PH_MAX_N) return 0;
    return ph_ws_layout(divup(n, PH_THREADS), nullptr, nullptr);
}

static int ph_loss_params(PHLossParams &p, long long n, int num_class, const float *weights, const float *code_weights) {
    if (!lidar_point_head_supported(n, 1, 0, 8, num_class, 0) || !weights || !code_weights) return LIDAR_ERR_ARG;
    p = PHLossParams{};
    for (int q = 0; q < 8; ++q) p.code_w[q] = code_weights[q];
    p.w_cls = weights[0]; p.w_box = weights[1]; p.w_part = weights[2];
    p.n = (int)n; p.num_class = num_class; p.tiles = divup(n, PH_THREADS);
    return LIDAR_OK;
}

LIDAR_EXPORT int lidar_point_loss_forward(const float *point_cls_preds, const float *point_box_preds, const float *point_part_preds,
                                          const long long *point_cls_labels, const float *point_box_labels,
                                          const float *point_part_labels, long long n, int num_class, const float *weights,
                                          const float *code_weights, float *out, void *ws, size_t ws_bytes, void *stream) {
    PHLossParams p;
    const int st = ph_loss_params(p, n, num_class, weights, code_weights);
    if (st != LIDAR_OK) return st;
    if (!out) return LIDAR_ERR_ARG;
    if (n == 0) {      // nothing to launch: zero losses, zero positives
        if (hipMemsetAsync(out, 0, 4 * sizeof(float), (hipStream_t)stream) != hipSuccess) return LIDAR_ERR_LAUNCH;
        return LIDAR_OK;
    }
    if (!point_cls_labels || !ws || (point_box_preds && !point_box_labels) || (point_part_preds && !point_part_labels))
        return LIDAR_ERR_ARG;
    PHWs w;
    if (ws_bytes < ph_ws_layout(p.tiles, &w, (char *)ws)) return LIDAR_ERR_WORKSPACE;
    hipLaunchKernelGGL(point_loss_tile_kernel, dim3((unsigned)p.tiles), dim3(PH_THREADS), 0, (hipStream_t)stream, p, point_cls_preds,
                       point_box_preds, point_part_preds, point_cls_labels, point_box_labels, point_part_labels, w);
    hipLaunchKernelGGL(point_loss_finalize_kernel, dim3(1), dim3(PH_THREADS), 0, (hipStream_t)stream, p, w, out);
    return lidar_check_launch("lidar_point_loss_forward");
}

LIDAR_EXPORT int lidar_point_loss_backward(const float *point_cls_preds, const float *point_box_preds, const float *point_part_preds,
                                           const long long *point_cls_labels, const float *point_box_labels,
                                           const float *point_part_labels, long long n, int num_class, const float *weights,
                                           const float *code_weights, const float *grad_out, float *d_cls_preds, float *d_box_preds,
                                           float *d_part_preds, void *ws, size_t ws_bytes, void *stream) {
    PHLossParams p;
    const int st = ph_loss_params(p, n, num_class, weights, code_weights);
    if (st != LIDAR_OK) return st;
    if (n == 0 || (!d_cls_preds && !d_box_preds && !d_part_preds)) return LIDAR_OK;
    if (!grad_out || !ws || !point_cls_labels || (d_cls_preds && !point_cls_preds) ||
        (d_box_preds && (!point_box_preds || !point_box_labels)) || (d_part_preds && (!point_part_preds || !point_part_labels)))
        return LIDAR_ERR_ARG;
    PHWs w;
    if (ws_bytes < ph_ws_layout(p.tiles, &w, (char *)ws)) return LIDAR_ERR_WORKSPACE;
    hipLaunchKernelGGL(point_loss_bwd_kernel, dim3((unsigned)p.tiles), dim3(PH_THREADS), 0, (hipStream_t)stream, p, point_cls_preds,
                       point_box_preds, point_part_preds, point_cls_labels, point_box_labels, point_part_labels, w, grad_out,
                       d_cls_preds, d_box_preds, d_part_preds);
    return lidar_check_launch("lidar_point_loss_backward");
}
