// RoI-head loss (RoIHeadTemplate.get_loss: get_box_cls_layer_loss + get_box_reg_layer_loss with the corner regulariser) for a
// whole batch of sampled rois: one fused forward launch and a scale-and-store backward.  Reference:
// pcdet/models/roi_heads/roi_head_template.py:133-233, pcdet/utils/box_coder_utils.py:13-77 (ResidualCoder encode / decode),
// pcdet/utils/loss_utils.py (WeightedSmoothL1Loss :75-136, get_corner_loss_lidar :209-232), pcdet/utils/box_utils.py:27-52
// (boxes_to_corners_3d), pcdet/utils/common_utils.py:66-88 (rotate_points_along_z).
//
//   forward   ONE workgroup of 1024 threads.  The workload is a few thousand rows at most and latency-bound, so the kernel is
//             sized for launch count: thread t takes rows t, t + 1024, ... in order, evaluates the three terms of its rows and
//             leaves each row's UNSCALED gradient pieces (d bce / d logit, d smooth-L1 / d code, d corner / d code) in the
//             workspace; the five sums (three losses, #fg, #valid) go through common.h's block_sum (wave64 shuffles, then the 16
//             waves in wave order).  No atomics of any kind: two calls are bit-equal.  Thread 0 normalises, writes the 5-float
//             record and keeps the two counts in the workspace.
//   backward  one thread per row: d_cls = g0 * w_cls / max(n_valid, 1) * piece, d_reg = g1 * w_reg / max(fg, 1) * piece_reg +
//             g2 * w_corner / max(fg, 1) * piece_corner, the upstream triple read from device memory.
//
// Classification is loss_dev.h's bce_logits: equal to the reference's binary_cross_entropy(sigmoid(x), t) wherever that function's
// -100 log clamp and 1e-12 denominator clamp do not engage, and continued past them (the one deliberate deviation).  The regression
// codes are loss_dev.h's smooth_l1.  Non-fg rows are skipped, not multiplied by 0.  The corner
// difference subtracts the roi centre from the gt instead of adding it to the prediction, and the flipped gt's corners are the
// unflipped ones with x and y offsets negated (a rotation by pi).  The corner gradient never divides by a zero distance: below the
// smooth-L1 knee (beta 1) d L / d diff is diff itself.
#include "common.h"
#include "loss_dev.h"
#include <math.h>

#define RL_THREADS 1024
#define RL_MAX_P LIDAR_ROI_LOSS_MAX_SAMPLES
#define RL_MAX_ROWS LIDAR_ROI_LOSS_MAX_ROWS
#define RL_BWD_THREADS 256

struct RLParams {
    float code_w[7];
    float w_cls, w_reg, w_corner;
    int n;         // rows
    int corner;    // CORNER_LOSS_REGULARIZATION
};

struct RLWs {
    float *g_cls;      // (n)     sigmoid(x) - t on valid rows, 0 elsewhere
    float *g_reg;      // (n, 7)  d sum_7 smooth-L1 / d rcnn_reg on fg rows, 0 elsewhere
    float *g_corner;   // (n, 7)  d (mean_8 smooth-L1(corner distance)) / d rcnn_reg on fg rows, 0 elsewhere
    int *counts;       // fg_sum, n_valid
};

static inline size_t rl_ws_layout(long long n, RLWs *w, char *base) {
    WsCarve c{base};
    char *p;
    p = c.take(sizeof(float) * (size_t)n);     if (w) w->g_cls = (float *)p;
    p = c.take(sizeof(float) * (size_t)n * 7); if (w) w->g_reg = (float *)p;
    p = c.take(sizeof(float) * (size_t)n * 7); if (w) w->g_corner = (float *)p;
    p = c.take(sizeof(int) * 2);               if (w) w->counts = (int *)p;
    return c.off;
}

// torch.clamp_min(x, 1e-5): a NaN stays a NaN (fmaxf would drop it)
__device__ __forceinline__ float rl_clamp_min(float x) { return x < 1e-5f ? 1e-5f : x; }

// the regression term of one fg row: ResidualCoder.encode_torch(gt (canonical frame), roi with centre and heading zeroed), NaN
// targets take the prediction, code weights, smooth-L1 beta 1/9 summed over the 7 codes; g[q] = d / d pred[q]
__device__ __forceinline__ float rl_reg(const RLParams &p, const float *pr, const float *roi, const float *gt, float *g) {
    const float dxa = rl_clamp_min(roi[3]), dya = rl_clamp_min(roi[4]), dza = rl_clamp_min(roi[5]);
    const float dxg = rl_clamp_min(gt[3]), dyg = rl_clamp_min(gt[4]), dzg = rl_clamp_min(gt[5]);
    const float diag = sqrtf(dxa * dxa + dya * dya);
    const float tg[7] = {gt[0] / diag, gt[1] / diag, gt[2] / dza, logf(dxg / dxa), logf(dyg / dya), logf(dzg / dza), gt[6]};
    float loss = 0.0f;
#pragma unroll
    for (int q = 0; q < 7; ++q) loss += smooth_l1(pr[q], tg[q], p.code_w[q], &g[q]);
    return loss;
}

// the corner term of one fg row: mean over the 8 corners of smooth-L1(min(|p - g|, |p - g_flip|), beta 1); g[q] = d / d pred[q]
__device__ __forceinline__ float rl_corner(const float *pr, const float *roi, const float *gs, float *g) {
    // decode_torch against the roi with its centre zeroed (heading kept, sizes not clamped)
    const float diag = sqrtf(roi[3] * roi[3] + roi[4] * roi[4]);
    const float xl = pr[0] * diag, yl = pr[1] * diag, zl = pr[2] * roi[5];
    const float ex = expf(pr[3]) * roi[3], ey = expf(pr[4]) * roi[4], ez = expf(pr[5]) * roi[5];
    const float rg = pr[6] + roi[6];
    // rotate_points_along_z by the roi heading; the roi centre goes to the gt side
    const float cr = cosf(roi[6]), sr = sinf(roi[6]);
    const float cx = xl * cr - yl * sr, cy = xl * sr + yl * cr, cz = zl;
    const float gx = gs[0] - roi[0], gy = gs[1] - roi[1], gz = gs[2] - roi[2];
    const float cp = cosf(rg), sp = sinf(rg), cg = cosf(gs[6]), sg = sinf(gs[6]);
    const float ux = cx - gx, uy = cy - gy, uz = cz - gz;      // centre difference
    float loss = 0.0f;
    float dcx = 0.f, dcy = 0.f, dcz = 0.f, dex = 0.f, dey = 0.f, dez = 0.f, drg = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        // boxes_to_corners_3d's template: x + + - - , y + - - + ; corner j lies below (z -) and corner j + 4 above (z +) the same
        // footprint point, so the pair shares its x / y differences
        const float sx = j < 2 ? 0.5f : -0.5f, sy = (j == 0 || j == 3) ? 0.5f : -0.5f;
        const float ox = sx * ex, oy = sy * ey;
        const float px = ox * cp - oy * sp, py = ox * sp + oy * cp;
        const float hx = sx * gs[3], hy = sy * gs[4];
        const float qx = hx * cg - hy * sg, qy = hx * sg + hy * cg;
        const float ax = ux + (px - qx), ay = uy + (py - qy);      // against the gt
        const float bx = ux + (px + qx), by = uy + (py + qy);      // against the gt turned by pi
        const float a2 = ax * ax + ay * ay, b2 = bx * bx + by * by;
        float wzs[2];
#pragma unroll
        for (int zi = 0; zi < 2; ++zi) {
            const float sz = zi ? 0.5f : -0.5f;
            const float dz = uz + (sz * ez - sz * gs[5]);
            const float da = sqrtf(a2 + dz * dz), db = sqrtf(b2 + dz * dz);
            const bool flip = db < da;                             // a tie takes the unflipped branch
            const float d = flip ? db : da, vx = flip ? bx : ax, vy = flip ? by : ay;
            const bool quad = d < 1.0f;
            loss += quad ? 0.5f * (d * d) : d - 0.5f;
            // d smooth-L1(|v|) / d v: v below the knee (0 at v == 0 without a division), v / |v| above it
            const float s = quad ? 1.0f : 1.0f / d;
            const float wx = vx * s, wy = vy * s;
            wzs[zi] = dz * s;
            dcx += wx; dcy += wy; dcz += wzs[zi];
            dex += sx * (wx * cp + wy * sp);
            dey += sy * (wy * cp - wx * sp);
            drg += wy * px - wx * py;
        }
        dez += 0.5f * (wzs[1] - wzs[0]);      // the pair's height terms cancel exactly when the two boxes are equally tall
    }
    const float m = 0.125f;
    g[0] = m * ((dcx * cr + dcy * sr) * diag);
    g[1] = m * ((dcy * cr - dcx * sr) * diag);
    g[2] = m * (dcz * roi[5]);
    g[3] = m * (dex * ex);
    g[4] = m * (dey * ey);
    g[5] = m * (dez * ez);
    g[6] = m * drg;
    return m * loss;
}

__global__ __launch_bounds__(RL_THREADS) void roi_loss_fwd_kernel(RLParams p, const float *__restrict__ rcnn_cls,
                                                                  const float *__restrict__ rcnn_reg,
                                                                  const float *__restrict__ rois, const float *__restrict__ gt,
                                                                  const float *__restrict__ gt_src,
                                                                  const long long *__restrict__ reg_valid,
                                                                  const float *__restrict__ labels, RLWs w,
                                                                  float *__restrict__ out) {
    __shared__ BlockSumLds<RL_THREADS / 64, 3, 2> s_red;
    const int t = threadIdx.x;
    float cls = 0.0f, reg = 0.0f, cor = 0.0f;
    int nfg = 0, nvalid = 0;
    for (int i = t; i < p.n; i += RL_THREADS) {
        const float tl = labels[i];
        float gc = 0.0f;
        if (tl >= 0.0f) {
            cls += bce_logits(rcnn_cls[i], tl, &gc);
            ++nvalid;
        }
        w.g_cls[i] = gc;
        float gr[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, gk[7] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        if (reg_valid[i] > 0) {
            float pr[7], ro[7], g7[7], s7[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) {
                pr[q] = rcnn_reg[(size_t)i * 7 + q];
                ro[q] = rois[(size_t)i * 7 + q];
                g7[q] = gt[(size_t)i * 8 + q];
                s7[q] = gt_src[(size_t)i * 8 + q];
            }
            reg += rl_reg(p, pr, ro, g7, gr);
            if (p.corner) cor += rl_corner(pr, ro, s7, gk);
            ++nfg;
        }
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            w.g_reg[(size_t)i * 7 + q] = gr[q];
            w.g_corner[(size_t)i * 7 + q] = gk[q];
        }
    }
    float sum[3] = {cls, reg, cor};
    int cnt[2] = {nfg, nvalid};
    block_sum(sum, cnt, s_red);      // fixed order: lanes by shuffle, then the 16 waves in order
    if (t == 0) {
        const int f = cnt[0], v = cnt[1];
        out[0] = sum[0] / fmaxf((float)v, 1.0f) * p.w_cls;
        out[1] = sum[1] / fmaxf((float)f, 1.0f) * p.w_reg;
        out[2] = sum[2] / fmaxf((float)f, 1.0f) * p.w_corner;      // 0 without fg rows or with the option off
        out[3] = (float)f;
        out[4] = (float)v;
        w.counts[0] = f;
        w.counts[1] = v;
    }
}

__global__ __launch_bounds__(RL_BWD_THREADS) void roi_loss_bwd_kernel(RLParams p, RLWs w, const float *__restrict__ grad,
                                                                      float *__restrict__ d_cls, float *__restrict__ d_reg) {
    const int i = blockIdx.x * RL_BWD_THREADS + threadIdx.x;
    if (i >= p.n) return;
    const float nf = fmaxf((float)w.counts[0], 1.0f), nv = fmaxf((float)w.counts[1], 1.0f);
    if (d_cls) d_cls[i] = (grad[0] * p.w_cls / nv) * w.g_cls[i];
    if (d_reg) {
        const float sr = grad[1] * p.w_reg / nf, sc = p.corner ? grad[2] * p.w_corner / nf : 0.0f;
#pragma unroll
        for (int q = 0; q < 7; ++q) {
            const float a = sr * w.g_reg[(size_t)i * 7 + q];
            d_reg[(size_t)i * 7 + q] = p.corner ? a + sc * w.g_corner[(size_t)i * 7 + q] : a;
        }
    }
}

// ---------------------------------------------------------------- host side
LIDAR_EXPORT int lidar_roi_loss_supported(int batch, int roi_per_image, int roi_dim, int gt_dim, int reg_dim, int cls_dim) {
    return batch >= 0 && roi_per_image >= 1 && roi_per_image <= RL_MAX_P && (long long)batch * roi_per_image <= RL_MAX_ROWS &&
           roi_dim == 7 && gt_dim == 8 && reg_dim == 7 && cls_dim == 1;
}

LIDAR_EXPORT size_t lidar_roi_loss_workspace_bytes(int batch, int roi_per_image) {
    if (!lidar_roi_loss_supported(batch, roi_per_image, 7, 8, 7, 1)) return 0;
    return rl_ws_layout((long long)batch * roi_per_image, nullptr, nullptr);
}

static int rl_params(RLParams &p, int batch, int roi_per_image, const float *weights, const float *code_weights, int flags) {
    if (!lidar_roi_loss_supported(batch, roi_per_image, 7, 8, 7, 1) || !weights || !code_weights || (flags & ~1)) return LIDAR_ERR_ARG;
    p = RLParams{};
    for (int q = 0; q < 7; ++q) p.code_w[q] = code_weights[q];
    p.w_cls = weights[0]; p.w_reg = weights[1]; p.w_corner = (flags & 1) ? weights[2] : 0.0f;
    p.n = batch * roi_per_image;
    p.corner = flags & 1;
    return LIDAR_OK;
}

LIDAR_EXPORT int lidar_roi_loss_forward(const float *rcnn_cls, const float *rcnn_reg, const float *rois, const float *gt_of_rois,
                                        const float *gt_of_rois_src, const long long *reg_valid_mask, const float *rcnn_cls_labels,
                                        int batch, int roi_per_image, const float *weights, const float *code_weights, int flags,
                                        float *out, void *ws, size_t ws_bytes, void *stream) {
    RLParams p;
    const int st = rl_params(p, batch, roi_per_image, weights, code_weights, flags);
    if (st != LIDAR_OK) return st;
    if (!out) return LIDAR_ERR_ARG;
    if (batch == 0) {      // nothing to launch: zero losses, zero counts
        if (hipMemsetAsync(out, 0, 5 * sizeof(float), (hipStream_t)stream) != hipSuccess) return LIDAR_ERR_LAUNCH;
        return LIDAR_OK;
    }
    if (!rcnn_cls || !rcnn_reg || !rois || !gt_of_rois || !gt_of_rois_src || !reg_valid_mask || !rcnn_cls_labels || !ws)
        return LIDAR_ERR_ARG;
    RLWs w;
    if (ws_bytes < rl_ws_layout(p.n, &w, (char *)ws)) return LIDAR_ERR_WORKSPACE;
    hipLaunchKernelGGL(roi_loss_fwd_kernel, dim3(1), dim3(RL_THREADS), 0, (hipStream_t)stream, p, rcnn_cls, rcnn_reg, rois,
                       gt_of_rois, gt_of_rois_src, reg_valid_mask, rcnn_cls_labels, w, out);
    return lidar_check_launch("lidar_roi_loss_forward");
}

LIDAR_EXPORT int lidar_roi_loss_backward(int batch, int roi_per_image, const float *weights, const float *code_weights, int flags,
                                         const float *grad_out, float *d_rcnn_cls, float *d_rcnn_reg, void *ws, size_t ws_bytes,
                                         void *stream) {
    RLParams p;
    const int st = rl_params(p, batch, roi_per_image, weights, code_weights, flags);
    if (st != LIDAR_OK) return st;
    if (batch == 0 || (!d_rcnn_cls && !d_rcnn_reg)) return LIDAR_OK;
    if (!grad_out || !ws) return LIDAR_ERR_ARG;
    RLWs w;
    if (ws_bytes < rl_ws_layout(p.n, &w, (char *)ws)) return LIDAR_ERR_WORKSPACE;
    hipLaunchKernelGGL(roi_loss_bwd_kernel, dim3((unsigned)divup(p.n, RL_BWD_THREADS)), dim3(RL_BWD_THREADS), 0,
                       (hipStream_t)stream, p, w, grad_out, d_rcnn_cls, d_rcnn_reg);
    return lidar_check_launch("lidar_roi_loss_backward");
}
