// Train-mode BatchNorm2d + ReLU on channels-last fp32 maps, forward and backward.
//   reference: pcdet/models/backbones_2d/base_bev_backbone.py:31-69 (Conv2d / ConvTranspose2d -> BatchNorm2d(eps, momentum) -> ReLU),
//              :103 (torch.cat of the deblock outputs)
//
// A map is (rows = B * H * W) x (C channels) with a row stride `ld` and a channel offset `off` (a slice of a wider map).  One call
// normalises up to BT_MAX_SEG such inputs ("segments") as ONE concatenated channel space: segment s owns channels [c0_s, c0_s + C_s)
// of the output (and of gamma, beta, the statistics), so the deblock outputs land in their slices of the concatenated map and their
// gradients are read back from the concatenated gradient without a torch.cat or a split.
//   forward:  per-channel sum z and sum z^2 in fp64 (one partial per block), a fixed-order reduction, a finalize that writes the
//             batch mean, the biased variance, 1 / sigma, fp32 scale = gamma / sigma and shift = beta - mu gamma / sigma, and the
//             running-statistics inputs (mean, unbiased variance); then y = max(z scale + shift, 0).
//   backward: delta = g [y > 0] with y recomputed from z bit for bit (no mask is stored); sum delta and sum delta z in fp64, reduced
//             the same way; dbeta = sum delta, dgamma = sum delta zh = (sum delta z - mu sum delta) / sigma,
//             dz = gamma / sigma (delta - dbeta / N - zh dgamma / N), evaluated per element in fp64 (fp64 coefficients and mu in
//             the workspace) and rounded once: the three terms cancel, to ~eps / var of their size at N = 2, where fp32
//             coefficients left dz at 4.5e-5 of its scale against float64 (now 6.8e-8).  The pass moves 12 bytes
//             per element for five fp64 operations; its time with fp64 has not been measured in isolation.
// No float atomics and no host read: every result is bitwise reproducible and every call can be captured in a graph.
//
// The residual form (SparseBasicBlock's bn2 -> += identity -> relu, spconv_backbone.py:57-62 of the reference) is the
// same kernels with RES = true: y = max(z scale + shift + r, 0) for a residual r (rows, C) at its own row stride, the backward's
// mask recomputed from that sum, and d_r = delta written beside dz.  The statistics, the reductions and the coefficients are the one
// copy above; RES = false compiles to the code the plain entry points always ran.
//
// The segment tables, the thread layout, the statistics kernels (forward passes 1 and 2, backward pass 2) and the reduction are in
// bn_train_dev.h, shared with csrc/sa_train.hip; so are the element math (y, delta, the fp64 dz) and the launch helpers; the
// reduction kernel is ordered_reduce.h's.  The four exported launchers are wrappers over bt_forward<RES> / bt_backward<RES>.
#include "bn_train_dev.h"

// forward pass 3: y = max(z scale + shift, 0) into channels [y_off + c0, + C) of the (rows, y_ld) output.  grid (nb, segments)
template <bool RES>
__global__ __launch_bounds__(256) void bt_apply_kernel(BtSegs segs, long long rows, int nb, const float *__restrict__ scale_shift,
                                                       float *__restrict__ y, int y_ld, int y_off) {
    const BtSeg sg = segs.s[blockIdx.y];
    const BtLane L = bt_lane(sg.C);
    if (!L.live) return;
    const int c = sg.c0 + 4 * L.q;
    const float4 sc = bt_ld4(scale_shift + c), sh = bt_ld4(scale_shift + segs.ctot + c);
    const float *src = sg.x + sg.off + 4 * L.q;
    float *dst = y + y_off + c;
    const long long step = (long long)nb * L.R;
    for (long long row = (long long)blockIdx.x * L.R + L.r; row < rows; row += step) {
        const float4 v = bt_ld4(src + row * sg.ld);
        float4 r;
        if constexpr (RES) r = bt_ld4(sg.r + 4 * L.q + row * sg.r_ld);
        bt_st4(dst + row * (long long)y_ld, bt_y4<RES>(v, sc, sh, r));
    }
}

// backward pass 1: sum delta, sum delta z (fp64) per channel and block.  grid (nb, segments)
template <bool RES>
__global__ __launch_bounds__(256) void bt_bwd_stats_kernel(BtSegs segs, long long rows, int nb, const float *__restrict__ scale_shift,
                                                           const float *__restrict__ g, int g_ld, int g_off, double *__restrict__ part) {
    const BtSeg sg = segs.s[blockIdx.y];
    const BtLane L = bt_lane(sg.C);
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (L.live) {
        const int c = sg.c0 + 4 * L.q;
        const float4 sc = bt_ld4(scale_shift + c), sh = bt_ld4(scale_shift + segs.ctot + c);
        const float *zs = sg.x + sg.off + 4 * L.q, *gs = g + g_off + c;
        const long long step = (long long)nb * L.R;
        long long row = (long long)blockIdx.x * L.R + L.r;
        for (; row + step < rows; row += 2 * step) {          // two rows in flight
            float4 z[2], gv[2], rv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                z[u] = bt_ld4(zs + (row + u * step) * sg.ld);
                gv[u] = bt_ld4(gs + (row + u * step) * (long long)g_ld);
                if constexpr (RES) rv[u] = bt_ld4(sg.r + 4 * L.q + (row + u * step) * sg.r_ld);
            }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                const float4 d = bt_delta4<RES>(z[u], gv[u], sc, sh, rv[u]);
                a[0] += d.x; a[1] += d.y; a[2] += d.z; a[3] += d.w;
                a[4] += (double)d.x * z[u].x; a[5] += (double)d.y * z[u].y; a[6] += (double)d.z * z[u].z; a[7] += (double)d.w * z[u].w;
            }
        }
        for (; row < rows; row += step) {
            const float4 z = bt_ld4(zs + row * sg.ld), gv = bt_ld4(gs + row * (long long)g_ld);
            float4 rv;
            if constexpr (RES) rv = bt_ld4(sg.r + 4 * L.q + row * sg.r_ld);
            const float4 d = bt_delta4<RES>(z, gv, sc, sh, rv);
            a[0] += d.x; a[1] += d.y; a[2] += d.z; a[3] += d.w;
            a[4] += (double)d.x * z.x; a[5] += (double)d.y * z.y; a[6] += (double)d.z * z.z; a[7] += (double)d.w * z.w;
        }
    }
    bt_block_partials(a, L, sg.C, sg.c0, segs.ctot, nb, part);
}

// backward pass 3: dz into the segment's dx (the row stride and channel offset of its z).  grid (nb, segments)
template <bool RES>
__global__ __launch_bounds__(256) void bt_bwd_apply_kernel(BtSegs segs, long long rows, int nb, const float *__restrict__ scale_shift,
                                                           const double *__restrict__ coef, const float *__restrict__ g, int g_ld,
                                                           int g_off) {
    const BtSeg sg = segs.s[blockIdx.y];
    const BtLane L = bt_lane(sg.C);
    if (!L.live) return;
    const int ct = segs.ctot, c = sg.c0 + 4 * L.q;
    const float4 sc = bt_ld4(scale_shift + c), sh = bt_ld4(scale_shift + ct + c);
    const BtCoef4 k = bt_coef4(coef, ct, c);
    const float *zs = sg.x + sg.off + 4 * L.q, *gs = g + g_off + c;
    float *ds = sg.dx + sg.off + 4 * L.q;
    const long long step = (long long)nb * L.R;
    for (long long row = (long long)blockIdx.x * L.R + L.r; row < rows; row += step) {
        const float4 z = bt_ld4(zs + row * sg.ld), gv = bt_ld4(gs + row * (long long)g_ld);
        float4 rv;
        if constexpr (RES) rv = bt_ld4(sg.r + 4 * L.q + row * sg.r_ld);
        const float4 d = bt_delta4<RES>(z, gv, sc, sh, rv);
        bt_st4(ds + row * sg.ld, bt_dz4(k, d, z));
        if constexpr (RES) bt_st4(sg.dr + 4 * L.q + row * sg.dr_ld, d);
    }
}

LIDAR_EXPORT size_t lidar_bn_relu_train_workspace_bytes(long long rows, int channels) { return bt_workspace_bytes(rows, channels); }

static bool bt_seg_ok(const void *x, int C, int ld, int off) {
    return bt_aligned(x) && C >= 4 && C <= BT_MAX_C && C % 4 == 0 && ld % 4 == 0 && off % 4 == 0 && off >= 0 && off + C <= ld;
}

// host segment tables -> BtSegs; LIDAR_ERR_ARG on anything the kernels do not take
static int bt_segs(int nseg, void *const *x, void *const *dx, const int *x_ld, const int *x_off, const int *seg_C, BtSegs &S) {
    if (nseg < 1 || nseg > BT_MAX_SEG || !x || !x_ld || !x_off || !seg_C) return LIDAR_ERR_ARG;
    S.n = nseg;
    S.ctot = 0;
    for (int i = 0; i < nseg; ++i) {
        if (!bt_seg_ok(x[i], seg_C[i], x_ld[i], x_off[i]) || (dx && !bt_aligned(dx[i]))) return LIDAR_ERR_ARG;
        S.s[i] = BtSeg{(const float *)x[i], dx ? (float *)dx[i] : nullptr, seg_C[i], x_ld[i], x_off[i], S.ctot, nullptr, nullptr, 0, 0};
        S.ctot += seg_C[i];
    }
    return LIDAR_OK;
}

// the residual form's table: one (rows, C) map; z / dz at x_ld, r at r_ld, d_r at dr_ld (dx, dr: the backward's outputs, or null)
static int bt_res_seg(const float *x, float *dx, int x_ld, const float *r, float *dr, int r_ld, int dr_ld, int C, BtSegs &S) {
    if (!bt_seg_ok(x, C, x_ld, 0) || !bt_aligned(r) || r_ld % 4 || r_ld < C) return LIDAR_ERR_ARG;
    if (dx && (!bt_aligned(dx) || !bt_aligned(dr) || dr_ld % 4 || dr_ld < C)) return LIDAR_ERR_ARG;
    bt_one_seg(x, dx, C, x_ld, S);
    S.s[0].r = r; S.s[0].dr = dr; S.s[0].r_ld = r_ld; S.s[0].dr_ld = dr_ld;
    return LIDAR_OK;
}

static bool bt_map_ok(const void *p, int ld, int off, int ctot) {
    return bt_aligned(p) && ld % 4 == 0 && off % 4 == 0 && off >= 0 && off + ctot <= ld;
}

// the forward of both forms on a checked table: stats -> reduce -> finalize -> apply
template <bool RES>
static int bt_forward(const char *who, const BtSegs &S, long long rows, const float *gamma, const float *beta, float eps, float *y,
                      int y_ld, int y_off, double *stats, float *scale_shift, float *batch_stats, void *ws, size_t ws_bytes,
                      void *stream) {
    if (rows < 2 || !gamma || !beta || !stats || !bt_aligned(scale_shift) || !batch_stats || !bt_aligned(ws) || !(eps >= 0.f))
        return LIDAR_ERR_ARG;
    if (!bt_map_ok(y, y_ld, y_off, S.ctot)) return LIDAR_ERR_ARG;
    if (ws_bytes < bt_workspace_bytes(rows, S.ctot)) return LIDAR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int nb = bt_launch_stats(S, rows, gamma, beta, eps, stats, scale_shift, batch_stats, ws, s);
    hipLaunchKernelGGL(bt_apply_kernel<RES>, dim3(nb, S.n), dim3(256), 0, s, S, rows, nb, scale_shift, y, y_ld, y_off);
    return lidar_check_launch(who);
}

// the backward of both forms on a checked table (dx, and dr when RES, set): stats -> reduce -> backward finalize -> apply
template <bool RES>
static int bt_backward(const char *who, const BtSegs &S, long long rows, const float *grad_y, int g_ld, int g_off, const float *gamma,
                       const double *stats, const float *scale_shift, float *d_gamma, float *d_beta, void *ws, size_t ws_bytes,
                       void *stream) {
    if (rows < 2 || !gamma || !stats || !bt_aligned(scale_shift) || !d_gamma || !d_beta || !bt_aligned(ws)) return LIDAR_ERR_ARG;
    if (!bt_map_ok(grad_y, g_ld, g_off, S.ctot)) return LIDAR_ERR_ARG;
    if (ws_bytes < bt_workspace_bytes(rows, S.ctot)) return LIDAR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int nb = bt_blocks(rows);
    const BtWs W = bt_ws_split(ws, S.ctot, nb);
    hipLaunchKernelGGL(bt_bwd_stats_kernel<RES>, dim3(nb, S.n), dim3(256), 0, s, S, rows, nb, scale_shift, grad_y, g_ld, g_off, W.part);
    bt_launch_bwd_finalize(W, S.ctot, nb, rows, gamma, stats, d_gamma, d_beta, s);
    hipLaunchKernelGGL(bt_bwd_apply_kernel<RES>, dim3(nb, S.n), dim3(256), 0, s, S, rows, nb, scale_shift, W.coef, grad_y, g_ld, g_off);
    return lidar_check_launch(who);
}

LIDAR_EXPORT int lidar_bn_relu_train_forward(int nseg, void *const *x, const int *x_ld, const int *x_off, const int *seg_C,
                                             long long rows, const float *gamma, const float *beta, float eps, float *y, int y_ld,
                                             int y_off, double *stats, float *scale_shift, float *batch_stats, void *ws,
                                             size_t ws_bytes, void *stream) {
    BtSegs S;
    if (bt_segs(nseg, x, nullptr, x_ld, x_off, seg_C, S) != LIDAR_OK) return LIDAR_ERR_ARG;
    return bt_forward<false>("lidar_bn_relu_train_forward", S, rows, gamma, beta, eps, y, y_ld, y_off, stats, scale_shift, batch_stats,
                             ws, ws_bytes, stream);
}

LIDAR_EXPORT int lidar_bn_relu_train_backward(int nseg, void *const *x, const int *x_ld, const int *x_off, const int *seg_C,
                                              long long rows, const float *grad_y, int g_ld, int g_off, const float *gamma,
                                              const double *stats, const float *scale_shift, void *const *dx, float *d_gamma,
                                              float *d_beta, void *ws, size_t ws_bytes, void *stream) {
    BtSegs S;
    if (!dx || bt_segs(nseg, x, dx, x_ld, x_off, seg_C, S) != LIDAR_OK) return LIDAR_ERR_ARG;
    return bt_backward<false>("lidar_bn_relu_train_backward", S, rows, grad_y, g_ld, g_off, gamma, stats, scale_shift, d_gamma, d_beta,
                              ws, ws_bytes, stream);
}

// ---- the residual form: y = max(BN(z) + r, 0) on one (rows, C) map; y at y_ld, grad_y at g_ld
LIDAR_EXPORT int lidar_bn_add_relu_train_forward(const float *x, int x_ld, const float *r, int r_ld, int channels, long long rows,
                                                 const float *gamma, const float *beta, float eps, float *y, int y_ld, double *stats,
                                                 float *scale_shift, float *batch_stats, void *ws, size_t ws_bytes, void *stream) {
    BtSegs S;
    if (bt_res_seg(x, nullptr, x_ld, r, nullptr, r_ld, 0, channels, S) != LIDAR_OK) return LIDAR_ERR_ARG;
    return bt_forward<true>("lidar_bn_add_relu_train_forward", S, rows, gamma, beta, eps, y, y_ld, 0, stats, scale_shift, batch_stats, ws,
                            ws_bytes, stream);
}

LIDAR_EXPORT int lidar_bn_add_relu_train_backward(const float *x, int x_ld, const float *r, int r_ld, int channels, long long rows,
                                                  const float *grad_y, int g_ld, const float *gamma, const double *stats,
                                                  const float *scale_shift, float *dx, float *d_r, int dr_ld, float *d_gamma,
                                                  float *d_beta, void *ws, size_t ws_bytes, void *stream) {
    BtSegs S;
    if (!dx || !d_r || bt_res_seg(x, dx, x_ld, r, d_r, r_ld, dr_ld, channels, S) != LIDAR_OK) return LIDAR_ERR_ARG;
    return bt_backward<true>("lidar_bn_add_relu_train_backward", S, rows, grad_y, g_ld, 0, gamma, stats, scale_shift, d_gamma, d_beta, ws,
                             ws_bytes, stream);
}

