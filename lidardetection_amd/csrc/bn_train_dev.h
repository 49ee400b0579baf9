// The parts of the train-mode BatchNorm + ReLU kernels that every file of that family shares (csrc/bn_train.hip: dense maps and
// sparse feature rows; csrc/sa_train.hip: BatchNorm + ReLU + max over a ball's samples): the segment tables, the thread layout, the
// fp64 per-channel sums with their fixed-order reduction, and the two finalize kernels.  One copy, so the statistics of every
// train-mode BatchNorm here are the same arithmetic.  The kernels are static: each including file owns its copy.
// Also here, one copy each: the element math (y of a quad with and without a residual, the backward's delta built on
// that very y, a quad's fp64 backward coefficients and dz), and the host helpers every launcher of the family calls (the one-segment
// table, the workspace split, "stats -> reduce -> finalize" and "reduce -> backward finalize").  The fixed-order reduce kernel itself
// is ordered_reduce.h's, shared with csrc/pfn_train.hip.
#pragma once
#include "ordered_reduce.h"

#define BT_MAX_SEG 4
#define BT_MAX_C 1024              // channels of one segment: a 256-thread block covers a row's C / 4 quads at once
#define BT_MAX_BLOCKS 1024

struct BtSeg {
    const float *x;                // z (forward and backward input)
    float *dx;                     // dz (backward output; same row stride and channel offset as x)
    int C, ld, off, c0;
    const float *r;                // RES only: the residual added before the ReLU, (rows, C) at row stride r_ld
    float *dr;                     // RES only: its gradient (backward output), (rows, C) at row stride dr_ld
    int r_ld, dr_ld;
};
struct BtSegs {
    BtSeg s[BT_MAX_SEG];
    int n, ctot;
};

// thread layout of every pass: Q = C / 4 channel quads per row, R = 256 / Q rows side by side; thread (r, q), rows r, r + R nb, ...
struct BtLane {
    int Q, R, r, q;
    bool live;
};
__device__ __forceinline__ BtLane bt_lane(int C) {
    BtLane L;
    L.Q = C >> 2;
    L.R = 256 / L.Q;
    L.r = (int)threadIdx.x / L.Q;
    L.q = (int)threadIdx.x - L.r * L.Q;
    L.live = L.r < L.R;
    return L;
}

__device__ __forceinline__ float4 bt_ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void bt_st4(float *p, float4 v) { *reinterpret_cast<float4 *>(p) = v; }

// ---- element math.  The backward's ReLU mask is recomputed from z through the helper the forward writes y with: the same bits by
// construction.  The explicit fmaf is the only fused operation (the build uses -ffp-contract=off).
__device__ __forceinline__ float bt_y(float z, float sc, float sh) { return fmaxf(fmaf(z, sc, sh), 0.f); }
__device__ __forceinline__ float bt_y(float z, float sc, float sh, float r) { return fmaxf(fmaf(z, sc, sh) + r, 0.f); }
// y of one quad; r is read only when RES
template <bool RES = false>
__device__ __forceinline__ float4 bt_y4(const float4 &z, const float4 &sc, const float4 &sh, const float4 &r = float4()) {
    if constexpr (RES)
        return make_float4(bt_y(z.x, sc.x, sh.x, r.x), bt_y(z.y, sc.y, sh.y, r.y), bt_y(z.z, sc.z, sh.z, r.z), bt_y(z.w, sc.w, sh.w, r.w));
    else
        return make_float4(bt_y(z.x, sc.x, sh.x), bt_y(z.y, sc.y, sh.y), bt_y(z.z, sc.z, sh.z), bt_y(z.w, sc.w, sh.w));
}
// delta = g where the forward's y is positive
__device__ __forceinline__ float bt_delta(float y, float g) { return y > 0.f ? g : 0.f; }
template <bool RES = false>
__device__ __forceinline__ float4 bt_delta4(const float4 &z, const float4 &g, const float4 &sc, const float4 &sh,
                                            const float4 &r = float4()) {
    const float4 y = bt_y4<RES>(z, sc, sh, r);
    return make_float4(bt_delta(y.x, g.x), bt_delta(y.y, g.y), bt_delta(y.z, g.z), bt_delta(y.w, g.w));
}

// the fp64 backward coefficients of the quad at channel c (bt_bwd_finalize_kernel's coef) and dz = A (delta - m1 - (z - mu) m2)
struct BtCoef4 {
    double A[4], m1[4], m2[4], mu[4];
};
__device__ __forceinline__ BtCoef4 bt_coef4(const double *__restrict__ coef, int ctot, int c) {
    BtCoef4 k;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        k.A[i] = coef[c + i]; k.m1[i] = coef[ctot + c + i]; k.m2[i] = coef[2 * ctot + c + i]; k.mu[i] = coef[3 * ctot + c + i];
    }
    return k;
}
__device__ __forceinline__ float4 bt_dz4(const BtCoef4 &k, const float4 &d, const float4 &z) {
    return make_float4((float)(k.A[0] * ((double)d.x - k.m1[0] - ((double)z.x - k.mu[0]) * k.m2[0])),
                       (float)(k.A[1] * ((double)d.y - k.m1[1] - ((double)z.y - k.mu[1]) * k.m2[1])),
                       (float)(k.A[2] * ((double)d.z - k.m1[2] - ((double)z.z - k.mu[2]) * k.m2[2])),
                       (float)(k.A[3] * ((double)d.w - k.m1[3] - ((double)z.w - k.mu[3]) * k.m2[3])));
}

// the per-block sums of thread (r, q) -> part[(which * ctot + channel) * nb + block], summed over r in a fixed order
__device__ __forceinline__ void bt_block_partials(const double (&a)[8], const BtLane &L, int C, int c0, int ctot, int nb,
                                                  double *__restrict__ part) {
    __shared__ double sh[8][256];
#pragma unroll
    for (int k = 0; k < 8; ++k) sh[k][threadIdx.x] = a[k];
    __syncthreads();
    for (int e = threadIdx.x; e < 2 * C; e += 256) {
        const int which = e >= C, c = e - which * C, q = c >> 2, k = which * 4 + (c & 3);
        double t = 0.0;
        for (int r = 0; r < L.R; ++r) t += sh[k][r * L.Q + q];
        part[((size_t)which * ctot + c0 + c) * nb + blockIdx.x] = t;
    }
}

// forward pass 1: sum z, sum z^2 (fp64) per channel and block.  grid (nb, segments)
static __global__ __launch_bounds__(256) void bt_stats_kernel(BtSegs segs, long long rows, int nb, double *__restrict__ part) {
    const BtSeg sg = segs.s[blockIdx.y];
    const BtLane L = bt_lane(sg.C);
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (L.live) {
        const float *base = sg.x + sg.off + 4 * L.q;
        const long long step = (long long)nb * L.R;
        long long row = (long long)blockIdx.x * L.R + L.r;
        for (; row + 3 * step < rows; row += 4 * step) {     // four rows in flight
            float4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) v[u] = bt_ld4(base + (row + u * step) * sg.ld);
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[0] += v[u].x; a[1] += v[u].y; a[2] += v[u].z; a[3] += v[u].w;
                a[4] += (double)v[u].x * v[u].x; a[5] += (double)v[u].y * v[u].y;
                a[6] += (double)v[u].z * v[u].z; a[7] += (double)v[u].w * v[u].w;
            }
        }
        for (; row < rows; row += step) {
            const float4 v = bt_ld4(base + row * sg.ld);
            a[0] += v.x; a[1] += v.y; a[2] += v.z; a[3] += v.w;
            a[4] += (double)v.x * v.x; a[5] += (double)v.y * v.y; a[6] += (double)v.z * v.z; a[7] += (double)v.w * v.w;
        }
    }
    bt_block_partials(a, L, sg.C, sg.c0, segs.ctot, nb, part);
}

// forward pass 2 (thread = channel): mean, biased variance, 1 / sigma in fp64; fp32 scale / shift; the running-statistics inputs
static __global__ __launch_bounds__(256) void bt_finalize_kernel(const double *__restrict__ tot, int ctot, long long rows,
                                                                 const float *__restrict__ gamma, const float *__restrict__ beta,
                                                                 float eps, double *__restrict__ stats,
                                                                 float *__restrict__ scale_shift, float *__restrict__ batch_stats) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ctot) return;
    const double N = (double)rows;
    const double mu = tot[c] / N;
    const double var = fmax(tot[ctot + c] / N - mu * mu, 0.0);
    const double inv = 1.0 / sqrt(var + (double)eps);
    const double a = (double)gamma[c] * inv;
    stats[c] = mu;
    stats[ctot + c] = inv;
    scale_shift[c] = (float)a;
    scale_shift[ctot + c] = (float)((double)beta[c] - mu * a);
    batch_stats[c] = (float)mu;
    batch_stats[ctot + c] = (float)var;
    batch_stats[2 * ctot + c] = (float)(var * N / (N - 1.0));
}

// backward pass 2 (thread = channel): dgamma, dbeta, and the fp64 coefficients of dz = A (delta - m1 - (z - mu) m2)
static __global__ __launch_bounds__(256) void bt_bwd_finalize_kernel(const double *__restrict__ tot, int ctot, long long rows,
                                                                     const float *__restrict__ gamma, const double *__restrict__ stats,
                                                                     double *__restrict__ coef, float *__restrict__ d_gamma,
                                                                     float *__restrict__ d_beta) {
    const int c = blockIdx.x * 256 + threadIdx.x;
    if (c >= ctot) return;
    const double N = (double)rows;
    const double mu = stats[c], inv = stats[ctot + c];
    const double db = tot[c], dg = (tot[ctot + c] - mu * db) * inv;
    coef[c] = (double)gamma[c] * inv;
    coef[ctot + c] = db / N;
    coef[2 * ctot + c] = dg / N * inv;
    coef[3 * ctot + c] = mu;
    d_gamma[c] = (float)dg;
    d_beta[c] = (float)db;
}

static int bt_blocks(long long rows) {
    const long long b = (rows + 255) / 256;
    return (int)(b < 1 ? 1 : (b > BT_MAX_BLOCKS ? BT_MAX_BLOCKS : b));
}

// [partials: 2 ctot nb doubles][totals: 2 ctot doubles][backward coefficients: 4 ctot doubles]
static size_t bt_workspace_bytes(long long rows, int channels) {
    if (rows < 1 || channels < 1) return 0;
    const size_t c = (size_t)channels;
    return align_up((2 * c * bt_blocks(rows) + 2 * c + 4 * c) * sizeof(double), 256);
}

static bool bt_aligned(const void *p) { return p && ((uintptr_t)p & 15) == 0; }

// the table of one (rows, C) matrix at row stride ld (dx: its gradient, or null), unchecked
static void bt_one_seg(const float *x, float *dx, int C, int ld, BtSegs &S) {
    S.n = 1;
    S.ctot = C;
    S.s[0] = BtSeg{x, dx, C, ld, 0, 0, nullptr, nullptr, 0, 0};
}

// the workspace of bt_workspace_bytes(rows, ctot), nb = bt_blocks(rows)
struct BtWs {
    double *part, *tot, *coef;
};
static BtWs bt_ws_split(void *ws, int ctot, int nb) {
    double *part = (double *)ws, *tot = part + (size_t)2 * ctot * nb;
    return BtWs{part, tot, tot + 2 * ctot};
}

// forward passes 1 and 2: stats -> reduce -> finalize over the segments' rows; -> nb, the blocks per segment of the row passes
static int bt_launch_stats(const BtSegs &S, long long rows, const float *gamma, const float *beta, float eps, double *stats,
                           float *scale_shift, float *batch_stats, void *ws, hipStream_t s) {
    const int nb = bt_blocks(rows);
    const BtWs W = bt_ws_split(ws, S.ctot, nb);
    hipLaunchKernelGGL(bt_stats_kernel, dim3(nb, S.n), dim3(256), 0, s, S, rows, nb, W.part);
    hipLaunchKernelGGL(ordered_reduce_kernel, dim3(2 * S.ctot), dim3(256), 0, s, W.part, nb, W.tot);
    hipLaunchKernelGGL(bt_finalize_kernel, dim3(divup(S.ctot, 256)), dim3(256), 0, s, W.tot, S.ctot, rows, gamma, beta, eps, stats,
                       scale_shift, batch_stats);
    return nb;
}

// backward pass 2: W.part's nb partials per entry -> reduce -> backward finalize (W.coef, d_gamma, d_beta)
static void bt_launch_bwd_finalize(const BtWs &W, int ctot, int nb, long long rows, const float *gamma, const double *stats,
                                   float *d_gamma, float *d_beta, hipStream_t s) {
    hipLaunchKernelGGL(ordered_reduce_kernel, dim3(2 * ctot), dim3(256), 0, s, W.part, nb, W.tot);
    hipLaunchKernelGGL(bt_bwd_finalize_kernel, dim3(divup(ctot, 256)), dim3(256), 0, s, W.tot, ctot, rows, gamma, stats, W.coef, d_gamma,
                       d_beta);
}
