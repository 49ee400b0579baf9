// The parts of the train-mode BatchNorm + ReLU kernels that every file of that family shares (csrc/bn_train.hip: dense maps and
// sparse feature rows; csrc/sa_train.hip: BatchNorm + ReLU + max over a ball's samples): the segment tables, the thread layout, the
// fp64 per-channel sums with their fixed-order reduction, and the two finalize kernels.  One copy, so the statistics of every
// train-mode BatchNorm here are the same arithmetic.  The kernels are static: each including file owns its copy.
#pragma once
#include "common.h"

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

// rows of `part` ([entries][nparts]) -> tot[entry]; one block per entry, fixed summation order
static __global__ __launch_bounds__(256) void bt_reduce_kernel(const double *__restrict__ part, int nparts, double *__restrict__ tot) {
    __shared__ double s[256];
    const double *row = part + (size_t)blockIdx.x * nparts;
    double a = 0.0;
    for (int b = threadIdx.x; b < nparts; b += 256) a += row[b];
    s[threadIdx.x] = a;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s[threadIdx.x] += s[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) tot[blockIdx.x] = s[0];
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
