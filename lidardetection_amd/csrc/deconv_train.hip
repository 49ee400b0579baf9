// The two gradients of ConvTranspose2d with kernel == stride == s and no bias (every deblock of BaseBEVBackbone:
// pcdet/models/backbones_2d/base_bev_backbone.py:51-57) on the fp32 matrix cores: the training counterpart of csrc/deconv_gemm.hip.
//
// With kernel == stride every input pixel p = (b, y, x) owns its own s x s patch of the output, so the layer is a plain GEMM on the NHWC
// map (deconv_gemm.hip) and so are both of its gradients.  W is the module's weight in torch's own layout (K, C_up, s, s); G is the
// gradient of the layer's output: (B, s h, s w) pixels of g_ld floats, channels [0, C_up).
//
//   input gradient    dx[p][k]          = sum_{ky,kx,c} G[b][s y + ky][s x + kx][c] * W[k][c][ky][kx]        M = P, N = K, reduction s^2 C_up
//   weight gradient   dw[k][c][ky][kx]  = sum_p         x[p][k] * G[b][s y + ky][s x + kx][c]                M = K, N = s^2 C_up, reduction P
//
// Input gradient (deconv_dgrad_kernel).  A workgroup (4 waves) owns 128 pixels x 128 output channels; wave v owns pixels [32 v, 32 v + 32)
// and four 32 x 32 accumulator tiles of v_mfma_f32_32x32x2_f32 (tiles at or beyond K are skipped).  The reduction runs in chunks of 32
// channels of one (ky, kx): the A rows of a chunk are 128-byte runs of G (one per pixel), the B rows are gathered from W at stride s^2.
// Both are prefetched into registers during the previous chunk's MFMAs, written to LDS as [row][32 reduction values] (pitch 36) and read
// back as one 16-byte load per lane and 4 MFMAs: lane (i, h) holds reduction values 4 (2 q + h) .. + 3 of row i, q = 0..3.  Pixels
// at or beyond P read zeros and store nothing; columns at or beyond K likewise.  No split of the reduction (at most 8192 long in the
// declared range, 2048 at the repo's shapes): one fixed summation order, bitwise reproducible.
//
// Weight gradient (deconv_wgrad_kernel + deconv_wgrad_finish_kernel).  A workgroup owns 64 input channels x four 32-column tiles of the
// (ky, kx, c)-ordered columns (a tile lies inside one (ky, kx) because C_up % 32 == 0) and one contiguous range of pixels, a "split";
// wave v owns column tile v and both 32-channel row tiles.  Per chunk of 32 pixels the x rows and the four G runs of each pixel are
// staged in LDS in their natural [pixel][channel] form, 16 K-steps of two pixels each.  The accumulation inside a split is fp32 (the
// MFMA's) over at most DW_MAX_SPLIT_PIX = 4096 pixels; each workgroup writes its partial to the caller's workspace with plain stores —
// every (split, k, column) exactly once, so nothing depends on what the workspace held.  The finishing kernel sums the splits in split
// order in fp64, rounds once to fp32 and writes torch's layout (the pattern of csrc/wino43_wgrad.hip).  No float atomics, no host read:
// bitwise reproducible and graph-capturable.  dw is overwritten, never read.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define DG_PIX 128                         // input gradient: pixels per workgroup
#define DG_COLS 128                        //                 output channels per workgroup
#define DG_PITCH 36                        // floats per staged row: 32 reduction values + 4 (16-byte aligned rows, shifted banks)

#define DW_PIX 32                          // weight gradient: pixels per chunk
#define DW_ROWS 64                         //                  input channels per workgroup
#define DW_COLS 128                        //                  (ky, kx, c) columns per workgroup: four tiles of 32
#define DW_X_PITCH 96                      // floats per staged pixel of x (64 + 32: the two pixels of a K-step on different banks)
#define DW_G_PITCH 160                     // ... of G (128 + 32)
#define DW_MAX_SPLIT_PIX 4096              // longest fp32 accumulation (pixels) before the fp64 sum over splits
#define DW_TARGET_WGS 512                  // workgroups the split count aims at (two per CU of a 256-CU part); a constant, so that the
                                           // workspace size is a pure function of the shape

struct DgArgs {
    const float *g, *W;
    float *dx;
    int g_ld, dx_ld, P, h, w, K, s, C_up;
};

__global__ __launch_bounds__(256) void deconv_dgrad_kernel(const DgArgs a) {
    __shared__ __attribute__((aligned(16))) float s_a[DG_PIX * DG_PITCH];      // [pixel][reduction value of the chunk]
    __shared__ __attribute__((aligned(16))) float s_b[DG_COLS * DG_PITCH];     // [output channel][reduction value of the chunk]
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, i = l & 31, hh = l >> 5;
    const int nnb = (a.K + DG_COLS - 1) / DG_COLS;
    const int nb = (int)(blockIdx.x % (unsigned)nnb), pb = (int)(blockIdx.x / (unsigned)nnb);     // the column blocks of one pixel block are neighbours
    const int n0 = nb * DG_COLS, p0 = pb * DG_PIX;
    const int ss = a.s * a.s, cpc = a.C_up >> 5, nch = ss * cpc, OW = a.s * a.w, hw = a.h * a.w;

    // staging roles.  A: pixels prow + 32 j of the block, floats [c4, c4 + 4) of the chunk;  B: reduction value rr, channels kq + 8 e
    const int c4 = (t & 7) * 4, prow = t >> 3, rr = t & 31, kq = t >> 5;
    int abase[4];                          // float offset of G[b][s y][s x][c4] for this lane's pixels; -1: no pixel
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int p = p0 + prow + 32 * j;
        abase[j] = -1;
        if (p < a.P) {
            const int b = p / hw, rem = p - b * hw, y = rem / a.w, x = rem - y * a.w;
            abase[j] = ((b * a.s * a.h + a.s * y) * OW + a.s * x) * a.g_ld + c4;
        }
    }
    float4 ar[4];
    float br[16];
    auto load = [&](int ch) {
        const int kk = ch / cpc, c0 = (ch - kk * cpc) * 32, ky = kk / a.s, kx = kk - ky * a.s;
        const int goff = (ky * OW + kx) * a.g_ld + c0;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            ar[j] = abase[j] >= 0 ? *reinterpret_cast<const float4 *>(a.g + abase[j] + goff) : make_float4(0.f, 0.f, 0.f, 0.f);
        const int woff = (c0 + rr) * ss + kk;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int k = n0 + kq + 8 * e;
            br[e] = k < a.K ? a.W[k * a.C_up * ss + woff] : 0.f;
        }
    };

    f32x16 acc[4];
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.f;

    load(0);
    for (int ch = 0; ch < nch; ++ch) {
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<float4 *>(s_a + (prow + 32 * j) * DG_PITCH + c4) = ar[j];
#pragma unroll
        for (int e = 0; e < 16; ++e) s_b[(kq + 8 * e) * DG_PITCH + rr] = br[e];
        __syncthreads();
        if (ch + 1 < nch) load(ch + 1);                   // in flight during the MFMAs
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float4 af = *reinterpret_cast<const float4 *>(s_a + (32 * wv + i) * DG_PITCH + 8 * q + 4 * hh);
#pragma unroll
            for (int nt = 0; nt < 4; ++nt) {
                if (n0 + 32 * nt < a.K) {                 // workgroup-uniform
                    const float4 bf = *reinterpret_cast<const float4 *>(s_b + (32 * nt + i) * DG_PITCH + 8 * q + 4 * hh);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.x, bf.x, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.y, bf.y, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.z, bf.z, acc[nt], 0, 0, 0);
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af.w, bf.w, acc[nt], 0, 0, 0);
                }
            }
        }
        __syncthreads();
    }

    // accumulator element r of lane l = row (pixel) 8 (r / 4) + 4 (l / 32) + r % 4, column (channel) l % 32
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
        const int col = n0 + 32 * nt + i;
        if (col < a.K) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int p = p0 + 32 * wv + 8 * (r >> 2) + 4 * hh + (r & 3);
                if (p < a.P) a.dx[p * a.dx_ld + col] = acc[nt][r];
            }
        }
    }
}

struct DwArgs {
    const float *x, *g;
    float *ws;
    int x_ld, g_ld, P, h, w, K, s, C_up, N;              // N = s^2 C_up
    int pix_per_split, n_tiles, n_nblocks;                 // n_tiles = row blocks x column blocks
};

__global__ __launch_bounds__(256) void deconv_wgrad_kernel(const DwArgs a) {
    __shared__ __attribute__((aligned(16))) float s_x[DW_PIX * DW_X_PITCH];    // [pixel of the chunk][input channel of the block]
    __shared__ __attribute__((aligned(16))) float s_g[DW_PIX * DW_G_PITCH];    // [pixel of the chunk][column of the block]
    const int t = threadIdx.x, l = t & 63, wv = t >> 6, i = l & 31, hh = l >> 5;
    const int tile = (int)(blockIdx.x % (unsigned)a.n_tiles), split = (int)(blockIdx.x / (unsigned)a.n_tiles);   // the tiles of one split are neighbours
    const int mb = tile / a.n_nblocks, nb = tile - mb * a.n_nblocks;
    const int k0 = mb * DW_ROWS, ct0 = nb * (DW_COLS / 32);
    const int pbeg = split * a.pix_per_split, pend = min(pbeg + a.pix_per_split, a.P);
    const int OW = a.s * a.w, hw = a.h * a.w;

    // staging role: pixel `pix` of the chunk, floats [f4, f4 + 4) of each 32-wide tile
    const int pix = t >> 3, f4 = (t & 7) * 4;
    int goff[4];                           // float offset of column tile q's (ky, kx, first channel) inside a pixel's patch; -1: no such tile
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int col0 = (ct0 + q) * 32;
        goff[q] = -1;
        if (col0 < a.N) {
            const int kk = col0 / a.C_up, c0 = col0 - kk * a.C_up, ky = kk / a.s, kx = kk - ky * a.s;
            goff[q] = (ky * OW + kx) * a.g_ld + c0 + f4;
        }
    }
    float4 xr[2], gr[4];
    auto load = [&](int pc) {              // pc: first pixel of the chunk
        const int p = pc + pix;
        const bool ok = p < pend;
        int gbase = 0;
        if (ok) {
            const int b = p / hw, rem = p - b * hw, y = rem / a.w, x = rem - y * a.w;
            gbase = ((b * a.s * a.h + a.s * y) * OW + a.s * x) * a.g_ld;
        }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            const int k = k0 + 32 * mt + f4;
            xr[mt] = (ok && k < a.K) ? *reinterpret_cast<const float4 *>(a.x + p * a.x_ld + k) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int q = 0; q < 4; ++q)
            gr[q] = (ok && goff[q] >= 0) ? *reinterpret_cast<const float4 *>(a.g + gbase + goff[q]) : make_float4(0.f, 0.f, 0.f, 0.f);
    };

    f32x16 acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[mt][r] = 0.f;
    const bool col_ok = (ct0 + wv) * 32 < a.N;            // this wave's column tile exists (wave-uniform)

    load(pbeg);
    for (int pc = pbeg; pc < pend; pc += DW_PIX) {
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) *reinterpret_cast<float4 *>(s_x + pix * DW_X_PITCH + 32 * mt + f4) = xr[mt];
#pragma unroll
        for (int q = 0; q < 4; ++q) *reinterpret_cast<float4 *>(s_g + pix * DW_G_PITCH + 32 * q + f4) = gr[q];
        __syncthreads();
        if (pc + DW_PIX < pend) load(pc + DW_PIX);        // in flight during the MFMAs
        if (col_ok) {
#pragma unroll
            for (int ks = 0; ks < DW_PIX / 2; ++ks) {     // K-step ks: pixels 2 ks + (l >> 5); A[m = input channel][k], B[k][n = column]
                const float bv = s_g[(2 * ks + hh) * DW_G_PITCH + 32 * wv + i];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    if (k0 + 32 * mt < a.K) {             // workgroup-uniform
                        const float av = s_x[(2 * ks + hh) * DW_X_PITCH + 32 * mt + i];
                        acc[mt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[mt], 0, 0, 0);
                    }
                }
            }
        }
        __syncthreads();
    }

    // partial of this split: [k][column]; accumulator element r of lane l = row 8 (r / 4) + 4 (l / 32) + r % 4, column l % 32
    if (col_ok) {
        float *o = a.ws + (size_t)split * a.K * a.N + (ct0 + wv) * 32 + i;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int k = k0 + 32 * mt + 8 * (r >> 2) + 4 * hh + (r & 3);
                if (k < a.K) o[(size_t)k * a.N] = acc[mt][r];
            }
    }
}

// dw[k][c][ky][kx] = (float) sum_{split, in order} ws[split][k][(ky, kx, c)]  in fp64
__global__ __launch_bounds__(256) void deconv_wgrad_finish_kernel(const float *__restrict__ ws, int n_splits, int K, int N, int C_up, int ss,
                                                                  float *__restrict__ dw) {
    const int idx = (int)(blockIdx.x * 256 + threadIdx.x), KN = K * N;
    if (idx >= KN) return;
    double sum = 0.;
    for (int s = 0; s < n_splits; ++s) sum += (double)ws[(size_t)s * KN + idx];      // fixed order
    const int k = idx / N, j = idx - k * N, kk = j / C_up, c = j - kk * C_up;
    dw[(k * C_up + c) * ss + kk] = (float)sum;
}

// ------------------------------------------------------------------ C ABI
LIDAR_EXPORT int lidar_deconv_train_supported(int K, int s, int C_up) {
    return (s == 1 || s == 2 || s == 4) && K >= LIDAR_DECONV_TRAIN_MIN_K && K <= LIDAR_DECONV_TRAIN_MAX_C && K % 8 == 0 &&
           C_up >= LIDAR_DECONV_TRAIN_MIN_CUP && C_up <= LIDAR_DECONV_TRAIN_MAX_C && C_up % 32 == 0;
}

struct DwPlan {
    int P, N, n_tiles, n_nblocks, n_splits, pix_per_split;
};

// pure host; false for unsupported, empty or oversize shapes
static bool dw_plan(int B, int h, int w, int K, int s, int C_up, DwPlan *p) {
    if (B <= 0 || h <= 0 || w <= 0 || !lidar_deconv_train_supported(K, s, C_up)) return false;
    const long long P = (long long)B * h * w;
    if (P > 0x3fffffffLL) return false;
    p->P = (int)P;
    p->N = s * s * C_up;
    p->n_nblocks = (p->N / 32 + DW_COLS / 32 - 1) / (DW_COLS / 32);
    p->n_tiles = ((K + DW_ROWS - 1) / DW_ROWS) * p->n_nblocks;
    long long splits = (DW_TARGET_WGS + p->n_tiles - 1) / p->n_tiles;
    const long long by_len = (P + DW_MAX_SPLIT_PIX - 1) / DW_MAX_SPLIT_PIX, by_chunks = (P + DW_PIX - 1) / DW_PIX;
    if (splits < by_len) splits = by_len;
    if (splits > by_chunks) splits = by_chunks;
    long long pps = (P + splits - 1) / splits;
    pps = (pps + DW_PIX - 1) / DW_PIX * DW_PIX;
    splits = (P + pps - 1) / pps;
    if (splits * p->n_tiles > 0x7fffffffLL) return false;
    p->n_splits = (int)splits;
    p->pix_per_split = (int)pps;
    return true;
}

LIDAR_EXPORT size_t lidar_deconv_wgrad_workspace_bytes(int B, int h, int w, int K, int s, int C_up) {
    DwPlan p;
    if (!dw_plan(B, h, w, K, s, C_up, &p)) return 0;
    return (size_t)p.n_splits * K * p.N * sizeof(float);
}

static bool dt_misaligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) != 0; }

// dx[p][k] = sum_{ky,kx,c} g[b][s y + ky][s x + kx][c] * W[k][c][ky][kx], rows of dx_ld floats
LIDAR_EXPORT int lidar_deconv_dgrad_nhwc(const float *g, int g_ld, const float *W, int B, int h, int w, int K, int s, int C_up, float *dx,
                                         int dx_ld, void *stream) {
    if (!g || !W || !dx || B <= 0 || h <= 0 || w <= 0 || !lidar_deconv_train_supported(K, s, C_up) || g_ld < C_up || dx_ld < K ||
        (g_ld & 3) || dt_misaligned(g))
        return LIDAR_ERR_ARG;
    const long long P = (long long)B * h * w;
    if (P * s * s * g_ld * 4 >= 0x7fffffffLL || P * dx_ld * 4 >= 0x7fffffffLL) return LIDAR_ERR_ARG;       // 32-bit offsets
    DgArgs a;
    a.g = g; a.W = W; a.dx = dx; a.g_ld = g_ld; a.dx_ld = dx_ld; a.P = (int)P; a.h = h; a.w = w; a.K = K; a.s = s; a.C_up = C_up;
    const long long grid = ((P + DG_PIX - 1) / DG_PIX) * ((K + DG_COLS - 1) / DG_COLS);
    hipLaunchKernelGGL(deconv_dgrad_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, a);
    return lidar_check_launch("lidar_deconv_dgrad_nhwc");
}

// dw[k][c][ky][kx] = sum_p x[p][k] * g[b][s y + ky][s x + kx][c], contiguous (K, C_up, s, s), overwritten
LIDAR_EXPORT int lidar_deconv_wgrad_nhwc(const float *x, int x_ld, const float *g, int g_ld, int B, int h, int w, int K, int s, int C_up,
                                         float *dw, void *ws, size_t ws_bytes, void *stream) {
    DwPlan p;
    if (!x || !g || !dw || B <= 0 || h <= 0 || w <= 0 || !lidar_deconv_train_supported(K, s, C_up) || x_ld < K || g_ld < C_up ||
        (x_ld & 3) || (g_ld & 3) || dt_misaligned(x) || dt_misaligned(g))
        return LIDAR_ERR_ARG;
    const long long P = (long long)B * h * w;
    if (P * x_ld * 4 >= 0x7fffffffLL || P * s * s * g_ld * 4 >= 0x7fffffffLL) return LIDAR_ERR_ARG;        // 32-bit offsets
    if (!dw_plan(B, h, w, K, s, C_up, &p)) return LIDAR_ERR_ARG;
    if (!ws || dt_misaligned(ws) || ws_bytes < lidar_deconv_wgrad_workspace_bytes(B, h, w, K, s, C_up)) return LIDAR_ERR_WORKSPACE;
    DwArgs a;
    a.x = x; a.g = g; a.ws = static_cast<float *>(ws);
    a.x_ld = x_ld; a.g_ld = g_ld; a.P = p.P; a.h = h; a.w = w; a.K = K; a.s = s; a.C_up = C_up; a.N = p.N;
    a.pix_per_split = p.pix_per_split; a.n_tiles = p.n_tiles; a.n_nblocks = p.n_nblocks;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(deconv_wgrad_kernel, dim3((unsigned)(p.n_splits * p.n_tiles)), dim3(256), 0, st, a);
    hipLaunchKernelGGL(deconv_wgrad_finish_kernel, dim3((unsigned)divup((long long)K * p.N, 256)), dim3(256), 0, st, a.ws, p.n_splits, K, p.N,
                       C_up, s * s, dw);
    return lidar_check_launch("lidar_deconv_wgrad_nhwc");
}
