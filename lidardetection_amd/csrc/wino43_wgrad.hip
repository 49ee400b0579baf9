// Weight gradient of the 3x3 / stride 1 / pad 1 fp32 convolution on NHWC maps as Winograd F(3x3, 4x4) on the fp32 matrix cores: the
// training counterpart of csrc/wino43_conv.hip for the stride-1 Conv2d layers of BaseBEVBackbone
// (pcdet/models/backbones_2d/base_bev_backbone.py:34-45), whose weight gradient torch hands to MIOpen.
//
//   dW[co, ci, a, b] = sum_{n,h,w} g[n, h, w, co] * x[n, h + a - 1, w + b - 1, ci]
//
// Cut the map into the 4 x 4 output tiles of the F(4x4, 3x3) forward.  Each tile contributes the 3 x 3 VALID correlation of its 6 x 6
// input patch with its 4 x 4 gradient patch: the minimal-filtering problem F(3x3, 4x4), 36 multiplications per (tile, ci, co) where
// the direct sum needs 144.  One dimension, y_k = sum_{i<4} g_i x_{i+k} (k < 3), interpolation points {0, 1, -1, 2, -2, inf}:
//   y = A^T [ (G g) .* (B^T x) ]
//   B^T = [4 0 -5 0 1 0; 0 -4 -4 1 1 0; 0 4 -4 -1 1 0; 0 -2 -1 2 1 0; 0 2 -1 -2 1 0; 0 4 0 -5 0 1]
//   G   = [1/4 0 0 0; -1/6 -1/6 -1/6 -1/6; -1/6 1/6 -1/6 1/6; 1/24 1/12 1/6 1/3; 1/24 -1/12 1/6 -1/3; 0 0 0 1]
//   A^T = [1 1 1 1 1 0; 0 1 -1 2 -2 0; 0 1 1 4 4 1]
// (the textbook points, not the {.., 1/2, ..} set of wino43_conv.hip: here the two transformed operands are both data, there is no
// constant filter to fold scale factors into).  Two dimensions: both sides.  In the transform domain the layer is 36 independent
// GEMMs whose reduction runs over the TILES:  M_p[co, ci] = sum_tiles V_p[tile, co] * U_p[tile, ci],  V = G g G^T,  U = B^T x B.
//
// Main kernel.  A workgroup (4 waves) owns one 32 (co) x 32 (ci) block of all 36 positions — 36 accumulator tiles of
// v_mfma_f32_32x32x2_f32, nine per wave, 144 registers per lane — and one contiguous range of tiles (a "split").  Per chunk of 8 tiles:
//   * every lane owns one (tile, channel) of the chunk: it transforms the 6 x 6 input patch of its ci and the 4 x 4 gradient patch of
//     its co (both prefetched into registers during the previous chunk's MFMAs; out-of-map pixels and tiles beyond the range are
//     zeros: x outside the map is the padding, g outside contributes nothing) and writes U / V to LDS as [position][tile][channel]:
//     one VALU burst, apart from the MFMAs (VALU does not overlap the MFMAs of its SIMD on this part);
//   * barrier; the global loads of the next chunk are issued; each wave runs 9 positions x 4 MFMAs (K = 2 tiles each), its operands
//     one conflict-free 256-byte LDS read each (lane l reads float 64 k + l of the position's 256); barrier.
// Both transforms live inside the kernel: x and g are read from memory once per workgroup that needs them, no transformed copy of
// either map exists.  The accumulation inside a split is fp32 (the MFMA's); a split is at most 512 tiles.
// Each workgroup writes its 36 x 32 x 32 partial to the caller's workspace with plain vector stores — every workgroup its own slot,
// every slot written in full, so nothing depends on what the workspace held.
//
// Finishing kernel.  One workgroup per (co, block of 32 ci): 36 positions x 8 float4 lanes sum the partials of all splits in split
// order in fp64, then 32 ci x 9 lanes apply A^T M A in fp64 and round once to fp32 (the pattern of csrc/bn_train.hip's moment sums).
// No float atomics anywhere: the result is bitwise reproducible run to run.
#include "common.h"

typedef float f32x16 __attribute__((ext_vector_type(16)));

#define WGR_TILES 8                        // tiles per chunk: 256 lanes = 8 tiles x 32 channels
#define WGR_MAX_SPLIT_TILES 512            // longest fp32 accumulation (tiles) before the fp64 sum over splits
#define WGR_TARGET_WGS 512                 // workgroups the split count aims at (two per CU of a 256-CU part); a constant, so that
                                           // the workspace size is a pure function of the shape
#define WGR_MAX_C 512                      // widest layer taken (wider ones are neither tested nor measured: they stay on the library)
#define WGR_LDS_BYTES (2 * 36 * 256 * 4)

struct WgradArgs {
    const float *x, *g;
    float *ws;
    int x_ld, g_ld, B, H, W;
    int tiles_y, tiles_x, n_tiles, tiles_per_split, n_ci, n_blocks;
};

// o = B^T d
__device__ __forceinline__ void wgr_bt(const float d[6], float o[6]) {
    const float a = fmaf(-4.f, d[2], d[4]), b = fmaf(-4.f, d[1], d[3]);
    const float c = d[4] - d[2], e = d[3] - d[1];
    o[0] = fmaf(4.f, d[0], fmaf(-5.f, d[2], d[4]));
    o[1] = a + b;
    o[2] = a - b;
    o[3] = fmaf(2.f, e, c);
    o[4] = fmaf(-2.f, e, c);
    o[5] = fmaf(4.f, d[1], fmaf(-5.f, d[3], d[5]));
}

// o = G d
__device__ __forceinline__ void wgr_g(const float d[4], float o[6]) {
    const float s = d[0] + d[2], t = d[1] + d[3];
    const float u = fmaf(4.f, d[2], d[0]), v = fmaf(4.f, d[3], d[1]);
    o[0] = 0.25f * d[0];
    o[1] = (-1.f / 6.f) * (s + t);
    o[2] = (-1.f / 6.f) * (s - t);
    o[3] = (1.f / 24.f) * fmaf(2.f, v, u);
    o[4] = (1.f / 24.f) * fmaf(-2.f, v, u);
    o[5] = d[3];
}

__global__ __launch_bounds__(256) void wino43_wgrad_kernel(const WgradArgs a) {
    extern __shared__ float s_wgr[];
    float *s_u = s_wgr;                    // [36 positions][8 tiles][32 ci]
    float *s_v = s_wgr + 36 * 256;         // [36 positions][8 tiles][32 co]
    const int t = threadIdx.x, l = t & 63, wv = t >> 6;
    const int j = t >> 5, c = t & 31;      // this lane's tile of the chunk and channel of the block
    const int blk = (int)(blockIdx.x % (unsigned)a.n_blocks), split = (int)(blockIdx.x / (unsigned)a.n_blocks);
    const int cb = blk / a.n_ci, ib = blk - cb * a.n_ci;
    const int t0 = split * a.tiles_per_split, t1 = min(t0 + a.tiles_per_split, a.n_tiles);
    const int H = a.H, W = a.W, tpi = a.tiles_y * a.tiles_x;
    const float *xc = a.x + ib * 32 + c, *gc = a.g + cb * 32 + c;

    float xr[36], gr[16];
    auto load = [&](int tile) {
        if (tile >= t1) {
#pragma unroll
            for (int k = 0; k < 36; ++k) xr[k] = 0.f;
#pragma unroll
            for (int k = 0; k < 16; ++k) gr[k] = 0.f;
            return;
        }
        const int b = tile / tpi, r = tile - b * tpi;
        const int ty = r / a.tiles_x, tx = r - ty * a.tiles_x;
        const int y0 = 4 * ty - 1, x0 = 4 * tx - 1;
        const int pix0 = (b * H + y0) * W + x0;          // may lie before the map for border tiles: only dereferenced where valid
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            const bool yok = (unsigned)(y0 + i) < (unsigned)H;
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                const bool ok = yok && (unsigned)(x0 + k) < (unsigned)W;
                xr[i * 6 + k] = ok ? xc[(long long)(pix0 + i * W + k) * a.x_ld] : 0.f;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool yok = y0 + 1 + i < H;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool ok = yok && x0 + 1 + k < W;
                gr[i * 4 + k] = ok ? gc[(long long)(pix0 + (i + 1) * W + k + 1) * a.g_ld] : 0.f;
            }
        }
    };

    f32x16 acc[9];
#pragma unroll
    for (int q = 0; q < 9; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[q][i] = 0.f;

    load(t0 + j);
    for (int tb = t0; tb < t1; tb += WGR_TILES) {
        {   // U = B^T x B
            float tm[6][6];
#pragma unroll
            for (int k = 0; k < 6; ++k) {
                float d[6], o[6];
#pragma unroll
                for (int i = 0; i < 6; ++i) d[i] = xr[i * 6 + k];
                wgr_bt(d, o);
#pragma unroll
                for (int i = 0; i < 6; ++i) tm[i][k] = o[i];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                float o[6];
                wgr_bt(tm[i], o);
#pragma unroll
                for (int k = 0; k < 6; ++k) s_u[(i * 6 + k) * 256 + t] = o[k];
            }
        }
        {   // V = G g G^T
            float tm[6][4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                float d[4], o[6];
#pragma unroll
                for (int i = 0; i < 4; ++i) d[i] = gr[i * 4 + k];
                wgr_g(d, o);
#pragma unroll
                for (int i = 0; i < 6; ++i) tm[i][k] = o[i];
            }
#pragma unroll
            for (int i = 0; i < 6; ++i) {
                float o[6];
                wgr_g(tm[i], o);
#pragma unroll
                for (int k = 0; k < 6; ++k) s_v[(i * 6 + k) * 256 + t] = o[k];
            }
        }
        __syncthreads();
        load(tb + WGR_TILES + j);                        // in flight during the MFMAs (zeros past the range, no access)
#pragma unroll
        for (int q = 0; q < 9; ++q) {
            const int p = wv * 9 + q;
#pragma unroll
            for (int k = 0; k < 4; ++k) {                // K-step k: tiles 2 k + (l >> 5); A[m = co][k], B[k][n = ci]
                const float av = s_v[p * 256 + k * 64 + l];
                const float bv = s_u[p * 256 + k * 64 + l];
                acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc[q], 0, 0, 0);
            }
        }
        __syncthreads();
    }

    // partial of this (split, block): [position][co][ci]; accumulator element i of lane l = row 8 (i / 4) + 4 (l / 32) + i % 4, column l % 32
    float *o = a.ws + ((size_t)blockIdx.x * 36 + wv * 9) * 1024;
#pragma unroll
    for (int q = 0; q < 9; ++q)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[q * 1024 + (8 * (i >> 2) + 4 * (l >> 5) + (i & 3)) * 32 + (l & 31)] = acc[q][i];
}

__global__ __launch_bounds__(288) void wino43_wgrad_finish_kernel(const float *__restrict__ ws, int n_splits, int n_blocks, int n_ci, int Cin,
                                                                  float *__restrict__ dw) {
    __shared__ double s_m[36 * 32];
    const int ib = blockIdx.x, co = blockIdx.y, t = threadIdx.x;
    const int blk = (co >> 5) * n_ci + ib;
    {
        const int p = t >> 3, q4 = t & 7;
        const float *src = ws + ((size_t)blk * 36 + p) * 1024 + (co & 31) * 32 + q4 * 4;
        const size_t stride = (size_t)n_blocks * 36 * 1024;
        double s0 = 0., s1 = 0., s2 = 0., s3 = 0.;
        for (int s = 0; s < n_splits; ++s) {             // fixed order
            const float4 v = *reinterpret_cast<const float4 *>(src + (size_t)s * stride);
            s0 += (double)v.x;
            s1 += (double)v.y;
            s2 += (double)v.z;
            s3 += (double)v.w;
        }
        double *d = s_m + p * 32 + q4 * 4;
        d[0] = s0; d[1] = s1; d[2] = s2; d[3] = s3;
    }
    __syncthreads();
    const double AT[3][6] = {{1., 1., 1., 1., 1., 0.}, {0., 1., -1., 2., -2., 0.}, {0., 1., 1., 4., 4., 1.}};
    const int ci_l = t / 9, ab = t - ci_l * 9, ka = ab / 3, kb = ab - ka * 3;
    double sum = 0.;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double row = 0.;
#pragma unroll
        for (int k = 0; k < 6; ++k) row += AT[kb][k] * s_m[(i * 6 + k) * 32 + ci_l];
        sum += AT[ka][i] * row;
    }
    dw[((size_t)co * Cin + ib * 32 + ci_l) * 9 + ab] = (float)sum;
}

// ------------------------------------------------------------------ C ABI
LIDAR_EXPORT int lidar_wino43_wgrad_supported(int Cin, int Cout) {
    return Cin >= 32 && Cout >= 32 && Cin <= WGR_MAX_C && Cout <= WGR_MAX_C && !(Cin & 31) && !(Cout & 31);
}

struct WgradPlan {
    int tiles_y, tiles_x, n_tiles, n_blocks, n_ci, n_splits, tiles_per_split;
};

// pure host; false for unsupported, empty or oversize shapes
static bool wgr_plan(int B, int H, int W, int Cin, int Cout, WgradPlan *p) {
    if (B <= 0 || H <= 0 || W <= 0 || !lidar_wino43_wgrad_supported(Cin, Cout)) return false;
    const long long ty = (H + 3LL) / 4, tx = (W + 3LL) / 4, nt = (long long)B * ty * tx;
    if (nt > 0x3fffffffLL) return false;
    p->tiles_y = (int)ty; p->tiles_x = (int)tx; p->n_tiles = (int)nt;
    p->n_ci = Cin / 32;
    p->n_blocks = (Cout / 32) * p->n_ci;
    long long splits = (WGR_TARGET_WGS + p->n_blocks - 1) / p->n_blocks;
    const long long by_len = (nt + WGR_MAX_SPLIT_TILES - 1) / WGR_MAX_SPLIT_TILES, by_chunks = (nt + WGR_TILES - 1) / WGR_TILES;
    if (splits < by_len) splits = by_len;
    if (splits > by_chunks) splits = by_chunks;
    long long tps = (nt + splits - 1) / splits;
    tps = (tps + WGR_TILES - 1) / WGR_TILES * WGR_TILES;
    splits = (nt + tps - 1) / tps;
    if (splits * p->n_blocks > 0x7fffffffLL) return false;
    p->n_splits = (int)splits;
    p->tiles_per_split = (int)tps;
    return true;
}

LIDAR_EXPORT size_t lidar_wino43_wgrad_workspace_bytes(int B, int H, int W, int Cin, int Cout) {
    WgradPlan p;
    if (!wgr_plan(B, H, W, Cin, Cout, &p)) return 0;
    return (size_t)p.n_splits * p.n_blocks * 36 * 1024 * sizeof(float);
}

// dw[co][ci][a][b] = sum_{n,h,w} g[n][h][w][co] * x[n][h + a - 1][w + b - 1][ci]   (zero padding), overwritten.
// x: (B, H, W) pixels of x_ld floats, channels [0, Cin); g: (B, H, W) pixels of g_ld floats, channels [0, Cout).
LIDAR_EXPORT int lidar_wino43_wgrad_nhwc(const float *x, int x_ld, const float *g, int g_ld, int B, int H, int W, int Cin, int Cout, float *dw,
                                         void *ws, size_t ws_bytes, void *stream) {
    WgradPlan p;
    if (!x || !g || !dw || !lidar_wino43_wgrad_supported(Cin, Cout) || B <= 0 || H <= 0 || W <= 0 || x_ld < Cin || g_ld < Cout)
        return LIDAR_ERR_ARG;
    if ((long long)B * H * W * x_ld * 4 >= 0x7fffffffLL || (long long)B * H * W * g_ld * 4 >= 0x7fffffffLL) return LIDAR_ERR_ARG;
    if (!wgr_plan(B, H, W, Cin, Cout, &p)) return LIDAR_ERR_ARG;
    if (!ws || (reinterpret_cast<uintptr_t>(ws) & 15) || ws_bytes < lidar_wino43_wgrad_workspace_bytes(B, H, W, Cin, Cout))
        return LIDAR_ERR_WORKSPACE;
    WgradArgs a;
    a.x = x; a.g = g; a.ws = static_cast<float *>(ws);
    a.x_ld = x_ld; a.g_ld = g_ld; a.B = B; a.H = H; a.W = W;
    a.tiles_y = p.tiles_y; a.tiles_x = p.tiles_x; a.n_tiles = p.n_tiles; a.tiles_per_split = p.tiles_per_split;
    a.n_ci = p.n_ci; a.n_blocks = p.n_blocks;
    hipStream_t s = (hipStream_t)stream;
    int dev_id = 0;
    (void)hipGetDevice(&dev_id);
    dev_id &= 63;
    static bool attr_set[64] = {};
    if (!attr_set[dev_id]) {
        (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&wino43_wgrad_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, WGR_LDS_BYTES);
        attr_set[dev_id] = true;
    }
    hipLaunchKernelGGL(wino43_wgrad_kernel, dim3((unsigned)(p.n_splits * p.n_blocks)), dim3(256), WGR_LDS_BYTES, s, a);
    hipLaunchKernelGGL(wino43_wgrad_finish_kernel, dim3((unsigned)p.n_ci, (unsigned)Cout), dim3(288), 0, s, a.ws, p.n_splits, p.n_blocks, p.n_ci,
                       Cin, dw);
    return lidar_check_launch("lidar_wino43_wgrad_nhwc");
}
