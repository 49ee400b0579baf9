// PointPillar's PillarVFE + single PFNLayer in TRAIN mode, forward and backward, and the backward of PointPillarScatter.
//   reference: pcdet/models/backbones_3d/vfe/pillar_vfe.py:29-49 (PFNLayer), :94-123 (PillarVFE.forward);
//              pcdet/models/backbones_2d/map_to_bev/pointpillar_scatter.py:14-37
//
// The layer is decorate -> Linear(bias=False) -> BatchNorm1d (batch statistics over ALL V*P rows, padded slots included) ->
// ReLU -> max over the P slots.  Nothing here materialises the (V, P, 64) tensors:
//   * statistics: z = W x has sum(z) = W S and sum(z^2) = diag(W G W^T) with S = sum x, G = sum x x^T over the real points
//     (a padded row is all zero: it adds nothing to S or G but counts in N = V * P).  One pass accumulates S and G in fp64
//     per block; a fixed-order reduction and a one-block finalize give the mean, the biased variance and scale / shift.
//   * max: the BatchNorm affine map is monotone in z (non-decreasing for gamma >= 0, non-increasing for gamma < 0), so
//     max_p relu(BN(z_p)) = relu(BN(z_sel)) with z_sel = max_p z (gamma >= 0) or min_p z (gamma < 0), the padded row's z = 0
//     included when n < P.  The same pass keeps z_sel and its slot per (pillar, channel); a light pass applies scale / shift.
//   * backward: only the selected row of each (pillar, channel) carries delta = g * [y > 0], so with zh = (z - mu) / sigma
//       dbeta = sum delta,  dgamma = sum delta zh,
//       dW_c = gamma_c / sigma_c (sum delta x_sel - dbeta_c / N S - dgamma_c / N (G w_c - mu_c S) / sigma_c);
//     one pass over (V, cout) re-reads the selected point of each pillar (and the pillar's points for its mean).
// Per-block partial sums in fp64, reduced in a fixed order (ordered_reduce.h's kernel, shared with the BatchNorm statistics of
// bn_train_dev.h): no float atomics, results are bitwise reproducible.
#include "ordered_reduce.h"

#define PT_WAVES 4                 // waves per 256-thread block
#define PT_MAX_BLOCKS 2048
#define PT_PAD_SLOT 255            // "the selected row is a padded (all-zero) slot"
// stats (fp64): [0, 136) S / G sums (upper triangle of the augmented (nf + 1)^2 moment matrix), mean, inverse std, N
#define PT_ST_MU 136
#define PT_ST_INV 200
#define PT_ST_N 264
#define PT_STATS_DOUBLES LIDAR_PFN_TRAIN_STATS_DOUBLES

struct PfnTrainParams {
    float vx, vy, vz, xo, yo, zo;
    int P, cout, coords_are_float, num_are_float;
};

// intra-wave ordering of LDS writes and reads by other lanes of the same wave
__device__ __forceinline__ void pt_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ float pt_wave_sum(float v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}

// the voxel's point count (clamped to [0, P]) and its pillar centre (x, y, z); wave-uniform
__device__ __forceinline__ int pt_head(const void *num_points, const void *coords, int v, const PfnTrainParams &p, float &ox, float &oy,
                                       float &oz) {
    int n = p.num_are_float ? (int)((const float *)num_points)[v] : ((const int *)num_points)[v];
    float cz, cy, cx;
    if (p.coords_are_float) {
        const float4 c = ((const float4 *)coords)[v];
        cz = c.y; cy = c.z; cx = c.w;
    } else {
        const int4 c = ((const int4 *)coords)[v];
        cz = (float)c.y; cy = (float)c.z; cx = (float)c.w;
    }
    ox = cx * p.vx + p.xo; oy = cy * p.vy + p.yo; oz = cz * p.vz + p.zo;
    return min(max(n, 0), p.P);
}

// lane l < n holds point l of voxel v, the other lanes zeros; returns the point mean (wave-uniform)
template <int C>
__device__ __forceinline__ void pt_points(const float *voxels, int v, int n, int P, float *pt, float &mx, float &my, float &mz) {
    const int l = lane_id();
#pragma unroll
    for (int k = 0; k < C; ++k) pt[k] = 0.f;
    if (l < n) {
        const float *q = voxels + ((size_t)v * P + l) * C;
#pragma unroll
        for (int k = 0; k < C; ++k) pt[k] = q[k];
    }
    const float fn = (float)n;
    mx = pt_wave_sum(pt[0]) / fn; my = pt_wave_sum(pt[1]) / fn; mz = pt_wave_sum(pt[2]) / fn;
}

// PillarVFE's decorated row: [point C | xyz - mean | xyz - pillar centre | |xyz|]
template <int C, bool DIST>
__device__ __forceinline__ void pt_decorate(const float *pt, float mx, float my, float mz, float ox, float oy, float oz, float *x) {
#pragma unroll
    for (int k = 0; k < C; ++k) x[k] = pt[k];
    x[C + 0] = pt[0] - mx; x[C + 1] = pt[1] - my; x[C + 2] = pt[2] - mz;
    x[C + 3] = pt[0] - ox; x[C + 4] = pt[1] - oy; x[C + 5] = pt[2] - oz;
    if (DIST) x[C + 6] = sqrtf(pt[0] * pt[0] + pt[1] * pt[1] + pt[2] * pt[2]);
}

// forward pass 1.  One wave per voxel: lanes = points for the decoration and the moments, lanes = channels for z.
// Lane l accumulates the moment entries e = l, l + 64, l + 128 of the augmented row [x | 1] (upper triangle, row-major).
template <int C, bool DIST>
__global__ __launch_bounds__(256) void pfn_train_stats_kernel(const float *__restrict__ voxels, const void *__restrict__ num_points,
                                                              const void *__restrict__ coords, const float *__restrict__ weight,
                                                              const float *__restrict__ gamma, const int *__restrict__ nvox_dev,
                                                              int nvox_host, PfnTrainParams p, float *__restrict__ zsel,
                                                              unsigned char *__restrict__ slot, double *__restrict__ part) {
    constexpr int NF = C + 6 + (DIST ? 1 : 0), D = NF + 1, NE = D * (D + 1) / 2;
    static_assert(NE <= 3 * 64, "moment entries exceed three per lane");
    __shared__ float s_x[PT_WAVES][64][D + 1];
    __shared__ double s_red[PT_WAVES][3 * 64];
    const int l = lane_id(), wv = threadIdx.x >> 6;
    const int nv = nvox_dev ? min(*nvox_dev, nvox_host) : nvox_host;
    const int wave = blockIdx.x * PT_WAVES + wv, nwaves = gridDim.x * PT_WAVES;
    const bool chan = l < p.cout;
    float wt[NF];
#pragma unroll
    for (int k = 0; k < NF; ++k) wt[k] = chan ? weight[l * NF + k] : 0.f;
    const bool neg = chan && gamma[l] < 0.f;
    int ea[3], eb[3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        int a = 0, r = l + 64 * j;
        while (a < D && r >= D - a) { r -= D - a; ++a; }
        ea[j] = a < D ? a : 0; eb[j] = a < D ? a + r : 0;
    }
    double acc[3] = {0.0, 0.0, 0.0};
    float(*xs)[D + 1] = s_x[wv];
    for (int v = wave; v < nv; v += nwaves) {
        float ox, oy, oz;
        const int n = pt_head(num_points, coords, v, p, ox, oy, oz);
        float pt[C], mx, my, mz;
        pt_points<C>(voxels, v, n, p.P, pt, mx, my, mz);
        float x[NF];
        pt_decorate<C, DIST>(pt, mx, my, mz, ox, oy, oz, x);
        if (l < n) {
#pragma unroll
            for (int k = 0; k < NF; ++k) xs[l][k] = x[k];
            xs[l][NF] = 1.f;
        }
        // z of every point in every channel; the padded row (z = 0) takes part when n < P
        float zmx = n < p.P ? 0.f : -INFINITY, zmn = n < p.P ? 0.f : INFINITY;
        int smx = PT_PAD_SLOT, smn = PT_PAD_SLOT;
        for (int q = 0; q < n; ++q) {                     // wave-uniform: readlane broadcasts
            float z = 0.f;
#pragma unroll
            for (int k = 0; k < NF; ++k) z = fmaf(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(x[k]), q)), wt[k], z);
            if (z > zmx) { zmx = z; smx = q; }
            if (z < zmn) { zmn = z; smn = q; }
        }
        if (chan) {
            zsel[(size_t)v * p.cout + l] = neg ? zmn : zmx;
            slot[(size_t)v * p.cout + l] = (unsigned char)(neg ? smn : smx);
        }
        pt_wave_sync();
        for (int q = 0; q < n; ++q) {
#pragma unroll
            for (int j = 0; j < 3; ++j) acc[j] += (double)xs[q][ea[j]] * (double)xs[q][eb[j]];
        }
        pt_wave_sync();                                   // the rows are read before the next voxel overwrites them
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) s_red[wv][64 * j + l] = acc[j];
    __syncthreads();
    for (int e = threadIdx.x; e < NE; e += 256)
        part[(size_t)e * gridDim.x + blockIdx.x] = ((s_red[0][e] + s_red[1][e]) + s_red[2][e]) + s_red[3][e];
}

__device__ __forceinline__ int pt_tri(int a, int b, int D) {   // index of (a, b), a <= b, in the row-major upper triangle
    if (a > b) { const int t = a; a = b; b = t; }
    return a * D - a * (a - 1) / 2 + (b - a);
}

// forward pass 2 (one block, thread = channel): batch mean / biased variance in fp64 from S, G; fp32 scale / shift
__global__ __launch_bounds__(64) void pfn_train_finalize_kernel(const float *__restrict__ weight, const float *__restrict__ gamma,
                                                                const float *__restrict__ beta, int nf, int cout, int P, float eps,
                                                                const int *__restrict__ nvox_dev, int nvox_host,
                                                                double *__restrict__ stats, float *__restrict__ scale_shift,
                                                                float *__restrict__ batch_stats) {
    const int c = threadIdx.x;
    if (c >= cout) return;
    const int D = nf + 1;
    const int nv = nvox_dev ? min(*nvox_dev, nvox_host) : nvox_host;
    const double N = (double)nv * P;
    const float *w = weight + c * nf;
    double ws = 0.0, wgw = 0.0;
    for (int k = 0; k < nf; ++k) {
        ws += (double)w[k] * stats[pt_tri(k, nf, D)];
        double gk = 0.0;
        for (int j = 0; j < nf; ++j) gk += stats[pt_tri(k, j, D)] * (double)w[j];
        wgw += (double)w[k] * gk;
    }
    const double mu = ws / N;
    const double var = fmax(wgw / N - mu * mu, 0.0);
    const double inv = 1.0 / sqrt(var + (double)eps);
    const double a = (double)gamma[c] * inv;
    stats[PT_ST_MU + c] = mu;
    stats[PT_ST_INV + c] = inv;
    if (c == 0) stats[PT_ST_N] = N;
    scale_shift[c] = (float)a;
    scale_shift[cout + c] = (float)((double)beta[c] - mu * a);
    batch_stats[c] = (float)mu;
    batch_stats[cout + c] = (float)var;
    batch_stats[2 * cout + c] = (float)(N > 1.0 ? var * N / (N - 1.0) : var);
}

// forward pass 3: y = relu(z_sel * scale + shift); rows past the device count are zero
__global__ __launch_bounds__(256) void pfn_train_apply_kernel(const float *__restrict__ zsel, const float *__restrict__ scale_shift,
                                                              int cout, const int *__restrict__ nvox_dev, int nvox_host,
                                                              float *__restrict__ out) {
    const int nv = nvox_dev ? min(*nvox_dev, nvox_host) : nvox_host;
    const long long total = (long long)nvox_host * cout, live = (long long)nv * cout;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int c = (int)(i % cout);
        out[i] = i < live ? fmaxf(fmaf(zsel[i], scale_shift[c], scale_shift[cout + c]), 0.f) : 0.f;
    }
}

// backward pass 1.  One wave per voxel, lane = channel: delta of the selected row, its normalised z and its decorated row
// (the selected point is fetched from the lane that loaded it).  Per lane, in fp64: T[k] = sum delta x_sel[k], dbeta, dgamma.
template <int C, bool DIST>
__global__ __launch_bounds__(256) void pfn_train_bwd_kernel(const float *__restrict__ voxels, const void *__restrict__ num_points,
                                                            const void *__restrict__ coords, const float *__restrict__ grad,
                                                            const float *__restrict__ zsel, const unsigned char *__restrict__ slot,
                                                            const float *__restrict__ scale_shift, const double *__restrict__ stats,
                                                            const int *__restrict__ nvox_dev, int nvox_host, PfnTrainParams p,
                                                            double *__restrict__ part) {
    constexpr int NF = C + 6 + (DIST ? 1 : 0), K = NF + 2;
    __shared__ double s_red[PT_WAVES][64][K];
    const int l = lane_id(), wv = threadIdx.x >> 6;
    const int nv = nvox_dev ? min(*nvox_dev, nvox_host) : nvox_host;
    const int wave = blockIdx.x * PT_WAVES + wv, nwaves = gridDim.x * PT_WAVES;
    const bool chan = l < p.cout;
    const float sc = chan ? scale_shift[l] : 0.f, sh = chan ? scale_shift[p.cout + l] : 0.f;
    const double mu = chan ? stats[PT_ST_MU + l] : 0.0, inv = chan ? stats[PT_ST_INV + l] : 0.0;
    double t[NF], db = 0.0, dg = 0.0;
#pragma unroll
    for (int k = 0; k < NF; ++k) t[k] = 0.0;
    for (int v = wave; v < nv; v += nwaves) {
        float ox, oy, oz;
        const int n = pt_head(num_points, coords, v, p, ox, oy, oz);
        float pt[C], mx, my, mz;
        pt_points<C>(voxels, v, n, p.P, pt, mx, my, mz);
        int s = PT_PAD_SLOT;
        float zs = 0.f, g = 0.f;
        if (chan) {
            const size_t i = (size_t)v * p.cout + l;
            s = slot[i]; zs = zsel[i]; g = grad[i];
        }
        const bool pad = s >= n;                          // the padded slot marker (or a slot past the count)
        float q[C];
#pragma unroll
        for (int k = 0; k < C; ++k) q[k] = __shfl(pt[k], pad ? 0 : s, 64);
        float x[NF];
        pt_decorate<C, DIST>(q, mx, my, mz, ox, oy, oz, x);
        const float y = fmaxf(fmaf(zs, sc, sh), 0.f);     // the forward output, bit for bit
        const double delta = (chan && y > 0.f) ? (double)g : 0.0;
        db += delta;
        dg += delta * (((double)zs - mu) * inv);
        if (!pad) {
#pragma unroll
            for (int k = 0; k < NF; ++k) t[k] += delta * (double)x[k];
        }
    }
#pragma unroll
    for (int k = 0; k < NF; ++k) s_red[wv][l][k] = t[k];
    s_red[wv][l][NF] = db;
    s_red[wv][l][NF + 1] = dg;
    __syncthreads();
    for (int e = threadIdx.x; e < p.cout * K; e += 256) {
        const int c = e / K, k = e - c * K;
        part[(size_t)e * gridDim.x + blockIdx.x] = ((s_red[0][c][k] + s_red[1][c][k]) + s_red[2][c][k]) + s_red[3][c][k];
    }
}

// backward pass 2 (one block, thread = channel): dW, dgamma, dbeta from the reduced sums and the forward's S, G, mu, sigma
__global__ __launch_bounds__(64) void pfn_train_bwd_finalize_kernel(const double *__restrict__ btot, const double *__restrict__ stats,
                                                                    const float *__restrict__ weight, const float *__restrict__ gamma,
                                                                    int nf, int cout, float *__restrict__ d_weight,
                                                                    float *__restrict__ d_gamma, float *__restrict__ d_beta) {
    const int c = threadIdx.x;
    if (c >= cout) return;
    const int D = nf + 1, K = nf + 2;
    const double *t = btot + (size_t)c * K;
    const double db = t[nf], dg = t[nf + 1];
    const double N = stats[PT_ST_N], mu = stats[PT_ST_MU + c], inv = stats[PT_ST_INV + c];
    const double a = (double)gamma[c] * inv;
    const float *w = weight + c * nf;
    for (int k = 0; k < nf; ++k) {
        const double sk = stats[pt_tri(k, nf, D)];
        double gw = 0.0;
        for (int j = 0; j < nf; ++j) gw += stats[pt_tri(k, j, D)] * (double)w[j];
        d_weight[c * nf + k] = (float)(a * (t[k] - db / N * sk - dg / N * inv * (gw - mu * sk)));
    }
    d_gamma[c] = (float)dg;
    d_beta[c] = (float)db;
}

static int pt_blocks(int num_voxels) {
    int b = divup(num_voxels, PT_WAVES * 8);          // ~8 voxels per wave
    return b < 1 ? 1 : (b > PT_MAX_BLOCKS ? PT_MAX_BLOCKS : b);
}

static int pt_nf(int num_features, int with_distance) { return num_features + 6 + (with_distance ? 1 : 0); }

LIDAR_EXPORT size_t lidar_pfn_train_workspace_bytes(int num_voxels, int num_features, int cout, int with_distance) {
    const int nf = pt_nf(num_features, with_distance), D = nf + 1;
    const size_t rows = (size_t)max(D * (D + 1) / 2, max(cout, 1) * (nf + 2));
    return align_up((rows * pt_blocks(num_voxels) + (size_t)64 * (nf + 2)) * sizeof(double), 256);
}

static int pt_params(const float *voxel_size3, const float *range6, int max_points, int cout, int coords_are_float, int num_are_float,
                     PfnTrainParams &p) {
    if (!voxel_size3 || !range6) return LIDAR_ERR_ARG;
    p.vx = voxel_size3[0]; p.vy = voxel_size3[1]; p.vz = voxel_size3[2];
    p.xo = p.vx / 2 + range6[0]; p.yo = p.vy / 2 + range6[1]; p.zo = p.vz / 2 + range6[2];
    p.P = max_points; p.cout = cout; p.coords_are_float = coords_are_float; p.num_are_float = num_are_float;
    return LIDAR_OK;
}

static bool pt_args_ok(int num_voxels, int max_points, int num_features, int cout) {
    return num_voxels > 0 && max_points > 0 && max_points <= 64 && num_features >= 3 && num_features <= 8 && cout > 0 && cout <= 64;
}

#define PT_DISPATCH(KERNEL, ...)                                                                                                  \
    switch (num_features * 2 + (with_distance ? 1 : 0)) {                                                                        \
        case 6: hipLaunchKernelGGL((KERNEL<3, false>), __VA_ARGS__); break;                                                       \
        case 7: hipLaunchKernelGGL((KERNEL<3, true>), __VA_ARGS__); break;                                                        \
        case 8: hipLaunchKernelGGL((KERNEL<4, false>), __VA_ARGS__); break;                                                       \
        case 9: hipLaunchKernelGGL((KERNEL<4, true>), __VA_ARGS__); break;                                                        \
        case 10: hipLaunchKernelGGL((KERNEL<5, false>), __VA_ARGS__); break;                                                      \
        case 11: hipLaunchKernelGGL((KERNEL<5, true>), __VA_ARGS__); break;                                                       \
        case 12: hipLaunchKernelGGL((KERNEL<6, false>), __VA_ARGS__); break;                                                      \
        case 13: hipLaunchKernelGGL((KERNEL<6, true>), __VA_ARGS__); break;                                                       \
        case 14: hipLaunchKernelGGL((KERNEL<7, false>), __VA_ARGS__); break;                                                      \
        case 15: hipLaunchKernelGGL((KERNEL<7, true>), __VA_ARGS__); break;                                                       \
        case 16: hipLaunchKernelGGL((KERNEL<8, false>), __VA_ARGS__); break;                                                      \
        case 17: hipLaunchKernelGGL((KERNEL<8, true>), __VA_ARGS__); break;                                                       \
        default: return LIDAR_ERR_ARG;                                                                                            \
    }

LIDAR_EXPORT int lidar_pfn_train_forward(const float *voxels, const void *num_points, const void *coords, int num_voxels,
                                         const int *num_voxels_dev, int max_points, int num_features, const float *weight,
                                         const float *gamma, const float *beta, int cout, float eps, const float *voxel_size3,
                                         const float *range6, int with_distance, int coords_are_float, int num_are_float, float *out,
                                         float *zsel, unsigned char *slot, double *stats, float *scale_shift, float *batch_stats,
                                         void *ws, size_t ws_bytes, void *stream) {
    if (!voxels || !num_points || !coords || !weight || !gamma || !beta || !out || !zsel || !slot || !stats || !scale_shift ||
        !batch_stats || !ws)
        return LIDAR_ERR_ARG;
    if (!pt_args_ok(num_voxels, max_points, num_features, cout)) return LIDAR_ERR_ARG;
    if (ws_bytes < lidar_pfn_train_workspace_bytes(num_voxels, num_features, cout, with_distance)) return LIDAR_ERR_WORKSPACE;
    PfnTrainParams p;
    if (pt_params(voxel_size3, range6, max_points, cout, coords_are_float, num_are_float, p) != LIDAR_OK) return LIDAR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nb = pt_blocks(num_voxels), nf = pt_nf(num_features, with_distance), D = nf + 1;
    double *part = (double *)ws;
    PT_DISPATCH(pfn_train_stats_kernel, dim3(nb), dim3(256), 0, s, voxels, num_points, coords, weight, gamma, num_voxels_dev, num_voxels,
                p, zsel, slot, part)
    hipLaunchKernelGGL(ordered_reduce_kernel, dim3(D * (D + 1) / 2), dim3(256), 0, s, part, nb, stats);
    hipLaunchKernelGGL(pfn_train_finalize_kernel, dim3(1), dim3(64), 0, s, weight, gamma, beta, nf, cout, max_points, eps,
                       num_voxels_dev, num_voxels, stats, scale_shift, batch_stats);
    int ab = divup((long long)num_voxels * cout, 256);
    if (ab > 4096) ab = 4096;
    hipLaunchKernelGGL(pfn_train_apply_kernel, dim3(ab), dim3(256), 0, s, zsel, scale_shift, cout, num_voxels_dev, num_voxels, out);
    return lidar_check_launch("lidar_pfn_train_forward");
}

LIDAR_EXPORT int lidar_pfn_train_backward(const float *voxels, const void *num_points, const void *coords, int num_voxels,
                                          const int *num_voxels_dev, int max_points, int num_features, const float *weight,
                                          const float *gamma, int cout, const float *voxel_size3, const float *range6, int with_distance,
                                          int coords_are_float, int num_are_float, const float *grad_out, const float *zsel,
                                          const unsigned char *slot, const double *stats, const float *scale_shift, float *d_weight,
                                          float *d_gamma, float *d_beta, void *ws, size_t ws_bytes, void *stream) {
    if (!voxels || !num_points || !coords || !weight || !gamma || !grad_out || !zsel || !slot || !stats || !scale_shift || !d_weight ||
        !d_gamma || !d_beta || !ws)
        return LIDAR_ERR_ARG;
    if (!pt_args_ok(num_voxels, max_points, num_features, cout)) return LIDAR_ERR_ARG;
    if (ws_bytes < lidar_pfn_train_workspace_bytes(num_voxels, num_features, cout, with_distance)) return LIDAR_ERR_WORKSPACE;
    PfnTrainParams p;
    if (pt_params(voxel_size3, range6, max_points, cout, coords_are_float, num_are_float, p) != LIDAR_OK) return LIDAR_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int nb = pt_blocks(num_voxels), nf = pt_nf(num_features, with_distance), K = nf + 2, D = nf + 1;
    double *part = (double *)ws;
    double *btot = part + (size_t)max(D * (D + 1) / 2, cout * K) * nb;
    PT_DISPATCH(pfn_train_bwd_kernel, dim3(nb), dim3(256), 0, s, voxels, num_points, coords, grad_out, zsel, slot, scale_shift, stats,
                num_voxels_dev, num_voxels, p, part)
    hipLaunchKernelGGL(ordered_reduce_kernel, dim3(cout * K), dim3(256), 0, s, part, nb, btot);
    hipLaunchKernelGGL(pfn_train_bwd_finalize_kernel, dim3(1), dim3(64), 0, s, btot, stats, weight, gamma, nf, cout, d_weight, d_gamma,
                       d_beta);
    return lidar_check_launch("lidar_pfn_train_backward");
}
#undef PT_DISPATCH

// ------------------------------------------------------------------ PointPillarScatter backward
// d features[v][c] = d canvas at the pillar's cell (the cell rule of scatter_index_kernel in pillar.hip); rows past the device
// count and pillars outside the canvas (x outside [0, nx) or y outside [0, ny) included: the flattened index would alias a cell
// of the neighbouring row) get zero.  channels_last: the gradient has NHWC strides (a cell's channels contiguous).
template <bool NHWC>
__global__ __launch_bounds__(256) void scatter_bwd_kernel(const float *__restrict__ gcanvas, const void *__restrict__ coords,
                                                          int coords_are_float, int nvox_host, const int *__restrict__ nvox_dev, int CH,
                                                          int B, int nx, int ny, float *__restrict__ gfeat) {
    const int nv = nvox_dev ? min(*nvox_dev, nvox_host) : nvox_host;
    const long long total = (long long)nvox_host * CH;
    const long long plane = (long long)nx * ny;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int v = (int)(i / CH), c = (int)(i - (long long)v * CH);
        float g = 0.f;
        if (v < nv) {
            int b, z, y, x;
            if (coords_are_float) {
                const float4 cc = ((const float4 *)coords)[v];
                b = (int)cc.x; z = (int)cc.y; y = (int)cc.z; x = (int)cc.w;
            } else {
                const int4 cc = ((const int4 *)coords)[v];
                b = cc.x; z = cc.y; y = cc.z; x = cc.w;
            }
            const long long cell = ((long long)z * ny + y) * nx + x;
            if (b >= 0 && b < B && x >= 0 && x < nx && y >= 0 && y < ny && cell >= 0 && cell < plane)
                g = NHWC ? gcanvas[((long long)b * plane + cell) * CH + c] : gcanvas[((long long)b * CH + c) * plane + cell];
        }
        gfeat[i] = g;
    }
}

LIDAR_EXPORT int lidar_pillar_scatter_backward(const float *grad_canvas, const void *coords, int coords_are_float, int num_voxels,
                                               const int *num_voxels_dev, int channels, int batch, int nx, int ny, int channels_last,
                                               float *grad_features, void *stream) {
    if (!grad_canvas || !coords || !grad_features) return LIDAR_ERR_ARG;
    if (batch <= 0 || nx <= 0 || ny <= 0 || num_voxels < 0) return LIDAR_ERR_ARG;
    if (channels != 64 && channels != 32 && channels != 128) return LIDAR_ERR_ARG;
    if (num_voxels == 0) return LIDAR_OK;
    hipStream_t s = (hipStream_t)stream;
    int nb = divup((long long)num_voxels * channels, 256);
    if (nb > 8192) nb = 8192;
    if (channels_last)
        hipLaunchKernelGGL(scatter_bwd_kernel<true>, dim3(nb), dim3(256), 0, s, grad_canvas, coords, coords_are_float, num_voxels,
                           num_voxels_dev, channels, batch, nx, ny, grad_features);
    else
        hipLaunchKernelGGL(scatter_bwd_kernel<false>, dim3(nb), dim3(256), 0, s, grad_canvas, coords, coords_are_float, num_voxels,
                           num_voxels_dev, channels, batch, nx, ny, grad_features);
    return lidar_check_launch("lidar_pillar_scatter_backward");
}
