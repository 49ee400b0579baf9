// Train-mode set abstraction (StackSAModuleMSG in grad mode, row-major): the gather of first-layer rows with its backward through an
// inverse index, and the last layer's BatchNorm (batch statistics) + ReLU + max over a ball's samples, forward and backward.
//   reference: pcdet/ops/pointnet2/pointnet2_stack/pointnet2_modules.py:58-92 (StackSAModuleMSG.forward: QueryAndGroup -> 1x1 Conv2d /
//              BatchNorm2d / ReLU -> max_pool2d over the samples), pointnet2_utils.py:104-160 (QueryAndGroup; :146-152 zeroes the
//              groups of empty balls), src/group_points_gpu.cu:15-45 (the grouping gradient, a float atomicAdd per element).
//
// Everything is (rows, H) row-major fp32 with rows = M * nsample and row (m, s) at m * nsample + s ("pair number").  idx (M, nsample)
// is the RAW ball-query result: indices within the query's frame, idx[m][0] < 0 marks an empty ball.
//   (a) z[(m, s)] = table[start_b + idx[m][s]] - query_term[m]; an empty ball's rows are exactly 0 (no bias, no ReLU: BatchNorm
//       follows, and the zero rows take part in its batch statistics as they do in the reference).
//   (b) the inverse index: key[pair] = the global source row (N for a pair that is left out), a stable sort of the keys by the
//       caller, and row_start[n] = the first sorted position whose key is >= n.  No atomics at all.
//   (c) d_table[n] = sum of dz over n's list in list order, d_query[m] = -sum_s dz[m, s] in ascending s; fp64 accumulators, one
//       thread per (row, channel quad), rounded once.  Every row is written.
//   (d) out[m] = max_s relu(z scale + shift) with arg[m] = the lowest s among equal maxima (the maximum is taken over y, so a
//       negative gamma is the minimum of z without a special case); the backward routes grad_out to row (m, arg) where y > 0 (y
//       recomputed bit for bit) and applies the full BatchNorm backward with bn_train.hip's fp64 coefficients.  The (rows, H)
//       post-activation tensor is never written.  The statistics kernels are bn_train_dev.h's, and so are y, delta and dz per quad,
//       the workspace split and the "stats -> reduce -> finalize" / "reduce -> backward finalize" launches.
// No float atomics, no host read: every result is bitwise reproducible.  Supported: H % 4 == 0, 4 <= H <= 128, 1 <= nsample <= 64,
// M * nsample < 2^31, 16-byte aligned pointers; a row index outside the table is treated as an empty slot and never dereferenced.
#include "bn_train_dev.h"

#define SAT_MAX_H 128
#define SAT_MAX_NS 64

// start of query m's frame in the source rows (frames ascending, counts on the device)
__device__ __forceinline__ long long sat_start_of(const int *__restrict__ idx_cnt, const int *__restrict__ feat_cnt, int B, int m) {
    int b = 0, acc = idx_cnt[0];
    for (int k = 1; k < B; ++k) {
        if (m < acc) break;
        acc += idx_cnt[k];
        b = k;
    }
    long long s = 0;
    for (int k = 0; k < b; ++k) s += feat_cnt[k];
    return s;
}

// (a) one block per query
__global__ __launch_bounds__(256) void sat_gather_kernel(int B, int N, int H4, int ns, const float4 *__restrict__ table,
                                                         const float4 *__restrict__ query_term, const int *__restrict__ feat_cnt,
                                                         const int *__restrict__ idx, const int *__restrict__ idx_cnt,
                                                         float4 *__restrict__ z) {
    __shared__ long long s_start;
    const int m = blockIdx.x, t = threadIdx.x;
    if (t == 0) s_start = sat_start_of(idx_cnt, feat_cnt, B, m);
    __syncthreads();
    const long long start = s_start;
    const int *row = idx + (size_t)m * ns;
    const bool empty = row[0] < 0;
    float4 *o = z + (size_t)m * ns * H4;
    for (int e = t; e < ns * H4; e += 256) {
        const int s = e / H4, c = e - s * H4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        const long long r = start + row[s];
        if (!empty && row[s] >= 0 && r < N) {
            v = table[(size_t)r * H4 + c];
            if (query_term) {
                const float4 q = query_term[(size_t)m * H4 + c];
                v.x -= q.x; v.y -= q.y; v.z -= q.z; v.w -= q.w;
            }
        }
        o[e] = v;
    }
}

// (b) pass 1: key of every pair = its global source row, N when the pair is left out (empty ball, or an index outside the table)
__global__ __launch_bounds__(256) void sat_keys_kernel(int B, int N, int ns, long long P, const int *__restrict__ feat_cnt,
                                                       const int *__restrict__ idx, const int *__restrict__ idx_cnt,
                                                       int *__restrict__ keys) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int m = (int)(p / ns);
    int key = N;
    if (idx[(size_t)m * ns] >= 0 && idx[p] >= 0) {
        const long long r = sat_start_of(idx_cnt, feat_cnt, B, m) + idx[p];
        if (r < N) key = (int)r;
    }
    keys[p] = key;
}

// (b) pass 2: sorted keys (ascending, values in [0, N]) -> row_start[n] = first position whose key is >= n, n in [0, N].
// Thread i in [0, P] writes the entries n in (key[i - 1], key[i]] (key[-1] = -1, key[P] = N): every entry exactly once.
__global__ __launch_bounds__(256) void sat_row_start_kernel(long long P, int N, const int *__restrict__ sorted_keys,
                                                            int *__restrict__ row_start) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i > P) return;
    int prev = i == 0 ? -1 : sorted_keys[i - 1];
    int cur = i == P ? N : sorted_keys[i];
    prev = min(max(prev, -1), N);
    cur = min(max(cur, -1), N);
    for (int n = prev + 1; n <= cur; ++n) row_start[n] = (int)i;
}

// (c) d_table: thread (r, q) sums source row n's list in list order.  grid ceil(N / R)
__global__ __launch_bounds__(256) void sat_dtable_kernel(int N, int H, long long P, const float *__restrict__ dz,
                                                         const int *__restrict__ row_start, const int *__restrict__ pairs,
                                                         float *__restrict__ d_table) {
    const BtLane L = bt_lane(H);
    if (!L.live) return;
    const long long n = (long long)blockIdx.x * L.R + L.r;
    if (n >= N) return;
    long long lo = row_start[n], hi = row_start[n + 1];
    lo = lo < 0 ? 0 : lo;
    hi = hi > P ? P : hi;
    const float *src = dz + 4 * L.q;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    long long i = lo;
    for (; i + 3 < hi; i += 4) {                               // four rows in flight, added in list order
        float4 v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long p = pairs[i + u];
            v[u] = (p >= 0 && p < P) ? bt_ld4(src + (size_t)p * H) : make_float4(0.f, 0.f, 0.f, 0.f);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { a0 += v[u].x; a1 += v[u].y; a2 += v[u].z; a3 += v[u].w; }
    }
    for (; i < hi; ++i) {
        const long long p = pairs[i];
        if (p < 0 || p >= P) continue;
        const float4 v = bt_ld4(src + (size_t)p * H);
        a0 += v.x; a1 += v.y; a2 += v.z; a3 += v.w;
    }
    bt_st4(d_table + (size_t)n * H + 4 * L.q, make_float4((float)a0, (float)a1, (float)a2, (float)a3));
}

// (c) d_query: thread (r, q) sums query m's rows in ascending s.  grid ceil(M / R)
__global__ __launch_bounds__(256) void sat_dquery_kernel(int M, int H, int ns, const float *__restrict__ dz,
                                                         const int *__restrict__ idx, float *__restrict__ d_query) {
    const BtLane L = bt_lane(H);
    if (!L.live) return;
    const long long m = (long long)blockIdx.x * L.R + L.r;
    if (m >= M) return;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    if (idx[(size_t)m * ns] >= 0) {
        const float *src = dz + (size_t)m * ns * H + 4 * L.q;
        for (int s = 0; s < ns; ++s) {
            const float4 v = bt_ld4(src + (size_t)s * H);
            a0 -= v.x; a1 -= v.y; a2 -= v.z; a3 -= v.w;
        }
    }
    bt_st4(d_query + (size_t)m * H + 4 * L.q, make_float4((float)a0, (float)a1, (float)a2, (float)a3));
}

// (d) forward: thread (r, q) walks query m's samples.  grid ceil(M / R)
__global__ __launch_bounds__(256) void sat_max_kernel(int M, int H, int ns, const float *__restrict__ z,
                                                      const float *__restrict__ scale_shift, float *__restrict__ out,
                                                      unsigned char *__restrict__ arg) {
    const BtLane L = bt_lane(H);
    if (!L.live) return;
    const long long m = (long long)blockIdx.x * L.R + L.r;
    if (m >= M) return;
    const float4 sc = bt_ld4(scale_shift + 4 * L.q), sh = bt_ld4(scale_shift + H + 4 * L.q);
    const float *src = z + (size_t)m * ns * H + 4 * L.q;
    float4 best = bt_y4(bt_ld4(src), sc, sh);
    uchar4 at = make_uchar4(0, 0, 0, 0);
    for (int s = 1; s < ns; ++s) {                            // strict >: the lowest s among equal maxima stays
        const float4 v = bt_ld4(src + (size_t)s * H);
        const float4 y = bt_y4(v, sc, sh);
        if (y.x > best.x) { best.x = y.x; at.x = (unsigned char)s; }
        if (y.y > best.y) { best.y = y.y; at.y = (unsigned char)s; }
        if (y.z > best.z) { best.z = y.z; at.z = (unsigned char)s; }
        if (y.w > best.w) { best.w = y.w; at.w = (unsigned char)s; }
    }
    bt_st4(out + (size_t)m * H + 4 * L.q, best);
    *reinterpret_cast<uchar4 *>(arg + (size_t)m * H + 4 * L.q) = at;
}

// delta of (m, channel): grad_out where the chosen row's y is positive (the forward's y, bit for bit); zv = z at the chosen row
__device__ __forceinline__ float sat_delta(const float *__restrict__ zrow0, int H, int ns, int c, unsigned a, float g, float sc,
                                           float sh, float &zv) {
    zv = 0.f;
    if (a >= (unsigned)ns) return 0.f;
    zv = zrow0[(size_t)a * H + c];
    return bt_delta(bt_y(zv, sc, sh), g);
}

// (d) backward pass 1: sum delta, sum delta z (fp64) per channel and block; only the M chosen rows of a channel are non-zero
__global__ __launch_bounds__(256) void sat_bwd_stats_kernel(int M, int H, int ns, int nb, const float *__restrict__ z,
                                                            const float *__restrict__ scale_shift, const float *__restrict__ g,
                                                            const unsigned char *__restrict__ arg, double *__restrict__ part) {
    const BtLane L = bt_lane(H);
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (L.live) {
        const int c = 4 * L.q;
        const float4 sc = bt_ld4(scale_shift + c), sh = bt_ld4(scale_shift + H + c);
        const long long step = (long long)nb * L.R;
        for (long long m = (long long)blockIdx.x * L.R + L.r; m < M; m += step) {
            const float4 gv = bt_ld4(g + (size_t)m * H + c);
            const uchar4 at = *reinterpret_cast<const uchar4 *>(arg + (size_t)m * H + c);
            const float *z0 = z + (size_t)m * ns * H;
            float zx, zy, zz, zw;
            const float dx = sat_delta(z0, H, ns, c, at.x, gv.x, sc.x, sh.x, zx), dy = sat_delta(z0, H, ns, c + 1, at.y, gv.y, sc.y, sh.y, zy);
            const float dz = sat_delta(z0, H, ns, c + 2, at.z, gv.z, sc.z, sh.z, zz), dw = sat_delta(z0, H, ns, c + 3, at.w, gv.w, sc.w, sh.w, zw);
            a[0] += dx; a[1] += dy; a[2] += dz; a[3] += dw;
            a[4] += (double)dx * zx; a[5] += (double)dy * zy; a[6] += (double)dz * zz; a[7] += (double)dw * zw;
        }
    }
    bt_block_partials(a, L, H, 0, H, nb, part);
}

// (d) backward pass 3: dz = A (delta - m1 - (z - mu) m2) for every row; thread (r, q) walks query m's samples.  grid ceil(M / R)
__global__ __launch_bounds__(256) void sat_bwd_apply_kernel(int M, int H, int ns, const float *__restrict__ z,
                                                            const float *__restrict__ scale_shift, const double *__restrict__ coef,
                                                            const float *__restrict__ g, const unsigned char *__restrict__ arg,
                                                            float *__restrict__ dzo) {
    const BtLane L = bt_lane(H);
    if (!L.live) return;
    const long long m = (long long)blockIdx.x * L.R + L.r;
    if (m >= M) return;
    const int c = 4 * L.q;
    const float4 sc = bt_ld4(scale_shift + c), sh = bt_ld4(scale_shift + H + c);
    const BtCoef4 k = bt_coef4(coef, H, c);
    const float4 gv = bt_ld4(g + (size_t)m * H + c);
    const uchar4 at = *reinterpret_cast<const uchar4 *>(arg + (size_t)m * H + c);
    const float *src = z + (size_t)m * ns * H + c;
    float *dst = dzo + (size_t)m * ns * H + c;
    for (int s = 0; s < ns; ++s) {
        const float4 v = bt_ld4(src + (size_t)s * H);
        const float4 on = bt_delta4(v, gv, sc, sh);            // delta if this row is the chosen one
        const float4 d = make_float4(s == at.x ? on.x : 0.f, s == at.y ? on.y : 0.f, s == at.z ? on.z : 0.f, s == at.w ? on.w : 0.f);
        bt_st4(dst + (size_t)s * H, bt_dz4(k, d, v));
    }
}

// ---------------------------------------------------------------- host side
LIDAR_EXPORT int lidar_sa_train_supported(int H, int nsample) {
    return H % 4 == 0 && H >= 4 && H <= SAT_MAX_H && nsample >= 1 && nsample <= SAT_MAX_NS;
}

// sizes every entry takes: -> LIDAR_OK, with P = M * nsample
static int sat_sizes(int M, int N, int H, int nsample, long long &P) {
    if (!lidar_sa_train_supported(H, nsample) || M < 0 || N < 0) return LIDAR_ERR_ARG;
    P = (long long)M * nsample;
    return P < (1ll << 31) ? LIDAR_OK : LIDAR_ERR_ARG;
}

static int sat_rows_grid(long long rows, int H) { return divup(rows, 256 / (H / 4)); }

LIDAR_EXPORT int lidar_sa_gather_train_forward(int B, int M, int N, int H, int nsample, const float *table, const float *query_term,
                                               const int *features_batch_cnt, const int *idx, const int *idx_batch_cnt, float *z,
                                               void *stream) {
    long long P;
    if (B <= 0 || sat_sizes(M, N, H, nsample, P) != LIDAR_OK) return LIDAR_ERR_ARG;
    if (M == 0) return LIDAR_OK;
    if ((N > 0 && !bt_aligned(table)) || (query_term && !bt_aligned(query_term)) || !features_batch_cnt || !idx || !idx_batch_cnt ||
        !bt_aligned(z))
        return LIDAR_ERR_ARG;
    hipLaunchKernelGGL(sat_gather_kernel, dim3(M), dim3(256), 0, (hipStream_t)stream, B, N, H / 4, nsample, (const float4 *)table,
                       (const float4 *)query_term, features_batch_cnt, idx, idx_batch_cnt, (float4 *)z);
    return lidar_check_launch("lidar_sa_gather_train_forward");
}

LIDAR_EXPORT int lidar_sa_pair_keys(int B, int M, int N, int nsample, const int *features_batch_cnt, const int *idx,
                                    const int *idx_batch_cnt, int *keys, void *stream) {
    long long P;
    if (B <= 0 || sat_sizes(M, N, 4, nsample, P) != LIDAR_OK) return LIDAR_ERR_ARG;
    if (P == 0) return LIDAR_OK;
    if (!features_batch_cnt || !idx || !idx_batch_cnt || !keys) return LIDAR_ERR_ARG;
    hipLaunchKernelGGL(sat_keys_kernel, dim3(divup(P, 256)), dim3(256), 0, (hipStream_t)stream, B, N, nsample, P, features_batch_cnt,
                       idx, idx_batch_cnt, keys);
    return lidar_check_launch("lidar_sa_pair_keys");
}

LIDAR_EXPORT int lidar_sa_row_start(long long num_pairs, int N, const int *sorted_keys, int *row_start, void *stream) {
    if (num_pairs < 0 || num_pairs >= (1ll << 31) || N < 0 || !row_start || (num_pairs > 0 && !sorted_keys)) return LIDAR_ERR_ARG;
    hipLaunchKernelGGL(sat_row_start_kernel, dim3(divup(num_pairs + 1, 256)), dim3(256), 0, (hipStream_t)stream, num_pairs, N,
                       sorted_keys, row_start);
    return lidar_check_launch("lidar_sa_row_start");
}

LIDAR_EXPORT int lidar_sa_gather_train_backward(int M, int N, int H, int nsample, const float *dz, const int *idx,
                                                const int *row_start, const int *pairs, float *d_table, float *d_query,
                                                void *stream) {
    long long P;
    if (sat_sizes(M, N, H, nsample, P) != LIDAR_OK) return LIDAR_ERR_ARG;
    if (P > 0 && (!bt_aligned(dz) || !idx || !pairs)) return LIDAR_ERR_ARG;
    if (N > 0 && (!row_start || !bt_aligned(d_table))) return LIDAR_ERR_ARG;
    if (d_query && !bt_aligned(d_query)) return LIDAR_ERR_ARG;
    if (N == 0 && (M == 0 || !d_query)) return LIDAR_OK;
    hipStream_t s = (hipStream_t)stream;
    if (N > 0)
        hipLaunchKernelGGL(sat_dtable_kernel, dim3(sat_rows_grid(N, H)), dim3(256), 0, s, N, H, P, dz, row_start, pairs, d_table);
    if (M > 0 && d_query)
        hipLaunchKernelGGL(sat_dquery_kernel, dim3(sat_rows_grid(M, H)), dim3(256), 0, s, M, H, nsample, dz, idx, d_query);
    return lidar_check_launch("lidar_sa_gather_train_backward");
}

LIDAR_EXPORT size_t lidar_bn_relu_max_train_workspace_bytes(int M, int nsample, int H) {
    long long P;
    if (sat_sizes(M, 0, H, nsample, P) != LIDAR_OK) return 0;
    return bt_workspace_bytes(P, H);
}

LIDAR_EXPORT int lidar_bn_relu_max_train_forward(const float *z, int M, int nsample, int H, const float *gamma, const float *beta,
                                                 float eps, float *out, unsigned char *arg, double *stats, float *scale_shift,
                                                 float *batch_stats, void *ws, size_t ws_bytes, void *stream) {
    long long P;
    if (sat_sizes(M, 0, H, nsample, P) != LIDAR_OK || P < 2) return LIDAR_ERR_ARG;
    if (!bt_aligned(z) || !gamma || !beta || !bt_aligned(out) || !bt_aligned(arg) || !stats || !bt_aligned(scale_shift) ||
        !batch_stats || !bt_aligned(ws) || !(eps >= 0.f))
        return LIDAR_ERR_ARG;
    if (ws_bytes < bt_workspace_bytes(P, H)) return LIDAR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    BtSegs S;
    bt_one_seg(z, nullptr, H, H, S);
    bt_launch_stats(S, P, gamma, beta, eps, stats, scale_shift, batch_stats, ws, s);
    hipLaunchKernelGGL(sat_max_kernel, dim3(sat_rows_grid(M, H)), dim3(256), 0, s, M, H, nsample, z, scale_shift, out, arg);
    return lidar_check_launch("lidar_bn_relu_max_train_forward");
}

LIDAR_EXPORT int lidar_bn_relu_max_train_backward(const float *z, int M, int nsample, int H, const float *grad_out,
                                                  const unsigned char *arg, const float *gamma, const double *stats,
                                                  const float *scale_shift, float *dz, float *d_gamma, float *d_beta, void *ws,
                                                  size_t ws_bytes, void *stream) {
    long long P;
    if (sat_sizes(M, 0, H, nsample, P) != LIDAR_OK || P < 2) return LIDAR_ERR_ARG;
    if (!bt_aligned(z) || !bt_aligned(grad_out) || !bt_aligned(arg) || !gamma || !stats || !bt_aligned(scale_shift) || !bt_aligned(dz) ||
        !d_gamma || !d_beta || !bt_aligned(ws))
        return LIDAR_ERR_ARG;
    if (ws_bytes < bt_workspace_bytes(P, H)) return LIDAR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    const int nb = bt_blocks(M);
    const BtWs W = bt_ws_split(ws, H, bt_blocks(P));             // laid out for bt_blocks(P) >= nb partials
    hipLaunchKernelGGL(sat_bwd_stats_kernel, dim3(nb), dim3(256), 0, s, M, H, nsample, nb, z, scale_shift, grad_out, arg, W.part);
    bt_launch_bwd_finalize(W, H, nb, P, gamma, stats, d_gamma, d_beta, s);
    hipLaunchKernelGGL(sat_bwd_apply_kernel, dim3(sat_rows_grid(M, H)), dim3(256), 0, s, M, H, nsample, z, scale_shift, W.coef, grad_out,
                       arg, dz);
    return lidar_check_launch("lidar_bn_relu_max_train_backward");
}
