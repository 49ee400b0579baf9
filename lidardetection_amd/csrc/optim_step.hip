// The tail of a training step in three launches: gradient-norm clip, decoupled weight decay and Adam with the one-cycle momentum,
// over every parameter tensor at once (include/lidar_hip.h "fused optimiser step").
//
// The reference's loop calls clip_grad_norm_(model.parameters(), GRAD_NORM_CLIP) and optimizer.step()
// (tools/train_utils/train_utils.py:36-42); with OPTIMIZER: adam_onecycle the step is fastai's OptimWrapper.step
// (tools/train_utils/optimization/fastai_optim.py:132-149: p.data.mul_(1 - wd * lr) per parameter) and then torch.optim.Adam.
//
// Multi-tensor layout: a device table of LIDAR_OPTIM_ENTRY 64-bit words per tensor (param, grad, exp_avg, exp_avg_sq addresses,
// numel, step lag) and a chunk map that cuts every tensor into LIDAR_OPTIM_CHUNK-element chunks, one 256-thread workgroup per
// chunk, thread i on elements [4i, 4i + 4) of the chunk.  A chunk whose pointers are all 16-byte aligned moves float4s; the last
// (< 4 element) group of a tensor and every chunk of a misaligned tensor take the scalar path.  Both paths give one thread the
// same four elements in the same order, so the norm does not depend on alignment.
//
// Norm: squares and sums in fp64 (an fp32 square is exact there); thread -> wave (xor butterfly) -> workgroup (waves in order) ->
// one workgroup over the chunk partials (strided, then the same tree).  No atomics: bitwise reproducible.
//
// The file is built with -ffp-contract=off: the update evaluates torch's single-tensor Adam expressions as written, without fused
// multiply-adds.
#include "common.h"

#define OPT_CHUNK LIDAR_OPTIM_CHUNK
#define OPT_THREADS 256
#define OPT_ENTRY LIDAR_OPTIM_ENTRY

struct OptEntry {
    float *p;
    float *g;
    float *m;
    float *v;
    long long numel;
    long long lag;
};
static_assert(sizeof(OptEntry) == OPT_ENTRY * sizeof(long long), "table entry layout");

// sum over the workgroup's 256 threads in a fixed order; valid in thread 0
__device__ __forceinline__ double opt_block_sum(double s, double *lds) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane_id() == 0) lds[threadIdx.x >> 6] = s;
    __syncthreads();
    return ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__device__ __forceinline__ bool opt_aligned16(const void *a) { return ((uintptr_t)a & 15) == 0; }

__global__ void __launch_bounds__(OPT_THREADS)
optim_sqsum_chunks_kernel(const OptEntry *__restrict__ table, int n_tensors, const int *__restrict__ chunk_tensor,
                          const int *__restrict__ chunk_index, double *__restrict__ partial) {
    __shared__ double lds[OPT_THREADS / 64];
    const long long c = blockIdx.x;
    const int ti = chunk_tensor[c];
    double s = 0.0;
    if (ti >= 0 && ti < n_tensors) {
        const OptEntry e = table[ti];
        const long long start = (long long)chunk_index[c] * OPT_CHUNK;
        if (e.g != nullptr && start < e.numel) {
            const long long left = e.numel - start;
            const int len = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
            const float *g = e.g + start;
            const int base = 4 * (int)threadIdx.x;
            if (opt_aligned16(g) && base + 4 <= len) {
                const float4 q = *reinterpret_cast<const float4 *>(g + base);
                s = (double)q.x * (double)q.x;
                s += (double)q.y * (double)q.y;
                s += (double)q.z * (double)q.z;
                s += (double)q.w * (double)q.w;
            } else {
                for (int k = 0; k < 4; ++k)
                    if (base + k < len) {
                        const double x = (double)g[base + k];
                        s += x * x;
                    }
            }
        }
    }
    s = opt_block_sum(s, lds);
    if (threadIdx.x == 0) partial[c] = s;
}

// norm_out[0] = total_norm, norm_out[1] = min(1, max_norm / (total_norm + 1e-6)) as torch.nn.utils.clip_grad_norm_ computes it
// (a NaN coefficient stays NaN: torch.clamp(max=1) keeps it)
__global__ void __launch_bounds__(OPT_THREADS)
optim_norm_final_kernel(const double *__restrict__ partial, long long n_chunks, float max_norm, float *__restrict__ norm_out) {
    __shared__ double lds[OPT_THREADS / 64];
    double s = 0.0;
    for (long long i = threadIdx.x; i < n_chunks; i += OPT_THREADS) s += partial[i];
    s = opt_block_sum(s, lds);
    if (threadIdx.x == 0) {
        const float total_norm = (float)sqrt(s);
        const float coef = max_norm / (total_norm + 1e-6f);
        norm_out[0] = total_norm;
        norm_out[1] = coef > 1.0f ? 1.0f : coef;
    }
}

struct OptScalars {
    float decay, w1, beta2, w2, eps, step_size, bc2_sqrt;
    double lr, beta1_d, beta2_d;
    long long t;
    int flags;
};

__device__ __forceinline__ void opt_update(float &p, float &g, float &m, float &v, float coef, const OptScalars &k, float step_size,
                                           float bc2_sqrt) {
    g = coef * g;
    p = p * k.decay;
    m = m + k.w1 * (g - m);                     // exp_avg.lerp_(grad, 1 - beta1)
    v = k.beta2 * v + (k.w2 * g) * g;           // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(v) / bc2_sqrt + k.eps;
    p = p + (-step_size) * (m / denom);         // param.addcdiv_(exp_avg, denom, value=-step_size)
    if (k.flags & LIDAR_OPTIM_ZERO_GRAD) g = 0.0f;
}

__global__ void __launch_bounds__(OPT_THREADS)
optim_adam_chunks_kernel(const OptEntry *__restrict__ table, int n_tensors, const int *__restrict__ chunk_tensor,
                         const int *__restrict__ chunk_index, const float *__restrict__ norm_out, OptScalars k) {
    const long long c = blockIdx.x;
    const int ti = chunk_tensor[c];
    if (ti < 0 || ti >= n_tensors) return;
    const OptEntry e = table[ti];
    const long long start = (long long)chunk_index[c] * OPT_CHUNK;
    if (e.p == nullptr || start >= e.numel) return;
    const long long left = e.numel - start;
    const int len = left < OPT_CHUNK ? (int)left : OPT_CHUNK;
    const int base = 4 * (int)threadIdx.x;
    if (base >= len) return;
    float *p = e.p + start;
    if (e.g == nullptr) {                        // requires_grad but no gradient this step: the decay loop alone touches it
        if (opt_aligned16(p) && base + 4 <= len) {
            float4 q = *reinterpret_cast<float4 *>(p + base);
            q.x *= k.decay, q.y *= k.decay, q.z *= k.decay, q.w *= k.decay;
            *reinterpret_cast<float4 *>(p + base) = q;
        } else {
            for (int j = 0; j < 4; ++j)
                if (base + j < len) p[base + j] *= k.decay;
        }
        return;
    }
    float step_size = k.step_size, bc2_sqrt = k.bc2_sqrt;
    if (e.lag != 0) {                            // this tensor has taken fewer steps than the optimiser (uniform per workgroup)
        const double t = (double)(k.t - e.lag);
        step_size = (float)(k.lr / (1.0 - pow(k.beta1_d, t)));
        bc2_sqrt = (float)sqrt(1.0 - pow(k.beta2_d, t));
    }
    const float coef = norm_out[1];
    float *g = e.g + start, *m = e.m + start, *v = e.v + start;
    if (opt_aligned16(p) && opt_aligned16(g) && opt_aligned16(m) && opt_aligned16(v) && base + 4 <= len) {
        float4 P = *reinterpret_cast<float4 *>(p + base), G = *reinterpret_cast<float4 *>(g + base);
        float4 M = *reinterpret_cast<float4 *>(m + base), V = *reinterpret_cast<float4 *>(v + base);
        opt_update(P.x, G.x, M.x, V.x, coef, k, step_size, bc2_sqrt);
        opt_update(P.y, G.y, M.y, V.y, coef, k, step_size, bc2_sqrt);
        opt_update(P.z, G.z, M.z, V.z, coef, k, step_size, bc2_sqrt);
        opt_update(P.w, G.w, M.w, V.w, coef, k, step_size, bc2_sqrt);
        *reinterpret_cast<float4 *>(p + base) = P;
        *reinterpret_cast<float4 *>(m + base) = M;
        *reinterpret_cast<float4 *>(v + base) = V;
        if (k.flags & (LIDAR_OPTIM_WRITE_CLIPPED | LIDAR_OPTIM_ZERO_GRAD)) *reinterpret_cast<float4 *>(g + base) = G;
    } else {
        for (int j = 0; j < 4; ++j) {
            const int i = base + j;
            if (i >= len) break;
            float P = p[i], G = g[i], M = m[i], V = v[i];
            opt_update(P, G, M, V, coef, k, step_size, bc2_sqrt);
            p[i] = P, m[i] = M, v[i] = V;
            if (k.flags & (LIDAR_OPTIM_WRITE_CLIPPED | LIDAR_OPTIM_ZERO_GRAD)) g[i] = G;
        }
    }
}

// ---------------------------------------------------------------- C ABI
#define OPT_MAX_CHUNKS 0x7fffffffLL

LIDAR_EXPORT long long lidar_optim_plan(const long long *numel, int n_tensors, int *chunk_tensor, int *chunk_index,
                                        long long capacity) {
    if (n_tensors < 0 || (n_tensors > 0 && !numel) || capacity < 0) return LIDAR_ERR_ARG;
    long long total = 0;
    for (int t = 0; t < n_tensors; ++t) {
        if (numel[t] < 0) return LIDAR_ERR_ARG;
        const long long chunks = (numel[t] + OPT_CHUNK - 1) / OPT_CHUNK;
        if (chunks > OPT_MAX_CHUNKS - total) return LIDAR_ERR_ARG;
        if (chunk_tensor && chunk_index)
            for (long long i = 0; i < chunks && total + i < capacity; ++i) {
                chunk_tensor[total + i] = t;
                chunk_index[total + i] = (int)i;
            }
        total += chunks;
    }
    return total;
}

LIDAR_EXPORT size_t lidar_optim_workspace_bytes(long long n_chunks) {
    if (n_chunks <= 0 || n_chunks > OPT_MAX_CHUNKS) return 0;
    return align_up((size_t)n_chunks * sizeof(double), 16);
}

static int opt_check_map(const long long *table, int n_tensors, const int *chunk_tensor, const int *chunk_index,
                         long long n_chunks) {
    if (n_tensors < 0 || n_chunks < 0 || n_chunks > OPT_MAX_CHUNKS) return LIDAR_ERR_ARG;
    if (n_chunks > 0 && (!table || !chunk_tensor || !chunk_index || n_tensors == 0)) return LIDAR_ERR_ARG;
    if (((uintptr_t)table & 7) != 0) return LIDAR_ERR_ARG;
    return LIDAR_OK;
}

LIDAR_EXPORT int lidar_optim_grad_norm(const long long *table, int n_tensors, const int *chunk_tensor, const int *chunk_index,
                                       long long n_chunks, float max_norm, float *norm_out, void *ws, size_t ws_bytes,
                                       void *stream) {
    if (int e = opt_check_map(table, n_tensors, chunk_tensor, chunk_index, n_chunks)) return e;
    if (!norm_out) return LIDAR_ERR_ARG;
    if (n_chunks > 0 && (!ws || ((uintptr_t)ws & 7) != 0)) return LIDAR_ERR_ARG;
    if (ws_bytes < lidar_optim_workspace_bytes(n_chunks)) return LIDAR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    double *partial = (double *)ws;
    if (n_chunks > 0)
        optim_sqsum_chunks_kernel<<<(unsigned)n_chunks, OPT_THREADS, 0, s>>>((const OptEntry *)table, n_tensors, chunk_tensor,
                                                                            chunk_index, partial);
    optim_norm_final_kernel<<<1, OPT_THREADS, 0, s>>>(partial, n_chunks, max_norm, norm_out);
    return lidar_check_launch("lidar_optim_grad_norm");
}

LIDAR_EXPORT int lidar_optim_adam_step(const long long *table, int n_tensors, const int *chunk_tensor, const int *chunk_index,
                                       long long n_chunks, const float *norm_out, double lr, double beta1, double beta2, double eps,
                                       double decay, long long t, int flags, void *stream) {
    if (int e = opt_check_map(table, n_tensors, chunk_tensor, chunk_index, n_chunks)) return e;
    if (!norm_out || t < 1 || flags < 0 || flags > LIDAR_OPTIM_ZERO_GRAD) return LIDAR_ERR_ARG;
    if (n_chunks == 0) return LIDAR_OK;
    OptScalars k;
    k.decay = (float)decay;
    k.w1 = (float)(1.0 - beta1);
    k.beta2 = (float)beta2;
    k.w2 = (float)(1.0 - beta2);
    k.eps = (float)eps;
    k.step_size = (float)(lr / (1.0 - pow(beta1, (double)t)));
    k.bc2_sqrt = (float)sqrt(1.0 - pow(beta2, (double)t));
    k.lr = lr, k.beta1_d = beta1, k.beta2_d = beta2;
    k.t = t;
    k.flags = flags;
    optim_adam_chunks_kernel<<<(unsigned)n_chunks, OPT_THREADS, 0, (hipStream_t)stream>>>((const OptEntry *)table, n_tensors,
                                                                                         chunk_tensor, chunk_index, norm_out, k);
    return lidar_check_launch("lidar_optim_adam_step");
}
