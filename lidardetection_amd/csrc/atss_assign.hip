// ATSS anchor target assignment (ATSSTargetAssigner) for a whole batch and every anchor set in one call, no host
// synchronisation.  Reference: pcdet/models/dense_heads/target_assigner/atss_target_assigner.py (assign_targets :16-73,
// assign_targets_single :75-141); rotated IoU pcdet/ops/iou3d_nms/iou3d_nms_utils.py:31-81 on the polygon clipper of
// csrc/iou3d_dev.h; rotate_points_along_z pcdet/utils/common_utils.py:66-88; ResidualCoder.encode_torch csrc/box_encode_dev.h.
//
//   zero     one bandwidth-bound launch clears the three outputs;
//   select   (one workgroup per frame, set and gt)  streams the set's anchors once: keeps the TOPK smallest 64-bit keys
//            (distance bits << 32 | anchor index) and the gt's IoU argmax over the whole set (the N x M matrices of :89-93 are
//            never stored; the rotated overlap is evaluated only for pairs that circles_apart / sat_separated do not reject,
//            whose overlap is exactly 0 in the reference too), then the candidates' IoUs, the gt's mean + std threshold
//            (:96-99) and the centre-in-box test (:102-111).  It leaves TOPK + 1 (anchor, priority) entries per gt;
//   resolve  (one workgroup per frame and set)  an entry wins its anchor when no other entry of the same anchor has a larger
//            priority; the winners write label, encoded targets and weight (:116-139).  Every anchor has one winner at most.
//
// The trailing-padding trim (:41-44) is recomputed by every workgroup of the frame with anchor_assign_prep_kernel's rule and
// summation order (left to right over the box columns): no prep launch, no count in the workspace.
//
// Ties, which the reference leaves to torch's kernels, are fixed here: top-k by ascending (distance, anchor index); an anchor
// positive for several gts takes the largest IoU, then the lowest gt; a gt's argmax over the set is the lowest anchor index (so
// a gt that overlaps nothing forces anchor 0, :126-128); of several gts forcing one anchor the highest gt wins (the sequential
// scatter of :127).  Priorities are unique per anchor, integer compares only: bitwise reproducible.
#include "common.h"
#include "box_encode_dev.h"
#include "iou3d_dev.h"
#include <math.h>

#define AT_MAX_SETS 16
#define AT_MAX_TOPK 32
#define AT_MAX_GT 256
#define AT_MAX_CODE 16
#define AT_MAX_ANCHORS (1ll << 30)   // per set: anchor indices and the scan's loop counter are 32-bit
#define AT_TPB 256
#define AT_PER_THREAD 4
#define AT_CHUNK (AT_TPB * AT_PER_THREAD)
#define AT_MAX_ENTRIES (AT_MAX_GT * (AT_MAX_TOPK + 1))

typedef unsigned long long at_u64;

struct ATSet {
    const float *anchors;   // (n, anchor_dim) DEVICE, output order
    long long out_off;      // first output anchor of the set inside a frame
    int n;
};

struct ATParams {
    ATSet set[AT_MAX_SETS];
    int nsets, anchor_dim, gt_cols, code_size, sincos, topk, match_height, batch, max_gt;
    long long n_total;
};

// workspace: per (frame, set, gt) TOPK candidate entries and one forced entry
struct ATWs {
    int *ent_anchor;     // (B, K, M, topk + 1)   anchor index, -1: not a positive candidate
    at_u64 *ent_key;     // (B, K, M, topk + 1)   priority: positive (iou bits << 32 | ~gt), forced (1 << 63 | gt)
};

static inline size_t at_ws_layout(int B, int M, int K, int topk, ATWs *w, char *base) {
    const size_t ents = (size_t)B * K * M * (topk + 1);
    const size_t key_off = align_up(sizeof(int) * ents, 256);
    if (w) {
        w->ent_anchor = (int *)base;
        w->ent_key = (at_u64 *)(base + key_off);
    }
    return key_off + align_up(sizeof(at_u64) * ents, 256);
}

// :41-44: the last row (>= 1) whose box columns do not sum to 0, else row 0 -> number of kept rows.  s_red: AT_TPB / 64 ints.
__device__ __forceinline__ int at_trim(const float *fgt, int M, int gt_cols, int *s_red) {
    const int t = threadIdx.x, D = gt_cols - 1;
    int last = 0;
    for (int r = 1 + t; r < M; r += AT_TPB) {
        const float *row = fgt + (size_t)r * gt_cols;
        float s = 0.0f;
        for (int q = 0; q < D; ++q) s += row[q];
        if (s != 0.0f) last = r;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) last = max(last, __shfl_xor(last, d, 64));
    if ((t & 63) == 0) s_red[t >> 6] = last;
    __syncthreads();
    int m = s_red[0];
#pragma unroll
    for (int k = 1; k < AT_TPB / 64; ++k) m = max(m, s_red[k]);
    return m + 1;
}

struct ATGt {
    BoxPre pre;
    float zlo, zhi, vol;
};

// boxes_iou_bev (iou3d_nms_utils.py:31-45) or boxes_iou3d_gpu (:48-81) of (anchor, gt); A = make_pre(a)
__device__ __forceinline__ float at_iou(const BoxPre &A, const float *a, const ATGt &G, int match_height, VertScratch<AT_TPB> &S,
                                        int t) {
    const float s = sat_separated(A, G.pre) ? 0.0f : box_overlap_pre<AT_TPB>(A, G.pre, S, t);
    if (!match_height) return iou_from_overlap(A.area, G.pre.area, s);
    const float a_zhi = a[2] + a[5] / 2, a_zlo = a[2] - a[5] / 2;
    const float oh = fmaxf(fminf(a_zhi, G.zhi) - fmaxf(a_zlo, G.zlo), 0.0f);
    const float s3 = s * oh;
    return s3 / fmaxf(a[3] * a[4] * a[5] + G.vol - s3, 1e-6f);
}

__device__ __forceinline__ at_u64 at_shfl_xor(at_u64 v, int d) {
    const unsigned lo = __shfl_xor((unsigned)v, d, 64), hi = __shfl_xor((unsigned)(v >> 32), d, 64);
    return ((at_u64)hi << 32) | lo;
}
__device__ __forceinline__ at_u64 at_shfl_up1(at_u64 v) {
    const unsigned lo = __shfl_up((unsigned)v, 1, 64), hi = __shfl_up((unsigned)(v >> 32), 1, 64);
    return ((at_u64)hi << 32) | lo;
}

// ---------------------------------------------------------------- zero: labels, targets and weights as one run of 32-bit words
__global__ __launch_bounds__(AT_TPB) void atss_zero_kernel(unsigned *__restrict__ labels, unsigned *__restrict__ targets,
                                                           unsigned *__restrict__ weights, size_t cells, size_t target_words) {
    const size_t total = 2 * cells + target_words, stride = (size_t)gridDim.x * AT_TPB;
    for (size_t i = (size_t)blockIdx.x * AT_TPB + threadIdx.x; i < total; i += stride) {
        if (i < target_words) targets[i] = 0u;
        else if (i < target_words + cells) labels[i - target_words] = 0u;
        else weights[i - target_words - cells] = 0u;
    }
}

// ---------------------------------------------------------------- select: one workgroup per (frame, set, gt)
__global__ __launch_bounds__(AT_TPB) void atss_select_kernel(ATParams p, ATWs w, const float *__restrict__ gt) {
    __shared__ VertScratch<AT_TPB> S;
    __shared__ at_u64 s_queue[AT_CHUNK];
    __shared__ at_u64 s_kth, s_best[AT_TPB / 64];
    __shared__ int s_qn, s_red[AT_TPB / 64];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, M = p.max_gt, topk = p.topk;
    const int j = blockIdx.x % M, k = (blockIdx.x / M) % p.nsets, b = blockIdx.x / (M * p.nsets);
    const float *fgt = gt + (size_t)b * M * p.gt_cols;
    if (t == 0) { s_kth = ~0ull; s_qn = 0; }
    const int cnt = at_trim(fgt, M, p.gt_cols, s_red);   // its barrier also publishes s_kth / s_qn
    if (j >= cnt) return;                                 // trimmed padding: the resolve pass never reads these entries
    const ATSet &set = p.set[k];
    const float *g = fgt + (size_t)j * p.gt_cols;
    ATGt G;
    G.pre = make_pre(g);
    G.zhi = g[2] + g[5] / 2;
    G.zlo = g[2] - g[5] / 2;
    G.vol = g[3] * g[4] * g[5];
    const float gx = g[0], gy = g[1], gz = g[2];
    const int n = set.n, D = p.anchor_dim;

    at_u64 top = ~0ull;                          // wave 0, lane l < topk: the l-th smallest key so far, ascending
    at_u64 best = 0xffffffffull;                 // iou bits << 32 | ~anchor index: iou 0 at anchor 0 unless something overlaps
    for (int c0 = 0; c0 < n; c0 += AT_CHUNK) {
        const at_u64 kth = s_kth;
        for (int r = 0; r < AT_PER_THREAD; ++r) {
            const int i = c0 + r * AT_TPB + t;
            if (i >= n) continue;
            const float *a = set.anchors + (size_t)i * D;
            const float ax = a[0], ay = a[1];
            const float dx = ax - gx, dy = ay - gy, dz = a[2] - gz;
            const float d2 = dx * dx + dy * dy;
            const float dist = sqrtf(d2 + dz * dz);                       // (a.xyz - g.xyz).norm(), :93
            const at_u64 key = ((at_u64)__float_as_uint(dist) << 32) | (unsigned)i;
            if (key < kth) s_queue[atomicAdd(&s_qn, 1)] = key;            // order in the queue is free: the kept SET is not
            // circles_apart(A, G) without A's trigonometry: the same expressions as make_pre / circles_apart
            const float hx = a[3] / 2, hy = a[4] / 2;
            const float rr = (sqrtf(hx * hx + hy * hy) * 1.0001f + 0.02f) + G.pre.rad;
            if (d2 > rr * rr) continue;
            const BoxPre A = make_pre(a);
            const float v = at_iou(A, a, G, p.match_height, S, t);
            if (v > 0.0f) {
                const at_u64 bk = ((at_u64)__float_as_uint(v) << 32) | (0xffffffffu - (unsigned)i);
                best = bk > best ? bk : best;
            }
        }
        __syncthreads();
        if (wv == 0) {
            const int qn = s_qn;
            for (int q = 0; q < qn; ++q) {
                const at_u64 x = s_queue[q];
                const int pos = __popcll(__ballot(lane < topk && top < x));
                if (pos < topk) {
                    const at_u64 up = at_shfl_up1(top);
                    if (lane == pos) top = x;
                    else if (lane > pos && lane < topk) top = up;
                }
            }
            if (lane == topk - 1) s_kth = top;
            if (lane == 0) s_qn = 0;
        }
        __syncthreads();
    }
    // the gt's argmax over the set (:126): largest IoU, lowest anchor index
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const at_u64 o = at_shfl_xor(best, d);
        best = o > best ? o : best;
    }
    if (lane == 0) s_best[wv] = best;
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int q = 1; q < AT_TPB / 64; ++q) best = s_best[q] > best ? s_best[q] : best;
    const int forced = (int)(0xffffffffu - (unsigned)(best & 0xffffffffull));

    // candidates (n >= topk: every slot is filled): IoU, centre inside the gt in BEV (:102-111)
    const bool cand = lane < topk;
    const int ci = cand ? (int)min((unsigned)(top & 0xffffffffull), (unsigned)(n - 1)) : 0;
    float iou = 0.0f;
    bool inside = false;
    if (cand) {
        const float *a = set.anchors + (size_t)ci * D;
        const BoxPre A = make_pre(a);
        iou = circles_apart(A, G.pre) ? 0.0f : at_iou(A, a, G, p.match_height, S, t);
        // rotate_points_along_z(a.xyz - g.xyz, -heading): cos(-h) == cos(h), sin(-h) == -sin(h) bit for bit
        const float lx = a[0] - gx, ly = a[1] - gy;
        const float rx = lx * G.pre.c + ly * G.pre.s, ry = lx * (-G.pre.s) + ly * G.pre.c;
        // the reference compares (x, y) with gt[3:5][[1, 0]] / 2 = (dy / 2, dx / 2) (:109-110)
        inside = rx <= G.pre.hy && rx >= -G.pre.hy && ry <= G.pre.hx && ry >= -G.pre.hx;
    }
    float sum = 0.0f;
    for (int l = 0; l < topk; ++l) sum += __shfl(iou, l, 64);
    const float mean = sum / (float)topk;
    float ss = 0.0f;
    for (int l = 0; l < topk; ++l) {
        const float dv = __shfl(iou, l, 64) - mean;
        ss += dv * dv;
    }
    const float thresh = (mean + sqrtf(ss / (float)(topk - 1))) + 1e-6f;     // :96-98, unbiased std
    const size_t base = (((size_t)b * p.nsets + k) * M + j) * (topk + 1);
    if (cand) {
        const bool pos = iou >= thresh && inside;
        w.ent_anchor[base + lane] = pos ? ci : -1;
        w.ent_key[base + lane] = pos ? (((at_u64)__float_as_uint(iou) << 32) | (0xffffffffu - (unsigned)j)) : 0ull;
    }
    if (lane == 0) {
        w.ent_anchor[base + topk] = forced;
        w.ent_key[base + topk] = (1ull << 63) | (unsigned)j;
    }
}

// ---------------------------------------------------------------- resolve: one workgroup per (frame, set)
__global__ __launch_bounds__(AT_TPB) void atss_resolve_kernel(ATParams p, ATWs w, const float *__restrict__ gt,
                                                              int *__restrict__ labels, float *__restrict__ targets,
                                                              float *__restrict__ weights) {
    __shared__ int s_anchor[AT_MAX_ENTRIES];
    __shared__ int s_red[AT_TPB / 64];
    const int t = threadIdx.x, M = p.max_gt, per = p.topk + 1;
    const int k = blockIdx.x % p.nsets, b = blockIdx.x / p.nsets;
    const float *fgt = gt + (size_t)b * M * p.gt_cols;
    const int cnt = at_trim(fgt, M, p.gt_cols, s_red);
    const int E = cnt * per;
    const size_t base = ((size_t)b * p.nsets + k) * M * per;
    for (int e = t; e < E; e += AT_TPB) s_anchor[e] = w.ent_anchor[base + e];
    __syncthreads();
    const ATSet &set = p.set[k];
    for (int e = t; e < E; e += AT_TPB) {
        const int a = s_anchor[e];
        if (a < 0) continue;
        const at_u64 key = w.ent_key[base + e];
        bool win = true;
        for (int f = 0; f < E; ++f)
            if (s_anchor[f] == a && w.ent_key[base + f] > key) { win = false; break; }
        if (!win) continue;
        const float *g = fgt + (size_t)(e / per) * p.gt_cols;
        const int label = (int)g[p.gt_cols - 1];                            // gt_classes[anchors_to_gt_indexs], :130
        const size_t o = (size_t)b * p.n_total + set.out_off + a;
        labels[o] = label;
        if (label > 0) {                                                    // pos_mask, :134-139
            float code[AT_MAX_CODE];
            residual_encode(g, set.anchors + (size_t)a * p.anchor_dim, code, p.sincos, p.code_size);
            for (int q = 0; q < p.code_size; ++q) targets[o * p.code_size + q] = code[q];
            weights[o] = 1.0f;
        }
    }
}

LIDAR_EXPORT int lidar_atss_assign_supported(const long long *counts, int num_sets, int anchor_dim, int gt_cols, int code_size,
                                             int sincos, int topk, int max_gt, int match_height) {
    if (!counts || num_sets < 1 || num_sets > AT_MAX_SETS || anchor_dim < 7 || gt_cols < 8) return 0;
    if (topk < 2 || topk > AT_MAX_TOPK || max_gt < 1 || max_gt > AT_MAX_GT) return 0;
    if ((sincos != 0 && sincos != 1) || (match_height != 0 && match_height != 1)) return 0;
    const int extra = min(anchor_dim - 7, gt_cols - 1 - 7);
    if (code_size != 6 + (sincos ? 2 : 1) + extra || code_size > AT_MAX_CODE) return 0;
    for (int k = 0; k < num_sets; ++k)
        if (counts[k] < topk || counts[k] > AT_MAX_ANCHORS) return 0;
    return 1;
}

LIDAR_EXPORT size_t lidar_atss_assign_workspace_bytes(int batch, int max_gt, int num_sets, int topk) {
    if (batch <= 0 || max_gt < 1 || max_gt > AT_MAX_GT || num_sets < 1 || num_sets > AT_MAX_SETS || topk < 2 || topk > AT_MAX_TOPK)
        return 0;
    return at_ws_layout(batch, max_gt, num_sets, topk, nullptr, nullptr);
}

LIDAR_EXPORT int lidar_atss_assign(const float *const *anchors, const long long *counts, int num_sets, int anchor_dim,
                                   const float *gt, int batch, int max_gt, int gt_cols, int code_size, int sincos, int topk,
                                   int match_height, int *labels, float *targets, float *weights, void *ws, size_t ws_bytes,
                                   void *stream) {
    if (!anchors || batch < 0 ||
        !lidar_atss_assign_supported(counts, num_sets, anchor_dim, gt_cols, code_size, sincos, topk, max_gt, match_height))
        return LIDAR_ERR_ARG;
    ATParams p{};
    long long n_total = 0;
    for (int k = 0; k < num_sets; ++k) {
        if (!anchors[k]) return LIDAR_ERR_ARG;
        p.set[k] = ATSet{anchors[k], n_total, (int)counts[k]};
        n_total += counts[k];
    }
    if (batch == 0) return LIDAR_OK;
    if ((long long)batch * num_sets * max_gt > 0x7fffffffll) return LIDAR_ERR_ARG;   // the select grid
    if (!gt || !labels || !targets || !weights || !ws) return LIDAR_ERR_ARG;
    ATWs w;
    if (ws_bytes < at_ws_layout(batch, max_gt, num_sets, topk, &w, (char *)ws)) return LIDAR_ERR_WORKSPACE;
    p.nsets = num_sets;
    p.anchor_dim = anchor_dim;
    p.gt_cols = gt_cols;
    p.code_size = code_size;
    p.sincos = sincos;
    p.topk = topk;
    p.match_height = match_height;
    p.batch = batch;
    p.max_gt = max_gt;
    p.n_total = n_total;
    hipStream_t st = (hipStream_t)stream;
    const size_t cells = (size_t)batch * (size_t)n_total;
    const size_t words = cells * (code_size + 2);
    const unsigned zero_grid = (unsigned)min((words + AT_TPB * 8 - 1) / (AT_TPB * 8), (size_t)(256 * 64));
    hipLaunchKernelGGL(atss_zero_kernel, dim3(zero_grid), dim3(AT_TPB), 0, st, (unsigned *)labels, (unsigned *)targets,
                       (unsigned *)weights, cells, cells * code_size);
    hipLaunchKernelGGL(atss_select_kernel, dim3((unsigned)(batch * num_sets * max_gt)), dim3(AT_TPB), 0, st, p, w, gt);
    hipLaunchKernelGGL(atss_resolve_kernel, dim3((unsigned)(batch * num_sets)), dim3(AT_TPB), 0, st, p, w, gt, labels, targets,
                       weights);
    return lidar_check_launch("lidar_atss_assign");
}
