// Second-stage RoI target assignment (ProposalTargetLayer + RoIHeadTemplate.assign_targets) for a whole batch in ONE launch, no host
// read, no atomics on floats, every store a plain vector store.  Reference:
//   pcdet/models/roi_heads/target_assigner/proposal_target_layer.py (forward :13-62, sample_rois_for_rcnn :64-125, subsample_rois
//   :127-172, sample_bg_inds :174-202, get_max_iou_with_same_class :204-238), pcdet/models/roi_heads/roi_head_template.py:101-131
//   (assign_targets), pcdet/ops/iou3d_nms/iou3d_nms_utils.py:48-81 (boxes_iou3d_gpu), pcdet/utils/common_utils.py:34-56
//   (rotate_points_along_z).
//
// One workgroup of 256 threads per frame; everything between the inputs and the outputs lives in LDS:
//   trim     k = M - 1; while k > 0 and row k sums to 0: k -= 1 (:94-97) — the row sum runs left to right in fp32 over ALL columns of
//            the row (class id included, as cur_gt[k].sum() does), on gt_boxes_enlarged when given (:93);
//   overlap  thread = roi (chunks of 256), the frame's kept gts staged 64 at a time (prologue of csrc/iou3d_dev.h per box); the 3D
//            IoU of boxes_iou3d_gpu on top of the shared polygon clipper; running max with the first-index argmax of torch.max
//            (:107, :234) — by class only against gts whose label equals the roi's (:225-236: the class loop runs over
//            [min, max] of the gt labels, which every gt label is in, so "has a gt of my label" is the whole condition);
//   lists    fg / hard bg / easy bg candidates in ascending roi index (nonzero(), :132-135) by ballot compaction;
//   sample   the four cases of :140-169 and the three of :176-200 under the randomness contract below;
//   gather   rois, labels, scores, IoU, gt_of_rois_src = gt[assignment[sampled]] (:111-123), reg_valid_mask and rcnn_cls_labels
//            (:36-55), and the canonical transform of assign_targets (roi_head_template.py:110-129).
//
// Randomness: the kernel draws nothing.  fg_keys (B, R) and draws (B, ROI_PER_IMAGE) in [0, 1) come from the caller:
//   * without-replacement fg choice (np.random.permutation, :144-145): the n_fg candidates with the smallest (key, roi index), in
//     that order (rank by counting: a total order on the key bits, so the ranks are a permutation whatever the keys hold);
//   * every with-replacement pick for output slot s is candidates[min(floor(draws[b, s] * n), n - 1)], the product in fp32.
//
// The reference raises NotImplementedError for a frame that has neither fg nor bg (only NaN overlaps do that, :166-169); here that
// frame's outputs are zeros and frame_status[b] = 1.
//
// Python scalars of the reference (thresholds, pi) are fp32 constants here, as torch casts them before comparing with or adding
// to an fp32 tensor; FG - BG of the roi_iou label and the hard-bg quota int(n * HARD_BG_RATIO) are Python double arithmetic and come
// from the host.  fp32 expressions keep the reference's op order (-ffp-contract=off).
#include "iou3d_dev.h"

#define PT_TPB 256
#define PT_GT_CHUNK 64

struct PTQuota { int q[LIDAR_PROPOSAL_TARGET_MAX_SAMPLES + 1]; };   // hard_quota, by value in the kernel arguments

struct PTParams {
    int R, M, D, P, fg_per_image, by_class, cls_type;
    float reg_fg, cls_fg, cls_bg, cls_bg_lo, fg_thresh, cls_span;
};

struct PTOut {
    float *rois, *gt_of_rois, *gt_of_rois_src, *iou, *scores, *cls_labels, *max_overlaps;
    long long *labels, *reg_valid;
    int *sampled, *status, *gt_assignment;
};

struct PTGtChunk {
    BoxPre pre[PT_GT_CHUNK];
    float zlo[PT_GT_CHUNK], zhi[PT_GT_CHUNK], vol[PT_GT_CHUNK];
    long long label[PT_GT_CHUNK];
};

struct PTPhaseIou {
    VertScratch<PT_TPB> S;
    PTGtChunk g;
};

struct PTPhaseSample {
    unsigned short fg[LIDAR_PROPOSAL_TARGET_MAX_ROIS], hard[LIDAR_PROPOSAL_TARGET_MAX_ROIS], easy[LIDAR_PROPOSAL_TARGET_MAX_ROIS];
    unsigned key[LIDAR_PROPOSAL_TARGET_MAX_ROIS];     // order-preserving bits of the fg candidates' keys, by candidate position
    int sampled[LIDAR_PROPOSAL_TARGET_MAX_SAMPLES];
};

union PTLds {
    PTPhaseIou iou;
    PTPhaseSample smp;
};

// torch's clamp(min=) and max / min propagate NaN; fmaxf / fminf drop it
__device__ __forceinline__ float pt_max(float a, float b) { return (a != a || b != b) ? (a + b) : fmaxf(a, b); }
__device__ __forceinline__ float pt_min(float a, float b) { return (a != a || b != b) ? (a + b) : fminf(a, b); }

// cur_gt[:, -1].long(): truncation toward zero; values a long cannot hold match no roi label
__device__ __forceinline__ long long pt_label_of(float v) {
    if (!(fabsf(v) < 9.0e18f)) return (long long)0x8000000000000000ull;
    return (long long)v;
}

// torch.remainder(x, m), m > 0 (Python's sign convention): fmod, then + m when the signs differ (may round up to m itself)
__device__ __forceinline__ float pt_mod(float x, float m) {
    float r = fmodf(x, m);
    if (r != 0.0f && r < 0.0f) r += m;
    return r;
}

// monotone map of a float to an unsigned: a total order that agrees with < on numbers (-0 counted as +0)
__device__ __forceinline__ unsigned pt_key_bits(float k) {
    const unsigned u = __float_as_uint(k + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// with-replacement pick: min(floor(draw * n), n - 1), never below 0 whatever the draw holds
__device__ __forceinline__ int pt_pick(float draw, int n) {
    const float f = floorf(draw * (float)n);
    int i = (f >= (float)n) ? n - 1 : (int)f;     // NaN compares false and converts to 0
    return min(max(i, 0), n - 1);
}

__global__ __launch_bounds__(PT_TPB) void proposal_target_kernel(const float *__restrict__ rois_all, const float *__restrict__ scores_all,
                                                                 const long long *__restrict__ labels_all,
                                                                 const float *__restrict__ gt_all, const float *__restrict__ gt_enl_all,
                                                                 const float *__restrict__ keys_all, const float *__restrict__ draws_all,
                                                                 PTParams p, PTQuota quota, PTOut o) {
    __shared__ PTLds u;
    __shared__ float s_ov[LIDAR_PROPOSAL_TARGET_MAX_ROIS];
    __shared__ int s_asg[LIDAR_PROPOSAL_TARGET_MAX_ROIS];
    __shared__ int s_red[PT_TPB / 64];
    __shared__ int s_wcnt[3][PT_TPB / 64];
    __shared__ int s_n[3];
    const int b = blockIdx.x, t = threadIdx.x, wv = t >> 6;
    const int R = p.R, M = p.M, D = p.D, P = p.P, G = p.D + 1;
    const float *rois = rois_all + (size_t)b * R * D;
    const float *gt = gt_all + (size_t)b * M * G;                            // gt_of_rois comes from these rows (:116-117)
    const float *gt_iou = (gt_enl_all ? gt_enl_all : gt_all) + (size_t)b * M * G;   // trimmed, matched and labelled from these (:93)
    const long long *roi_labels = labels_all + (size_t)b * R;

    // ---- trim (:94-97): the last row (>= 1) whose sum is not 0, else row 0
    int last = 0;
    for (int r = 1 + t; r < M; r += PT_TPB) {
        const float *row = gt_iou + (size_t)r * G;
        float s = 0.0f;
        for (int q = 0; q < G; ++q) s += row[q];
        if (s != 0.0f) last = r;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) last = max(last, __shfl_xor(last, d, 64));
    if ((t & 63) == 0) s_red[wv] = last;
    __syncthreads();
    const int ngt = max(max(s_red[0], s_red[1]), max(s_red[2], s_red[3])) + 1;

    // ---- max_overlaps, gt_assignment
    for (int r0 = 0; r0 < R; r0 += PT_TPB) {
        const int i = r0 + t;
        const bool valid = i < R;
        const float *rb = rois + (size_t)(valid ? i : 0) * D;
        const BoxPre A = make_pre(rb);
        const float a_zhi = rb[2] + rb[5] / 2, a_zlo = rb[2] - rb[5] / 2;      // iou3d_nms_utils.py:60-61
        const float a_vol = rb[3] * rb[4] * rb[5];                            // :76
        const long long a_label = roi_labels[valid ? i : 0];
        float best = 0.0f;
        int arg = 0;
        bool have = false;
        for (int j0 = 0; j0 < ngt; j0 += PT_GT_CHUNK) {
            const int n = min(PT_GT_CHUNK, ngt - j0);
            __syncthreads();                          // the previous chunk has been read by every thread
            if (t < n) {
                const float *g = gt_iou + (size_t)(j0 + t) * G;
                u.iou.g.pre[t] = make_pre(g);
                u.iou.g.zhi[t] = g[2] + g[5] / 2;
                u.iou.g.zlo[t] = g[2] - g[5] / 2;
                u.iou.g.vol[t] = g[3] * g[4] * g[5];
                u.iou.g.label[t] = pt_label_of(g[G - 1]);
            }
            __syncthreads();
            if (valid) {
                for (int j = 0; j < n; ++j) {
                    if (p.by_class && u.iou.g.label[j] != a_label) continue;
                    const BoxPre B = u.iou.g.pre[j];
                    const float s = circles_apart(A, B) ? 0.0f : box_overlap_pre<PT_TPB>(A, B, u.iou.S, t);
                    const float dz = pt_min(a_zhi, u.iou.g.zhi[j]) - pt_max(a_zlo, u.iou.g.zlo[j]);   // :69-71
                    const float oh = pt_max(dz, 0.0f);
                    const float s3 = s * oh;                                                          // :74
                    const float v = s3 / pt_max(a_vol + u.iou.g.vol[j] - s3, 1e-6f);                  // :79
                    // torch.max over the row: the first maximum; a NaN wins over every number, the first NaN stays
                    if (!have || v > best || (v != v && best == best)) { best = v; arg = j0 + j; have = true; }
                }
            }
        }
        if (valid) {
            s_ov[i] = best;          // no gt of the roi's label: overlap 0, assignment 0 (:222-223)
            s_asg[i] = arg;
            o.max_overlaps[(size_t)b * R + i] = best;
            o.gt_assignment[(size_t)b * R + i] = arg;
        }
    }
    if (t < 3) s_n[t] = 0;
    __syncthreads();                                  // s_ov / s_asg complete; the IoU view of the union is dead from here

    // ---- candidate lists in ascending roi index (:132-135)
    for (int r0 = 0; r0 < R; r0 += PT_TPB) {
        const int i = r0 + t;
        const float ov = i < R ? s_ov[i] : 0.0f;
        const bool in = i < R;
        const bool f0 = in && ov >= p.fg_thresh;
        const bool f1 = in && ov < p.reg_fg && ov >= p.cls_bg_lo;
        const bool f2 = in && ov < p.cls_bg_lo;
        const unsigned long long b0 = __ballot(f0), b1 = __ballot(f1), b2 = __ballot(f2);
        if ((t & 63) == 0) {
            s_wcnt[0][wv] = __popcll(b0);
            s_wcnt[1][wv] = __popcll(b1);
            s_wcnt[2][wv] = __popcll(b2);
        }
        __syncthreads();
        int base0 = s_n[0], base1 = s_n[1], base2 = s_n[2];
        for (int w = 0; w < wv; ++w) {
            base0 += s_wcnt[0][w];
            base1 += s_wcnt[1][w];
            base2 += s_wcnt[2][w];
        }
        const unsigned long long lt = lanemask_lt();
        if (f0) u.smp.fg[base0 + __popcll(b0 & lt)] = (unsigned short)i;
        if (f1) u.smp.hard[base1 + __popcll(b1 & lt)] = (unsigned short)i;
        if (f2) u.smp.easy[base2 + __popcll(b2 & lt)] = (unsigned short)i;
        __syncthreads();
        if (t < 3) s_n[t] += s_wcnt[t][0] + s_wcnt[t][1] + s_wcnt[t][2] + s_wcnt[t][3];
        __syncthreads();
    }
    const int n_fg = s_n[0], n_hard = s_n[1], n_easy = s_n[2], n_bg = n_hard + n_easy;
    const float *draws = draws_all + (size_t)b * P;

    // ---- sampling (:137-171): slots [0, fg_n) fg, [fg_n, fg_n + hard_n) hard bg, the rest easy bg
    const bool failed = n_fg == 0 && n_bg == 0;
    int fg_n = 0, hard_n = 0;
    bool fg_perm = false;
    if (n_fg > 0 && n_bg > 0) { fg_n = min(p.fg_per_image, n_fg); fg_perm = true; }
    else if (n_fg > 0) fg_n = P;                                                  // :153-158
    const int bg_n = P - fg_n;
    if (bg_n > 0 && n_bg > 0) {
        if (n_hard > 0 && n_easy > 0) hard_n = min(quota.q[bg_n], n_hard);         // :176-178
        else if (n_hard > 0) hard_n = bg_n;
    }
    if (fg_perm) {
        const float *keys = keys_all + (size_t)b * R;
        for (int c = t; c < n_fg; c += PT_TPB) u.smp.key[c] = pt_key_bits(keys[u.smp.fg[c]]);
        __syncthreads();
        // rank of candidate c among (key, roi index); the list is ascending in roi index, so ties break by position
        for (int c = t; c < n_fg; c += PT_TPB) {
            const unsigned k = u.smp.key[c];
            int rank = 0;
            for (int e = 0; e < n_fg; ++e) {
                const unsigned ke = u.smp.key[e];
                rank += (ke < k || (ke == k && e < c)) ? 1 : 0;
            }
            if (rank < fg_n) u.smp.sampled[rank] = u.smp.fg[c];
        }
    }
    for (int s = t; s < P; s += PT_TPB) {
        int idx = 0;
        if (failed) idx = 0;
        else if (s < fg_n) {
            if (fg_perm) continue;                                               // written by the ranking above
            idx = u.smp.fg[pt_pick(draws[s], n_fg)];
        } else if (s < fg_n + hard_n) idx = u.smp.hard[pt_pick(draws[s], n_hard)];
        else idx = u.smp.easy[pt_pick(draws[s], n_easy)];
        u.smp.sampled[s] = idx;
    }
    __syncthreads();
    if (t == 0) o.status[b] = failed ? 1 : 0;

    // ---- gather, labels, canonical transform: one output slot per thread
    const float PI_F = 3.14159265358979323846f, TWO_PI_F = 6.28318530717958647692f;
    const float HALF_PI_F = 1.57079632679489661923f, PI_15_F = 4.71238898038468985769f;
    for (int s = t; s < P; s += PT_TPB) {
        const size_t os = (size_t)b * P + s;
        float *orow = o.rois + os * D, *osrc = o.gt_of_rois_src + os * G, *ocan = o.gt_of_rois + os * G;
        if (failed) {
            for (int q = 0; q < D; ++q) orow[q] = 0.0f;
            for (int q = 0; q < G; ++q) { osrc[q] = 0.0f; ocan[q] = 0.0f; }
            o.iou[os] = 0.0f; o.scores[os] = 0.0f; o.cls_labels[os] = 0.0f;
            o.labels[os] = 0; o.reg_valid[os] = 0; o.sampled[os] = 0;
            continue;
        }
        const int idx = u.smp.sampled[s];
        const float ov = s_ov[idx];
        const float *rb = rois + (size_t)idx * D;
        const float *g = gt + (size_t)s_asg[idx] * G;
        for (int q = 0; q < D; ++q) orow[q] = rb[q];
        for (int q = 0; q < G; ++q) osrc[q] = g[q];
        o.iou[os] = ov;
        o.scores[os] = scores_all[(size_t)b * R + idx];
        o.labels[os] = roi_labels[idx];
        o.sampled[os] = idx;
        o.reg_valid[os] = ov > p.reg_fg ? 1 : 0;                                  // :36
        float lab;
        if (p.cls_type == 0) {                                                   // 'cls' (:39-43)
            lab = ov > p.cls_fg ? 1.0f : 0.0f;
            if (ov > p.cls_bg && ov < p.cls_fg) lab = -1.0f;
        } else {                                                                 // 'roi_iou' (:44-53)
            const bool fg = ov > p.cls_fg, bg = ov < p.cls_bg;
            lab = fg ? 1.0f : 0.0f;
            if (!fg && !bg) lab = (ov - p.cls_bg) / p.cls_span;
        }
        o.cls_labels[os] = lab;
        // assign_targets (roi_head_template.py:110-129)
        const float ry = pt_mod(rb[6], TWO_PI_F);                                // :112
        const float x = g[0] - rb[0], y = g[1] - rb[1], z = g[2] - rb[2];        // :113
        const float hd = g[6] - ry;                                              // :114
        // rotate_points_along_z by -ry: [x y z] @ [[c, s, 0], [-s, c, 0], [0, 0, 1]] with c = cos(-ry), s = sin(-ry)
        float cs, sn;
        heading_cs(ry, cs, sn);
        ocan[0] = x * cs + y * sn;
        ocan[1] = y * cs - x * sn;
        ocan[2] = z;
        for (int q = 3; q < G; ++q) ocan[q] = g[q];
        float h = pt_mod(hd, TWO_PI_F);                                          // :122
        if (h > HALF_PI_F && h < PI_15_F) h = pt_mod(h + PI_F, TWO_PI_F);        // :123-124
        if (h > PI_F) h = h - TWO_PI_F;                                          // :125-126
        h = pt_min(pt_max(h, -HALF_PI_F), HALF_PI_F);                            // :127
        ocan[6] = h;
    }
}

LIDAR_EXPORT int lidar_proposal_target_supported(int num_rois, int max_gt, int roi_per_image, int box_dim) {
    return num_rois >= 1 && num_rois <= LIDAR_PROPOSAL_TARGET_MAX_ROIS && max_gt >= 1 && max_gt <= LIDAR_PROPOSAL_TARGET_MAX_GT &&
           roi_per_image >= 1 && roi_per_image <= LIDAR_PROPOSAL_TARGET_MAX_SAMPLES && box_dim >= 7 &&
           box_dim <= LIDAR_PROPOSAL_TARGET_MAX_DIM;
}

LIDAR_EXPORT int lidar_proposal_target(const float *rois, const float *roi_scores, const long long *roi_labels, const float *gt_boxes,
                                       const float *gt_boxes_enlarged, int batch, int num_rois, int max_gt, int box_dim,
                                       int roi_per_image, int fg_rois_per_image, const int *hard_quota, int by_class,
                                       int cls_score_type, float reg_fg_thresh, float cls_fg_thresh, float cls_bg_thresh,
                                       float cls_bg_thresh_lo, float cls_fg_minus_bg, const float *fg_keys, const float *draws,
                                       float *out_rois, float *out_gt_of_rois, float *out_gt_of_rois_src, float *out_iou,
                                       float *out_scores, long long *out_labels, long long *out_reg_valid, float *out_cls_labels,
                                       int *out_sampled, int *frame_status, float *max_overlaps, int *gt_assignment, void *stream) {
    if (batch < 0 || !lidar_proposal_target_supported(num_rois, max_gt, roi_per_image, box_dim)) return LIDAR_ERR_ARG;
    if (fg_rois_per_image < 0 || fg_rois_per_image > roi_per_image || !hard_quota || (cls_score_type != 0 && cls_score_type != 1))
        return LIDAR_ERR_ARG;
    PTQuota quota{};
    for (int n = 0; n <= roi_per_image; ++n) {
        if (hard_quota[n] < 0 || hard_quota[n] > n) return LIDAR_ERR_ARG;
        quota.q[n] = hard_quota[n];
    }
    if (batch == 0) return LIDAR_OK;
    if (!rois || !roi_scores || !roi_labels || !gt_boxes || !fg_keys || !draws || !out_rois || !out_gt_of_rois ||
        !out_gt_of_rois_src || !out_iou || !out_scores || !out_labels || !out_reg_valid || !out_cls_labels || !out_sampled ||
        !frame_status || !max_overlaps || !gt_assignment)
        return LIDAR_ERR_ARG;
    PTParams p{};
    p.R = num_rois; p.M = max_gt; p.D = box_dim; p.P = roi_per_image;
    p.fg_per_image = fg_rois_per_image;
    p.by_class = by_class ? 1 : 0;
    p.cls_type = cls_score_type;
    p.reg_fg = reg_fg_thresh; p.cls_fg = cls_fg_thresh; p.cls_bg = cls_bg_thresh; p.cls_bg_lo = cls_bg_thresh_lo;
    p.fg_thresh = reg_fg_thresh < cls_fg_thresh ? reg_fg_thresh : cls_fg_thresh;      // :130
    p.cls_span = cls_fg_minus_bg;
    PTOut o{out_rois, out_gt_of_rois, out_gt_of_rois_src, out_iou, out_scores, out_cls_labels, max_overlaps,
            out_labels, out_reg_valid, out_sampled, frame_status, gt_assignment};
    hipLaunchKernelGGL(proposal_target_kernel, dim3(batch), dim3(PT_TPB), 0, (hipStream_t)stream, rois, roi_scores, roi_labels,
                       gt_boxes, gt_boxes_enlarged, fg_keys, draws, p, quota, o);
    return lidar_check_launch("lidar_proposal_target");
}
