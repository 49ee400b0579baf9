// KITTI AP evaluation on the device: per-frame overlaps, clean_data's ignore flags, the greedy matcher of compute_statistics_jit in
// both of its modes, get_thresholds and the precision / recall / AOS curves of eval_class
// (pcdet/datasets/kitti/kitti_object_eval_python/eval.py; numba on the CPU plus numba.cuda in the reference).
//
// Rows: every frame's gt and dt boxes stacked, frame f owning rows [off[f], off[f + 1]).  A row is KE_GT_COLS / KE_DT_COLS doubles
// (include/lidar_hip.h).  Frame f's overlap block is (dt_f x gt_f), dt-major, at ov_off[f]: the layout eval_class hands to the matcher.
//
// Mapping.  A matching problem (one frame, one class / difficulty / min_overlap, one score threshold) is a sequential greedy walk, so
// a LANE owns a problem and runs the reference's loops as they are written; the 64 lanes of a wave share the frame:
//   pass 1 (compute_fp False, thresh 0)   lane = configuration (class, difficulty, min_overlap), 64 per wave
//   pass 2 (compute_fp True)              wave = configuration, lane = threshold (at most 41)
// so every lane walks the same overlap block in the same order (uniform addresses, only the predicates diverge).  The per-lane
// "assigned" set of up to KE_MAX_DT dets is a bit mask in LDS, word-major ([word][lane]): a lane touches only its own column, so there
// is no barrier and no bank conflict.  Counts are integers; the similarity is written per (configuration, frame, threshold) and summed
// over frames in frame order in fp64 by ke_curves_kernel: no float atomics, the same bits on every run.
#include "eval_iou_dev.h"

#include <math.h>

// short names of the header's constants (include/lidar_hip.h states the values and the row layouts)
#define KE_MAX_GT LIDAR_KITTI_EVAL_MAX_GT             // gt rows of one frame
#define KE_MAX_DT LIDAR_KITTI_EVAL_MAX_DT             // dt rows of one frame
#define KE_MAX_CLASS LIDAR_KITTI_EVAL_MAX_CLASS
#define KE_MAX_DIFF LIDAR_KITTI_EVAL_MAX_DIFF
#define KE_MAX_OVERLAP LIDAR_KITTI_EVAL_MAX_OVERLAP
#define KE_MAX_FRAMES LIDAR_KITTI_EVAL_MAX_FRAMES
#define KE_MAX_TOTAL_GT LIDAR_KITTI_EVAL_MAX_TOTAL_GT
#define KE_MAX_TOTAL_DT LIDAR_KITTI_EVAL_MAX_TOTAL_DT
#define KE_PTS LIDAR_KITTI_EVAL_PTS                   // N_SAMPLE_PTS
#define KE_GT_COLS LIDAR_KITTI_EVAL_GT_COLS
#define KE_DT_COLS LIDAR_KITTI_EVAL_DT_COLS
#define KE_CLS_DONTCARE LIDAR_KITTI_EVAL_CLS_DONTCARE

namespace {

struct KeCfg {                    // host values handed over in the kernel arguments
    int C, D, K;
    int classes[KE_MAX_CLASS];
    int diffs[KE_MAX_DIFF];
    double min_overlap[KE_MAX_CLASS * KE_MAX_OVERLAP];   // [class slot][overlap row]
};

struct KeFrames {
    const int *gt_off, *dt_off;
    const long long *ov_off;
    long long total_gt, total_dt, ov_total;
    int frames, max_gt, max_dt;
};

struct KeFrame { int g0, ng, d0, nd; long long o0; };

// A frame whose offsets leave the declared totals or per-frame bounds takes no part (it counts as empty): nothing is read or written
// outside the arrays whatever the offsets hold.
__device__ __forceinline__ KeFrame ke_frame(const KeFrames &F, int f) {
    KeFrame r;
    r.g0 = F.gt_off[f];
    r.d0 = F.dt_off[f];
    r.o0 = F.ov_off[f];
    const long long ng = (long long)F.gt_off[f + 1] - r.g0, nd = (long long)F.dt_off[f + 1] - r.d0;
    const bool ok = r.g0 >= 0 && r.d0 >= 0 && r.o0 >= 0 && ng >= 0 && nd >= 0 && ng <= F.max_gt && nd <= F.max_dt &&
                    r.g0 + ng <= F.total_gt && r.d0 + nd <= F.total_dt && r.o0 + ng * nd <= F.ov_total;
    r.ng = ok ? (int)ng : 0;
    r.nd = ok ? (int)nd : 0;
    if (!ok) r.g0 = r.d0 = 0, r.o0 = 0;
    return r;
}

// ---------------------------------------------------------------------------------------------------------------- overlaps
// image_box_overlap (eval.py:86-113) in fp64: b = boxes[n] (the dt role), q = query_boxes[k]
__device__ __forceinline__ double ke_image_overlap(const double *b, const double *q, int criterion) {
    const double qarea = (q[2] - q[0]) * (q[3] - q[1]);
    const double iw = fmin(b[2], q[2]) - fmax(b[0], q[0]);
    if (!(iw > 0)) return 0.0;
    const double ih = fmin(b[3], q[3]) - fmax(b[1], q[1]);
    if (!(ih > 0)) return 0.0;
    double ua;
    if (criterion == -1) ua = (b[2] - b[0]) * (b[3] - b[1]) + qarea - iw * ih;
    else if (criterion == 0) ua = (b[2] - b[0]) * (b[3] - b[1]);
    else if (criterion == 1) ua = qarea;
    else ua = 1.0;
    return iw * ih / ua;
}

// the (x, z, dx, dz, ry) box of calculate_iou_partly (:365-378), rounded to fp32 as rotate_iou_gpu_eval does (rotate_iou.py:308)
__device__ __forceinline__ void ke_bev_box(const double *row, float *rb) {
    rb[0] = (float)row[4];
    rb[1] = (float)row[6];
    rb[2] = (float)row[7];
    rb[3] = (float)row[9];
    rb[4] = (float)row[10];
}

// d3_box_overlap (:150-154): the criterion-2 intersection area rounded to fp32, d3_box_overlap_kernel's arithmetic (:121-147) in
// fp64 on the fp64 boxes, and the result rounded to fp32 again, as the reference stores it in place in the fp32 array
__device__ __forceinline__ float ke_d3_overlap(const double *b, const double *q, int criterion) {
    float rq[5], rb[5];
    ke_bev_box(q, rq);
    ke_bev_box(b, rb);
    const float rinc = ev_rotate_iou(rq, rb, 2);
    if (!(rinc > 0.f)) return rinc;
    const double iw = fmin(b[5], q[5]) - fmax(b[5] - b[8], q[5] - q[8]);
    if (!(iw > 0)) return 0.f;
    const double area1 = b[7] * b[8] * b[9], area2 = q[7] * q[8] * q[9];
    const double inc = iw * (double)rinc;
    double ua;
    if (criterion == -1) ua = area1 + area2 - inc;
    else if (criterion == 0) ua = area1;
    else if (criterion == 1) ua = area2;
    else ua = inc;
    return (float)(inc / ua);
}

__global__ __launch_bounds__(256) void ke_overlaps_kernel(int metric, int criterion, const double *__restrict__ gt,
                                                          const double *__restrict__ dt, KeFrames F, double *__restrict__ out) {
    const KeFrame fr = ke_frame(F, (int)blockIdx.x);
    const long long e = (long long)blockIdx.y * 256 + threadIdx.x;
    if (e >= (long long)fr.nd * fr.ng) return;
    const int j = (int)(e / fr.ng), i = (int)(e - (long long)j * fr.ng);
    const double *b = dt + (size_t)(fr.d0 + j) * KE_DT_COLS, *q = gt + (size_t)(fr.g0 + i) * KE_GT_COLS;
    double r;
    if (metric == 0) r = ke_image_overlap(b, q, criterion);
    else if (metric == 1) {
        float rq[5], rb[5];
        ke_bev_box(q, rq);
        ke_bev_box(b, rb);
        r = (double)ev_rotate_iou(rq, rb, criterion);
    } else r = (double)ke_d3_overlap(b, q, criterion);
    out[fr.o0 + e] = r;
}

// ---------------------------------------------------------------------------------------------------------------- clean_data
// One workgroup per (class slot, difficulty slot): ignored_gt / ignored_dt of every row (:30-83), the valid-gt count, and the fill of
// the pass-1 score slots of its K configurations with -inf (= "this gt emitted no score").
__global__ __launch_bounds__(256) void ke_flags_kernel(KeCfg cfg, const double *__restrict__ gt, const double *__restrict__ dt,
                                                       const int *__restrict__ gt_cls, const int *__restrict__ dt_cls,
                                                       long long total_gt, long long total_dt, signed char *__restrict__ ign_gt,
                                                       signed char *__restrict__ ign_dt, int *__restrict__ num_valid,
                                                       double *__restrict__ matched) {
    const int ml = (int)blockIdx.x, m = ml / cfg.D, l = ml - m * cfg.D;
    const int cur = cfg.classes[m], diff = cfg.diffs[l];
    const double min_height = diff == 0 ? 40.0 : 25.0;                       // MIN_HEIGHT
    const double max_occ = (double)diff;                                      // MAX_OCCLUSION
    const double max_trunc = diff == 0 ? 0.15 : (diff == 1 ? 0.3 : 0.5);      // MAX_TRUNCATION
    __shared__ int s_count[4];
    int count = 0;
    for (long long r = threadIdx.x; r < total_gt; r += 256) {
        const double *g = gt + (size_t)r * KE_GT_COLS;
        const int c = gt_cls[r];
        const double height = g[3] - g[1];
        int valid_class = -1;
        if (c == cur) valid_class = 1;
        else if (cur == 1 && c == 4) valid_class = 0;       // Person_sitting for Pedestrian
        else if (cur == 0 && c == 3) valid_class = 0;       // Van for Car
        const bool ignore = g[12] > max_occ || g[13] > max_trunc || height <= min_height;
        signed char v;
        if (valid_class == 1 && !ignore) { v = 0; ++count; }
        else if (valid_class == 0 || (ignore && valid_class == 1)) v = 1;
        else v = -1;
        ign_gt[(size_t)ml * total_gt + r] = v;
        for (int k = 0; k < cfg.K; ++k) matched[((size_t)ml * cfg.K + k) * total_gt + r] = -INFINITY;
    }
    for (long long r = threadIdx.x; r < total_dt; r += 256) {
        const double *d = dt + (size_t)r * KE_DT_COLS;
        const double height = fabs(d[3] - d[1]);
        ign_dt[(size_t)ml * total_dt + r] = height < min_height ? 1 : (dt_cls[r] == cur ? 0 : -1);   // the height test comes first
    }
    count = wave_sum(count);
    if (lane_id() == 0) s_count[threadIdx.x >> 6] = count;
    __syncthreads();
    if (threadIdx.x == 0) num_valid[ml] = s_count[0] + s_count[1] + s_count[2] + s_count[3];
}

// ---------------------------------------------------------------------------------------------------------------- the matcher
// compute_statistics_jit (:157-275) for one lane.  mask: this lane's column of the LDS bit mask (stride 64 words).
struct KeStat { int tp, fp, fn; double sim; };

template <bool FP>
__device__ __forceinline__ KeStat ke_match(const KeFrame &fr, const double *__restrict__ gt, const double *__restrict__ dt,
                                           const int *__restrict__ gt_cls, const signed char *__restrict__ ign_gt,
                                           const signed char *__restrict__ ign_dt, const double *__restrict__ ov,
                                           const double *__restrict__ dc_ov, double min_overlap, double thresh, bool aos,
                                           unsigned *mask, double *__restrict__ matched) {
    const double NO_DETECTION = -10000000.0;
    KeStat s = {0, 0, 0, 0.0};
    for (int w = 0; w < (fr.nd + 31) / 32; ++w) mask[w * 64] = 0u;
    for (int i = 0; i < fr.ng; ++i) {
        const int ig = ign_gt[i];
        if (ig == -1) continue;
        int det_idx = -1;
        double valid_detection = NO_DETECTION, max_overlap = 0.0;
        bool assigned_ignored_det = false;
        for (int j = 0; j < fr.nd; ++j) {
            const int id = ign_dt[j];
            if (id == -1) continue;
            if (mask[(j >> 5) * 64] >> (j & 31) & 1u) continue;
            const double score = dt[(size_t)j * KE_DT_COLS + 12];
            if (FP && score < thresh) continue;
            const double overlap = ov[(size_t)j * fr.ng + i];
            if (!(overlap > min_overlap)) continue;
            if (!FP) {
                if (score > valid_detection) { det_idx = j; valid_detection = score; }
            } else if ((overlap > max_overlap || assigned_ignored_det) && id == 0) {
                max_overlap = overlap;
                det_idx = j;
                valid_detection = 1.0;
                assigned_ignored_det = false;
            } else if (valid_detection == NO_DETECTION && id == 1) {
                det_idx = j;
                valid_detection = 1.0;
                assigned_ignored_det = true;
            }
        }
        const bool found = valid_detection != NO_DETECTION;
        if (!found) {
            if (ig == 0) ++s.fn;
            continue;
        }
        mask[(det_idx >> 5) * 64] |= 1u << (det_idx & 31);
        if (ig == 1 || ign_dt[det_idx] == 1) continue;          // assigned, but not counted
        ++s.tp;
        if (!FP) matched[i] = dt[(size_t)det_idx * KE_DT_COLS + 12];
        if (FP && aos) s.sim += (1.0 + cos(gt[(size_t)i * KE_GT_COLS + 11] - dt[(size_t)det_idx * KE_DT_COLS + 11])) / 2.0;
    }
    if (FP) {
        for (int j = 0; j < fr.nd; ++j) {
            if (ign_dt[j] != 0 || (mask[(j >> 5) * 64] >> (j & 31) & 1u) || dt[(size_t)j * KE_DT_COLS + 12] < thresh) continue;
            ++s.fp;
            if (!dc_ov) continue;
            // metric 0: a det left over a DontCare box is "stuff", not a false positive (:248-262); each det counts once
            for (int i = 0; i < fr.ng; ++i)
                if (gt_cls[i] == KE_CLS_DONTCARE && dc_ov[(size_t)j * fr.ng + i] > min_overlap) { --s.fp; break; }
        }
        // the reference returns similarity -1 when tp == 0 and fp == 0 and then does not add it: the sum is 0 then anyway
    }
    return s;
}

struct KeData {
    const double *gt, *dt, *ov, *dc_ov;
    const int *gt_cls;
    const signed char *ign_gt, *ign_dt;
};

__global__ __launch_bounds__(64) void ke_pass1_kernel(KeCfg cfg, KeFrames F, KeData d, double *__restrict__ matched) {
    __shared__ unsigned s_mask[(KE_MAX_DT / 32) * 64];
    const KeFrame fr = ke_frame(F, (int)blockIdx.x);
    const int c = (int)blockIdx.y * 64 + lane_id();
    if (c >= cfg.C * cfg.D * cfg.K || fr.ng == 0) return;
    const int ml = c / cfg.K, k = c - ml * cfg.K, m = ml / cfg.D;
    ke_match<false>(fr, d.gt + (size_t)fr.g0 * KE_GT_COLS, d.dt + (size_t)fr.d0 * KE_DT_COLS, d.gt_cls + fr.g0,
                    d.ign_gt + (size_t)ml * F.total_gt + fr.g0, d.ign_dt + (size_t)ml * F.total_dt + fr.d0, d.ov + fr.o0, nullptr,
                    cfg.min_overlap[m * KE_MAX_OVERLAP + k], 0.0, false, s_mask + lane_id(),
                    matched + (size_t)c * F.total_gt + fr.g0);
}

__global__ __launch_bounds__(64) void ke_pass2_kernel(KeCfg cfg, KeFrames F, KeData d, const double *__restrict__ thresholds,
                                                      const int *__restrict__ num_thresholds, int aos, int *__restrict__ part_cnt,
                                                      double *__restrict__ part_sim) {
    __shared__ unsigned s_mask[(KE_MAX_DT / 32) * 64];
    const int f = (int)blockIdx.x, c = (int)blockIdx.y, t = lane_id();
    if (t >= num_thresholds[c]) return;
    const KeFrame fr = ke_frame(F, f);
    const int ml = c / cfg.K, k = c - ml * cfg.K, m = ml / cfg.D;
    const KeStat s = ke_match<true>(fr, d.gt + (size_t)fr.g0 * KE_GT_COLS, d.dt + (size_t)fr.d0 * KE_DT_COLS, d.gt_cls + fr.g0,
                                    d.ign_gt + (size_t)ml * F.total_gt + fr.g0, d.ign_dt + (size_t)ml * F.total_dt + fr.d0,
                                    d.ov + fr.o0, d.dc_ov ? d.dc_ov + fr.o0 : nullptr, cfg.min_overlap[m * KE_MAX_OVERLAP + k],
                                    thresholds[c * KE_PTS + t], aos != 0, s_mask + t, nullptr);
    const size_t o = ((size_t)c * F.frames + f) * KE_PTS + t;
    part_cnt[o * 3] = s.tp;
    part_cnt[o * 3 + 1] = s.fp;
    part_cnt[o * 3 + 2] = s.fn;
    part_sim[o] = s.sim;
}

// ---------------------------------------------------------------------------------------------------------------- get_thresholds
// One workgroup per configuration: its pass-1 scores (one slot per gt row, -inf = none) sorted descending by a bitonic network in
// global memory, then thread 0 runs the reference's sequential scan (:9-27) as written, in fp64.
__global__ __launch_bounds__(1024) void ke_thresholds_kernel(KeCfg cfg, const double *__restrict__ matched, long long total_gt,
                                                             long long padded, const int *__restrict__ num_valid,
                                                             double *__restrict__ sorted, double *__restrict__ thresholds,
                                                             int *__restrict__ num_thresholds) {
    const int c = (int)blockIdx.x;
    double *v = sorted + (size_t)c * padded;
    const double *src = matched + (size_t)c * total_gt;
    __shared__ int s_n[16];
    int n = 0;
    for (long long r = threadIdx.x; r < padded; r += 1024) {
        const double x = r < total_gt ? src[r] : -INFINITY;
        v[r] = x;
        n += x != -INFINITY;
    }
    n = wave_sum(n);
    if (lane_id() == 0) s_n[threadIdx.x >> 6] = n;
    __syncthreads();
    for (long long size = 2; size <= padded; size <<= 1)
        for (long long stride = size >> 1; stride > 0; stride >>= 1) {
            for (long long p = threadIdx.x; p < padded / 2; p += 1024) {
                const long long lo = 2 * p - (p & (stride - 1)), hi = lo + stride;
                const double a = v[lo], b = v[hi];
                const bool desc = (lo & size) == 0;
                if (desc ? a < b : a > b) { v[lo] = b; v[hi] = a; }
            }
            __syncthreads();
        }
    if (threadIdx.x != 0) return;
    n = 0;
    for (int w = 0; w < 16; ++w) n += s_n[w];
    const double num_gt = (double)num_valid[c / cfg.K];
    double current_recall = 0.0;
    int count = 0;
    for (int i = 0; i < n && count < KE_PTS; ++i) {
        const double l_recall = (double)(i + 1) / num_gt;
        const double r_recall = i < n - 1 ? (double)(i + 2) / num_gt : l_recall;
        if ((r_recall - current_recall) < (current_recall - l_recall) && i < n - 1) continue;
        thresholds[c * KE_PTS + count++] = v[i];
        current_recall += 1.0 / (KE_PTS - 1.0);
    }
    for (int i = count; i < KE_PTS; ++i) thresholds[c * KE_PTS + i] = 0.0;
    num_thresholds[c] = count;
}

// ---------------------------------------------------------------------------------------------------------------- curves
// One wave per configuration, lane = threshold: the partials summed over frames in frame order, recall / precision / AOS (:537-541),
// then the running maximum from the right over the first len(thresholds) entries (:542-547; NaN propagates as np.max does).
__device__ __forceinline__ double ke_npmax(double a, double b) { return (isnan(a) || isnan(b)) ? NAN : fmax(a, b); }

__global__ __launch_bounds__(64) void ke_curves_kernel(int frames, int aos, const int *__restrict__ num_thresholds,
                                                       const int *__restrict__ part_cnt, const double *__restrict__ part_sim,
                                                       long long *__restrict__ counts, double *__restrict__ curves, int n_cfg) {
    __shared__ double s_v[3][KE_PTS];
    const int c = (int)blockIdx.x, t = lane_id(), nt = num_thresholds[c];
    long long tp = 0, fp = 0, fn = 0;
    double sim = 0.0;
    if (t < nt)
        for (int f = 0; f < frames; ++f) {
            const size_t o = ((size_t)c * frames + f) * KE_PTS + t;
            tp += part_cnt[o * 3];
            fp += part_cnt[o * 3 + 1];
            fn += part_cnt[o * 3 + 2];
            sim += part_sim[o];
        }
    if (t < KE_PTS) {
        counts[((size_t)c * KE_PTS + t) * 3] = tp;
        counts[((size_t)c * KE_PTS + t) * 3 + 1] = fp;
        counts[((size_t)c * KE_PTS + t) * 3 + 2] = fn;
        s_v[0][t] = t < nt ? (double)tp / ((double)tp + (double)fp) : 0.0;       // precision
        s_v[1][t] = t < nt ? (double)tp / ((double)tp + (double)fn) : 0.0;       // recall
        s_v[2][t] = t < nt && aos ? sim / ((double)tp + (double)fp) : 0.0;       // orientation
    }
    __syncthreads();
    if (t >= KE_PTS) return;
    for (int q = 0; q < 3; ++q) {
        // precision[i] = max(precision[i:]) over ALL 41 entries, for i < len(thresholds): the entries past them are 0
        double v = s_v[q][t];
        if (t < nt)
            for (int u = t + 1; u < KE_PTS; ++u) v = ke_npmax(v, s_v[q][u]);
        curves[((size_t)q * n_cfg + c) * KE_PTS + t] = v;
    }
}

int ke_bounds_ok(int frames, long long total_gt, long long total_dt, int max_gt, int max_dt) {
    return frames >= 0 && frames <= KE_MAX_FRAMES && total_gt >= 0 && total_gt <= KE_MAX_TOTAL_GT && total_dt >= 0 &&
           total_dt <= KE_MAX_TOTAL_DT && max_gt >= 0 && max_gt <= KE_MAX_GT && max_dt >= 0 && max_dt <= KE_MAX_DT;
}

long long ke_pow2(long long n) {
    long long p = 2;
    while (p < n) p <<= 1;
    return p;
}

struct KeWs { signed char *ign_gt, *ign_dt; double *sorted, *part_sim; int *part_cnt; };

size_t ke_ws_layout(int frames, long long total_gt, long long total_dt, int C, int D, int K, KeWs *w, char *base) {
    WsCarve cv{base};
    const size_t ml = (size_t)C * D, n_cfg = ml * K;
    signed char *a = (signed char *)cv.take(ml * (size_t)total_gt);
    signed char *b = (signed char *)cv.take(ml * (size_t)total_dt);
    double *s = (double *)cv.take(n_cfg * (size_t)ke_pow2(total_gt) * sizeof(double));
    double *ps = (double *)cv.take(n_cfg * (size_t)frames * KE_PTS * sizeof(double));
    int *pc = (int *)cv.take(n_cfg * (size_t)frames * KE_PTS * 3 * sizeof(int));
    if (w) *w = KeWs{a, b, s, ps, pc};
    return cv.off;
}

}  // namespace

LIDAR_EXPORT int lidar_kitti_eval_supported(int frames, long long total_gt, long long total_dt, int max_gt, int max_dt,
                                            int num_class, int num_diff, int num_overlap) {
    return ke_bounds_ok(frames, total_gt, total_dt, max_gt, max_dt) && num_class >= 1 && num_class <= KE_MAX_CLASS &&
           num_diff >= 1 && num_diff <= KE_MAX_DIFF && num_overlap >= 1 && num_overlap <= KE_MAX_OVERLAP;
}

LIDAR_EXPORT size_t lidar_kitti_eval_workspace_bytes(int frames, long long total_gt, long long total_dt, int max_gt, int max_dt,
                                                     int num_class, int num_diff, int num_overlap) {
    if (!lidar_kitti_eval_supported(frames, total_gt, total_dt, max_gt, max_dt, num_class, num_diff, num_overlap)) return 0;
    return ke_ws_layout(frames, total_gt, total_dt, num_class, num_diff, num_overlap, nullptr, nullptr);
}

LIDAR_EXPORT int lidar_kitti_eval_overlaps(int metric, int criterion, const double *gt, const double *dt, const int *gt_off,
                                           const int *dt_off, const long long *ov_off, int frames, long long total_gt,
                                           long long total_dt, long long ov_total, int max_gt, int max_dt, double *overlaps,
                                           void *stream) {
    if (metric < 0 || metric > 2 || ov_total < 0) return LIDAR_ERR_ARG;
    if (frames < 0 || total_gt < 0 || total_dt < 0 || max_gt < 0 || max_dt < 0) return LIDAR_ERR_ARG;
    if (!ke_bounds_ok(frames, total_gt, total_dt, max_gt, max_dt)) return LIDAR_ERR_UNSUPPORTED;
    if (frames == 0 || ov_total == 0 || max_gt == 0 || max_dt == 0) return LIDAR_OK;
    if (!gt || !dt || !gt_off || !dt_off || !ov_off || !overlaps) return LIDAR_ERR_ARG;
    const KeFrames F{gt_off, dt_off, ov_off, total_gt, total_dt, ov_total, frames, max_gt, max_dt};
    const dim3 grid((unsigned)frames, (unsigned)divup((long long)max_gt * max_dt, 256));
    hipLaunchKernelGGL(ke_overlaps_kernel, grid, dim3(256), 0, (hipStream_t)stream, metric, criterion, gt, dt, F, overlaps);
    return lidar_check_launch("lidar_kitti_eval_overlaps");
}

LIDAR_EXPORT int lidar_kitti_eval_class(int metric, const double *gt, const double *dt, const int *gt_cls, const int *dt_cls,
                                        const int *gt_off, const int *dt_off, const long long *ov_off, const double *overlaps,
                                        const double *dc_overlaps, int frames, long long total_gt, long long total_dt,
                                        long long ov_total, int max_gt, int max_dt, const int *classes, int num_class,
                                        const int *difficulties, int num_diff, const double *min_overlaps, int num_overlap,
                                        int compute_aos, double *matched, int *num_valid_gt, double *thresholds,
                                        int *num_thresholds, long long *counts, double *curves, void *ws, size_t ws_bytes,
                                        void *stream) {
    if (metric < 0 || metric > 2 || ov_total < 0) return LIDAR_ERR_ARG;
    if (frames < 0 || total_gt < 0 || total_dt < 0 || max_gt < 0 || max_dt < 0) return LIDAR_ERR_ARG;
    if (num_class < 0 || num_diff < 0 || num_overlap < 0 || !classes || !difficulties || !min_overlaps) return LIDAR_ERR_ARG;
    if (!lidar_kitti_eval_supported(frames, total_gt, total_dt, max_gt, max_dt, num_class, num_diff, num_overlap))
        return LIDAR_ERR_UNSUPPORTED;
    KeCfg cfg;
    cfg.C = num_class, cfg.D = num_diff, cfg.K = num_overlap;
    for (int m = 0; m < num_class; ++m) {
        if (classes[m] < 0 || classes[m] > 5) return LIDAR_ERR_ARG;
        cfg.classes[m] = classes[m];
        for (int k = 0; k < num_overlap; ++k) cfg.min_overlap[m * KE_MAX_OVERLAP + k] = min_overlaps[k * num_class + m];
    }
    for (int l = 0; l < num_diff; ++l) {
        if (difficulties[l] < 0 || difficulties[l] > 2) return LIDAR_ERR_ARG;
        cfg.diffs[l] = difficulties[l];
    }
    if (!num_valid_gt || !thresholds || !num_thresholds || !counts || !curves) return LIDAR_ERR_ARG;
    if ((total_gt > 0 && (!gt || !gt_cls || !matched)) || (total_dt > 0 && (!dt || !dt_cls))) return LIDAR_ERR_ARG;
    if (frames > 0 && (!gt_off || !dt_off || !ov_off)) return LIDAR_ERR_ARG;
    if (ov_total > 0 && (!overlaps || (metric == 0 && !dc_overlaps))) return LIDAR_ERR_ARG;
    KeWs w;
    const size_t need = ke_ws_layout(frames, total_gt, total_dt, num_class, num_diff, num_overlap, &w, (char *)ws);
    if (need > 0 && (!ws || ws_bytes < need)) return LIDAR_ERR_WORKSPACE;
    const hipStream_t st = (hipStream_t)stream;
    const int ml = num_class * num_diff, n_cfg = ml * num_overlap;
    const KeFrames F{gt_off, dt_off, ov_off, total_gt, total_dt, ov_total, frames, max_gt, max_dt};
    const KeData d{gt, dt, overlaps, metric == 0 ? dc_overlaps : nullptr, gt_cls, w.ign_gt, w.ign_dt};
    hipLaunchKernelGGL(ke_flags_kernel, dim3(ml), dim3(256), 0, st, cfg, gt, dt, gt_cls, dt_cls, total_gt, total_dt, w.ign_gt,
                       w.ign_dt, num_valid_gt, matched);
    if (frames > 0 && total_gt > 0)
        hipLaunchKernelGGL(ke_pass1_kernel, dim3(frames, divup(n_cfg, 64)), dim3(64), 0, st, cfg, F, d, matched);
    hipLaunchKernelGGL(ke_thresholds_kernel, dim3(n_cfg), dim3(1024), 0, st, cfg, matched, total_gt, ke_pow2(total_gt),
                       num_valid_gt, w.sorted, thresholds, num_thresholds);
    if (frames > 0)
        hipLaunchKernelGGL(ke_pass2_kernel, dim3(frames, n_cfg), dim3(64), 0, st, cfg, F, d, thresholds, num_thresholds,
                           compute_aos, w.part_cnt, w.part_sim);
    hipLaunchKernelGGL(ke_curves_kernel, dim3(n_cfg), dim3(64), 0, st, frames, compute_aos, num_thresholds, w.part_cnt,
                       w.part_sim, counts, curves, n_cfg);
    return lidar_check_launch("lidar_kitti_eval_class");
}
