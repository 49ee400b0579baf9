// Anchor target assignment (AxisAlignedTargetAssigner, deterministic path) for a whole batch and every anchor class in three
// launches, no host synchronisation.  Reference: pcdet/models/dense_heads/target_assigner/axis_aligned_target_assigner.py
// (assign_targets :37-129, assign_targets_single :131-210) with POS_FRACTION < 0 and MATCH_HEIGHT False; nearest-BEV IoU
// pcdet/utils/box_utils.py:238-287; limit_period pcdet/utils/common_utils.py:52-55; ResidualCoder.encode_torch
// pcdet/utils/box_coder_utils.py:13-42.
//
//   prep   (one wave per frame)  trims the frame's trailing padding rows (:54-57), groups the surviving gts per anchor class in
//          their original order (the class mask of :61-66), precomputes each gt's axis-aligned BEV box and area, and zeroes the
//          per-gt max slots;
//   gtmax  (anchor tile x frame group)  the IoU of every anchor against the gts of its class, per-gt max over the tile folded
//          into the workspace with an integer atomicMax on the float bits (IoU >= 0: order-independent, deterministic);
//   assign (same tiles)  recomputes the IoU row with the same device function (the N x M matrix is never stored), takes the max
//          and the first-index argmax (numpy argmax, :150), the force flag (:153-158), the label (:160-190), the encoded
//          targets of gt[argmax] (:192-199) and the regression weight (:201-207); every output element is written exactly once.
//   norm   (NORM_BY_NUM_EXAMPLES only)  reg_weights = 1 / max(#labels >= 0, 1) of the (frame, class) for labels > 0.
//
// fp32 expressions keep the reference's op order (the library builds with -ffp-contract=off); the reference's Python scalars
// (pi, pi/4, the thresholds, 1e-6, 1e-5) are fp32 constants, as torch casts them before comparing or dividing.
#include "common.h"
#include "box_encode_dev.h"
#include <math.h>

#define AA_MAX_CLASSES 16
#define AA_ID_MIN (-64)   // gt class ids AA_ID_MIN .. -AA_ID_MIN - 1 have a table entry
#define AA_NUM_IDS 128
#define AA_MAX_CODE 16
#define AA_TILE 256
#define AA_CHUNK 256

struct AAClass {
    const float *anchors;   // (n, anchor_dim) DEVICE
    long long n;            // anchors of this class
    long long per_loc;      // anchors per output location (single head: R_c; multihead: n)
    long long out_off;      // offset inside a location (single head) / of the class's block (multihead)
    int tile_start;         // first anchor tile of this class in the flattened tile space
    int remap;              // > 0: every label of this class is this id (SEPERATE_MULTIHEAD); else the gt's own class id
    float matched, unmatched;
};

struct AAParams {
    AAClass cls[AA_MAX_CLASSES];
    signed char class_of_id[AA_NUM_IDS];   // gt class id - AA_ID_MIN -> anchor class index, -1: none
    int ncls, tiles_total, anchor_dim, gt_cols, code_size, sincos, frames_per_block, batch, max_gt;
    long long n_total, a_total;            // anchors per frame; output anchors per location (single head)
};

// workspace views (all sized by max_gt M per frame)
struct AAWs {
    int *cls_start;          // (B, ncls + 1) slot prefix per class inside a frame
    int *num_examples;       // (B, ncls)
    float4 *bev;             // (B, M) x1, y1, x2, y2 by slot
    float *area;             // (B, M)
    int *gt_row;             // (B, M) original row of the slot
    int *label;              // (B, M) label value of the slot
    unsigned *gtmax;         // (B, M) float bits of the per-gt max IoU over the class's anchors
};

static inline size_t aa_ws_layout(int B, int M, int ncls, AAWs *w, char *base) {
    WsCarve c{base};
    char *p;
    p = c.take(sizeof(int) * (size_t)B * (ncls + 1)); if (w) w->cls_start = (int *)p;
    p = c.take(sizeof(int) * (size_t)B * ncls);       if (w) w->num_examples = (int *)p;
    p = c.take(sizeof(float4) * (size_t)B * M);       if (w) w->bev = (float4 *)p;
    p = c.take(sizeof(float) * (size_t)B * M);        if (w) w->area = (float *)p;
    p = c.take(sizeof(int) * (size_t)B * M);          if (w) w->gt_row = (int *)p;
    p = c.take(sizeof(int) * (size_t)B * M);          if (w) w->label = (int *)p;
    p = c.take(sizeof(unsigned) * (size_t)B * M);     if (w) w->gtmax = (unsigned *)p;
    return c.off;
}

// boxes3d_lidar_to_aligned_bev_boxes (box_utils.py:261-272): |limit_period(h, 0.5, pi)| < pi/4 keeps (dx, dy), else swaps
__device__ __forceinline__ float4 aa_bev(float x, float y, float dx, float dy, float h) {
    const float PI_F = 3.14159265358979323846f, QPI_F = 0.78539816339744830962f;
    const float rot = fabsf(h - floorf(h / PI_F + 0.5f) * PI_F);
    const bool keep = rot < QPI_F;
    const float cx = keep ? dx : dy, cy = keep ? dy : dx;
    return make_float4(x - cx / 2, y - cy / 2, x + cx / 2, y + cy / 2);
}

__device__ __forceinline__ float aa_area(float4 b) { return (b.z - b.x) * (b.w - b.y); }

// boxes_iou_normal (box_utils.py:238-258) for one pair; inter == 0 gives exactly 0 there, so the division is skipped
__device__ __forceinline__ float aa_iou(float4 a, float area_a, float4 g, float area_g) {
    const float xl = fmaxf(fminf(a.z, g.z) - fmaxf(a.x, g.x), 0.0f);
    const float yl = fmaxf(fminf(a.w, g.w) - fmaxf(a.y, g.y), 0.0f);
    const float inter = xl * yl;
    float iou = 0.0f;
    if (inter > 0.0f) iou = inter / fmaxf(area_a + area_g - inter, 1e-6f);
    return iou;
}

// The reference masks a gt of id c into the anchor class named class_names[c - 1] (numpy indexing, :61-66): id 0 wraps to the last
// name, negative ids wrap further, and an id past the name list raises IndexError there.  The host table reproduces the wrap for
// ids -64..63; an id past the name list (or outside the table) matches no anchor class here instead of raising.
__device__ __forceinline__ int aa_class_of(const AAParams &p, const float *row) {
    const float v = row[p.gt_cols - 1];
    if (!(v > (float)(AA_ID_MIN - 1) && v < (float)(AA_NUM_IDS + AA_ID_MIN))) return -1;
    return p.class_of_id[(int)v - AA_ID_MIN];     // .int() truncates toward zero, as the C cast
}

// ---------------------------------------------------------------- prep: one wave per frame
__global__ __launch_bounds__(64) void anchor_assign_prep_kernel(const float *__restrict__ gt, AAParams p, AAWs w) {
    const int b = blockIdx.x, lane = threadIdx.x, M = p.max_gt, D = p.gt_cols - 1;
    const float *fgt = gt + (size_t)b * M * p.gt_cols;
    // trailing padding: `while cnt > 0 and cur_gt[cnt].sum() == 0: cnt -= 1` — a row SUM over the box columns, here left to right.
    // torch may reduce the row in another order; the two can disagree only for rows whose large values cancel exactly in one
    // order and not in the other (e.g. [1e20, 1, -1e20]); padding rows and real boxes are far from that.
    int last = 0;
    for (int r = 1 + lane; r < M; r += 64) {
        const float *row = fgt + (size_t)r * p.gt_cols;
        float s = 0.0f;
        for (int q = 0; q < D; ++q) s += row[q];
        if (s != 0.0f) last = r;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) last = max(last, __shfl_xor(last, d, 64));
    const int cnt = M > 0 ? last + 1 : 0;
    // class counts -> slot prefix
    __shared__ int s_base[AA_MAX_CLASSES + 1];
    if (lane <= p.ncls) s_base[lane] = 0;
    __syncthreads();
    for (int r0 = 0; r0 < cnt; r0 += 64) {
        const int r = r0 + lane;
        const int k = r < cnt ? aa_class_of(p, fgt + (size_t)r * p.gt_cols) : -1;
        if (k >= 0) atomicAdd(&s_base[k + 1], 1);
    }
    __syncthreads();
    if (lane == 0) {
        for (int k = 0; k < p.ncls; ++k) s_base[k + 1] += s_base[k];
        for (int k = 0; k <= p.ncls; ++k) w.cls_start[b * (p.ncls + 1) + k] = s_base[k];
        for (int k = 0; k < p.ncls; ++k) w.num_examples[b * p.ncls + k] = 0;
    }
    __syncthreads();
    // stable placement: rank among the chunk's rows of the same class by ballot, running base per class
    for (int r0 = 0; r0 < cnt; r0 += 64) {
        const int r = r0 + lane;
        const float *row = fgt + (size_t)min(r, cnt - 1) * p.gt_cols;
        const int k = r < cnt ? aa_class_of(p, row) : -1;
        for (int kk = 0; kk < p.ncls; ++kk) {
            const unsigned long long bal = __ballot(k == kk);
            if (!bal) continue;
            if (k == kk) {
                const int slot = s_base[kk] + __popcll(bal & lanemask_lt());
                const size_t o = (size_t)b * M + slot;
                const float4 bx = aa_bev(row[0], row[1], row[3], row[4], row[6]);
                w.bev[o] = bx;
                w.area[o] = aa_area(bx);
                w.gt_row[o] = r;
                w.label[o] = p.cls[kk].remap > 0 ? p.cls[kk].remap : (int)row[p.gt_cols - 1];
                w.gtmax[o] = 0u;
            }
            __syncthreads();   // every lane has read s_base[kk]
            if (lane == 0) s_base[kk] += __popcll(bal);
            __syncthreads();
        }
    }
}

// which class owns anchor tile `t` (wave-uniform)
__device__ __forceinline__ int aa_tile_class(const AAParams &p, int t) {
    int c = 0;
    for (int k = 1; k < p.ncls; ++k)
        if (t >= p.cls[k].tile_start) c = k;
    return c;
}

struct AAGtLds {
    float4 bev[AA_CHUNK];
    float area[AA_CHUNK];
    float gmax[AA_CHUNK];
};

__device__ __forceinline__ void aa_stage(AAGtLds &s, const AAWs &w, size_t base, int n, bool with_max) {
    const int t = threadIdx.x;
    if (t < n) {
        s.bev[t] = w.bev[base + t];
        s.area[t] = w.area[base + t];
        if (with_max) s.gmax[t] = __uint_as_float(w.gtmax[base + t]);
    }
}

// ---------------------------------------------------------------- gtmax: per-gt max IoU over all anchors of its class
__global__ __launch_bounds__(AA_TILE) void anchor_assign_gtmax_kernel(AAParams p, AAWs w) {
    __shared__ AAGtLds s;
    const int tile = blockIdx.x, c = aa_tile_class(p, tile);
    const AAClass &C = p.cls[c];
    const long long i = (long long)(tile - C.tile_start) * AA_TILE + threadIdx.x;
    const bool valid = i < C.n;
    float4 ab = make_float4(0.f, 0.f, 0.f, 0.f);
    float aarea = 0.f;
    if (valid) {
        const float *a = C.anchors + i * p.anchor_dim;
        ab = aa_bev(a[0], a[1], a[3], a[4], a[6]);
        aarea = aa_area(ab);
    }
    const int b0 = blockIdx.y * p.frames_per_block, b1 = min(b0 + p.frames_per_block, p.batch);
    for (int b = b0; b < b1; ++b) {
        const int s0 = w.cls_start[b * (p.ncls + 1) + c], s1 = w.cls_start[b * (p.ncls + 1) + c + 1];
        for (int j0 = s0; j0 < s1; j0 += AA_CHUNK) {
            const int n = min(AA_CHUNK, s1 - j0);
            const size_t base = (size_t)b * p.max_gt + j0;
            aa_stage(s, w, base, n, false);
            __syncthreads();
            for (int j = 0; j < n; ++j) {
                float v = valid ? aa_iou(ab, aarea, s.bev[j], s.area[j]) : 0.0f;
                if (__ballot(v > 0.0f)) {
#pragma unroll
                    for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
                    if (lane_id() == 0) atomicMax(&w.gtmax[base + j], __float_as_uint(v));
                }
            }
            __syncthreads();
        }
    }
}

// ResidualCoder.encode_torch (box_coder_utils.py:13-42) of one (gt, anchor) pair: csrc/box_encode_dev.h
__device__ __forceinline__ void aa_encode(const AAParams &p, const float *g, const float *a, float *out) {
    residual_encode(g, a, out, p.sincos, p.code_size);   // zip(cgs, cas): code_size was checked on the host
}

// ---------------------------------------------------------------- assign: labels, targets, weights
__global__ __launch_bounds__(AA_TILE) void anchor_assign_kernel(AAParams p, AAWs w, const float *__restrict__ gt,
                                                                const float *__restrict__ gt_enc, int *__restrict__ labels,
                                                                float *__restrict__ targets, float *__restrict__ weights,
                                                                int count_examples) {
    __shared__ AAGtLds s;
    __shared__ float s_out[AA_TILE * AA_MAX_CODE];
    __shared__ long long s_orow[AA_TILE];
    __shared__ int s_cnt;
    const int tile = blockIdx.x, c = aa_tile_class(p, tile), t = threadIdx.x;
    const AAClass &C = p.cls[c];
    const long long i0 = (long long)(tile - C.tile_start) * AA_TILE;
    const long long i = i0 + t;
    const int nt = (int)min((long long)AA_TILE, C.n - i0);     // anchors of this tile
    const bool valid = t < nt;
    const float *a = C.anchors + (valid ? i : 0) * p.anchor_dim;
    float4 ab = make_float4(0.f, 0.f, 0.f, 0.f);
    float aarea = 0.f;
    if (valid) {
        ab = aa_bev(a[0], a[1], a[3], a[4], a[6]);
        aarea = aa_area(ab);
    }
    // output anchor index: (i / R) * A_total + off + i % R (single head's view(*fmap, -1) + cat(dim=-1), :102-115);
    // multihead: R = n, so off + i (plain concatenation, :92-100)
    auto out_index = [&](long long ii) { return (ii / C.per_loc) * p.a_total + C.out_off + ii % C.per_loc; };
    const long long o = out_index(valid ? i : i0);
    s_orow[t] = o;
    const int code = p.code_size;
    const unsigned div_mul = (65536u + code - 1) / code;   // e / code == (e * div_mul) >> 16 for e < AA_TILE * AA_MAX_CODE
    const int b0 = blockIdx.y * p.frames_per_block, b1 = min(b0 + p.frames_per_block, p.batch);
    for (int b = b0; b < b1; ++b) {
        const int s0 = w.cls_start[b * (p.ncls + 1) + c], s1 = w.cls_start[b * (p.ncls + 1) + c + 1];
        float best = -1.0f;
        int arg = s0;
        bool forced = false;
        for (int j0 = s0; j0 < s1; j0 += AA_CHUNK) {
            const int n = min(AA_CHUNK, s1 - j0);
            const size_t base = (size_t)b * p.max_gt + j0;
            aa_stage(s, w, base, n, true);
            __syncthreads();
            if (valid) {
                for (int j = 0; j < n; ++j) {
                    const float v = aa_iou(ab, aarea, s.bev[j], s.area[j]);
                    if (v > best) { best = v; arg = j0 + j; }                  // first maximum, as numpy argmax
                    const float gm = s.gmax[j];
                    forced |= (gm > 0.0f) && (v == gm);                        // a gt max of 0 became -1 (:157-158)
                }
            }
            __syncthreads();
        }
        int label = 0;
        bool encode = false;
        if (s1 > s0) {
            const int lab = w.label[(size_t)b * p.max_gt + arg];
            if (forced) label = lab;
            else if (best < C.unmatched) label = 0;
            else if (best >= C.matched) label = lab;
            else label = -1;
            // the reference takes fg_inds (whose targets it encodes) before the background overwrite (:176 vs :187-190): with
            // matched < unmatched an anchor in [matched, unmatched) ends with label 0 but still gets targets (weight 0)
            encode = (forced || best >= C.matched) && lab > 0;
        }
        const bool fg = label > 0;
        float *my = s_out + t * code;
        if (valid && encode) {
            const float *g = gt_enc + ((size_t)b * p.max_gt + w.gt_row[(size_t)b * p.max_gt + arg]) * p.gt_cols;
            aa_encode(p, g, a, my);
        } else {
            for (int q = 0; q < code; ++q) my[q] = 0.0f;
        }
        const size_t fo = (size_t)b * p.n_total;
        if (valid) {
            labels[fo + o] = label;
            weights[fo + o] = fg ? 1.0f : 0.0f;
        }
        if (count_examples) {
            if (t == 0) s_cnt = 0;
            __syncthreads();
            const unsigned long long bal = __ballot(valid && label >= 0);
            if (lane_id() == 0 && bal) atomicAdd(&s_cnt, __popcll(bal));
        }
        __syncthreads();
        if (count_examples && t == 0 && s_cnt) atomicAdd(&w.num_examples[b * p.ncls + c], s_cnt);
        // coalesced target stores: element e of the tile -> anchor e / code, column e % code
        for (int e = t; e < nt * code; e += AA_TILE) {
            const int ta = (int)(((unsigned)e * div_mul) >> 16), q = e - ta * code;
            targets[(fo + s_orow[ta]) * code + q] = s_out[e];
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------- norm: NORM_BY_NUM_EXAMPLES (:201-205)
__global__ __launch_bounds__(AA_TILE) void anchor_assign_norm_kernel(AAParams p, AAWs w, const int *__restrict__ labels,
                                                                     float *__restrict__ weights) {
    const int tile = blockIdx.x, c = aa_tile_class(p, tile);
    const AAClass &C = p.cls[c];
    const long long i = (long long)(tile - C.tile_start) * AA_TILE + threadIdx.x;
    if (i >= C.n) return;
    const long long o = (i / C.per_loc) * p.a_total + C.out_off + i % C.per_loc;
    const int b0 = blockIdx.y * p.frames_per_block, b1 = min(b0 + p.frames_per_block, p.batch);
    for (int b = b0; b < b1; ++b) {
        const size_t fo = (size_t)b * p.n_total + o;
        if (labels[fo] > 0) weights[fo] = 1.0f / (float)max(w.num_examples[b * p.ncls + c], 1);
    }
}

LIDAR_EXPORT size_t lidar_anchor_assign_workspace_bytes(int batch, int max_gt, int num_classes) {
    if (batch <= 0 || max_gt < 0 || num_classes <= 0 || num_classes > AA_MAX_CLASSES) return 0;
    return aa_ws_layout(batch, max_gt, num_classes, nullptr, nullptr);
}

LIDAR_EXPORT int lidar_anchor_assign(const float *const *anchors, const long long *counts, const long long *per_loc,
                                     const long long *out_off, const float *matched, const float *unmatched, const int *remap,
                                     int num_classes, int anchor_dim, long long a_total, const signed char *class_of_id,
                                     const float *gt, const float *gt_enlarged, int batch, int max_gt, int gt_cols, int code_size,
                                     int sincos, int norm_by_num_examples, int *labels, float *targets, float *weights, void *ws,
                                     size_t ws_bytes, void *stream) {
    if (num_classes <= 0 || num_classes > AA_MAX_CLASSES || batch < 0 || max_gt < 0 || anchor_dim < 7 || gt_cols < 8 ||
        a_total <= 0 || !anchors || !counts || !per_loc || !out_off || !matched || !unmatched || !remap || !class_of_id)
        return LIDAR_ERR_ARG;
    const int extra = min(anchor_dim - 7, gt_cols - 1 - 7);
    if (code_size != 6 + (sincos ? 2 : 1) + extra || code_size > AA_MAX_CODE) return LIDAR_ERR_ARG;
    AAParams p{};
    long long n_total = 0;
    int tiles = 0;
    for (int k = 0; k < num_classes; ++k) {
        if (counts[k] < 0 || per_loc[k] <= 0 || out_off[k] < 0 || (counts[k] > 0 && !anchors[k])) return LIDAR_ERR_ARG;
        p.cls[k] = AAClass{anchors[k], counts[k], per_loc[k], out_off[k], tiles, remap[k], matched[k], unmatched[k]};
        n_total += counts[k];
        const long long t = (counts[k] + AA_TILE - 1) / AA_TILE;
        if (tiles + t > 0x7fffffffll) return LIDAR_ERR_ARG;
        tiles += (int)t;
    }
    for (int id = 0; id < AA_NUM_IDS; ++id) {
        if (class_of_id[id] >= num_classes) return LIDAR_ERR_ARG;
        p.class_of_id[id] = class_of_id[id] < 0 ? -1 : class_of_id[id];
    }
    for (int k = 0; k < num_classes; ++k) {   // every output index stays inside the frame's n_total anchors
        const long long n = counts[k];
        if (n > 0 && ((n - 1) / per_loc[k]) * a_total + out_off[k] + min(per_loc[k] - 1, n - 1) >= n_total) return LIDAR_ERR_ARG;
    }
    if (batch == 0 || n_total == 0) return LIDAR_OK;
    if (!gt && max_gt > 0) return LIDAR_ERR_ARG;
    if (!labels || !targets || !weights || !ws) return LIDAR_ERR_ARG;
    AAWs w;
    if (ws_bytes < aa_ws_layout(batch, max_gt, num_classes, &w, (char *)ws)) return LIDAR_ERR_WORKSPACE;
    p.ncls = num_classes;
    p.tiles_total = tiles;
    p.anchor_dim = anchor_dim;
    p.gt_cols = gt_cols;
    p.code_size = code_size;
    p.sincos = sincos ? 1 : 0;
    p.batch = batch;
    p.max_gt = max_gt;
    p.n_total = n_total;
    p.a_total = a_total;
    // a few frames per workgroup: the anchor tile's BEV boxes are computed once for them, and the grid stays >= ~1000 tiles x groups
    p.frames_per_block = 4;
    const dim3 grid((unsigned)tiles, (unsigned)((batch + p.frames_per_block - 1) / p.frames_per_block));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(anchor_assign_prep_kernel, dim3(batch), dim3(64), 0, st, gt, p, w);
    hipLaunchKernelGGL(anchor_assign_gtmax_kernel, grid, dim3(AA_TILE), 0, st, p, w);
    hipLaunchKernelGGL(anchor_assign_kernel, grid, dim3(AA_TILE), 0, st, p, w, gt, gt_enlarged ? gt_enlarged : gt, labels, targets,
                       weights, norm_by_num_examples ? 1 : 0);
    if (norm_by_num_examples)
        hipLaunchKernelGGL(anchor_assign_norm_kernel, grid, dim3(AA_TILE), 0, st, p, w, labels, weights);
    return lidar_check_launch("lidar_anchor_assign");
}
