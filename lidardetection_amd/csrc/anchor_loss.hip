// Anchor-head RPN loss (AnchorHeadTemplate / AnchorHeadMulti .get_loss) for a whole batch and every head: forward + finalize, and a
// backward that writes the gradients of the three loss terms with respect to the predictions.  No float atomics: every sum runs in a
// fixed order, so losses and gradients are bitwise reproducible.  Reference: pcdet/models/dense_heads/anchor_head_template.py
// (get_cls_layer_loss :102-137, add_sin_difference :139-146, get_direction_target :148-161, get_box_reg_layer_loss :163-215),
// anchor_head_multi.py:245-370 (the multi-head overrides), pcdet/utils/loss_utils.py (SigmoidFocalClassificationLoss α 0.25 γ 2
// :9-72, WeightedSmoothL1Loss β 1/9 :75-136, WeightedL1Loss :139-178, WeightedCrossEntropyLoss :181-205), limit_period
// pcdet/utils/common_utils.py:52-55.
//
//   forward  (256-anchor tile of one head x frame)  stages the tile's class logits through LDS (one flat coalesced read), evaluates
//            the focal loss of every cared anchor and, for the positives only, the box and direction terms (their rows are
//            gathered: a negative's box / dir term is a finite value times weight 0 in the reference).  Writes one partial
//            (cls, loc, dir, #positives) per (tile, frame): the sums are UNNORMALISED, the normaliser is global per frame.
//   finalize (one workgroup, a wave per frame)  sums the partials of each frame in tile order, divides by clamp(npos, 1) and B,
//            applies the loss weights, writes the three losses and keeps npos per frame in the workspace for backward.
//   backward (same tiles)  d cls for every element, d box / d dir for the positives (zeros elsewhere), each scaled by its
//            grad_output scalar read from device memory; staged through LDS so the stores run along the rows.
//
// The focal element and the conventions of the element math and its gradients are loss_dev.h's; the box term (al_box: sin
// difference, L1 option, upstream factor folded into the gradient) and the direction term (al_dir) follow them in this file.
// The ordered sums are common.h's block_sum / wave_sum.
#include "common.h"
#include "loss_dev.h"
#include <math.h>

#define AL_MAX_HEADS 16
#define AL_MAX_CODE 16
#define AL_MAX_COLS 16    // class columns of one head
#define AL_MAX_BINS 8
#define AL_TILE 256
#define AL_FIN_THREADS 1024

struct ALHead {
    const float *cls, *box, *dir;    // (B, n, c), (B, n, code), (B, n, bins) DEVICE; dir NULL without a direction classifier
    float *dcls, *dbox, *ddir;       // backward outputs in the same layouts (NULL: not wanted)
    long long n, a_off;              // anchors of the head, its first anchor in the frame's label / target / anchor order
    int c, c_idx, tile_start;        // class columns, first one-hot column (SEPARATE_MULTIHEAD), first tile
};

struct ALParams {
    ALHead h[AL_MAX_HEADS];
    float code_w[AL_MAX_CODE];
    float pos_w, neg_w;              // class weights of positives / negatives (template: 1, 1)
    float w_cls, w_loc, w_dir;       // LOSS_WEIGHTS cls_weight, loc_weight, dir_weight
    float dir_offset, dir_bin;       // DIR_OFFSET; 2 pi / NUM_DIR_BINS (rounded once from double, as torch casts the scalar)
    long long n_total;               // anchors per frame
    int nheads, tiles, batch, num_class, code, bins, anchor_dim, sin_diff, l1;
};

struct ALWs {
    float4 *part;   // (B, tiles) cls, loc, dir, #positives (int bits)
    int *npos;      // (B)
};

static inline size_t al_ws_layout(int B, int tiles, ALWs *w, char *base) {
    WsCarve c{base};
    char *p;
    p = c.take(sizeof(float4) * (size_t)B * tiles); if (w) w->part = (float4 *)p;
    p = c.take(sizeof(int) * (size_t)B);            if (w) w->npos = (int *)p;
    return c.off;
}

__device__ __forceinline__ int al_tile_head(const ALParams &p, int t) {
    int h = 0;
    for (int k = 1; k < p.nheads; ++k)
        if (t >= p.h[k].tile_start) h = k;
    return h;
}

// the one-hot target of column j of head H: box_cls_labels * cared scattered into num_class + 1 columns, column 0 dropped, the
// head's slice starting at c_idx (:123-131, multi :274-293); num_class == 1 relabels positives to 1 first (:112-114)
__device__ __forceinline__ float al_onehot(const ALParams &p, const ALHead &H, int lab, int j) {
    const int le = (p.num_class == 1 && lab > 0) ? 1 : lab;
    return (lab >= 0 && le == H.c_idx + j + 1) ? 1.0f : 0.0f;
}

// the anchor's direction bin (get_direction_target :148-161): floor(limit_period(t6 + a6 - off, 0, 2 pi) / (2 pi / bins)), clamped
__device__ __forceinline__ int al_dir_bin(const ALParams &p, float t6, float a6) {
    const float TWO_PI_F = 6.28318530717958647692f;
    const float v = (t6 + a6) - p.dir_offset;
    const float r = v - floorf(v / TWO_PI_F + 0.0f) * TWO_PI_F;
    const int k = (int)floorf(r / p.dir_bin);
    return min(max(k, 0), p.bins - 1);
}

// one positive anchor's box term: sum over the code of the (smooth) L1 of code_w * (pred - target), the heading column through
// add_sin_difference when p.sin_diff; NaN targets take the prediction (loss_utils.py:122, :164).  g != 0: d(pred row) * g into dbox.
__device__ __forceinline__ float al_box(const ALParams &p, const float *bx, const float *tg, float g, float *dbox) {
    const float BETA = (float)(1.0 / 9.0), HALF_BETA = (float)(0.5 / 9.0);
    float loss = 0.0f;
    for (int q = 0; q < p.code; ++q) {
        float in = bx[q], t = tg[q];
        float s6 = 0.f, c6 = 0.f, st = 0.f, ct = 0.f;
        const bool ang = p.sin_diff && q == 6;
        if (ang) {
            s6 = sinf(in); c6 = cosf(in); st = sinf(t); ct = cosf(t);
            in = s6 * ct;
            t = c6 * st;
        }
        const bool nan_t = isnan(t);
        if (nan_t) t = in;
        const float d = (in - t) * p.code_w[q];
        const float n = fabsf(d);
        const bool quad = !p.l1 && n < BETA;
        loss += p.l1 ? n : (quad ? 0.5f * (n * n) / BETA : n - HALF_BETA);
        if (dbox) {
            const float dn = quad ? (g * 0.5f / BETA) * (2.0f * n) : g;       // d loss / d n
            const float dd = (dn * sign0(d)) * p.code_w[q];                    // d loss / d (in - t)
            const float din = nan_t ? 0.0f : dd;                                // a NaN target: in - in, exactly 0
            const float dt = nan_t ? 0.0f : -dd;
            dbox[q] = ang ? din * ct * c6 + dt * st * (-s6) : din;
        }
    }
    return loss;
}

// WeightedCrossEntropyLoss of one positive anchor: -log_softmax(x)[k]; g != 0: d x * g into ddir
__device__ __forceinline__ float al_dir(const ALParams &p, const float *x, int k, float g, float *ddir) {
    float m = x[0];
    for (int j = 1; j < p.bins; ++j) m = fmaxf(m, x[j]);
    float s = 0.0f;
    for (int j = 0; j < p.bins; ++j) s += expf(x[j] - m);
    const float ls = logf(s);
    if (ddir)
        for (int j = 0; j < p.bins; ++j) ddir[j] = g * (expf((x[j] - m) - ls) - (j == k ? 1.0f : 0.0f));
    return -((x[k] - m) - ls);
}

// ---------------------------------------------------------------- forward: unnormalised partial sums per (tile, frame)
__global__ __launch_bounds__(AL_TILE) void anchor_loss_fwd_kernel(ALParams p, const int *__restrict__ labels,
                                                                  const float *__restrict__ targets,
                                                                  const float *__restrict__ anchors, ALWs w) {
    __shared__ float s_buf[AL_TILE * AL_MAX_COLS];
    __shared__ BlockSumLds<AL_TILE / 64, 3, 1> s_red;
    const int tile = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const ALHead &H = p.h[al_tile_head(p, tile)];
    const long long i0 = (long long)(tile - H.tile_start) * AL_TILE;
    const int nt = (int)min((long long)AL_TILE, H.n - i0);
    const bool valid = t < nt;
    const long long g = H.a_off + i0 + t;
    const int lab = valid ? labels[(size_t)b * p.n_total + g] : -1;
    const float *src = H.cls + ((size_t)b * H.n + i0) * H.c;
    for (int e = t; e < nt * H.c; e += AL_TILE) s_buf[e] = src[e];
    __syncthreads();
    float sum[3] = {0.0f, 0.0f, 0.0f};      // cls, loc, dir
    if (lab >= 0) {
        const float cw = (lab > 0 ? p.pos_w : 0.0f) + (lab == 0 ? p.neg_w : 0.0f);
        float a = 0.0f;
        for (int j = 0; j < H.c; ++j) a += sigmoid_focal(s_buf[t * H.c + j], al_onehot(p, H, lab, j), nullptr);
        sum[0] = a * cw;
    }
    if (lab > 0) {
        const size_t row = (size_t)b * H.n + i0 + t;
        const float *tg = targets + ((size_t)b * p.n_total + g) * p.code;
        sum[1] = al_box(p, H.box + row * p.code, tg, 0.0f, nullptr);
        if (H.dir) {
            const int k = al_dir_bin(p, tg[6], anchors[(size_t)g * p.anchor_dim + 6]);
            sum[2] = al_dir(p, H.dir + row * p.bins, k, 0.0f, nullptr);
        }
    }
    int np[1] = {lab > 0 ? 1 : 0};
    block_sum(sum, np, s_red);
    if (t == 0) w.part[(size_t)b * p.tiles + tile] = make_float4(sum[0], sum[1], sum[2], __int_as_float(np[0]));
}

// ---------------------------------------------------------------- finalize: one workgroup, wave f sums frames f, f + 16, ...
__global__ __launch_bounds__(AL_FIN_THREADS) void anchor_loss_finalize_kernel(ALParams p, ALWs w, float *__restrict__ losses) {
    __shared__ float3 s_frame[AL_FIN_THREADS / 64];
    const int wave = threadIdx.x >> 6, lane = lane_id(), nw = AL_FIN_THREADS / 64;
    float3 acc = make_float3(0.f, 0.f, 0.f);   // thread 0 only: frames in order
    for (int b0 = 0; b0 < p.batch; b0 += nw) {
        const int b = b0 + wave;
        if (b < p.batch) {
            float c = 0.f, l = 0.f, d = 0.f;
            int n = 0;
            for (int k = lane; k < p.tiles; k += 64) {
                const float4 r = w.part[(size_t)b * p.tiles + k];
                c += r.x; l += r.y; d += r.z; n += __float_as_int(r.w);
            }
            c = wave_sum(c); l = wave_sum(l); d = wave_sum(d); n = wave_sum(n);
            if (lane == 0) {
                w.npos[b] = n;
                const float norm = fmaxf((float)n, 1.0f);   // torch.clamp(pos_normalizer, min=1.0)
                s_frame[wave] = make_float3(c / norm, l / norm, d / norm);
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int k = 0; k < nw && b0 + k < p.batch; ++k) {
                acc.x += s_frame[k].x; acc.y += s_frame[k].y; acc.z += s_frame[k].z;
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const float B = (float)p.batch;
        losses[0] = acc.x / B * p.w_cls;
        losses[1] = acc.y / B * p.w_loc;
        losses[2] = acc.z / B * p.w_dir;
    }
}

// ---------------------------------------------------------------- backward: gradients scaled by grad_output (device scalars)
__global__ __launch_bounds__(AL_TILE) void anchor_loss_bwd_kernel(ALParams p, const int *__restrict__ labels,
                                                                  const float *__restrict__ targets,
                                                                  const float *__restrict__ anchors, ALWs w,
                                                                  const float *__restrict__ grad) {
    __shared__ float s_buf[AL_TILE * AL_MAX_COLS];
    const int tile = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const ALHead &H = p.h[al_tile_head(p, tile)];
    const long long i0 = (long long)(tile - H.tile_start) * AL_TILE;
    const int nt = (int)min((long long)AL_TILE, H.n - i0);
    const bool valid = t < nt;
    const long long g = H.a_off + i0 + t;
    const int lab = valid ? labels[(size_t)b * p.n_total + g] : -1;
    const float norm = fmaxf((float)w.npos[b], 1.0f);
    const float B = (float)p.batch;
    // autograd's chain from each loss: (grad * weight) / B, then times the element's anchor weight (its class weight / norm)
    const float gc = grad[0] * p.w_cls / B, gl = grad[1] * p.w_loc / B, gd = grad[2] * p.w_dir / B;
    const size_t row = (size_t)b * H.n + i0 + t;
    if (H.dcls) {
        const float *src = H.cls + ((size_t)b * H.n + i0) * H.c;
        for (int e = t; e < nt * H.c; e += AL_TILE) s_buf[e] = src[e];
        __syncthreads();
        if (valid) {
            const float cw = (lab > 0 ? p.pos_w : 0.0f) + (lab == 0 ? p.neg_w : 0.0f);
            const float G = gc * (cw / norm);
            for (int j = 0; j < H.c; ++j) {
                float dx = 0.0f;
                if (lab >= 0) sigmoid_focal(s_buf[t * H.c + j], al_onehot(p, H, lab, j), &dx);
                s_buf[t * H.c + j] = lab >= 0 ? G * dx : 0.0f;
            }
        }
        __syncthreads();
        float *dst = H.dcls + ((size_t)b * H.n + i0) * H.c;
        for (int e = t; e < nt * H.c; e += AL_TILE) dst[e] = s_buf[e];
        __syncthreads();
    }
    const float *tg = targets + ((size_t)b * p.n_total + g) * p.code;
    if (H.dbox) {
        for (int e = t; e < nt * p.code; e += AL_TILE) s_buf[e] = 0.0f;
        __syncthreads();
        if (lab > 0) al_box(p, H.box + row * p.code, tg, gl * (1.0f / norm), s_buf + t * p.code);
        __syncthreads();
        float *dst = H.dbox + ((size_t)b * H.n + i0) * p.code;
        for (int e = t; e < nt * p.code; e += AL_TILE) dst[e] = s_buf[e];
        __syncthreads();
    }
    if (H.dir && H.ddir) {
        for (int e = t; e < nt * p.bins; e += AL_TILE) s_buf[e] = 0.0f;
        __syncthreads();
        if (lab > 0) {
            const int k = al_dir_bin(p, tg[6], anchors[(size_t)g * p.anchor_dim + 6]);
            al_dir(p, H.dir + row * p.bins, k, gd * (1.0f / norm), s_buf + t * p.bins);
        }
        __syncthreads();
        float *dst = H.ddir + ((size_t)b * H.n + i0) * p.bins;
        for (int e = t; e < nt * p.bins; e += AL_TILE) dst[e] = s_buf[e];
    }
}

// ---------------------------------------------------------------- host side
static int al_params(ALParams &p, const float *const *cls, const float *const *box, const float *const *dir,
                     const long long *counts, const int *cols, const int *col_off, int num_heads, long long n_total,
                     const float *anchors, int anchor_dim, int batch, int num_class, int code_size, int num_dir_bins,
                     const float *code_weights, const float *weights, int flags) {
    if (num_heads <= 0 || num_heads > AL_MAX_HEADS || batch <= 0 || n_total <= 0 || num_class <= 0 || code_size < 7 ||
        code_size > AL_MAX_CODE || !cls || !box || !counts || !cols || !col_off || !code_weights || !weights)
        return LIDAR_ERR_ARG;
    const int use_dir = (flags & 4) ? 1 : 0;
    if (use_dir && (!dir || !anchors || anchor_dim < 7 || num_dir_bins < 1 || num_dir_bins > AL_MAX_BINS)) return LIDAR_ERR_ARG;
    p = ALParams{};
    long long sum = 0;
    int tiles = 0;
    for (int k = 0; k < num_heads; ++k) {
        if (counts[k] <= 0 || cols[k] <= 0 || cols[k] > AL_MAX_COLS || col_off[k] < 0 || col_off[k] + cols[k] > num_class ||
            !cls[k] || !box[k] || (use_dir && !dir[k]))
            return LIDAR_ERR_ARG;
        p.h[k] = ALHead{cls[k], box[k], use_dir ? dir[k] : nullptr, nullptr, nullptr, nullptr, counts[k], sum, cols[k], col_off[k],
                        tiles};
        sum += counts[k];
        const long long tk = (counts[k] + AL_TILE - 1) / AL_TILE;
        if (tiles + tk > 0x7fffffffll) return LIDAR_ERR_ARG;
        tiles += (int)tk;
    }
    if (sum != n_total || batch > 65535) return LIDAR_ERR_ARG;
    for (int q = 0; q < code_size; ++q) p.code_w[q] = code_weights[q];
    p.w_cls = weights[0]; p.w_loc = weights[1]; p.w_dir = weights[2];
    p.pos_w = weights[3]; p.neg_w = weights[4];
    p.dir_offset = weights[5]; p.dir_bin = weights[6];
    p.n_total = n_total;
    p.nheads = num_heads;
    p.tiles = tiles;
    p.batch = batch;
    p.num_class = num_class;
    p.code = code_size;
    p.bins = use_dir ? num_dir_bins : 0;
    p.anchor_dim = anchor_dim;
    p.sin_diff = (flags & 1) ? 1 : 0;
    p.l1 = (flags & 2) ? 1 : 0;
    return LIDAR_OK;
}

LIDAR_EXPORT size_t lidar_anchor_loss_workspace_bytes(int batch, const long long *counts, int num_heads) {
    if (batch <= 0 || num_heads <= 0 || num_heads > AL_MAX_HEADS || !counts) return 0;
    long long tiles = 0;
    for (int k = 0; k < num_heads; ++k) {
        if (counts[k] <= 0) return 0;
        tiles += (counts[k] + AL_TILE - 1) / AL_TILE;
    }
    if (tiles > 0x7fffffffll) return 0;
    return al_ws_layout(batch, (int)tiles, nullptr, nullptr);
}

LIDAR_EXPORT int lidar_anchor_loss_forward(const float *const *cls, const float *const *box, const float *const *dir,
                                           const long long *counts, const int *cols, const int *col_off, int num_heads,
                                           const int *labels, const float *targets, const float *anchors, int anchor_dim,
                                           int batch, long long n_total, int num_class, int code_size, int num_dir_bins,
                                           const float *code_weights, const float *weights, int flags, float *losses, void *ws,
                                           size_t ws_bytes, void *stream) {
    ALParams p;
    const int st = al_params(p, cls, box, dir, counts, cols, col_off, num_heads, n_total, anchors, anchor_dim, batch, num_class,
                             code_size, num_dir_bins, code_weights, weights, flags);
    if (st != LIDAR_OK) return st;
    if (!labels || !targets || !losses || !ws) return LIDAR_ERR_ARG;
    ALWs w;
    if (ws_bytes < al_ws_layout(batch, p.tiles, &w, (char *)ws)) return LIDAR_ERR_WORKSPACE;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(anchor_loss_fwd_kernel, dim3((unsigned)p.tiles, (unsigned)batch), dim3(AL_TILE), 0, s, p, labels, targets,
                       anchors, w);
    hipLaunchKernelGGL(anchor_loss_finalize_kernel, dim3(1), dim3(AL_FIN_THREADS), 0, s, p, w, losses);
    return lidar_check_launch("lidar_anchor_loss_forward");
}

LIDAR_EXPORT int lidar_anchor_loss_backward(const float *const *cls, const float *const *box, const float *const *dir,
                                            const long long *counts, const int *cols, const int *col_off, int num_heads,
                                            const int *labels, const float *targets, const float *anchors, int anchor_dim,
                                            int batch, long long n_total, int num_class, int code_size, int num_dir_bins,
                                            const float *code_weights, const float *weights, int flags, const float *grad_losses,
                                            float *const *d_cls, float *const *d_box, float *const *d_dir, void *ws,
                                            size_t ws_bytes, void *stream) {
    ALParams p;
    const int st = al_params(p, cls, box, dir, counts, cols, col_off, num_heads, n_total, anchors, anchor_dim, batch, num_class,
                             code_size, num_dir_bins, code_weights, weights, flags);
    if (st != LIDAR_OK) return st;
    if (!labels || !targets || !grad_losses || !ws) return LIDAR_ERR_ARG;
    for (int k = 0; k < num_heads; ++k) {
        p.h[k].dcls = d_cls ? d_cls[k] : nullptr;
        p.h[k].dbox = d_box ? d_box[k] : nullptr;
        p.h[k].ddir = (d_dir && p.bins) ? d_dir[k] : nullptr;
    }
    ALWs w;
    if (ws_bytes < al_ws_layout(batch, p.tiles, &w, (char *)ws)) return LIDAR_ERR_WORKSPACE;
    hipLaunchKernelGGL(anchor_loss_bwd_kernel, dim3((unsigned)p.tiles, (unsigned)batch), dim3(AL_TILE), 0, (hipStream_t)stream, p,
                       labels, targets, anchors, w, grad_losses);
    return lidar_check_launch("lidar_anchor_loss_backward");
}
