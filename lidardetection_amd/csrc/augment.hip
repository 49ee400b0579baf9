// Train-time augmentation for a whole batch on the device: GT sampling (collision test, road plane, sample rotation, paste and
// carve), world flip / rotation / scaling, range mask and stable compaction.  No host read, no float atomics, every store a plain
// vector store, bitwise reproducible, graph-capturable; the kernels draw nothing (include/lidar_hip.h has the contract).  Reference:
//   pcdet/datasets/augmentor/database_sampler.py (__call__ :181-232, add_sampled_boxes_to_scene :118-179, put_boxes_on_road_planes
//   :98-116), pcdet/datasets/augmentor/augmentor_utils.py (random_flip_along_x :6-30, random_flip_along_y :33-57, global_rotation
//   :60-86, global_scaling :89-109), pcdet/datasets/augmentor/data_augmentor.py:108-134 (forward, limit_period),
//   pcdet/datasets/processor/data_processor.py:19-34 (mask_points_and_boxes_outside_range), pcdet/utils/common_utils.py:52-94
//   (limit_period, rotate_points_along_z, mask_points_by_range), pcdet/utils/box_utils.py:27-88, :136-149 (boxes_to_corners_3d,
//   mask_boxes_outside_range_numpy, remove_points_in_boxes3d, enlarge_box3d), pcdet/ops/roiaware_pool3d/src/roiaware_pool3d.cpp:121-168
//   (points_in_boxes_cpu, MARGIN 1e-2), pcdet/ops/iou3d_nms/src/iou3d_cpu.cpp:232-252 (boxes_iou_bev_cpu).
//
// Five launches on the caller's stream:
//   aug_frame_kernel   one workgroup of 128 threads per frame, everything in LDS.  Collision test (:194-227): the groups in order; the
//                      pair tests of a group (candidate x (existing boxes + the group's other candidates)) spread over the lanes, on
//                      the polygon clipper of csrc/iou3d_dev.h; a candidate stays iff every IoU is exactly 0.  Then per valid sample
//                      the road-plane height, the sample rotation and the carving box go to the workspace, and the frame's boxes
//                      (trained input rows, then the valid samples) are world-transformed, range-masked and compacted in order.
//                      lidar_augment_mf (template flag MF): the thread that owns a box row also moves the row's poses in the stacked
//                      sweeps (aug_pose_row) and writes them at the box's rank; the other four kernels are the same for both.
//   aug_plan_kernel    one workgroup: the frame's virtual rows (valid objects' points, then the scene points) are cut into blocks of
//                      256 rows; block offsets of the frames by an exclusive scan.
//   aug_flag_kernel    one thread per virtual row, the frame's carving boxes in LDS: keep flag (carve test for scene rows, range test
//                      on the transformed coordinates for all) and the block's count.
//   aug_scan_kernel    one workgroup: exclusive scan of the block counts.
//   aug_write_kernel   the same rows again: rank within the block by ballot, coordinates transformed once, row written.
//
// fp32 expressions keep the reference's op order (-ffp-contract=off); cos / sin of a heading are taken in double and rounded once
// (heading_cs), the world rotation's come from the host.  Python scalars of the reference (pi, 2 pi, 0.5) are fp32 constants here,
// as numpy / torch cast them before combining them with a float32 array.
#include "iou3d_dev.h"
#include "pt_in_box_dev.h"

#define AUG_TPB 128          // aug_frame_kernel
#define AUG_ROWS 256         // rows per block of the streaming kernels == their threads per block
#define AUG_T LIDAR_AUGMENT_MAX_BOXES
#define AUG_REC 16           // workspace words per valid sample
#define AUG_PI_F 3.14159265358979323846f

struct AugP {
    int B, M, G, S, C, T, n_points, n_obj, db_rows, cap, nblk;
    int has_cw, has_plane, has_srot, has_scale, remove_outside, min_corners;
    float cw[3], rw[3], range[6];
};

struct AugIn {
    const float *points, *gt, *db_points, *db_boxes, *rot, *rot_cs, *scale, *sample_rot, *plane;
    const int *point_offsets, *gt_counts, *db_offsets, *db_cls, *cand, *flip_x, *flip_y;
};

struct AugWs {
    int *objrows, *vrows, *nvalid, *blk_off, *blk_cnt, *blk_base, *spre;
    float *rec;
    unsigned char *flags;
};

struct AugOut {
    float *points, *gt;
    int *offsets, *gt_counts, *valid;
};

// lidar_augment_mf only: every gt's pose in each of the F stacked sweeps, carried through the last section of aug_frame_kernel
struct AugPose {
    const float *gt_loc, *gt_ry, *db_loc, *db_ry;
    float *out_loc, *out_ry;
    int F;
};

struct AugWorld {
    int fx, fy, has_scale;
    float rot, c, s, sc;
};

__device__ __forceinline__ AugWorld aug_world_of(const AugIn &in, const AugP &p, int b) {
    AugWorld w;
    w.fx = in.flip_x[b] != 0;
    w.fy = in.flip_y[b] != 0;
    w.rot = in.rot[b];
    w.c = in.rot_cs[2 * b];
    w.s = in.rot_cs[2 * b + 1];
    w.has_scale = p.has_scale;
    w.sc = p.has_scale ? in.scale[b] : 1.0f;
    return w;
}

// flips, [x y z] @ [[c, s, 0], [-s, c, 0], [0, 0, 1]] (rotate_points_along_z), scaling
__device__ __forceinline__ void aug_world_xyz(const AugWorld &w, float &x, float &y, float &z) {
    if (w.fx) y = -y;
    if (w.fy) x = -x;
    const float rx = x * w.c + y * (-w.s), ry = x * w.s + y * w.c;
    x = rx; y = ry;
    if (w.has_scale) { x = x * w.sc; y = y * w.sc; z = z * w.sc; }
}

// a database index the kernels may follow: inside the database and with a sane point range
__device__ __forceinline__ int aug_cand(const AugIn &in, const AugP &p, int b, int k) {
    const int c = in.cand[(size_t)b * p.T + k];
    return (c >= 0 && c < p.n_obj) ? c : -1;
}

__device__ __forceinline__ void aug_db_span(const AugIn &in, const AugP &p, int c, int &row0, int &n) {
    const int lo = in.db_offsets[c], hi = in.db_offsets[c + 1];
    row0 = min(max(lo, 0), p.db_rows);
    n = max(min(hi, p.db_rows) - row0, 0);
}

// box (7) of sample k as it joins the scene: road plane (:109-115), then heading += sample_rot (:141).  mv: the height it moved by
__device__ __forceinline__ void aug_sample_box(const AugIn &in, const AugP &p, int b, int k, int c, float *box, float &mv) {
    const float *src = in.db_boxes + (size_t)c * 7;
#pragma unroll
    for (int q = 0; q < 7; ++q) box[q] = src[q];
    mv = 0.0f;
    if (p.has_plane) {
        const float *q = in.plane + (size_t)b * 4;
        const float h = q[0] * box[0] + q[1] * box[1] + q[2] * box[2] + q[3];
        mv = box[2] - box[5] / 2 - h;
        box[2] = box[2] - mv;
    }
    if (p.has_srot) box[6] = box[6] + in.sample_rot[(size_t)b * p.T + k];
}

// world flip / rotation / scaling / limit_period of a box (augmentor_utils.py, data_augmentor.py:122-124)
__device__ __forceinline__ void aug_world_box(const AugWorld &w, float *box) {
    const float TWO_PI_F = 6.28318530717958647692f;
    if (w.fx) box[6] = -box[6];
    if (w.fy) box[6] = -(box[6] + AUG_PI_F);
    aug_world_xyz(w, box[0], box[1], box[2]);
    box[6] = box[6] + w.rot;
    if (w.has_scale) { box[3] = box[3] * w.sc; box[4] = box[4] * w.sc; box[5] = box[5] * w.sc; }
    box[6] = box[6] - floorf(box[6] / TWO_PI_F + 0.5f) * TWO_PI_F;
}

// the F poses of one kept row, written at the row's compacted rank.  i >= 0: input row i; otherwise sample k = database object c, whose
// box centre after the road plane is ctr and which moved down by mv (database_sampler.py:165-177: z -= mv; rotations_y += a, locations
// turned by a about the box centre with the [cos, sin] the object's points get).  Then the world flips, rotation and scaling of
// augmentor_utils.py:24-28, :51-55, :80-84, :105-107; rotations_y is NOT folded by limit_period (data_augmentor.py:122 folds the
// boxes' heading only)
__device__ __forceinline__ void aug_pose_row(const AugIn &in, const AugP &p, const AugPose &ps, const AugWorld &w, int b, int i, int k,
                                             int c, const float *ctr, float mv, int rank) {
    const int F = ps.F;
    const bool pasted = i < 0, srot = pasted && p.has_srot;
    const size_t src = pasted ? (size_t)c * F : ((size_t)b * p.M + i) * F, dst = ((size_t)b * (p.M + p.T) + rank) * F;
    const float *sl = (pasted ? ps.db_loc : ps.gt_loc) + src * 3, *sr = (pasted ? ps.db_ry : ps.gt_ry) + src;
    float a = 0.0f, rc = 1.0f, rs = 0.0f;
    if (srot) {
        a = in.sample_rot[(size_t)b * p.T + k];
        heading_cs(a, rc, rs);
    }
    for (int s = 0; s < F; ++s) {
        float x = sl[s * 3], y = sl[s * 3 + 1], z = sl[s * 3 + 2], ry = sr[s];
        if (pasted && p.has_plane) z = z - mv;
        if (srot) {
            ry = ry + a;
            x = x - ctr[0]; y = y - ctr[1]; z = z - ctr[2];
            const float nx = x * rc + y * (-rs), ny = x * rs + y * rc;
            x = nx + ctr[0]; y = ny + ctr[1]; z = z + ctr[2];
        }
        if (w.fx) ry = -ry;
        if (w.fy) ry = -(ry + AUG_PI_F);
        aug_world_xyz(w, x, y, z);
        ry = ry + w.rot;
        float *ol = ps.out_loc + (dst + s) * 3;
        ol[0] = x; ol[1] = y; ol[2] = z;
        ps.out_ry[dst + s] = ry;
    }
}

// corners of boxes_to_corners_3d inside the closed 3-D range
__device__ __forceinline__ int aug_corners_inside(const float *box, const float *r) {
    float c, s;
    heading_cs(box[6], c, s);
    int cnt = 0;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
        const float sx = ((k & 3) == 0 || (k & 3) == 1) ? 0.5f : -0.5f;
        const float sy = ((k & 3) == 0 || (k & 3) == 3) ? 0.5f : -0.5f;
        const float sz = (k & 4) ? 0.5f : -0.5f;
        const float lx = box[3] * sx, ly = box[4] * sy, lz = box[5] * sz;
        const float x = (lx * c + ly * (-s)) + box[0], y = (lx * s + ly * c) + box[1], z = lz + box[2];
        cnt += (x >= r[0] && x <= r[3] && y >= r[1] && y <= r[4] && z >= r[2] && z <= r[5]) ? 1 : 0;
    }
    return cnt;
}

// points_in_boxes_cpu (roiaware_pool3d.cpp:121-168): MARGIN 1e-2, float -> double promoted comparisons as written there
__device__ __forceinline__ bool aug_pt_in_box(const float *b, float x, float y, float z) {
    const float MARGIN = 1e-2f;
    if ((double)fabsf(z - b[2]) > (double)b[5] / 2.0) return false;
    const float sx = x - b[0], sy = y - b[1];
    const float lx = sx * b[6] + sy * (-b[7]);
    const float ly = sx * b[7] + sy * b[6];
    return ((double)fabsf(lx) < (double)b[3] / 2.0 + (double)MARGIN) && ((double)fabsf(ly) < (double)b[4] / 2.0 + (double)MARGIN);
}

struct AugFrameLds {
    BoxPre pre[AUG_T];                     // [0, M): input rows; M + k: candidate k
    VertScratch<AUG_TPB> S;
    int cand[AUG_T];
    int pre_rows[AUG_T + 1];               // sizes, then their exclusive prefix, by valid rank
    unsigned short exist[AUG_T];           // slots of the boxes a candidate must not touch: real input rows, then the valid samples
    int coll[64];
    int wcnt[AUG_TPB / 64];
    int n_exist, n_out;
};

// MF: the rows' poses follow their boxes (lidar_augment_mf); without it `ps` is not read
template <bool MF>
__global__ __launch_bounds__(AUG_TPB) void aug_frame_kernel(AugIn in, AugP p, AugWs ws, AugOut o, AugPose ps) {
    __shared__ AugFrameLds L;
    const int b = blockIdx.x, t = threadIdx.x, wv = t >> 6;
    const int M = p.M, S = p.S, T = p.T;
    const int n = min(max(in.gt_counts[b], 0), M);
    const float *gt = in.gt + (size_t)b * M * 8;
    const float cw0 = p.has_cw ? p.cw[0] : 0.0f, cw1 = p.has_cw ? p.cw[1] : 0.0f;

    // ---- stage the boxes of the collision test, dims + collide_extra_width (:206-211)
    for (int i = t; i < n; i += AUG_TPB) {
        float tmp[7];
#pragma unroll
        for (int q = 0; q < 7; ++q) tmp[q] = gt[(size_t)i * 8 + q];
        if (p.has_cw) { tmp[3] = tmp[3] + cw0; tmp[4] = tmp[4] + cw1; }
        L.pre[i] = make_pre(tmp);
        L.exist[i] = (unsigned short)i;
    }
    for (int k = t; k < T; k += AUG_TPB) {
        const int c = aug_cand(in, p, b, k);
        L.cand[k] = c;
        if (c >= 0) {
            float tmp[7];
#pragma unroll
            for (int q = 0; q < 7; ++q) tmp[q] = in.db_boxes[(size_t)c * 7 + q];
            if (p.has_cw) { tmp[3] = tmp[3] + cw0; tmp[4] = tmp[4] + cw1; }
            L.pre[M + k] = make_pre(tmp);
        }
    }
    if (t == 0) L.n_exist = n;
    __syncthreads();

    // ---- collision test, group by group (:194-225)
    for (int g = 0; g < p.G; ++g) {
        if (t < 64) L.coll[t] = 0;
        __syncthreads();
        const int n_exist = L.n_exist, W = n_exist + S;
        for (int pr = t; pr < S * W; pr += AUG_TPB) {
            const int s = pr / W, j = pr - s * W;
            if (L.cand[g * S + s] < 0) continue;
            int slot;
            if (j < n_exist) slot = L.exist[j];
            else {
                const int s2 = j - n_exist;
                if (s2 == s || L.cand[g * S + s2] < 0) continue;          // the diagonal is set to 0 (:218)
                slot = M + g * S + s2;
            }
            const BoxPre A = L.pre[M + g * S + s], Bx = L.pre[slot];
            const float ov = (circles_apart(A, Bx) || sat_separated(A, Bx)) ? 0.0f : box_overlap_pre<AUG_TPB>(A, Bx, L.S, t);
            const float iou = iou_from_overlap(A.area, Bx.area, ov);
            if (!(iou == 0.0f)) L.coll[s] = 1;                             // every writer stores the same value
        }
        __syncthreads();
        if (t < 64) {
            const bool v = t < S && L.cand[g * S + t] >= 0 && L.coll[t] == 0;
            const unsigned long long bal = __ballot(v);
            if (v) L.exist[n_exist + __popcll(bal & lanemask_lt())] = (unsigned short)(M + g * S + t);
            if (t < S) o.valid[(size_t)b * T + g * S + t] = v ? 1 : 0;
            if (t == 0) L.n_exist = n_exist + __popcll(bal);
        }
        __syncthreads();
    }
    const int nv = L.n_exist - n;

    // ---- per valid sample: carving box, object transform, source rows
    for (int j = t; j < nv; j += AUG_TPB) {
        const int k = (int)L.exist[n + j] - M, c = L.cand[k];
        float box[7], mv;
        aug_sample_box(in, p, b, k, c, box, mv);
        int row0, rows;
        aug_db_span(in, p, c, row0, rows);
        L.pre_rows[j] = rows;
        float *rec = ws.rec + ((size_t)b * T + j) * AUG_REC;
        rec[0] = box[0]; rec[1] = box[1]; rec[2] = box[2];
        rec[3] = box[3] + p.rw[0]; rec[4] = box[4] + p.rw[1]; rec[5] = box[5] + p.rw[2];          // enlarge_box3d (:155-157)
        const float na = -box[6];
        rec[6] = (float)cos((double)na);
        rec[7] = (float)sin((double)na);
        float rc = 1.0f, rs = 0.0f;
        if (p.has_srot) heading_cs(in.sample_rot[(size_t)b * T + k], rc, rs);
        rec[8] = rc; rec[9] = rs;
        const float *src = in.db_boxes + (size_t)c * 7;
        rec[10] = src[0]; rec[11] = src[1]; rec[12] = src[2];                                     // obj_points += box3d_lidar[:3] (:144)
        rec[13] = mv;
        rec[14] = __int_as_float(row0);
        rec[15] = 0.0f;
    }
    __syncthreads();
    if (t < 64) {                                    // exclusive prefix of the sizes, 64 at a time
        int carry = 0;
        for (int base = 0; base < nv; base += 64) {
            const int v = base + t < nv ? L.pre_rows[base + t] : 0;
            const int incl = wave_incl_scan(v);
            if (base + t < nv) L.pre_rows[base + t] = carry + incl - v;
            carry += __shfl(incl, 63, 64);
        }
        if (t == 0) {
            L.pre_rows[nv] = carry;
            const int lo = in.point_offsets[b], hi = in.point_offsets[b + 1];
            const int np = max(min(hi, p.n_points) - min(max(lo, 0), p.n_points), 0);
            ws.objrows[b] = carry;
            ws.vrows[b] = carry + np;
            ws.nvalid[b] = nv;
        }
    }
    __syncthreads();
    for (int j = t; j <= nv; j += AUG_TPB) ws.spre[(size_t)b * (T + 1) + j] = L.pre_rows[j];

    // ---- the frame's boxes: trained input rows, then the valid samples; world transform, range mask, stable compaction
    const AugWorld w = aug_world_of(in, p, b);
    float *og = o.gt + (size_t)b * (M + T) * 8;
    if (t == 0) L.n_out = 0;
    __syncthreads();
    const int rows = n + nv;
    for (int r0 = 0; r0 < rows; r0 += AUG_TPB) {
        const int i = r0 + t;
        bool keep = false;
        float box[8], ctr[3] = {0.0f, 0.0f, 0.0f}, mv = 0.0f;
        int k = -1, c = -1;
        if (i < rows) {
            if (i < n) {
#pragma unroll
                for (int q = 0; q < 8; ++q) box[q] = gt[(size_t)i * 8 + q];
                keep = box[7] >= 1.0f;               // class id 0: annotated, but not a trained class
            } else {
                k = (int)L.exist[i] - M;
                c = L.cand[k];
                aug_sample_box(in, p, b, k, c, box, mv);
                if (MF) { ctr[0] = box[0]; ctr[1] = box[1]; ctr[2] = box[2]; }
                box[7] = (float)in.db_cls[c];
                keep = true;
            }
            aug_world_box(w, box);
            if (keep && p.remove_outside) keep = aug_corners_inside(box, p.range) >= p.min_corners;
        }
        const unsigned long long bal = __ballot(keep);
        if ((t & 63) == 0) L.wcnt[wv] = __popcll(bal);
        __syncthreads();
        int base = L.n_out;
        for (int q = 0; q < wv; ++q) base += L.wcnt[q];
        if (keep) {
            const int rank = base + __popcll(bal & lanemask_lt());
            float *dst = og + (size_t)rank * 8;
            *reinterpret_cast<float4 *>(dst) = make_float4(box[0], box[1], box[2], box[3]);
            *reinterpret_cast<float4 *>(dst + 4) = make_float4(box[4], box[5], box[6], box[7]);
            if (MF) aug_pose_row(in, p, ps, w, b, i < n ? i : -1, k, c, ctr, mv, rank);
        }
        __syncthreads();
        if (t == 0) {
            int add = 0;
            for (int q = 0; q < AUG_TPB / 64; ++q) add += L.wcnt[q];
            L.n_out += add;
        }
        __syncthreads();
    }
    const int n_out = L.n_out;
    if (t == 0) o.gt_counts[b] = n_out;
    for (int i = n_out * 2 + t; i < (M + T) * 2; i += AUG_TPB) reinterpret_cast<float4 *>(og)[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    if (MF) {                                        // rows at and past the count are zero in both pose arrays
        float *ol = ps.out_loc + (size_t)b * (M + T) * ps.F * 3, *orr = ps.out_ry + (size_t)b * (M + T) * ps.F;
        for (int i = n_out * ps.F * 3 + t; i < (M + T) * ps.F * 3; i += AUG_TPB) ol[i] = 0.0f;
        for (int i = n_out * ps.F + t; i < (M + T) * ps.F; i += AUG_TPB) orr[i] = 0.0f;
    }
}

// inclusive scan over the block's AUG_ROWS threads; total: the block's sum.  s_w: AUG_ROWS / 64 ints
__device__ __forceinline__ int aug_block_scan(int v, int *s_w, int &total) {
    const int t = threadIdx.x, wv = t >> 6;
    int incl = wave_incl_scan(v);
    __syncthreads();
    if ((t & 63) == 63) s_w[wv] = incl;
    __syncthreads();
    total = 0;
#pragma unroll
    for (int q = 0; q < AUG_ROWS / 64; ++q) {
        if (q < wv) incl += s_w[q];
        total += s_w[q];
    }
    return incl;
}

__global__ __launch_bounds__(AUG_ROWS) void aug_plan_kernel(AugP p, AugWs ws) {
    __shared__ int s_w[AUG_ROWS / 64];
    const int t = threadIdx.x;
    int carry = 0;
    for (int base = 0; base < p.B; base += AUG_ROWS) {
        const int b = base + t;
        const int v = b < p.B ? (ws.vrows[b] + AUG_ROWS - 1) / AUG_ROWS : 0;
        int total;
        const int incl = aug_block_scan(v, s_w, total);
        if (b < p.B) ws.blk_off[b] = carry + incl - v;
        carry += total;
    }
    if (t == 0) ws.blk_off[p.B] = carry;
}

// the frame of block blk: blk_off[b] <= blk < blk_off[b + 1]; -1 past the last frame's blocks
__device__ __forceinline__ int aug_frame_of(const int *blk_off, int B, int blk) {
    if (blk >= blk_off[B]) return -1;
    int lo = 0, hi = B;                          // blk_off[lo] <= blk < blk_off[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (blk_off[mid] <= blk) lo = mid; else hi = mid;
    }
    return lo;
}

struct AugRowLds {
    float box[AUG_T][8];
    int spre[AUG_T + 1];
};

// virtual row vr of frame b -> its C values with the coordinates as the carve test sees them (object rows: rotated by sample_rot,
// moved to the box centre, z -= mv, :142-148); is_obj: an object row
__device__ __forceinline__ void aug_load_row(const AugIn &in, const AugP &p, const AugWs &ws, const AugRowLds &L, int b, int vr,
                                             int objrows, int nv, float *row, bool &is_obj) {
    const int C = p.C;
    is_obj = vr < objrows;
    const float *src;
    if (is_obj) {
        int lo = 0, hi = nv;                     // spre[lo] <= vr < spre[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (L.spre[mid] <= vr) lo = mid; else hi = mid;
        }
        const float *rec = ws.rec + ((size_t)b * p.T + lo) * AUG_REC;
        src = in.db_points + (size_t)(__float_as_int(rec[14]) + (vr - L.spre[lo])) * C;
        if (C == 4) {
            const float4 v = *reinterpret_cast<const float4 *>(src);
            row[0] = v.x; row[1] = v.y; row[2] = v.z; row[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < LIDAR_AUGMENT_MAX_FEATURES; ++q)
                if (q < C) row[q] = src[q];
        }
        const float x = row[0], y = row[1];
        row[0] = (x * rec[8] + y * (-rec[9])) + rec[10];
        row[1] = (x * rec[9] + y * rec[8]) + rec[11];
        row[2] = (row[2] + rec[12]) - rec[13];
    } else {
        const int first = min(max(in.point_offsets[b], 0), p.n_points);
        src = in.points + (size_t)(first + (vr - objrows)) * C;
        if (C == 4) {
            const float4 v = *reinterpret_cast<const float4 *>(src);
            row[0] = v.x; row[1] = v.y; row[2] = v.z; row[3] = v.w;
        } else {
#pragma unroll
            for (int q = 0; q < LIDAR_AUGMENT_MAX_FEATURES; ++q)
                if (q < C) row[q] = src[q];
        }
    }
}

// stages the frame's carving boxes and object prefix; -> false when the block has no frame
__device__ __forceinline__ bool aug_row_setup(const AugP &p, const AugWs &ws, AugRowLds &L, int &b, int &vr, int &vrows, int &objrows,
                                              int &nv) {
    const int t = threadIdx.x, blk = blockIdx.x;
    b = aug_frame_of(ws.blk_off, p.B, blk);
    if (b < 0) return false;
    vr = (blk - ws.blk_off[b]) * AUG_ROWS + t;
    vrows = ws.vrows[b];
    objrows = ws.objrows[b];
    nv = min(ws.nvalid[b], p.T);
    for (int i = t; i < nv * 8; i += AUG_ROWS) L.box[i >> 3][i & 7] = ws.rec[((size_t)b * p.T + (i >> 3)) * AUG_REC + (i & 7)];
    for (int i = t; i <= nv; i += AUG_ROWS) L.spre[i] = ws.spre[(size_t)b * (p.T + 1) + i];
    __syncthreads();
    return true;
}

__global__ __launch_bounds__(AUG_ROWS) void aug_flag_kernel(AugIn in, AugP p, AugWs ws) {
    __shared__ AugRowLds L;
    __shared__ int s_cnt[AUG_ROWS / 64];
    const int t = threadIdx.x, blk = blockIdx.x;
    int b, vr, vrows, objrows, nv;
    if (!aug_row_setup(p, ws, L, b, vr, vrows, objrows, nv)) return;
    bool keep = false;
    if (vr < vrows) {
        float row[LIDAR_AUGMENT_MAX_FEATURES];
        bool is_obj;
        aug_load_row(in, p, ws, L, b, vr, objrows, nv, row, is_obj);
        float x = row[0], y = row[1], z = row[2];
        keep = true;
        if (!is_obj)                                                       // remove_points_in_boxes3d (:158)
            for (int j = 0; j < nv; ++j)
                if (aug_pt_in_box(L.box[j], x, y, z)) { keep = false; break; }
        const AugWorld w = aug_world_of(in, p, b);
        aug_world_xyz(w, x, y, z);
        keep = keep && x >= p.range[0] && x <= p.range[3] && y >= p.range[1] && y <= p.range[4];   // mask_points_by_range
    }
    ws.flags[(size_t)blk * AUG_ROWS + t] = keep ? 1 : 0;
    const unsigned long long bal = __ballot(keep);
    if ((t & 63) == 0) s_cnt[t >> 6] = __popcll(bal);
    __syncthreads();
    if (t == 0) {
        int c = 0;
        for (int q = 0; q < AUG_ROWS / 64; ++q) c += s_cnt[q];
        ws.blk_cnt[blk] = c;
    }
}

__global__ __launch_bounds__(AUG_ROWS) void aug_scan_kernel(AugP p, AugWs ws) {
    __shared__ int s_w[AUG_ROWS / 64];
    const int t = threadIdx.x;
    const int nb = min(ws.blk_off[p.B], p.nblk);
    int carry = 0;
    for (int base = 0; base < nb; base += AUG_ROWS) {
        const int i = base + t;
        const int v = i < nb ? ws.blk_cnt[i] : 0;
        int total;
        const int incl = aug_block_scan(v, s_w, total);
        if (i < nb) ws.blk_base[i] = carry + incl - v;
        carry += total;
    }
    if (t == 0) ws.blk_base[nb] = carry;
}

__global__ __launch_bounds__(AUG_ROWS) void aug_write_kernel(AugIn in, AugP p, AugWs ws, AugOut o) {
    __shared__ AugRowLds L;
    __shared__ int s_cnt[AUG_ROWS / 64];
    const int t = threadIdx.x, blk = blockIdx.x, wv = t >> 6;
    if (blk == 0) {
        const int nb = min(ws.blk_off[p.B], p.nblk);
        for (int f = t; f <= p.B; f += AUG_ROWS) o.offsets[f] = min(ws.blk_base[min(ws.blk_off[f], nb)], p.cap);
    }
    int b, vr, vrows, objrows, nv;
    if (blk >= p.nblk || !aug_row_setup(p, ws, L, b, vr, vrows, objrows, nv)) return;
    const bool keep = ws.flags[(size_t)blk * AUG_ROWS + t] != 0;
    const unsigned long long bal = __ballot(keep);
    if ((t & 63) == 0) s_cnt[wv] = __popcll(bal);
    __syncthreads();
    int pos = ws.blk_base[blk] + __popcll(bal & lanemask_lt());
    for (int q = 0; q < wv; ++q) pos += s_cnt[q];
    if (!keep || pos >= p.cap) return;
    float row[LIDAR_AUGMENT_MAX_FEATURES];
    bool is_obj;
    aug_load_row(in, p, ws, L, b, vr, objrows, nv, row, is_obj);
    const AugWorld w = aug_world_of(in, p, b);
    aug_world_xyz(w, row[0], row[1], row[2]);
    float *dst = o.points + (size_t)pos * p.C;
    if (p.C == 4) *reinterpret_cast<float4 *>(dst) = make_float4(row[0], row[1], row[2], row[3]);
    else {
#pragma unroll
        for (int q = 0; q < LIDAR_AUGMENT_MAX_FEATURES; ++q)
            if (q < p.C) dst[q] = row[q];
    }
}

// ------------------------------------------------------------------ host
static int aug_blocks(int batch, int cap) { return divup(cap, AUG_ROWS) + batch; }

static AugWs aug_carve(void *base, int batch, int T, int nblk, size_t *bytes) {
    size_t off = 0;
    auto take = [&](size_t n) { const size_t at = off; off = align_up(off + n, 256); return at; };
    const size_t a_obj = take(sizeof(int) * batch), a_vr = take(sizeof(int) * batch), a_nv = take(sizeof(int) * batch);
    const size_t a_off = take(sizeof(int) * (batch + 1)), a_cnt = take(sizeof(int) * nblk), a_base = take(sizeof(int) * (nblk + 1));
    const size_t a_spre = take(sizeof(int) * (size_t)batch * (T + 1)), a_rec = take(sizeof(float) * (size_t)batch * T * AUG_REC);
    const size_t a_flags = take((size_t)nblk * AUG_ROWS);
    if (bytes) *bytes = off;
    char *w = static_cast<char *>(base);
    AugWs ws{};
    if (w) {
        ws.objrows = (int *)(w + a_obj); ws.vrows = (int *)(w + a_vr); ws.nvalid = (int *)(w + a_nv); ws.blk_off = (int *)(w + a_off);
        ws.blk_cnt = (int *)(w + a_cnt); ws.blk_base = (int *)(w + a_base); ws.spre = (int *)(w + a_spre);
        ws.rec = (float *)(w + a_rec); ws.flags = (unsigned char *)(w + a_flags);
    }
    return ws;
}

LIDAR_EXPORT int lidar_augment_supported(int num_features, int max_gt, int groups, int per_group) {
    return num_features >= 3 && num_features <= LIDAR_AUGMENT_MAX_FEATURES && groups >= 1 && groups <= LIDAR_AUGMENT_MAX_GROUPS &&
           per_group >= 0 && per_group <= LIDAR_AUGMENT_MAX_PER_GROUP && max_gt >= 0 &&
           (long long)max_gt + (long long)groups * per_group <= LIDAR_AUGMENT_MAX_BOXES;
}

LIDAR_EXPORT size_t lidar_augment_workspace_bytes(int batch, int groups, int per_group, int cap) {
    if (batch <= 0 || groups < 0 || per_group < 0 || cap < 0) return 0;
    size_t bytes = 0;
    aug_carve(nullptr, batch, groups * per_group, aug_blocks(batch, cap), &bytes);
    return bytes;
}

// both entry points: `ps` NULL is lidar_augment, otherwise the poses follow the boxes through aug_frame_kernel<true>
static int aug_run(const char *what, const AugPose *ps, const float *points, const int *point_offsets, int n_points, int num_features,
                   const float *gt_boxes, const int *gt_counts, int batch, int max_gt, const float *db_points, const int *db_offsets,
                   const float *db_boxes, const int *db_cls, int n_obj, int db_rows, const int *cand, int groups, int per_group,
                   const int *flip_x, const int *flip_y, const float *rot, const float *rot_cs, const float *scale,
                   const float *sample_rot, const float *plane, const float *remove_extra_width, const float *collide_extra_width,
                   const float *pc_range, int remove_outside_boxes, int min_num_corners, long long obj_rows_bound, int cap,
                   float *out_points, int *out_offsets, float *out_gt_boxes, int *out_gt_counts, int *sample_valid, void *ws,
                   size_t ws_bytes, void *stream) {
    if (batch < 0 || !lidar_augment_supported(num_features, max_gt, groups, per_group)) return LIDAR_ERR_ARG;
    if (ps && (ps->F < 1 || ps->F > LIDAR_AUGMENT_MF_MAX_FRAMES)) return LIDAR_ERR_ARG;
    if (n_points < 0 || n_obj < 0 || db_rows < 0 || obj_rows_bound < 0 || cap < 0 || !remove_extra_width || !pc_range) return LIDAR_ERR_ARG;
    if ((long long)n_points + obj_rows_bound > (long long)cap) return LIDAR_ERR_ARG;
    if (min_num_corners < 0 || min_num_corners > 8) return LIDAR_ERR_ARG;
    if (batch == 0) return LIDAR_OK;
    const int T = groups * per_group;
    if (!point_offsets || !gt_counts || !flip_x || !flip_y || !rot || !rot_cs || !out_offsets || !out_gt_boxes || !out_gt_counts ||
        (T && (!cand || !sample_valid)) || (max_gt && !gt_boxes) || (n_points && !points) || (cap && !out_points) ||
        (n_obj && (!db_offsets || !db_boxes || !db_cls)) || (db_rows && !db_points) || !ws)
        return LIDAR_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(out_gt_boxes) & 15) || (num_features == 4 && ((reinterpret_cast<uintptr_t>(points) & 15) ||
        (reinterpret_cast<uintptr_t>(db_points) & 15) || (reinterpret_cast<uintptr_t>(out_points) & 15))))
        return LIDAR_ERR_ARG;
    if (ps) {
        if (!ps->out_loc || !ps->out_ry || (max_gt && (!ps->gt_loc || !ps->gt_ry)) || (n_obj && (!ps->db_loc || !ps->db_ry)))
            return LIDAR_ERR_ARG;
        for (const void *q : {(const void *)ps->gt_loc, (const void *)ps->gt_ry, (const void *)ps->db_loc, (const void *)ps->db_ry,
                              (const void *)ps->out_loc, (const void *)ps->out_ry})
            if (reinterpret_cast<uintptr_t>(q) & 3) return LIDAR_ERR_ARG;
    }
    const int nblk = aug_blocks(batch, cap);
    size_t need = 0;
    const AugWs w = aug_carve(ws, batch, T, nblk, &need);
    if (ws_bytes < need) return LIDAR_ERR_WORKSPACE;
    AugP p{};
    p.B = batch; p.M = max_gt; p.G = groups; p.S = per_group; p.C = num_features; p.T = T;
    p.n_points = n_points; p.n_obj = n_obj; p.db_rows = db_rows; p.cap = cap; p.nblk = nblk;
    p.has_cw = collide_extra_width != nullptr; p.has_plane = plane != nullptr; p.has_srot = sample_rot != nullptr;
    p.has_scale = scale != nullptr; p.remove_outside = remove_outside_boxes ? 1 : 0; p.min_corners = min_num_corners;
    for (int q = 0; q < 3; ++q) {
        p.cw[q] = collide_extra_width ? collide_extra_width[q] : 0.0f;
        p.rw[q] = remove_extra_width[q];
    }
    for (int q = 0; q < 6; ++q) p.range[q] = pc_range[q];
    const AugIn in{points, gt_boxes, db_points, db_boxes, rot, rot_cs, scale, sample_rot, plane,
                   point_offsets, gt_counts, db_offsets, db_cls, cand, flip_x, flip_y};
    const AugOut o{out_points, out_gt_boxes, out_offsets, out_gt_counts, sample_valid};
    hipStream_t st = (hipStream_t)stream;
    if (ps) hipLaunchKernelGGL(aug_frame_kernel<true>, dim3(batch), dim3(AUG_TPB), 0, st, in, p, w, o, *ps);
    else hipLaunchKernelGGL(aug_frame_kernel<false>, dim3(batch), dim3(AUG_TPB), 0, st, in, p, w, o, AugPose{});
    hipLaunchKernelGGL(aug_plan_kernel, dim3(1), dim3(AUG_ROWS), 0, st, p, w);
    hipLaunchKernelGGL(aug_flag_kernel, dim3(nblk), dim3(AUG_ROWS), 0, st, in, p, w);
    hipLaunchKernelGGL(aug_scan_kernel, dim3(1), dim3(AUG_ROWS), 0, st, p, w);
    hipLaunchKernelGGL(aug_write_kernel, dim3(nblk), dim3(AUG_ROWS), 0, st, in, p, w, o);
    return lidar_check_launch(what);
}

LIDAR_EXPORT int lidar_augment(const float *points, const int *point_offsets, int n_points, int num_features, const float *gt_boxes,
                               const int *gt_counts, int batch, int max_gt, const float *db_points, const int *db_offsets,
                               const float *db_boxes, const int *db_cls, int n_obj, int db_rows, const int *cand, int groups,
                               int per_group, const int *flip_x, const int *flip_y, const float *rot, const float *rot_cs,
                               const float *scale, const float *sample_rot, const float *plane, const float *remove_extra_width,
                               const float *collide_extra_width, const float *pc_range, int remove_outside_boxes, int min_num_corners,
                               long long obj_rows_bound, int cap, float *out_points, int *out_offsets, float *out_gt_boxes,
                               int *out_gt_counts, int *sample_valid, void *ws, size_t ws_bytes, void *stream) {
    return aug_run("lidar_augment", nullptr, points, point_offsets, n_points, num_features, gt_boxes, gt_counts, batch, max_gt, db_points,
                   db_offsets, db_boxes, db_cls, n_obj, db_rows, cand, groups, per_group, flip_x, flip_y, rot, rot_cs, scale, sample_rot,
                   plane, remove_extra_width, collide_extra_width, pc_range, remove_outside_boxes, min_num_corners, obj_rows_bound, cap,
                   out_points, out_offsets, out_gt_boxes, out_gt_counts, sample_valid, ws, ws_bytes, stream);
}

LIDAR_EXPORT int lidar_augment_mf_supported(int num_features, int max_gt, int groups, int per_group, int stack_frames) {
    return lidar_augment_supported(num_features, max_gt, groups, per_group) && stack_frames >= 1 &&
           stack_frames <= LIDAR_AUGMENT_MF_MAX_FRAMES;
}

LIDAR_EXPORT int lidar_augment_mf(const float *points, const int *point_offsets, int n_points, int num_features, const float *gt_boxes,
                                  const int *gt_counts, int batch, int max_gt, const float *db_points, const int *db_offsets,
                                  const float *db_boxes, const int *db_cls, int n_obj, int db_rows, const int *cand, int groups,
                                  int per_group, const int *flip_x, const int *flip_y, const float *rot, const float *rot_cs,
                                  const float *scale, const float *sample_rot, const float *plane, const float *remove_extra_width,
                                  const float *collide_extra_width, const float *pc_range, int remove_outside_boxes,
                                  int min_num_corners, long long obj_rows_bound, int cap, const float *gt_locations,
                                  const float *gt_rotations_y, const float *db_locations, const float *db_rotations_y, int stack_frames,
                                  float *out_points, int *out_offsets, float *out_gt_boxes, int *out_gt_counts, int *sample_valid,
                                  float *out_locations, float *out_rotations_y, void *ws, size_t ws_bytes, void *stream) {
    const AugPose ps{gt_locations, gt_rotations_y, db_locations, db_rotations_y, out_locations, out_rotations_y, stack_frames};
    return aug_run("lidar_augment_mf", &ps, points, point_offsets, n_points, num_features, gt_boxes, gt_counts, batch, max_gt, db_points,
                   db_offsets, db_boxes, db_cls, n_obj, db_rows, cand, groups, per_group, flip_x, flip_y, rot, rot_cs, scale, sample_rot,
                   plane, remove_extra_width, collide_extra_width, pc_range, remove_outside_boxes, min_num_corners, obj_rows_bound, cap,
                   out_points, out_offsets, out_gt_boxes, out_gt_counts, sample_valid, ws, ws_bytes, stream);
}
