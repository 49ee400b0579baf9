// The box and direction columns of the merged 1x1 anchor head for a LIST of anchors instead of every location: AnchorHeadSingle
// computes conv_box / conv_dir_cls on the whole map (pcdet/models/dense_heads/anchor_head_single.py:45-55), but post-processing
// reads them only at the NMS_PRE_MAXSIZE anchors class_agnostic_nms selects (pcdet/models/model_utils/model_nms_utils.py:6-25).
// PointPillar-KITTI bs 16: 65 536 (row, anchor) pairs instead of 857 088 rows x 54 columns.
//
//   out[f][j][q] = bias[col(a, q)] + sum_i x[f][loc][i] * W[i][col(a, q)]          idx = list[f][j] (or j: all anchors),
//   loc = idx / A, a = idx % A, col(a, q) = box_off + 7 a + q (q < 7), dir_off + nbins a + (q - 7) (q >= 7)
//
// x: up to two NHWC part maps (the concat buffers of the split forward), frames_per_part frames of locs_per_frame rows of C floats
// each; W (C, ldw) and bias as FoldedBEVBackbone holds them (head_wt, head_b).
//
// ORDER OF THE SUM (row-independent: a value depends on its row's C inputs and its column's weights, never on the list, the slot,
// the frame, the part, the mode or where the weights were read from).  One wave per candidate.  Lane l starts from 0.0f and adds,
// for g = l, l + 64, l + 128, ... < C / 4 in this order, the four products of float4 group g with fmaf in element order
// (acc = fmaf(x[4g+e], w[4g+e], acc), e = 0..3).  The 64 lane sums then go through the xor butterfly 32, 16, 8, 4, 2, 1
// (wave_sum, common.h: every lane ends with the same bits), and the bias is added last.  No atomics.
//
// The weight columns in use are staged once per workgroup in LDS, transposed to [column][C + 4] (PointPillar: 54 x 388 floats =
// 84 KB), so a lane reads its group of a column as one 16-byte LDS load; configurations whose slice does not fit read the same
// values through L2.  A wave prefetches its next candidate's index and first two row groups under the current one's arithmetic.
#include "common.h"

#define HR_THREADS 1024
#define HR_WAVES (HR_THREADS / 64)
#define HR_MAX_C LIDAR_HEAD_ROWS_MAX_C
#define HR_MAX_A LIDAR_HEAD_ROWS_MAX_ANCHORS
#define HR_MAX_BINS LIDAR_HEAD_ROWS_MAX_DIR_BINS
#define HR_LDS_MAX (128 * 1024)          // weight slices up to here are staged in LDS

struct HrArgs {
    const float *part[2];
    const float *wt, *bias;
    const long long *list;               // (batch, k) anchor ids, or nullptr: all anchors (k == locs * A)
    float *out;                          // (batch, k, 7 + nbins)
    long long locs, k, total;            // rows per frame, candidates per frame, batch * k
    int frames_per_part, C, ldw, box_off, dir_off, A;
};

template <int NB>
__device__ __forceinline__ int hr_col(const HrArgs &p, int a, int q) {
    return q < 7 ? p.box_off + a * 7 + q : p.dir_off + a * NB + (q - 7);
}

// candidate j -> its row and anchor slot.  Indices are the caller's to keep inside [0, locs * A); they are clamped so that a bad
// list cannot leave the maps.
__device__ __forceinline__ const float4 *hr_row(const HrArgs &p, long long j, int &a) {
    const long long f = j / p.k;
    long long idx = p.list ? p.list[j] : j - f * p.k;
    idx = min(max(idx, 0ll), p.locs * p.A - 1);
    const long long loc = idx / p.A;
    a = (int)(idx - loc * p.A);
    const int part = (int)(f / p.frames_per_part);
    const long long lf = f - (long long)part * p.frames_per_part;
    return reinterpret_cast<const float4 *>(p.part[part] + (lf * p.locs + loc) * p.C);
}

template <int NB, bool LDSW>
__device__ __forceinline__ void hr_group(const HrArgs &p, const float *s_w, int pitch, int a, int g, const float4 x, float (&acc)[7 + NB]) {
    constexpr int NC = 7 + NB;
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        float4 w;
        if (LDSW) {
            w = *reinterpret_cast<const float4 *>(s_w + (size_t)(a * NC + q) * pitch + 4 * g);
        } else {
            const float *c = p.wt + (size_t)(4 * g) * p.ldw + hr_col<NB>(p, a, q);
            w = make_float4(c[0], c[p.ldw], c[2 * (size_t)p.ldw], c[3 * (size_t)p.ldw]);
        }
        acc[q] = fmaf(x.x, w.x, acc[q]);
        acc[q] = fmaf(x.y, w.y, acc[q]);
        acc[q] = fmaf(x.z, w.z, acc[q]);
        acc[q] = fmaf(x.w, w.w, acc[q]);
    }
}

template <int NB, bool LDSW>
__global__ __launch_bounds__(HR_THREADS) void head_rows_kernel(const HrArgs p) {
    constexpr int NC = 7 + NB;
    extern __shared__ float4 s_hr4[];
    float *s_w = reinterpret_cast<float *>(s_hr4);
    const int pitch = p.C + 4;           // columns start 4 banks apart: the transposing fill below spreads over the banks
    if (LDSW) {
        const int ncol = p.A * NC;
        for (int e = threadIdx.x; e < p.C * ncol; e += HR_THREADS) {
            const int i = e / ncol, cl = e - i * ncol;
            const int a = cl / NC, q = cl - a * NC;
            s_w[(size_t)cl * pitch + i] = p.wt[(size_t)i * p.ldw + hr_col<NB>(p, a, q)];
        }
        __syncthreads();
    }
    const int lane = lane_id(), c4 = p.C >> 2;
    const long long nw = (long long)gridDim.x * HR_WAVES;
    long long j = (long long)blockIdx.x * HR_WAVES + (threadIdx.x >> 6);
    if (j >= p.total) return;
    const float4 zero4 = make_float4(0.f, 0.f, 0.f, 0.f);
    int a = 0;
    const float4 *row = hr_row(p, j, a);
    float4 x0 = lane < c4 ? row[lane] : zero4, x1 = lane + 64 < c4 ? row[lane + 64] : zero4;
    while (true) {
        const long long jn = j + nw;
        int an = 0;
        const float4 *rown = row;
        float4 n0 = zero4, n1 = zero4;
        if (jn < p.total) {              // the next candidate's loads fly under this one's arithmetic
            rown = hr_row(p, jn, an);
            if (lane < c4) n0 = rown[lane];
            if (lane + 64 < c4) n1 = rown[lane + 64];
        }
        float acc[NC];
#pragma unroll
        for (int q = 0; q < NC; ++q) acc[q] = 0.0f;
        if (lane < c4) hr_group<NB, LDSW>(p, s_w, pitch, a, lane, x0, acc);
        if (lane + 64 < c4) hr_group<NB, LDSW>(p, s_w, pitch, a, lane + 64, x1, acc);
        for (int g = lane + 128; g < c4; g += 64) hr_group<NB, LDSW>(p, s_w, pitch, a, g, row[g], acc);
        float mine = 0.0f;
        int col = 0;
#pragma unroll
        for (int q = 0; q < NC; ++q) {
            const float s = wave_sum(acc[q]);
            if (lane == q) { mine = s; col = hr_col<NB>(p, a, q); }
        }
        if (lane < NC) p.out[j * NC + lane] = mine + p.bias[col];
        if (jn >= p.total) break;
        j = jn; a = an; row = rown; x0 = n0; x1 = n1;
    }
}

static int hr_cu_count() {
    static int cus[64] = {};
    int dev = 0, n = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    dev &= 63;
    if (cus[dev] == 0) cus[dev] = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
    return cus[dev];
}

template <int NB>
static int hr_launch(const HrArgs &p, hipStream_t stream) {
    const size_t lds = (size_t)p.A * (7 + NB) * (p.C + 4) * sizeof(float);
    long long blocks = (p.total + HR_WAVES - 1) / HR_WAVES;
    const long long cap = (long long)hr_cu_count() * (lds <= HR_LDS_MAX ? 1 : 2);      // resident workgroups: waves stride over the list
    if (blocks > cap) blocks = cap;
    if (lds <= HR_LDS_MAX) {
        static bool attr_set[64] = {};                    // the LDS opt-in is a per-device function attribute
        int dev_id = 0;
        (void)hipGetDevice(&dev_id);
        dev_id &= 63;
        if (!attr_set[dev_id]) {
            (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&head_rows_kernel<NB, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                      HR_LDS_MAX);
            attr_set[dev_id] = true;
        }
        hipLaunchKernelGGL((head_rows_kernel<NB, true>), dim3((unsigned)blocks), dim3(HR_THREADS), lds, stream, p);
    } else {
        hipLaunchKernelGGL((head_rows_kernel<NB, false>), dim3((unsigned)blocks), dim3(HR_THREADS), 0, stream, p);
    }
    return lidar_check_launch("lidar_head_rows");
}

// C % 4 == 0, 4 <= C <= 1024, 1 <= A <= 8, 0 <= nbins <= 4, every part map under 2^31 - 1 bytes.  Pure host arithmetic.
LIDAR_EXPORT int lidar_head_rows_supported(int C, int anchors_per_loc, int num_dir_bins, long long part_bytes) {
    return C >= 4 && C <= HR_MAX_C && (C & 3) == 0 && anchors_per_loc >= 1 && anchors_per_loc <= HR_MAX_A && num_dir_bins >= 0 &&
           num_dir_bins <= HR_MAX_BINS && part_bytes >= 0 && part_bytes < 0x7fffffffll;
}

LIDAR_EXPORT int lidar_head_rows(const float *part0, const float *part1, int n_parts, int frames_per_part, long long locs_per_frame, int C,
                                 const float *head_wt, int ldw, const float *head_b, int box_off, int dir_off, int anchors_per_loc,
                                 int num_dir_bins, const long long *idx, int batch, long long k, float *out, void *stream) {
    if (batch < 0 || k < 0 || locs_per_frame < 0 || frames_per_part <= 0 || n_parts < 1 || n_parts > 2 || ldw <= 0 || box_off < 0 ||
        dir_off < 0 || locs_per_frame > 0x7fffffffll / 4 ||
        !lidar_head_rows_supported(C, anchors_per_loc, num_dir_bins, (long long)frames_per_part * locs_per_frame * (C > 0 ? C : 1) * 4))
        return LIDAR_ERR_ARG;
    if (box_off + anchors_per_loc * 7 > ldw || (num_dir_bins > 0 && dir_off + anchors_per_loc * num_dir_bins > ldw) ||
        (long long)n_parts * frames_per_part < batch)
        return LIDAR_ERR_ARG;
    if (!idx && k != locs_per_frame * anchors_per_loc) return LIDAR_ERR_ARG;             // all anchors: k is the anchor count
    if (batch == 0 || k == 0) return LIDAR_OK;
    if (locs_per_frame == 0) return LIDAR_ERR_ARG;
    if (!part0 || (n_parts == 2 && !part1) || !head_wt || !head_b || !out) return LIDAR_ERR_ARG;
    if ((reinterpret_cast<uintptr_t>(part0) & 15) || (reinterpret_cast<uintptr_t>(part1) & 15)) return LIDAR_ERR_ARG;
    if ((long long)batch * k > 0x7fffffffll * 16) return LIDAR_ERR_ARG;
    HrArgs p;
    p.part[0] = part0; p.part[1] = n_parts == 2 ? part1 : part0;
    p.wt = head_wt; p.bias = head_b; p.list = idx; p.out = out;
    p.locs = locs_per_frame; p.k = k; p.total = (long long)batch * k;
    p.frames_per_part = frames_per_part; p.C = C; p.ldw = ldw; p.box_off = box_off; p.dir_off = dir_off; p.A = anchors_per_loc;
    switch (num_dir_bins) {
    case 0: return hr_launch<0>(p, (hipStream_t)stream);
    case 1: return hr_launch<1>(p, (hipStream_t)stream);
    case 2: return hr_launch<2>(p, (hipStream_t)stream);
    case 3: return hr_launch<3>(p, (hipStream_t)stream);
    default: return hr_launch<4>(p, (hipStream_t)stream);
    }
}
