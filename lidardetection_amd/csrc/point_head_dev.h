// What point_head.hip (single-frame point heads) and point_head_mf.hip (PointHeadSimpleMultiFrame) share, moved here from
// point_head.hip without changing an operation: the tile width, the declared limits, the gt row as it is staged in LDS, and the
// contiguous tile copies of a row-major matrix through LDS.  The in-box test is pt_in_box_dev.h's, the element math loss_dev.h's,
// the ordered workgroup sum common.h's block_sum.
#pragma once
#include "common.h"
#include "pt_in_box_dev.h"

#define PH_THREADS 256
#define PH_MAX_N LIDAR_POINT_HEAD_MAX_POINTS
#define PH_MAX_B LIDAR_POINT_HEAD_MAX_BATCH
#define PH_MAX_M LIDAR_POINT_HEAD_MAX_GT

struct PHGt {
    BoxCS b;               // the gt box: centre, dims, cos / sin of -rz
    float ex, ey, ez;      // enlarged dims (float32 sums, as enlarge_box3d forms them)
    float rz, cls;
};

// a gt row [box7 | class] as the target kernels stage it; extra: GT_EXTRA_WIDTH
__device__ __forceinline__ PHGt ph_stage_gt(const float *row, const float *extra) {
    PHGt r;
    r.b = make_boxcs(row);
    r.ex = row[3] + extra[0]; r.ey = row[4] + extra[1]; r.ez = row[5] + extra[2];
    r.rz = row[6]; r.cls = row[7];
    return r;
}

// the staged row with its enlarged dims
__device__ __forceinline__ BoxCS ph_enlarged(const PHGt &r) {
    BoxCS e = r.b;
    e.dx = r.ex; e.dy = r.ey; e.dz = r.ez;
    return e;
}

// the frame a point's bs_idx names, -1 for a value that names none of [0, batch)
__device__ __forceinline__ int ph_frame_of(float bs, int batch) {
    return (bs >= 0.0f && bs < (float)batch && bs == (float)(int)bs) ? (int)bs : -1;
}

// the range [lo, hi] of the frames the workgroup's threads name (frame -1: none); s_lo / s_hi: one int per wave.  Ends with every
// thread holding the range; lo > hi when no thread names a frame.
__device__ __forceinline__ void ph_frame_range(int frame, int batch, int *s_lo, int *s_hi, int &lo, int &hi) {
    lo = frame >= 0 ? frame : batch; hi = frame;
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        lo = min(lo, __shfl_xor(lo, d, 64));
        hi = max(hi, __shfl_xor(hi, d, 64));
    }
    if (lane_id() == 0) { s_lo[threadIdx.x >> 6] = lo; s_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < PH_THREADS / 64; ++k) { lo = min(lo, s_lo[k]); hi = max(hi, s_hi[k]); }
}

// the rows [row0, row0 + PH_THREADS) x width floats of a row-major matrix -> s (contiguous global reads)
__device__ __forceinline__ void ph_tile_load(float *s, const float *__restrict__ src, long long row0, int n, int width) {
    const long long base = row0 * width;
    const int cnt = (int)min((long long)PH_THREADS * width, (long long)n * width - base);
    for (int k = threadIdx.x; k < cnt; k += PH_THREADS) s[k] = src[base + k];
}

__device__ __forceinline__ void ph_tile_store(const float *s, float *__restrict__ dst, long long row0, int n, int width) {
    const long long base = row0 * width;
    const int cnt = (int)min((long long)PH_THREADS * width, (long long)n * width - base);
    for (int k = threadIdx.x; k < cnt; k += PH_THREADS) dst[base + k] = s[k];
}
