// KITTI-eval rotated BEV IoU: rotate_iou_gpu_eval / rotate_iou_kernel_eval of the reference
// (pcdet/datasets/kitti/kitti_object_eval_python/rotate_iou.py:256-330, numba.cuda — not available on ROCm).
// Box format (x, y, w, l, angle); criterion -1: IoU, 0: inter / area(query), 1: inter / area(box), 2: inter.
// One thread per (box, query) pair; the arithmetic follows numba's typing of the reference source (float32 arrays, mixed
// int / float-literal expressions in float64, intersection area accumulated in float64), without FMA contraction.
#include "eval_iou_dev.h"   // the geometry, shared with kitti_eval.hip

namespace {

__global__ __launch_bounds__(256) void rotate_iou_eval_kernel(const float *__restrict__ boxes, int N,
                                                              const float *__restrict__ qboxes, int K, int criterion,
                                                              float *__restrict__ iou) {
    const long long e = (long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= (long long)N * K) return;
    const int n = (int)(e / K), k = (int)(e - (long long)n * K);
    float rb1[5], rb2[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) { rb1[i] = qboxes[(size_t)k * 5 + i]; rb2[i] = boxes[(size_t)n * 5 + i]; }
    iou[e] = ev_rotate_iou(rb1, rb2, criterion);
}

}  // namespace

LIDAR_EXPORT int lidar_rotate_iou_eval(const float *boxes, int n, const float *query_boxes, int k, int criterion, float *iou,
                                       void *stream) {
    if (n < 0 || k < 0 || criterion < -1 || criterion > 2) return LIDAR_ERR_ARG;
    if (n == 0 || k == 0) return LIDAR_OK;
    if (!boxes || !query_boxes || !iou) return LIDAR_ERR_ARG;
    const long long pairs = (long long)n * k;
    const long long blocks = (pairs + 255) / 256;
    if (blocks > 0x7fffffffll) return LIDAR_ERR_ARG;
    hipLaunchKernelGGL(rotate_iou_eval_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, boxes, n, query_boxes, k,
                       criterion, iou);
    return lidar_check_launch("lidar_rotate_iou_eval");
}
