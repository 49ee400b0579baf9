// The point-in-box test shared by roi_pool.hip (RoI pooling, points_in_boxes) and point_head.hip (point-head targets), moved
// here from roi_pool.hip without changing an operation.  Reference: check_pt_in_box3d,
// pcdet/ops/roiaware_pool3d/src/roiaware_pool3d_kernel.cu:23-36 == pcdet/ops/roipoint_pool3d/src/roipoint_pool3d_kernel.cu:22-35,
// evaluated exactly as written there (including its float->double promoted comparisons).
#pragma once
#include "common.h"

struct BoxCS {
    float cx, cy, cz, dx, dy, dz, cosa, sina;
};

// cos(-rz), sin(-rz): correctly rounded fp32 via double (see iou3d.hip heading_cs)
__device__ __forceinline__ BoxCS make_boxcs(const float *b) {
    BoxCS r;
    r.cx = b[0]; r.cy = b[1]; r.cz = b[2]; r.dx = b[3]; r.dy = b[4]; r.dz = b[5];
    const float a = -b[6];
    r.cosa = (float)cos((double)a);
    r.sina = (float)sin((double)a);
    return r;
}

// check_pt_in_box3d (roiaware_pool3d_kernel.cu:23-36 == roipoint_pool3d_kernel.cu:22-35), MARGIN = 1e-5f
__device__ __forceinline__ bool pt_in_box(const BoxCS &b, float x, float y, float z, float &lx, float &ly) {
    const float MARGIN = 1e-5f;
    if ((double)fabsf(z - b.cz) > (double)b.dz / 2.0) return false;
    const float sx = x - b.cx, sy = y - b.cy;
    lx = sx * b.cosa + sy * (-b.sina);
    ly = sx * b.sina + sy * b.cosa;
    return ((double)fabsf(lx) < (double)b.dx / 2.0 + (double)MARGIN) && ((double)fabsf(ly) < (double)b.dy / 2.0 + (double)MARGIN);
}
