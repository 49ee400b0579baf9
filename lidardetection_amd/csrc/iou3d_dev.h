// Device code of one rotated-box pair, shared by csrc/iou3d.hip (pairwise matrices, NMS) and csrc/proposal_target.hip (RoI
// target assignment): the per-box prologue, the reference's polygon clipper and the exact-zero early-outs.
// Reference: pcdet/ops/iou3d_nms/src/iou3d_nms_kernel.cu:14-234.  The expressions follow the reference one by one in fp32
// (the library builds with -ffp-contract=off); see csrc/iou3d.hip for what is organised differently.
#pragma once
#include "common.h"
#include <math.h>

#define IOU_EPS 1e-8f

struct __attribute__((aligned(16))) BoxPre {
    float cx, cy, hx, hy;     // centre, dx/2, dy/2  (hx,hy as computed by the reference: box[3]/2)
    float c, s;               // cosf(heading), sinf(heading)
    float area, rad;          // dx*dy ; conservative bounding radius incl. margins
    float px[4], py[4];       // rotated corners, reference order
};

struct pt2 { float x, y; };

__device__ __forceinline__ float cross3(pt2 p1, pt2 p2, pt2 p0) {
    return (p1.x - p0.x) * (p2.y - p0.y) - (p2.x - p0.x) * (p1.y - p0.y);
}

// float trig of the heading.  Evaluated in double and rounded once: this is the correctly rounded
// fp32 result except in ~1e-8 of cases, which is what a good host libm returns as well.
__device__ __forceinline__ void heading_cs(float a, float &c, float &s) {
    c = (float)cos((double)a);
    s = (float)sin((double)a);
}

__device__ __forceinline__ BoxPre make_pre(const float *b) {
    BoxPre r;
    r.cx = b[0]; r.cy = b[1];
    r.hx = b[3] / 2; r.hy = b[4] / 2;
    heading_cs(b[6], r.c, r.s);
    r.area = b[3] * b[4];
    const float x1 = r.cx - r.hx, y1 = r.cy - r.hy, x2 = r.cx + r.hx, y2 = r.cy + r.hy;
    const float xs[4] = {x1, x2, x2, x1}, ys[4] = {y1, y1, y2, y2};
#pragma unroll
    for (int k = 0; k < 4; ++k) {  // rotate_around_center, kernel.cu:94-98
        r.px[k] = (xs[k] - r.cx) * r.c + (ys[k] - r.cy) * (-r.s) + r.cx;
        r.py[k] = (xs[k] - r.cx) * r.s + (ys[k] - r.cy) * r.c + r.cy;
    }
    r.rad = sqrtf(r.hx * r.hx + r.hy * r.hy) * 1.0001f + 0.02f;
    return r;
}

// check_in_box2d (kernel.cu:51-61): cos(-h) == cos(h), sin(-h) == -sin(h) bit for bit
__device__ __forceinline__ bool in_box2d(const BoxPre &B, float px, float py) {
    const float MARGIN = 1e-2f;
    const float ac = B.c, as = -B.s;
    const float rx = (px - B.cx) * ac + (py - B.cy) * (-as);
    const float ry = (px - B.cx) * as + (py - B.cy) * ac;
    return (fabsf(rx) < B.hx + MARGIN) && (fabsf(ry) < B.hy + MARGIN);
}

// intersection (kernel.cu:63-92)
__device__ __forceinline__ bool seg_intersect(pt2 p1, pt2 p0, pt2 q1, pt2 q0, pt2 &ans) {
    const bool rc = fminf(p0.x, p1.x) <= fmaxf(q0.x, q1.x) && fminf(q0.x, q1.x) <= fmaxf(p0.x, p1.x) &&
                    fminf(p0.y, p1.y) <= fmaxf(q0.y, q1.y) && fminf(q0.y, q1.y) <= fmaxf(p0.y, p1.y);
    if (!rc) return false;
    const float s1 = cross3(q0, p1, p0);
    const float s2 = cross3(p1, q1, p0);
    const float s3 = cross3(p0, q1, q0);
    const float s4 = cross3(q1, p1, q0);
    if (!(s1 * s2 > 0 && s3 * s4 > 0)) return false;
    const float s5 = cross3(q1, p1, p0);
    if (fabsf(s5 - s1) > IOU_EPS) {
        ans.x = (s5 * q0.x - s1 * q1.x) / (s5 - s1);
        ans.y = (s5 * q0.y - s1 * q1.y) / (s5 - s1);
    } else {
        const float a0 = p0.y - p1.y, b0 = p1.x - p0.x, c0 = p0.x * p1.y - p1.x * p0.y;
        const float a1 = q0.y - q1.y, b1 = q1.x - q0.x, c1 = q0.x * q1.y - q1.x * q0.y;
        const float D = a0 * b1 - a1 * b0;
        ans.x = (b0 * c1 - b1 * c0) / D;
        ans.y = (a1 * c0 - a0 * c1) / D;
    }
    return true;
}

__device__ __forceinline__ bool circles_apart(const BoxPre &A, const BoxPre &B) {
    const float dx = A.cx - B.cx, dy = A.cy - B.cy;
    const float rr = A.rad + B.rad;
    return dx * dx + dy * dy > rr * rr;
}

// Separating-axis test on the two rectangles, each inflated by the reference's in-box margin (and a
// little more for rounding): if an axis of either box separates them, the reference finds no edge
// crossing and no contained corner, i.e. it returns exactly 0 for the pair.
__device__ __forceinline__ bool sat_separated_one(const BoxPre &A, const BoxPre &B) {
    const float m = 0.011f;
    float umin = 3.0e38f, umax = -3.0e38f, vmin = 3.0e38f, vmax = -3.0e38f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const float dx = B.px[k] - A.cx, dy = B.py[k] - A.cy;
        const float u = dx * A.c + dy * A.s, v = dy * A.c - dx * A.s;
        umin = fminf(umin, u); umax = fmaxf(umax, u);
        vmin = fminf(vmin, v); vmax = fmaxf(vmax, v);
    }
    const float ex = A.hx * 1.0001f + m, ey = A.hy * 1.0001f + m;
    return (umin > ex) || (umax < -ex) || (vmin > ey) || (vmax < -ey);
}
__device__ __forceinline__ bool sat_separated(const BoxPre &A, const BoxPre &B) {
    return sat_separated_one(A, B) || sat_separated_one(B, A);
}

// Per-thread vertex scratch lives in LDS, laid out [slot][thread] (conflict-free): the polygon vertices
// are APPENDED there (data-dependent count, write-only, no waiting); sorting and the area sum then run
// on registers with statically indexed, predicated steps.  TPB = threads per block of the caller.
template <int TPB>
struct VertScratch {
    float x[16][TPB], y[16][TPB];
};

// the reference's bubble sort by atan2 around the centre (strict >, kernel.cu:199-209) and shoelace
// fan (:218-224), as the same sequence of compare/swap decisions on M register slots
template <int M, int TPB>
__device__ __forceinline__ float polygon_area_sorted(const VertScratch<TPB> &S, int t, int cnt, float ctrx, float ctry) {
    float vx[M], vy[M], va[M];
#pragma unroll
    for (int k = 0; k < M; ++k) {
        vx[k] = S.x[k][t];
        vy[k] = S.y[k][t];
    }
#pragma unroll
    for (int k = 0; k < M; ++k) va[k] = atan2f(vy[k] - ctry, vx[k] - ctrx);
#pragma unroll
    for (int j = 0; j < M - 1; ++j) {
#pragma unroll
        for (int i = 0; i < M - 1 - j; ++i) {
            const bool sw = (i < cnt - j - 1) && (va[i] > va[i + 1]);
            const float ax = vx[i], ay = vy[i], aa = va[i];
            vx[i] = sw ? vx[i + 1] : ax; vy[i] = sw ? vy[i + 1] : ay; va[i] = sw ? va[i + 1] : aa;
            vx[i + 1] = sw ? ax : vx[i + 1]; vy[i + 1] = sw ? ay : vy[i + 1]; va[i + 1] = sw ? aa : va[i + 1];
        }
    }
    float area = 0.f;
#pragma unroll
    for (int k = 0; k < M - 1; ++k) {
        const float ax = vx[k] - vx[0], ay = vy[k] - vy[0];
        const float bx = vx[k + 1] - vx[0], by = vy[k + 1] - vy[0];
        const float term = ax * by - ay * bx;
        if (k < cnt - 1) area += term;
    }
    return fabsf(area) * 0.5f;
}

// box_overlap (kernel.cu:104-225) on pre-computed boxes.  Polygon of at most 16 vertices.
template <int TPB>
__device__ float box_overlap_pre(const BoxPre &A, const BoxPre &B, VertScratch<TPB> &S, int t) {
    int cnt = 0;
    float sumx = 0.f, sumy = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const pt2 a0 = {A.px[i], A.py[i]}, a1 = {A.px[(i + 1) & 3], A.py[(i + 1) & 3]};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const pt2 b0 = {B.px[j], B.py[j]}, b1 = {B.px[(j + 1) & 3], B.py[(j + 1) & 3]};
            pt2 ans;
            if (seg_intersect(a1, a0, b1, b0, ans)) {
                sumx = sumx + ans.x;
                sumy = sumy + ans.y;
                if (cnt < 16) { S.x[cnt][t] = ans.x; S.y[cnt][t] = ans.y; }
                cnt++;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (in_box2d(A, B.px[k], B.py[k])) {
            sumx = sumx + B.px[k]; sumy = sumy + B.py[k];
            if (cnt < 16) { S.x[cnt][t] = B.px[k]; S.y[cnt][t] = B.py[k]; }
            cnt++;
        }
        if (in_box2d(B, A.px[k], A.py[k])) {
            sumx = sumx + A.px[k]; sumy = sumy + A.py[k];
            if (cnt < 16) { S.x[cnt][t] = A.px[k]; S.y[cnt][t] = A.py[k]; }
            cnt++;
        }
    }
    if (cnt == 0) return 0.f;
    if (cnt > 16) cnt = 16;  // the reference's buffer is Point[16]; unreachable for convex quads
    const float ctrx = sumx / cnt, ctry = sumy / cnt;
    if (cnt <= 8) return polygon_area_sorted<8, TPB>(S, t, cnt, ctrx, ctry);
    return polygon_area_sorted<16, TPB>(S, t, cnt, ctrx, ctry);
}

__device__ __forceinline__ float iou_from_overlap(float sa, float sb, float s) {
    return s / fmaxf(sa + sb - s, IOU_EPS);
}
