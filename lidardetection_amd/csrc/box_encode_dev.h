// ResidualCoder.encode_torch (pcdet/utils/box_coder_utils.py:13-42) of one (gt, anchor) pair, shared by the anchor target
// assigners (csrc/anchor_assign.hip, csrc/atss_assign.hip).  log / sin / cos are evaluated in double and rounded once; every
// other column is the reference's fp32 expression (the library builds with -ffp-contract=off).
#pragma once
#include "common.h"
#include <math.h>

// g: gt box (>= 7 columns, extras from column 7), a: anchor (same), out: code_size floats.  The caller has checked that
// code_size == 6 + (sincos ? 2 : 1) + min(gt extras, anchor extras) (zip(cgs, cas)).
__device__ __forceinline__ void residual_encode(const float *g, const float *a, float *out, int sincos, int code_size) {
    const float xa = a[0], ya = a[1], za = a[2], ra = a[6];
    const float dxa = fmaxf(a[3], 1e-5f), dya = fmaxf(a[4], 1e-5f), dza = fmaxf(a[5], 1e-5f);
    const float dxg = fmaxf(g[3], 1e-5f), dyg = fmaxf(g[4], 1e-5f), dzg = fmaxf(g[5], 1e-5f);
    const float diagonal = sqrtf(dxa * dxa + dya * dya);
    out[0] = (g[0] - xa) / diagonal;
    out[1] = (g[1] - ya) / diagonal;
    out[2] = (g[2] - za) / dza;
    out[3] = (float)log((double)(dxg / dxa));
    out[4] = (float)log((double)(dyg / dya));
    out[5] = (float)log((double)(dzg / dza));
    const float rg = g[6];
    int q = 6;
    if (sincos) {
        out[q++] = (float)cos((double)rg) - (float)cos((double)ra);
        out[q++] = (float)sin((double)rg) - (float)sin((double)ra);
    } else {
        out[q++] = rg - ra;
    }
    for (int e = 7; q < code_size; ++e) out[q++] = g[e] - a[e];
}
