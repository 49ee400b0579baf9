// Element math shared by the loss kernels (anchor_loss.hip, roi_loss.hip, point_head.hip), device only.  Each function follows the
// reference's torch expression op by op in fp32 (the library builds with -ffp-contract=off): expf / log1pf are the device library's
// correctly-rounded-within-an-ulp fp32 functions, as torch's kernels call them.  Reference: pcdet/utils/loss_utils.py
// (SigmoidFocalClassificationLoss :9-72, WeightedSmoothL1Loss :75-136).
//
// The derivatives are those torch autograd forms for the reference's expression, not a simplification of them:
//   clamp(min=0) passes the gradient at 0;  abs has derivative sign0, which is 0 at 0;  torch.where(n < beta, ...) takes the
//   quadratic branch below beta and the linear one AT n == beta;  the focal weight is not detached.
#pragma once
#include "common.h"
#include <math.h>

__device__ __forceinline__ float sign0(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }

// BCE-with-logits in its stable form max(x, 0) - x t + log1p(exp(-|x|)); *dx = sigmoid(x) - t, the sigmoid formed without overflow.
// Equal to binary_cross_entropy(sigmoid(x), t) wherever that function's -100 log clamp does not engage, and continued past it.
__device__ __forceinline__ float bce_logits(float x, float t, float *dx) {
    const float e = expf(-fabsf(x));
    if (dx) *dx = (x >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e)) - t;
    return (fmaxf(x, 0.0f) - x * t) + log1pf(e);
}

// SigmoidFocalClassificationLoss.forward of one element (alpha 0.25, gamma 2) before the anchor / row weight; *dx: d(element)/dx
__device__ __forceinline__ float sigmoid_focal(float x, float tg, float *dx) {
    const float p = 1.0f / (1.0f + expf(-x));                                // torch.sigmoid
    const float aw = tg * 0.25f + (1.0f - tg) * 0.75f;                       // alpha_weight
    const float pt = tg * (1.0f - p) + (1.0f - tg) * p;
    const float fw = aw * (pt * pt);                                         // torch.pow(pt, 2.0) == pt * pt
    const float bce = bce_logits(x, tg, nullptr);
    if (dx) {
        // fw = aw * pt^2, pt(p), p = sigmoid(x): pow backward 2 * pt, sigmoid backward (1 - p) * p
        const float dpt = aw * (2.0f * pt);
        const float dp = dpt * (-tg) + dpt * (1.0f - tg);
        const float dfw = dp * (1.0f - p) * p;
        // bce term by term, as autograd differentiates clamp(x, min=0) - x * t + log1p(exp(-abs(x))): NOT bce_logits' sigmoid(x) - t
        const float e = expf(-fabsf(x));
        const float dbce = (x >= 0.0f ? 1.0f : 0.0f) - tg - (e / (1.0f + e)) * sign0(x);
        *dx = dfw * bce + fw * dbce;
    }
    return fw * bce;
}

// one code of WeightedSmoothL1Loss (beta 1/9): smooth-L1 of (pred - label) * cw, a NaN label taking the prediction (an exact 0
// with gradient 0, loss_utils.py:122); *dx = d / d pred
__device__ __forceinline__ float smooth_l1(float pred, float label, float cw, float *dx) {
    const float BETA = (float)(1.0 / 9.0), HALF_BETA = (float)(0.5 / 9.0);
    const bool nan_t = isnan(label);
    const float d = nan_t ? 0.0f : (pred - label) * cw;
    const float n = fabsf(d);
    const bool quad = n < BETA;
    if (dx) *dx = nan_t ? 0.0f : ((quad ? n / BETA : 1.0f) * sign0(d)) * cw;
    return quad ? 0.5f * (n * n) / BETA : n - HALF_BETA;
}
