// The IoU the comparator's claim (homography.hip) and its compliance report (report.hip) share: one expression, one set of bits.
#pragma once
#include <hip/hip_runtime.h>

struct HgIouTerms { float inter, uni; };      // the IoU's numerator and denominator

// inter is >= 0 or a NaN (both of its factors are, by the two comparisons with 0)
__device__ __forceinline__ HgIouTerms hg_iou_terms(float4 a, float4 b) {
#pragma clang fp contract(off)
    const float area_a = (a.z - a.x) * (a.w - a.y), area_b = (b.z - b.x) * (b.w - b.y);
    float w = fminf(a.z, b.z) - fmaxf(a.x, b.x);
    float h = fminf(a.w, b.w) - fmaxf(a.y, b.y);
    w = w < 0.f ? 0.f : w;
    h = h < 0.f ? 0.f : h;
    const float inter = w * h;
    return {inter, (area_a + area_b) - inter};
}

// IoU of an expected position a with a detection b: the expression evalmatch.hip holds to the bits of metrics.box_iou
__device__ __forceinline__ float hg_iou(float4 a, float4 b) {
    const HgIouTerms t = hg_iou_terms(a, b);
    return __fdiv_rn(t.inter, t.uni);
}
