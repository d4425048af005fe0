// The anchor of one grid cell: torchvision's AnchorGenerator.grid_anchors as the detector's decode (detect.hip) and the head losses
// (headloss.hip) share it -- one expression, one set of bits.
#pragma once
#include <hip/hip_runtime.h>

// base anchor `an` of `level` shifted to cell (x, y): shift + base, one fp32 add per coordinate (the shift itself is a product of two
// small integers, exact in fp32, so a contracted multiply-add gives the same bits).  base_anchors: [L][A][4].
__device__ __forceinline__ float4 grid_anchor(const float* __restrict__ base_anchors, int level, int A, int an, int x, int y, int stride_w,
                                              int stride_h) {
    const float shx = (float)x * (float)stride_w, shy = (float)y * (float)stride_h;
    const float* ba = base_anchors + ((size_t)level * A + an) * 4;
    return make_float4(shx + ba[0], shy + ba[1], shx + ba[2], shy + ba[3]);
}
