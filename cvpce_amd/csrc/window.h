// What the comparator's re-classification (reclass.hip) and its compliance report (report.hip) share: an image's slice of a packed
// table, the validity test of a projected position, and the way from a plan slot to the gallery row its crop was matched to -- one
// expression each, one set of bits.  The tail's per-image status both read is homography.hip's (CVPCE_HOMOGRAPHY_OK).
#pragma once
#include <hip/hip_runtime.h>
#include "../../include/cvpce_amd_homography.h"

struct WnSlice { int at, n; };                  // first row and row count

// image p's rows of a table of `total` rows packed image by image: its two offsets, clamped into the table and into ascending order
__device__ __forceinline__ WnSlice wn_slice(const int* __restrict__ off, int p, int total) {
    const int a0 = min(max(off[p], 0), total), a1 = min(max(off[p + 1], a0), total);
    return {a0, a1 - a0};
}

// torch.clamp(min=lo, max=hi) on the host, comparison by comparison: a NaN fails both and stays, -0 is not below 0 and stays
__device__ __forceinline__ float wn_clamp(float v, float lo, float hi) {
    const float t = v < lo ? lo : v;
    return hi < t ? hi : t;
}

// a projected position clamped to its image of wf x hf pixels
__device__ __forceinline__ float4 wn_clamp_box(float4 b, float wf, float hf) {
    b.x = wn_clamp(b.x, 0.f, wf);
    b.z = wn_clamp(b.z, 0.f, wf);
    b.y = wn_clamp(b.y, 0.f, hf);
    b.w = wn_clamp(b.w, 0.f, hf);
    return b;
}

// whether a clamped position is in view: more than a pixel wide and high, the two subtractions rounded on their own (false on NaN)
__device__ __forceinline__ bool wn_in_view(float4 b) {
#pragma clang fp contract(off)
    return (b.z - b.x > 1.f) && (b.w - b.y > 1.f);
}

// Slot s of an image's plan (row0: the image's first slot; n1: its expected boxes) -> whether it resolves: e, the slot's expected
// index, and j, the gallery row its crop was matched to first (column 0 of its row of the [M][k] match result).  None -- false --
// where the expected index, the crop row or the gallery row (of G) is out of range; e and j are not to be read then.
__device__ __forceinline__ bool wn_slot_gallery_row(const int* __restrict__ expected_index, const int* __restrict__ slot_row,
                                                    const long long* __restrict__ indices, size_t row0, int s, int n1, int M, int k, int G,
                                                    int& e, long long& j) {
    e = expected_index[row0 + s];
    if (e < 0 || e >= n1) return false;
    const int row = slot_row[row0 + s];
    if (row < 0 || row >= M) return false;
    j = indices[(size_t)row * k];
    return !(j < 0 || j >= (long long)G);
}
