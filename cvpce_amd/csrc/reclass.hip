// The comparator's re-classification on the device (include/cvpce_amd_reclass.h; the rule of DESIGN.md 4b): which of the
// expected-but-undetected positions are cropped and classified again, and what the classification makes of the verdict.
//
//   reclass_plan_kernel     one workgroup per image: clamps the projected positions of the unmatched expected boxes to the image,
//                           keeps the ones more than a pixel wide and high, and writes them densely IN INDEX ORDER -- per-wave
//                           ballots, a prefix over the four waves, a running base over the chunks of 256 boxes; no atomics
//   reclass_verdict_kernel  one workgroup per image: the image's found flags in LDS (matched, or re-classified as the expected
//                           label), written out and summed with an integer tree
//
// Compiled with -ffp-contract=off like its neighbours: the two subtractions of the validity test are rounded on their own.
#include "common.h"
#include "window.h"
#include "../../include/cvpce_amd_reclass.h"

#define RC_THREADS CVPCE_RECLASS_THREADS
#define RC_WAVES (RC_THREADS / WAVE)
#define RC_MAX_NODES CVPCE_RECLASS_MAX_NODES

__global__ __launch_bounds__(RC_THREADS) void reclass_plan_kernel(
    const int* __restrict__ status, const int* __restrict__ matched_expected, const float4* __restrict__ positions,
    const int* __restrict__ off1, const int* __restrict__ image, int sumN1, int cap,
    float4* __restrict__ boxes, int* __restrict__ expected_index, int* __restrict__ count) {
#pragma clang fp contract(off)
    __shared__ int s_wave[RC_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const WnSlice expected = wn_slice(off1, p, sumN1);
    const int a0 = expected.at, n1 = expected.n;
    if (status[p] != CVPCE_HOMOGRAPHY_OK || image[3 * p + 2] == 0 || n1 > cap) {      // (uniform)
        if (tid == 0) count[p] = 0;
        return;
    }
    const float hf = (float)image[3 * p], wf = (float)image[3 * p + 1];
    const size_t row0 = (size_t)p * cap;
    int base = 0;
    for (int c0 = 0; c0 < n1; c0 += RC_THREADS) {                             // (uniform: barriers inside)
        const int i = c0 + tid;
        bool valid = false;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (i < n1 && matched_expected[a0 + i] == 0) {
            b = wn_clamp_box(positions[a0 + i], wf, hf);
            valid = wn_in_view(b);                                            // (false on NaN)
        }
        const unsigned long long ballot = __ballot(valid);
        if (lane == 0) s_wave[wave] = __popcll(ballot);
        __syncthreads();
        int before = base, total = 0;
#pragma unroll
        for (int w = 0; w < RC_WAVES; ++w) {
            const int c = s_wave[w];
            before += w < wave ? c : 0;
            total += c;
        }
        if (valid) {
            const int slot = before + __popcll(ballot & ((1ull << lane) - 1ull));          // < n1 <= cap
            boxes[row0 + slot] = b;
            expected_index[row0 + slot] = i;
        }
        base += total;
        __syncthreads();
    }
    if (tid == 0) count[p] = base;
}

__global__ __launch_bounds__(RC_THREADS) void reclass_verdict_kernel(
    const int* __restrict__ expected_index, const int* __restrict__ count, const int* __restrict__ slot_row,
    const long long* __restrict__ indices, const int* __restrict__ gallery_label_id, const int* __restrict__ expected_label_id,
    const int* __restrict__ matched_expected, const int* __restrict__ off1, const int* __restrict__ status,
    int sumN1, int cap, int M, int k, int G, int* __restrict__ found, int* __restrict__ found_count) {
    __shared__ int s_found[RC_MAX_NODES];
    __shared__ int s_sum[RC_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const WnSlice expected = wn_slice(off1, p, sumN1);
    const int a0 = expected.at, n1 = expected.n;
    if (status[p] != CVPCE_HOMOGRAPHY_OK || n1 > cap) {                        // (uniform)
        if (tid == 0) found_count[p] = -1;
        return;
    }
    for (int i = tid; i < n1; i += RC_THREADS) s_found[i] = matched_expected[a0 + i] != 0;
    __syncthreads();
    const int c = min(max(count[p], 0), cap);
    const size_t row0 = (size_t)p * cap;
    for (int s = tid; s < c; s += RC_THREADS) {
        int e;
        long long j;
        if (!wn_slot_gallery_row(expected_index, slot_row, indices, row0, s, n1, M, k, G, e, j)) continue;
        const int want = expected_label_id[a0 + e];
        if (want >= 0 && gallery_label_id[j] == want) s_found[e] = 1;          // (two slots of one box store the same 1)
    }
    __syncthreads();
    int sum = 0;
    for (int i = tid; i < n1; i += RC_THREADS) {
        const int v = s_found[i];
        found[a0 + i] = v;
        sum += v;
    }
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) sum += __shfl_down(sum, d, WAVE);
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < RC_WAVES; ++w) total += s_sum[w];
        found_count[p] = total;
    }
}

static bool rc_common_ok(const int* status, const int* matched_expected, const int* off1, int B, int sumN1, int cap) {
    if (B < 0 || B > 65535 || sumN1 < 0 || cap < 1 || cap > RC_MAX_NODES) return false;
    if (B == 0) return true;
    return status && off1 && (sumN1 == 0 || matched_expected);
}

extern "C" int cvpce_reclass_plan(const int* status, const int* matched_expected, const float* expected_positions, const int* off1,
                                  const int* image, int B, int sumN1, int cap, float* boxes, int* expected_index, int* count, void* stream) {
    if (!rc_common_ok(status, matched_expected, off1, B, sumN1, cap)) return CVPCE_ERR_ARG;
    if (B == 0) return CVPCE_OK;
    if (!image || !boxes || !expected_index || !count || (sumN1 > 0 && !expected_positions)) return CVPCE_ERR_ARG;
    if (((uintptr_t)expected_positions & 15) || ((uintptr_t)boxes & 15)) return CVPCE_ERR_ARG;
    hipLaunchKernelGGL(reclass_plan_kernel, dim3((unsigned)B), dim3(RC_THREADS), 0, (hipStream_t)stream, status, matched_expected,
                       (const float4*)expected_positions, off1, image, sumN1, cap, (float4*)boxes, expected_index, count);
    return cvpce_check_launch();
}

extern "C" int cvpce_reclass_verdict(const int* expected_index, const int* count, const int* slot_row, const long long* indices,
                                     const int* gallery_label_id, const int* expected_label_id, const int* matched_expected, const int* off1,
                                     const int* status, int B, int sumN1, int cap, int M, int k, int G, int* found, int* found_count,
                                     void* stream) {
    if (!rc_common_ok(status, matched_expected, off1, B, sumN1, cap)) return CVPCE_ERR_ARG;
    if (M < 0 || k < 1 || G < 0) return CVPCE_ERR_ARG;
    if (B == 0) return CVPCE_OK;
    if (!expected_index || !count || !slot_row || !found_count || (sumN1 > 0 && (!expected_label_id || !found))) return CVPCE_ERR_ARG;
    if ((M > 0 && !indices) || (G > 0 && !gallery_label_id) || ((uintptr_t)indices & 7)) return CVPCE_ERR_ARG;
    hipLaunchKernelGGL(reclass_verdict_kernel, dim3((unsigned)B), dim3(RC_THREADS), 0, (hipStream_t)stream, expected_index, count, slot_row,
                       indices, gallery_label_id, expected_label_id, matched_expected, off1, status, sumN1, cap, M, k, G, found, found_count);
    return cvpce_check_launch();
}
