// The comparator's compliance report on the device (include/cvpce_amd_report.h; the report rule of DESIGN.md 4b): what became of
// every expected position, which unclaimed detection sits on a position that was not detected, which sit on none.
//
//   report_positions_kernel  one workgroup per image.  The image's detection boxes are staged in LDS once, as float4 in index order
//                            (lane l of a wave reads box c0 + l with one ds_read_b128: the 16 lanes of each of its four lane groups
//                            cover the 16 slots of one 256-byte bank row, no conflict), beside a flag per detection: unclaimed.  One
//                            WAVE per undetected position: its lanes walk the detections in ascending j, each keeps its best (largest
//                            IoU, first j; the division only where the boxes overlap), and an ordered butterfly -- larger IoU, then
//                            lower j: a total order, so every lane ends with the same winner whatever the pairing -- reduces the 64.
//                            Lane 0 writes the position's row and marks the occupant in an LDS flag array (every writer stores 1); the
//                            strays are read off it after a barrier.
//   report_reclass_kernel    one workgroup per image: the lowest slot of every position by an LDS integer minimum, a recovered flag
//                            (every writer stores 1), then one pass over the positions.
//
// Compiled with -ffp-contract=off like its neighbours: the validity test is reclass.hip's (window.h), the IoU is homography.hip's (iou.h).
#include "common.h"
#include "iou.h"
#include "window.h"
#include "../../include/cvpce_amd_report.h"
#include <limits.h>

#define RP_THREADS CVPCE_REPORT_THREADS
#define RP_WAVES (RP_THREADS / WAVE)
#define RP_MAX_NODES CVPCE_REPORT_MAX_NODES

// whether candidate (iou, j) comes before (best, bj): larger IoU, then lower index; j == INT_MAX stands for "none" and loses to all
__device__ __forceinline__ bool rp_before(float iou, int j, float best, int bj) {
    return j != INT_MAX && (bj == INT_MAX || iou > best || (iou == best && j < bj));
}

__global__ __launch_bounds__(RP_THREADS) void report_positions_kernel(
    const int* __restrict__ status, const int* __restrict__ matched_expected, const int* __restrict__ matched_actual,
    const float4* __restrict__ positions, const float4* __restrict__ boxes, const int* __restrict__ off1, const int* __restrict__ off2,
    const int* __restrict__ image, const int* __restrict__ actual_row, double iou_thr, int sumN1, int sumN2,
    int* __restrict__ outcome, int* __restrict__ occupant, float* __restrict__ occupant_iou, int* __restrict__ occupant_row,
    int* __restrict__ stray) {
#pragma clang fp contract(off)
    __shared__ float4 s_box[RP_MAX_NODES];
    __shared__ int s_free[RP_MAX_NODES];            // matched_actual == 0
    __shared__ int s_occupant[RP_MAX_NODES];        // some position's occupant
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const WnSlice expected = wn_slice(off1, p, sumN1), actual = wn_slice(off2, p, sumN2);
    const int a0 = expected.at, n1 = expected.n, b0 = actual.at, n2 = actual.n;
    if (status[p] != CVPCE_HOMOGRAPHY_OK || n1 > RP_MAX_NODES || n2 > RP_MAX_NODES) return;      // (uniform)
    for (int j = tid; j < n2; j += RP_THREADS) {
        s_box[j] = boxes[b0 + j];
        s_free[j] = matched_actual[b0 + j] == 0;
        s_occupant[j] = 0;
    }
    __syncthreads();
    const bool any_iou = !(iou_thr > 0.0);          // a threshold that an IoU of 0 may pass (or a NaN): no pair is skipped
    const int enabled = image[3 * p + 2];
    const float hf = (float)image[3 * p], wf = (float)image[3 * p + 1];
    for (int e = wave; e < n1; e += RP_WAVES) {                                          // (uniform per wave: shuffles inside)
        const bool matched = matched_expected[a0 + e] != 0;
        const float4 pos = positions[a0 + e];
        float best = -1.f;
        int bj = INT_MAX;
        if (!matched) {
            for (int j = lane; j < n2; j += WAVE) {
                const HgIouTerms t = hg_iou_terms(pos, s_box[j]);
                // the numerator is >= 0 or a NaN: where it is not above 0 the IoU is 0, -0 or a NaN and fails a threshold above 0 --
                // the pairs that do not overlap, nearly all of them, cost no division
                if (s_free[j] && (t.inter > 0.f || any_iou)) {
                    const float iou = __fdiv_rn(t.inter, t.uni);                         // (hg_iou's bits)
                    if ((double)iou >= iou_thr && rp_before(iou, j, best, bj)) {         // (false on NaN)
                        best = iou;
                        bj = j;
                    }
                }
            }
#pragma unroll
            for (int d = WAVE / 2; d > 0; d >>= 1) {
                const float o = __shfl_xor(best, d, WAVE);
                const int oj = __shfl_xor(bj, d, WAVE);
                if (rp_before(o, oj, best, bj)) {
                    best = o;
                    bj = oj;
                }
            }
        }
        if (lane == 0) {
            int code = CVPCE_REPORT_DETECTED;
            if (!matched) {
                if (enabled == 0) {
                    code = CVPCE_REPORT_UNCHECKED;
                } else {
                    code = wn_in_view(wn_clamp_box(pos, wf, hf)) ? CVPCE_REPORT_PENDING : CVPCE_REPORT_OUT_OF_VIEW;      // (false on NaN)
                }
            }
            const bool has = bj != INT_MAX;                                              // (then 0 <= bj < n2)
            outcome[a0 + e] = code;
            occupant[a0 + e] = has ? bj : -1;
            occupant_iou[a0 + e] = has ? best : -1.f;
            occupant_row[a0 + e] = has && actual_row ? actual_row[b0 + bj] : -1;
            if (has) s_occupant[bj] = 1;                                                 // (any writer: they all write 1)
        }
    }
    __syncthreads();
    for (int j = tid; j < n2; j += RP_THREADS) stray[b0 + j] = s_free[j] && !s_occupant[j] ? 1 : 0;
}

__global__ __launch_bounds__(RP_THREADS) void report_reclass_kernel(
    const int* __restrict__ expected_index, const int* __restrict__ count, const int* __restrict__ slot_row,
    const long long* __restrict__ indices, const float* __restrict__ distances, const int* __restrict__ gallery_label_id,
    const int* __restrict__ expected_label_id, const int* __restrict__ off1, const int* __restrict__ status, int sumN1, int cap, int M,
    int k, int G, int* __restrict__ outcome, int* __restrict__ seen_row, float* __restrict__ seen_distance) {
    __shared__ int s_first[RP_MAX_NODES];           // the lowest slot of the position with an in-range row and index
    __shared__ int s_recovered[RP_MAX_NODES];
    const int p = blockIdx.x, tid = threadIdx.x;
    const WnSlice expected = wn_slice(off1, p, sumN1);
    const int a0 = expected.at, n1 = expected.n;
    if (status[p] != CVPCE_HOMOGRAPHY_OK || n1 > cap) return;                           // (uniform)
    for (int i = tid; i < n1; i += RP_THREADS) {
        s_first[i] = INT_MAX;
        s_recovered[i] = 0;
    }
    __syncthreads();
    const int c = min(max(count[p], 0), cap);
    const size_t row0 = (size_t)p * cap;
    for (int s = tid; s < c; s += RP_THREADS) {
        int e;
        long long j;
        if (!wn_slot_gallery_row(expected_index, slot_row, indices, row0, s, n1, M, k, G, e, j)) continue;
        atomicMin(&s_first[e], s);                                                       // (LDS integer minimum: any order, one result)
        const int want = expected_label_id[a0 + e];
        if (want >= 0 && gallery_label_id[j] == want) s_recovered[e] = 1;                // (any writer: they all write 1)
    }
    __syncthreads();
    for (int i = tid; i < n1; i += RP_THREADS) {
        int row_seen = -1;
        float dist = -1.f;
        if (outcome[a0 + i] == CVPCE_REPORT_PENDING) {
            const int s = s_first[i];
            if (s != INT_MAX) {                                                          // (slot, row and index were checked above)
                const size_t at = (size_t)slot_row[row0 + s] * k;
                row_seen = (int)indices[at];
                dist = distances[at];
            }
            outcome[a0 + i] = s_recovered[i] ? CVPCE_REPORT_RECOVERED : CVPCE_REPORT_MISSING;
        }
        seen_row[a0 + i] = row_seen;
        seen_distance[a0 + i] = dist;
    }
}

static bool rp_common_ok(const int* status, const int* off1, int B, int sumN1) {
    if (B < 0 || B > 65535 || sumN1 < 0) return false;
    if (B == 0) return true;
    return status && off1;
}

extern "C" int cvpce_report_positions(const int* status, const int* matched_expected, const int* matched_actual, const float* expected_positions,
                                      const float* actual_boxes, const int* off1, const int* off2, const int* image, const int* actual_row,
                                      double iou_threshold, int B, int sumN1, int sumN2, int* outcome, int* occupant, float* occupant_iou,
                                      int* occupant_row, int* stray, void* stream) {
    if (!rp_common_ok(status, off1, B, sumN1) || sumN2 < 0) return CVPCE_ERR_ARG;
    if (B == 0) return CVPCE_OK;
    if (!off2 || !image) return CVPCE_ERR_ARG;
    if (sumN1 > 0 && (!matched_expected || !expected_positions || !outcome || !occupant || !occupant_iou || !occupant_row)) return CVPCE_ERR_ARG;
    if (sumN2 > 0 && (!matched_actual || !actual_boxes || !stray)) return CVPCE_ERR_ARG;
    if (((uintptr_t)expected_positions & 15) || ((uintptr_t)actual_boxes & 15)) return CVPCE_ERR_ARG;
    hipLaunchKernelGGL(report_positions_kernel, dim3((unsigned)B), dim3(RP_THREADS), 0, (hipStream_t)stream, status, matched_expected,
                       matched_actual, (const float4*)expected_positions, (const float4*)actual_boxes, off1, off2, image, actual_row,
                       iou_threshold, sumN1, sumN2, outcome, occupant, occupant_iou, occupant_row, stray);
    return cvpce_check_launch();
}

extern "C" int cvpce_report_reclass(const int* expected_index, const int* count, const int* slot_row, const long long* indices,
                                    const float* distances, const int* gallery_label_id, const int* expected_label_id, const int* off1,
                                    const int* status, int B, int sumN1, int cap, int M, int k, int G, int* outcome, int* seen_row,
                                    float* seen_distance, void* stream) {
    if (!rp_common_ok(status, off1, B, sumN1) || cap < 1 || cap > RP_MAX_NODES || M < 0 || k < 1 || G < 0) return CVPCE_ERR_ARG;
    if (B == 0) return CVPCE_OK;
    if (!expected_index || !count || !slot_row) return CVPCE_ERR_ARG;
    if (sumN1 > 0 && (!expected_label_id || !outcome || !seen_row || !seen_distance)) return CVPCE_ERR_ARG;
    if ((M > 0 && (!indices || !distances)) || (G > 0 && !gallery_label_id) || ((uintptr_t)indices & 7)) return CVPCE_ERR_ARG;
    hipLaunchKernelGGL(report_reclass_kernel, dim3((unsigned)B), dim3(RP_THREADS), 0, (hipStream_t)stream, expected_index, count, slot_row,
                       indices, distances, gallery_label_id, expected_label_id, off1, status, sumN1, cap, M, k, G, outcome, seen_row,
                       seen_distance);
    return cvpce_check_launch();
}
