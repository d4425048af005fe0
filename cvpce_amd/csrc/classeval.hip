// The classification harness's comparison on the device (include/cvpce_amd_classeval.h): per ground-truth box, the
// rank of the first neighbour that carries the wanted label and the label of the nearest one.
//
//   classeval_rank_kernel   one wave per query row, four rows per workgroup: the lanes stride over the row's K neighbours and keep
//                           the smallest rank that matches, a shuffle tree takes the wave's minimum, lane 0 stores the record
//
// Integers only.  A row of K = 16 neighbours is two cache lines: nothing here is worth tuning.
#include "common.h"
#include "../../include/cvpce_amd_classeval.h"

#define CE_THREADS CVPCE_CLASSEVAL_THREADS
#define CE_ROWS (CE_THREADS / WAVE)

__global__ __launch_bounds__(CE_THREADS) void classeval_rank_kernel(
    const long long* __restrict__ indices, const int* __restrict__ gallery_label_id, const int* __restrict__ want,
    int Q, int K, int G, int2* __restrict__ records) {
    const int lane = threadIdx.x & (WAVE - 1), wave = threadIdx.x / WAVE;
    const long long q = (long long)blockIdx.x * CE_ROWS + wave;
    if (q >= Q) return;                                                            // (uniform per wave; no barrier below)
    const long long* row = indices + (size_t)q * K;
    const int w = want[q];
    int best = K;
    if (w >= 0) {
        for (int j = lane; j < K; j += WAVE) {                                     // (ascending per lane: the first hit is the lane's smallest)
            const long long g = row[j];
            if (g >= 0 && g < (long long)G && gallery_label_id[g] == w) {
                best = j;
                break;
            }
        }
    }
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) best = min(best, __shfl_xor(best, d, WAVE));
    if (lane == 0) {
        const long long g0 = row[0];
        records[q] = make_int2(best, (g0 >= 0 && g0 < (long long)G) ? gallery_label_id[g0] : -1);
    }
}

extern "C" int cvpce_classeval_rank(const long long* indices, const int* gallery_label_id, const int* want, int Q, int K, int G,
                                    int* records, void* stream) {
    if (K < 1 || Q < 0 || G < 1) return CVPCE_ERR_ARG;
    if (Q == 0) return CVPCE_OK;
    if (!indices || !gallery_label_id || !want || !records) return CVPCE_ERR_ARG;
    if (((uintptr_t)indices & 7) || ((uintptr_t)records & 7)) return CVPCE_ERR_ARG;
    const unsigned blocks = (unsigned)(((long long)Q + CE_ROWS - 1) / CE_ROWS);
    hipLaunchKernelGGL(classeval_rank_kernel, dim3(blocks), dim3(CE_THREADS), 0, (hipStream_t)stream, indices, gallery_label_id, want,
                       Q, K, G, (int2*)records);
    return cvpce_check_launch();
}
