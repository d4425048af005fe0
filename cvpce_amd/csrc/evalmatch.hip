// Detection-to-ground-truth matching for the mAP harnesses (include/cvpce_amd_eval.h): one launch, N images, K thresholds.
//
// Closed form of cvpce_amd.metrics.check_matches: a prediction is a true positive iff it is the first prediction, in
// confidence order, that covers some target at IoU >= threshold -- per target a min over the covering predictions' ranks.
//
// One workgroup per (image, tile of 64 targets).  Every wave holds the tile's 64 targets, one per lane, in registers; the
// four waves stride over the image's predictions, staged through LDS 1024 at a time (box, rank, class id: one LDS address
// per wave per read = a broadcast).  Each lane keeps K running minima of rank; the four waves' minima meet in LDS, then
// `first` is stored and a byte 1 goes to tp[rank] (several targets may store the same 1).  No atomics, no workspace.
//
// The IoU must have the bits of metrics.box_iou on the CPU: the whole file is compiled with FMA contraction off (Makefile)
// and the kernel body repeats it as a pragma; the division is the correctly rounded one.
#include "common.h"
#include "../../include/cvpce_amd_eval.h"
#include <limits.h>

#define EM_THREADS 256
#define EM_WAVES (EM_THREADS / WAVE)
#define EM_TILE 64
#define EM_CHUNK 1024

template <int KT>
__global__ __launch_bounds__(EM_THREADS) void evalmatch_kernel(
    const float4* __restrict__ pred, const int* __restrict__ poff, const int* __restrict__ rank, const int* __restrict__ pcls,
    const float4* __restrict__ tgt, const int* __restrict__ toff, const int* __restrict__ tcls, const float* __restrict__ thr,
    int sumP, int sumT, int tiles, int K, int* __restrict__ first, unsigned char* __restrict__ tp) {
#pragma clang fp contract(off)
    __shared__ float4 s_box[EM_CHUNK];
    __shared__ int s_rank[EM_CHUNK];
    __shared__ int s_cls[EM_CHUNK];
    __shared__ int s_min[EM_WAVES][KT][EM_TILE];

    const int img = blockIdx.x / tiles, tile = blockIdx.x - img * tiles;
    // offsets are device data: clamp them into the packed arrays so that a bad offset table cannot index outside them
    const int t0 = min(max(toff[img], 0), sumT), t1 = min(max(toff[img + 1], t0), sumT);
    const int nt = t1 - t0;
    if (tile * EM_TILE >= nt) return;                      // (uniform over the workgroup)
    const int p0 = min(max(poff[img], 0), sumP), p1 = min(max(poff[img + 1], p0), sumP);
    const int np = p1 - p0;
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;

    const int ti = tile * EM_TILE + lane;
    const bool has = ti < nt;
    const float qnan = __builtin_nanf("");
    float4 tb = make_float4(qnan, qnan, qnan, qnan);       // a lane without a target: NaN IoU, never covered
    int tc = 0;
    if (has) {
        tb = tgt[t0 + ti];
        if (tcls) tc = tcls[t0 + ti];
    }
    const float area_t = (tb.z - tb.x) * (tb.w - tb.y);
    float th[KT];
    int best[KT];
#pragma unroll
    for (int k = 0; k < KT; ++k) {
        th[k] = k < K ? thr[k] : qnan;                     // iou >= NaN is false: padded thresholds never match
        best[k] = INT_MAX;
    }

    for (int c0 = 0; c0 < np; c0 += EM_CHUNK) {
        const int n = min(EM_CHUNK, np - c0);
        __syncthreads();
        for (int i = tid; i < n; i += EM_THREADS) {
            s_box[i] = pred[p0 + c0 + i];
            s_rank[i] = rank[p0 + c0 + i];
            s_cls[i] = pcls ? pcls[p0 + c0 + i] : 0;
        }
        __syncthreads();
        for (int i = wave; i < n; i += EM_WAVES) {
            const float4 pb = s_box[i];
            const int r = s_rank[i];
            const bool same = s_cls[i] == tc;
            const float area_p = (pb.z - pb.x) * (pb.w - pb.y);
            float w = fminf(pb.z, tb.z) - fmaxf(pb.x, tb.x);
            float h = fminf(pb.w, tb.w) - fmaxf(pb.y, tb.y);
            w = w < 0.f ? 0.f : w;
            h = h < 0.f ? 0.f : h;
            const float inter = w * h;
            const float uni = (area_p + area_t) - inter;
            const float iou = __fdiv_rn(inter, uni);
#pragma unroll
            for (int k = 0; k < KT; ++k)
                best[k] = (same && iou >= th[k]) ? min(best[k], r) : best[k];
        }
    }

#pragma unroll
    for (int k = 0; k < KT; ++k) s_min[wave][k][lane] = best[k];
    __syncthreads();
    for (int idx = tid; idx < K * EM_TILE; idx += EM_THREADS) {
        const int k = idx / EM_TILE, l = idx % EM_TILE;
        const int t = tile * EM_TILE + l;
        if (t >= nt) continue;
        int m = s_min[0][k][l];
#pragma unroll
        for (int wv = 1; wv < EM_WAVES; ++wv) m = min(m, s_min[wv][k][l]);
        first[(size_t)k * sumT + t0 + t] = m == INT_MAX ? -1 : m;
        if (m >= 0 && m < np) tp[(size_t)k * sumP + p0 + m] = 1;      // (a rank outside the image is not a valid input: never stored)
    }
}

template <int KT>
static int evalmatch_launch(const float* pred, const int* pred_off, const int* rank, const int* pred_cls, const float* tgt,
                            const int* tgt_off, const int* tgt_cls, const float* thr, int N, int sumP, int sumT, int tiles, int K,
                            int* first, unsigned char* tp, hipStream_t s) {
    hipLaunchKernelGGL(evalmatch_kernel<KT>, dim3((unsigned)(N * tiles)), dim3(EM_THREADS), 0, s, (const float4*)pred, pred_off, rank,
                       pred_cls, (const float4*)tgt, tgt_off, tgt_cls, thr, sumP, sumT, tiles, K, first, tp);
    return cvpce_check_launch();
}

extern "C" int cvpce_eval_match_detections(const float* pred, const int* pred_off, const int* rank, const int* pred_cls,
                                           const float* tgt, const int* tgt_off, const int* tgt_cls, const float* thr,
                                           int N, int sumP, int sumT, int max_targets, int K,
                                           int* first, unsigned char* tp, void* stream) {
    if (K < 1 || K > 16 || N < 0 || sumP < 0 || sumT < 0 || max_targets < 0) return CVPCE_ERR_ARG;
    // (an empty array may come as a null pointer: the both-or-neither rule can only be told where both sides have boxes)
    if (sumP > 0 && sumT > 0 && (pred_cls == nullptr) != (tgt_cls == nullptr)) return CVPCE_ERR_ARG;
    if (((uintptr_t)pred & 15) || ((uintptr_t)tgt & 15)) return CVPCE_ERR_ARG;
    if (N == 0 || sumT == 0 || max_targets == 0) return CVPCE_OK;       // no target anywhere: nothing to write, tp stays zero
    if (!pred_off || !tgt_off || !thr || !first || !tgt || (sumP > 0 && (!pred || !rank || !tp))) return CVPCE_ERR_ARG;
    const long long tiles = ((long long)max_targets + EM_TILE - 1) / EM_TILE;
    if ((long long)N * tiles > 0x7fffffffLL) return CVPCE_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
#define EM_GO(KT) evalmatch_launch<KT>(pred, pred_off, rank, pred_cls, tgt, tgt_off, tgt_cls, thr, N, sumP, sumT, (int)tiles, K, first, tp, s)
    if (K == 1) return EM_GO(1);
    if (K == 2) return EM_GO(2);
    if (K <= 4) return EM_GO(4);
    if (K <= 8) return EM_GO(8);
    return EM_GO(16);
#undef EM_GO
}
