// Tonioni's common-subgraph search for a batch of (expected, actual) graph pairs (include/ext/cvpce_amd_tonioni.h; the Tonioni
// rule of DESIGN.md 4b).  Integers only.
//
// tonioni_hyp_kernel: one workgroup per pair.  The hypothesis builder of the match kernel (pg_hypotheses.h) writes the pair's seed
// pairs in their final order to the workspace, and their number.
//
// tonioni_run_kernel: one workgroup per (pair, start).  The pair's hypotheses from `start` on are copied into LDS as 32-bit keys
// -- (TN_OFF + score8) << 20 | n1 << 10 | n2, score8 = -agree - 8 * bumps: ascending key = ascending (score, n1, n2), and the keys
// of a run are distinct because (n1, n2) is -- and the run is played to its end (tn_run).  Its size F and the minimum M of its
// bound go to the workspace; nothing is given up here, because only the best size so far couples the starts.
//
// tonioni_select_kernel: one workgroup per pair.  Every thread walks the (M, F) of the pair in start order (the scan below), the
// adopted start is played again, and this time its pairs are written, in the order they were taken.
//
// The key's score field is 11 bits wide: agree <= 8 and bumps <= 254 fit.  Under the graph rule a hypothesis (x1, x2) is bumped at
// most 8 times: it is bumped by a head (n1, n2) with nbr1[n1][d] == x1, edges are symmetric, so n1 = nbr1[x1][d + 4] -- at most
// one n1 per direction, and a node is head once.  Tables that break the rule are still safe: the field saturates.
#include "common.h"
#include "../../include/ext/cvpce_amd_tonioni.h"
#include "../../include/cvpce_amd_planogram.h"
#include <limits.h>
#include "pg_hypotheses.h"

#define TN_THREADS PG_THREADS
#define TN_WAVES (TN_THREADS / WAVE)
#define TN_MAX_NODES CVPCE_PLANOGRAM_MAX_NODES
#define TN_DEAD 0xFFFFFFFFu
#define TN_OFF 2040                    // score field = TN_OFF + score8, 0 .. 2040

// word offsets of the workspace's three parts: hypotheses [sum_hyp], (M, F) [sum_hyp][2], hypothesis counts [P]
__host__ __device__ static inline size_t tn_ws_mf(long long sum_hyp) { return (size_t)sum_hyp; }
__host__ __device__ static inline size_t tn_ws_count(long long sum_hyp) { return (size_t)sum_hyp * 3; }

struct TnHypLds {
    int nl2, lab1, lab2, un, nb1, nb2, total;
};

__host__ __device__ static inline TnHypLds tn_hyp_lds(int n1, int n2) {
    TnHypLds l;
    int o = 0;
    l.nl2 = o; o += 4 * 8 * n2;
    l.lab1 = o; o += 4 * n1;
    l.lab2 = o; o += 4 * n2;
    l.un = o; o += 4 * 9 * n1;
    l.nb1 = o; o += 2 * 8 * n1;
    l.nb2 = o; o += 2 * 8 * n2;
    l.total = o;
    return l;
}

__global__ __launch_bounds__(TN_THREADS) void tonioni_hyp_kernel(
    const int* __restrict__ nbr1, const int* __restrict__ label1, const int* __restrict__ off1,
    const int* __restrict__ nbr2, const int* __restrict__ label2, const int* __restrict__ off2,
    const int* __restrict__ hyp_off, int sumN1, int sumN2, int max_n1, int max_n2, int max_hyp, int sum_hyp,
    int* __restrict__ hyp, int* __restrict__ hcount) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_part[PG_THREADS];
    __shared__ int s_total;
    const int p = blockIdx.x, tid = threadIdx.x;
    // every table below is device data: clamped into its array
    const int a0 = min(max(off1[p], 0), sumN1), a1 = min(max(off1[p + 1], a0), sumN1);
    const int b0 = min(max(off2[p], 0), sumN2), b1 = min(max(off2[p + 1], b0), sumN2);
    const int h0 = min(max(hyp_off[p], 0), sum_hyp), h1 = min(max(hyp_off[p + 1], h0), sum_hyp);
    int n1 = a1 - a0, n2 = b1 - b0;
    const int hcap = min(h1 - h0, max_hyp);
    if (n1 > max_n1 || n2 > max_n2) n1 = n2 = 0;                       // not a valid input: no hypotheses
    const TnHypLds L = tn_hyp_lds(max_n1, max_n2);
    int* nl2 = (int*)(smem + L.nl2);
    int* lab1 = (int*)(smem + L.lab1);
    int* lab2 = (int*)(smem + L.lab2);
    int* un = (int*)(smem + L.un);
    short* nb1 = (short*)(smem + L.nb1);
    short* nb2 = (short*)(smem + L.nb2);
    for (int i = tid; i < n1 * 8; i += TN_THREADS) {
        const int v = nbr1[(size_t)a0 * 8 + i];
        nb1[i] = (short)((v >= 0 && v < n1) ? v : -1);
    }
    for (int i = tid; i < n2 * 8; i += TN_THREADS) {
        const int v = nbr2[(size_t)b0 * 8 + i];
        nb2[i] = (short)((v >= 0 && v < n2) ? v : -1);
    }
    for (int i = tid; i < n1; i += TN_THREADS) lab1[i] = label1[a0 + i] & INT_MAX;
    for (int i = tid; i < n2; i += TN_THREADS) lab2[i] = label2[b0 + i] & INT_MAX;
    for (int i = tid; i < 9 * n1; i += TN_THREADS) un[i] = 0;
    if (tid == 0) s_total = 0;
    __syncthreads();
    for (int i = tid; i < n2 * 8; i += TN_THREADS) {
        const int e = nb2[i];
        nl2[i] = e >= 0 ? lab2[e] : -2;
    }
    __syncthreads();
    pg_build_hypotheses(n1, n2, nb1, nb2, lab1, lab2, nl2, un, s_part, &s_total, hyp + h0, hcap);
    if (tid == 0) hcount[p] = min(s_total, hcap);
}

// minimum of `key` and sum of `cnt` over the workgroup, for all threads.  s_min / s_cnt [TN_WAVES]: the caller keeps a barrier
// between two calls' reads and writes (tn_run has two in every step).
__device__ __forceinline__ void tn_reduce(unsigned& key, int& cnt, unsigned* s_min, int* s_cnt) {
#pragma unroll
    for (int m = WAVE / 2; m > 0; m >>= 1) {
        key = min(key, (unsigned)__shfl_xor((int)key, m));
        cnt += __shfl_xor(cnt, m);
    }
    if ((threadIdx.x & (WAVE - 1)) == 0) {
        s_min[threadIdx.x / WAVE] = key;
        s_cnt[threadIdx.x / WAVE] = cnt;
    }
    __syncthreads();
    key = s_min[0];
    cnt = s_cnt[0];
#pragma unroll
    for (int w = 1; w < TN_WAVES; ++w) {
        key = min(key, s_min[w]);
        cnt += s_cnt[w];
    }
}

struct TnResult {
    int m, f;
};

// One run: hyp[0 .. cnt-1] are the hypotheses from the start on, cnt <= the length of `keys`.  nbr1 / nbr2: the pair's own rows.
// lim: a head whose score field is above it ends the run.  WRITE: the pairs go to `pairs` (at most min(n1, n2) rows).
// Every loop is bounded: steps <= min(n1, n2) (a step kills every hypothesis of its n1 and of its n2), strides over cnt.
template <bool WRITE>
__device__ __forceinline__ TnResult tn_run(const int* __restrict__ hyp, int cnt, int n1, int n2, const int* __restrict__ nbr1,
                                           const int* __restrict__ nbr2, int lim, unsigned* keys, unsigned* min1, unsigned* min2,
                                           unsigned* s_min, int* s_cnt, int* __restrict__ pairs) {
    const int tid = threadIdx.x;
    unsigned kmin = TN_DEAD;
    int bound = 0;
    for (int k = tid; k < cnt; k += TN_THREADS) {
        const int h = hyp[k];
        const int agree = h >> 20, a = (h >> 10) & 1023, b = h & 1023;
        const unsigned key = (h >= 0 && agree <= 8 && a < n1 && b < n2) ? ((unsigned)(TN_OFF - agree) << 20) | (unsigned)(a << 10) | (unsigned)b : TN_DEAD;
        keys[k] = key;
        kmin = min(kmin, key);
    }
    tn_reduce(kmin, bound, s_min, s_cnt);
    TnResult r;
    r.m = INT_MAX;
    r.f = 0;
    const int mn = min(n1, n2);
    for (int t = 0; t < mn; ++t) {
        if (kmin == TN_DEAD || (int)(kmin >> 20) > lim) break;         // nothing left, or the head's score is above min_score
        const int a = (int)(kmin >> 10) & 1023, b = (int)kmin & 1023;  // (a < n1, b < n2: only such keys are alive)
        if (WRITE && tid == 0) {
            pairs[2 * r.f] = a;
            pairs[2 * r.f + 1] = b;
        }
        ++r.f;
        int e1[8], e2[8];
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int v1 = nbr1[a * 8 + d], v2 = nbr2[b * 8 + d];
            e1[d] = (v1 >= 0 && v1 < n1) ? v1 : -1;
            e2[d] = (v2 >= 0 && v2 < n2) ? v2 : -2;
        }
        for (int x = tid; x < n1; x += TN_THREADS) min1[x] = TN_DEAD;
        for (int x = tid; x < n2; x += TN_THREADS) min2[x] = TN_DEAD;
        __syncthreads();
        // the head's row and column die; of the survivors, the first of every n1 and of every n2 in the order BEFORE the bumps
        for (int k = tid; k < cnt; k += TN_THREADS) {
            const unsigned key = keys[k];
            if (key == TN_DEAD) continue;
            const int x1 = (int)(key >> 10) & 1023, x2 = (int)key & 1023;
            if (x1 == a || x2 == b) {
                keys[k] = TN_DEAD;
            } else {
                atomicMin(&min1[x1], key);
                atomicMin(&min2[x2], key);
            }
        }
        __syncthreads();
        // the bound counts the survivors that are both; the bumps decide the next head
        kmin = TN_DEAD;
        bound = 0;
        for (int k = tid; k < cnt; k += TN_THREADS) {
            unsigned key = keys[k];
            if (key == TN_DEAD) continue;
            const int x1 = (int)(key >> 10) & 1023, x2 = (int)key & 1023;
            bound += (min1[x1] == key && min2[x2] == key) ? 1 : 0;
            bool step = false;
#pragma unroll
            for (int d = 0; d < 8; ++d) step = step || (e1[d] == x1 && e2[d] == x2);
            if (step && (key >> 20) >= 8u) {                          // (below 8 the field is saturated: tables that break the rule)
                key -= 8u << 20;
                keys[k] = key;
            }
            kmin = min(kmin, key);
        }
        tn_reduce(kmin, bound, s_min, s_cnt);
        r.m = min(r.m, r.f + bound);
    }
    return r;
}

// the score field's limit for a score8 limit given by the host
__device__ __forceinline__ int tn_field_limit(int limit) { return min(max(limit, -TN_OFF - 1), 7) + TN_OFF; }

__global__ __launch_bounds__(TN_THREADS) void tonioni_run_kernel(
    const int* __restrict__ nbr1, const int* __restrict__ off1, const int* __restrict__ nbr2, const int* __restrict__ off2,
    const int* __restrict__ params, const int* __restrict__ hyp_off, int P, int sumN1, int sumN2, int max_n1, int max_n2,
    int max_hyp, int sum_hyp, const int* __restrict__ hyp, const int* __restrict__ hcount, int* __restrict__ mf) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned s_min[TN_WAVES];
    __shared__ int s_cnt[TN_WAVES];
    const int g = blockIdx.x;
    // the pair whose slice holds hypothesis g: the last p with hyp_off[p] <= g (a table that does not ascend finds some pair, whose
    // own test below then fails)
    int lo = 0, hi = P - 1;
    for (int it = 0; it < 32 && lo < hi; ++it) {
        const int mid = (lo + hi + 1) >> 1;
        if (hyp_off[mid] <= g) lo = mid; else hi = mid - 1;
    }
    const int p = lo;
    const int a0 = min(max(off1[p], 0), sumN1), a1 = min(max(off1[p + 1], a0), sumN1);
    const int b0 = min(max(off2[p], 0), sumN2), b1 = min(max(off2[p + 1], b0), sumN2);
    const int h0 = min(max(hyp_off[p], 0), sum_hyp), h1 = min(max(hyp_off[p + 1], h0), sum_hyp);
    const int n1 = a1 - a0, n2 = b1 - b0;
    const int H = min(min(max(hcount[p], 0), h1 - h0), max_hyp);
    const int start = g - h0;
    if (n1 > max_n1 || n2 > max_n2 || start < 0 || start >= H) return;  // (uniform over the workgroup)
    unsigned* keys = (unsigned*)smem;
    unsigned* min1 = keys + max_hyp;
    unsigned* min2 = min1 + max_n1;
    const TnResult r = tn_run<false>(hyp + h0 + start, H - start, n1, n2, nbr1 + (size_t)a0 * 8, nbr2 + (size_t)b0 * 8,
                                     tn_field_limit(params[p]), keys, min1, min2, s_min, s_cnt, nullptr);
    if (threadIdx.x == 0) {
        mf[2 * (size_t)(h0 + start)] = r.m;
        mf[2 * (size_t)(h0 + start) + 1] = r.f;
    }
}

#define TN_SCAN 256

__global__ __launch_bounds__(TN_THREADS) void tonioni_select_kernel(
    const int* __restrict__ nbr1, const int* __restrict__ off1, const int* __restrict__ nbr2, const int* __restrict__ off2,
    const int* __restrict__ params, const int* __restrict__ hyp_off, const int* __restrict__ out_off, int sumN1, int sumN2,
    int max_n1, int max_n2, int max_hyp, int sum_out, int sum_hyp, const int* __restrict__ hyp, const int* __restrict__ hcount,
    const int* __restrict__ mf, int* __restrict__ pairs, int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ unsigned s_min[TN_WAVES];
    __shared__ int s_cnt[TN_WAVES];
    __shared__ int s_m[TN_SCAN], s_f[TN_SCAN];
    const int p = blockIdx.x, tid = threadIdx.x;
    const int a0 = min(max(off1[p], 0), sumN1), a1 = min(max(off1[p + 1], a0), sumN1);
    const int b0 = min(max(off2[p], 0), sumN2), b1 = min(max(off2[p + 1], b0), sumN2);
    const int r0 = min(max(out_off[p], 0), sum_out), r1 = min(max(out_off[p + 1], r0), sum_out);
    const int h0 = min(max(hyp_off[p], 0), sum_hyp), h1 = min(max(hyp_off[p + 1], h0), sum_hyp);
    const int n1 = a1 - a0, n2 = b1 - b0, rows = r1 - r0;
    int H = min(min(max(hcount[p], 0), h1 - h0), max_hyp);
    if (n1 > max_n1 || n2 > max_n2 || min(n1, n2) > rows) H = 0;        // not a valid input: count 0
    // the scan: start i is adopted when its bound never fell below the best size so far and it ends strictly larger; it ends when
    // more pairs are held than hypotheses are left.  Every thread walks the same values.
    int best = 0, arg = -1;
    bool done = false;
    for (int base = 0; base < H && !done; base += TN_SCAN) {
        const int c = min(TN_SCAN, H - base);
        for (int j = tid; j < c; j += TN_THREADS) {
            s_m[j] = mf[2 * (size_t)(h0 + base + j)];
            s_f[j] = mf[2 * (size_t)(h0 + base + j) + 1];
        }
        __syncthreads();
        for (int j = 0; j < c; ++j) {
            if (best > H - (base + j)) {
                done = true;
                break;
            }
            if (s_m[j] >= best && s_f[j] > best) {
                best = s_f[j];
                arg = base + j;
            }
        }
        __syncthreads();
    }
    int outc = 0;
    if (arg >= 0) {
        unsigned* keys = (unsigned*)smem;
        unsigned* min1 = keys + max_hyp;
        unsigned* min2 = min1 + max_n1;
        outc = tn_run<true>(hyp + h0 + arg, H - arg, n1, n2, nbr1 + (size_t)a0 * 8, nbr2 + (size_t)b0 * 8, tn_field_limit(params[p]),
                            keys, min1, min2, s_min, s_cnt, pairs + (size_t)r0 * 2).f;
    }
    for (int x = outc + tid; x < rows; x += TN_THREADS) {
        pairs[(size_t)(r0 + x) * 2] = -1;
        pairs[(size_t)(r0 + x) * 2 + 1] = -1;
    }
    if (tid == 0) count[p] = outc;
}

static inline size_t tn_run_lds(int max_hyp, int max_n1, int max_n2) { return 4 * ((size_t)max_hyp + max_n1 + max_n2); }

extern "C" size_t cvpce_tonioni_workspace_bytes(long long hypotheses, int P) {
    return (hypotheses >= 0 && P >= 0) ? ((size_t)hypotheses * 3 + (size_t)P) * sizeof(int) : 0;
}

static bool tn_bad_common(int P, int sumN1, int sumN2, int max_n1, int max_n2, int max_hyp, long long sum_hyp, const void* workspace,
                          size_t workspace_bytes) {
    if (sumN1 < 0 || sumN2 < 0 || sum_hyp < 0 || sum_hyp > INT_MAX / 4) return true;
    if (max_n1 < 1 || max_n1 > TN_MAX_NODES || max_n2 < 1 || max_n2 > TN_MAX_NODES) return true;
    if (max_hyp < 0 || max_hyp > CVPCE_TONIONI_MAX_HYPOTHESES) return true;
    return workspace_bytes < cvpce_tonioni_workspace_bytes(sum_hyp, P) || !workspace || ((uintptr_t)workspace & 3);
}

extern "C" int cvpce_tonioni_run(const int* nbr1, const int* label1, const int* off1, const int* nbr2, const int* label2, const int* off2,
                                 const int* params, const int* hyp_off, int P, int sumN1, int sumN2, int max_n1, int max_n2,
                                 int max_hyp, long long sum_hyp, void* workspace, size_t workspace_bytes, void* stream) {
    if (P < 0) return CVPCE_ERR_ARG;
    if (P == 0) return CVPCE_OK;
    if (tn_bad_common(P, sumN1, sumN2, max_n1, max_n2, max_hyp, sum_hyp, workspace, workspace_bytes)) return CVPCE_ERR_ARG;
    if (!off1 || !off2 || !params || !hyp_off) return CVPCE_ERR_ARG;
    if ((sumN1 > 0 && (!nbr1 || !label1)) || (sumN2 > 0 && (!nbr2 || !label2))) return CVPCE_ERR_ARG;
    int* ws = (int*)workspace;
    if (!cvpce_smem_attr_done<tonioni_hyp_kernel>((const void*)tonioni_hyp_kernel, tn_hyp_lds(TN_MAX_NODES, TN_MAX_NODES).total)) return CVPCE_ERR_LAUNCH;
    if (!cvpce_smem_attr_done<tonioni_run_kernel>((const void*)tonioni_run_kernel, (int)tn_run_lds(CVPCE_TONIONI_MAX_HYPOTHESES, TN_MAX_NODES, TN_MAX_NODES)))
        return CVPCE_ERR_LAUNCH;
    hipLaunchKernelGGL(tonioni_hyp_kernel, dim3((unsigned)P), dim3(TN_THREADS), (size_t)tn_hyp_lds(max_n1, max_n2).total, (hipStream_t)stream,
                       nbr1, label1, off1, nbr2, label2, off2, hyp_off, sumN1, sumN2, max_n1, max_n2, max_hyp, (int)sum_hyp,
                       ws, ws + tn_ws_count(sum_hyp));
    if (cvpce_check_launch() != CVPCE_OK) return CVPCE_ERR_LAUNCH;
    if (sum_hyp == 0 || max_hyp == 0) return CVPCE_OK;
    hipLaunchKernelGGL(tonioni_run_kernel, dim3((unsigned)sum_hyp), dim3(TN_THREADS), tn_run_lds(max_hyp, max_n1, max_n2), (hipStream_t)stream,
                       nbr1, off1, nbr2, off2, params, hyp_off, P, sumN1, sumN2, max_n1, max_n2, max_hyp, (int)sum_hyp,
                       ws, ws + tn_ws_count(sum_hyp), ws + tn_ws_mf(sum_hyp));
    return cvpce_check_launch();
}

extern "C" int cvpce_tonioni_select(const int* nbr1, const int* off1, const int* nbr2, const int* off2, const int* params,
                                    const int* hyp_off, const int* out_off, int P, int sumN1, int sumN2, int max_n1, int max_n2,
                                    int max_hyp, int sum_out, long long sum_hyp, const void* workspace, size_t workspace_bytes,
                                    int* pairs, int* count, void* stream) {
    if (P < 0 || sum_out < 0) return CVPCE_ERR_ARG;
    if (P == 0) return CVPCE_OK;
    if (tn_bad_common(P, sumN1, sumN2, max_n1, max_n2, max_hyp, sum_hyp, workspace, workspace_bytes)) return CVPCE_ERR_ARG;
    if (!off1 || !off2 || !params || !hyp_off || !out_off || !count || (sum_out > 0 && !pairs)) return CVPCE_ERR_ARG;
    if ((sumN1 > 0 && !nbr1) || (sumN2 > 0 && !nbr2)) return CVPCE_ERR_ARG;
    const int* ws = (const int*)workspace;
    if (!cvpce_smem_attr_done<tonioni_select_kernel>((const void*)tonioni_select_kernel,
                                                     (int)tn_run_lds(CVPCE_TONIONI_MAX_HYPOTHESES, TN_MAX_NODES, TN_MAX_NODES)))
        return CVPCE_ERR_LAUNCH;
    hipLaunchKernelGGL(tonioni_select_kernel, dim3((unsigned)P), dim3(TN_THREADS), tn_run_lds(max_hyp, max_n1, max_n2), (hipStream_t)stream,
                       nbr1, off1, nbr2, off2, params, hyp_off, out_off, sumN1, sumN2, max_n1, max_n2, max_hyp, sum_out, (int)sum_hyp,
                       ws, ws + tn_ws_count(sum_hyp), ws + tn_ws_mf(sum_hyp), pairs, count);
    return cvpce_check_launch();
}
