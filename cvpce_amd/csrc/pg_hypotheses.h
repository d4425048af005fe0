// The hypothesis builder of the planogram matchers (planogram.hip: planogram_match_kernel; tonioni.hip: tonioni_hyp_kernel): the
// equal-label seed pairs of one (expected, actual) graph pair in their final order -- agree descending, then n1, then n2, which is
// sorted((-agree / 8, n1, n2)) -- written without a sort.  All threads count, per expected node and agree level, the equal-label
// pairs; a prefix sum over (level descending, n1) turns the counts into places; a second pass writes the hypotheses.
#pragma once
#include "common.h"

#define PG_THREADS 256

// One workgroup of PG_THREADS threads, all of them, after a barrier behind the tables' fill.  LDS: nb1 [n1][8], nb2 [n2][8]
// (neighbour or -1), lab1 [n1], lab2 [n2], nl2 [n2][8] (the label of nb2's neighbour, -2 for none), un [9 * n1] ZEROED, s_part
// [PG_THREADS], s_total.  hyp: this pair's slice of the workspace, hcap hypotheses long; one beyond it is counted, not written.
// A hypothesis is (agree << 20) | (n1 << 10) | n2.  On return *s_total is the pair's hypothesis count and a barrier has been passed.
__device__ __forceinline__ void pg_build_hypotheses(int n1, int n2, const short* nb1, const short* nb2, const int* lab1, const int* lab2,
                                                    const int* nl2, int* un, int* s_part, int* s_total, int* __restrict__ hyp, int hcap) {
    const int tid = threadIdx.x;
    for (int pass = 0; pass < 2; ++pass) {
        for (int a = tid; a < n1; a += PG_THREADS) {
            int nl1[8];
#pragma unroll
            for (int d = 0; d < 8; ++d) {
                const int e = nb1[a * 8 + d];
                nl1[d] = e >= 0 ? lab1[e] : -1;
            }
            const int la = lab1[a];
            for (int b = 0; b < n2; ++b) {
                if (lab2[b] != la) continue;
                int agree = 0;
#pragma unroll
                for (int d = 0; d < 8; ++d) agree += nl1[d] == nl2[b * 8 + d] ? 1 : 0;
                const int at = (8 - agree) * n1 + a;                 // (this thread's own entry)
                if (pass == 0) {
                    un[at] += 1;
                } else {
                    const int pos = un[at]++;
                    if (pos < hcap) hyp[pos] = (agree << 20) | (a << 10) | b;
                }
            }
        }
        __syncthreads();
        if (pass == 0) {
            const int total = 9 * n1, chunk = (total + PG_THREADS - 1) / PG_THREADS;
            const int e0 = min(tid * chunk, total), e1 = min(e0 + chunk, total);
            int sum = 0;
            for (int e = e0; e < e1; ++e) sum += un[e];
            s_part[tid] = sum;
            __syncthreads();
            if (tid == 0) {
                int run = 0;
                for (int t = 0; t < PG_THREADS; ++t) {
                    const int v = s_part[t];
                    s_part[t] = run;
                    run += v;
                }
                *s_total = run;
            }
            __syncthreads();
            int run = s_part[tid];
            for (int e = e0; e < e1; ++e) {
                const int v = un[e];
                un[e] = run;
                run += v;
            }
            __syncthreads();
        }
    }
}
