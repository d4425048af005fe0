// The two graph stages of the planogram comparator (include/cvpce_amd_planogram.h): neighbour graphs and common subgraph.
//
// planogram_graphs_kernel: one workgroup per graph.  The three [n][8] slot tables (neighbour, weight, stamp) and the centres
// live in LDS for the whole kernel.  Node i's row is produced when its turn comes: all 256 threads compute d(i, .) and the
// sector, keep the candidates the greedy could still take (d <= thresh, d > 0, a direction i still wants) as 64-bit keys
// (d bits | j | sector: ascending key = ascending (d, j)), and order them by counting -- a key's place is the number of smaller
// keys (keys are distinct: j is).  Wave 0 then walks the ordered row 64 candidates at a time: every lane tests its candidate
// against the tables, the first acceptable one is linked by lane 0, and the lanes behind it are tested AGAIN, because the link
// changed what i wants and may have unlinked a rival that a later candidate is asked about.
//
// planogram_match_kernel: one workgroup per (expected, actual) pair.  All threads count, per expected node and agree level, the
// equal-label seed pairs, a prefix sum over (level descending, n1) turns the counts into places, and a second pass writes the
// hypotheses in their final order to the workspace -- no sort.  Wave 0 then grows them one after the other in LDS.
//
// The distances must have the bits of the rule's fp32 expression: the file is compiled with FMA contraction off (Makefile),
// the kernel repeats it as a pragma, and the square root is the correctly rounded one.
#include "common.h"
#include "../../include/cvpce_amd_planogram.h"
#include <limits.h>
#include "pg_hypotheses.h"

#define PG_MAX CVPCE_PLANOGRAM_MAX_NODES
#define PG_TAN_PI_8 0.41421356f
#define PG_TAN_3PI_8 2.41421356f

typedef unsigned long long u64;

// 8-way sector of the direction (dx, dy) != (0, 0): 0 = E, then in steps of 45 degrees towards +y
__device__ __forceinline__ int pg_sector(float dx, float dy) {
#pragma clang fp contract(off)
    const float ax = fabsf(dx), ay = fabsf(dy);
    if (ay <= PG_TAN_PI_8 * ax) return dx > 0.f ? 0 : 4;
    if (ay > PG_TAN_3PI_8 * ax) return dy > 0.f ? 2 : 6;
    return dy > 0.f ? (dx > 0.f ? 1 : 3) : (dx > 0.f ? 7 : 5);
}

static inline size_t pg_graphs_lds(int max_n) { return (size_t)max_n * (8 + 8 + 4 + 4 + 3 * 8 * 4); }

__global__ __launch_bounds__(PG_THREADS) void planogram_graphs_kernel(
    const float4* __restrict__ boxes, const int* __restrict__ offsets, const float* __restrict__ thresh, int sumN, int max_n,
    int* __restrict__ g_nbr, float* __restrict__ g_w, int* __restrict__ g_st) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_m;
    const int g = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1);
    // offsets are device data: clamp them into the packed arrays so that a bad offset table cannot index outside them
    const int o0 = min(max(offsets[g], 0), sumN), o1 = min(max(offsets[g + 1], o0), sumN);
    const int n = o1 - o0;
    if (n < 1 || n > max_n) return;                                  // (uniform over the workgroup)
    u64* cand = (u64*)smem;
    u64* sorted = cand + max_n;
    float* cx = (float*)(sorted + max_n);
    float* cy = cx + max_n;
    int* nb = (int*)(cy + max_n);
    float* w = (float*)(nb + 8 * max_n);
    int* st = (int*)(w + 8 * max_n);

    for (int i = tid; i < n; i += PG_THREADS) {
        const float4 b = boxes[o0 + i];
        cx[i] = (b.x + b.z) * 0.5f;
        cy[i] = (b.y + b.w) * 0.5f;
    }
    for (int i = tid; i < n * 8; i += PG_THREADS) {
        nb[i] = -1;
        w[i] = 0.f;
        st[i] = -1;
    }
    if (tid == 0) s_m = 0;
    const float thr = thresh[g];
    int stamp = 0;                                                    // (wave 0's copy counts)
    __syncthreads();

    for (int i = 0; i < n; ++i) {
        unsigned wanted = 0;
#pragma unroll
        for (int s = 0; s < 8; ++s) wanted |= (nb[i * 8 + s] < 0 ? 1u : 0u) << s;
        if (!wanted) continue;                                        // (uniform)
        const float xi = cx[i], yi = cy[i];
        for (int j = tid; j < n; j += PG_THREADS) {
            if (j == i) continue;
            const float dx = cx[j] - xi, dy = cy[j] - yi;
            const float d = sqrtf(dx * dx + dy * dy);                    // (IEEE root; __fsqrt_rn is the 1-ulp native one here)
            if (!(d > 0.f) || d > thr) continue;                      // d = 0: no direction; d > thresh: where the host's walk ends
            const int s = pg_sector(dx, dy);
            if (!((wanted >> s) & 1)) continue;
            const int slot = atomicAdd(&s_m, 1);                      // (any order: the keys are ordered below)
            cand[slot] = ((u64)__float_as_uint(d) << 32) | (unsigned)((j << 3) | s);
        }
        __syncthreads();
        const int m = s_m;                                            // <= n - 1
        for (int p = tid; p < m; p += PG_THREADS) {
            const u64 key = cand[p];
            int r = 0;
            for (int q = 0; q < m; ++q) r += cand[q] < key ? 1 : 0;
            sorted[r] = key;
        }
        __syncthreads();
        if (tid < WAVE) {
            volatile int* vnb = nb;
            volatile float* vw = w;
            volatile int* vst = st;
            for (int base = 0; base < m && wanted; base += WAVE) {
                const bool have = base + lane < m;
                const u64 key = have ? sorted[base + lane] : 0ull;
                const float d = __uint_as_float((unsigned)(key >> 32));
                const int j = (int)((unsigned)key >> 3), s = (int)(key & 7), back = (s + 4) & 7;
                int from = 0;                                         // lanes from here on are still to be tested
                for (int round = 0; round < 8; ++round) {             // a node takes at most 8 neighbours
                    bool ok = have && lane >= from && ((wanted >> s) & 1);
                    if (ok && vnb[j * 8 + back] >= 0 && vw[j * 8 + back] <= d) ok = false;   // j has a closer neighbour on i's side
                    const u64 bal = __ballot(ok);
                    if (!bal) break;
                    const int f = __ffsll((long long)bal) - 1;
                    const int fj = __shfl(j, f), fs = __shfl(s, f), fb = (fs + 4) & 7;
                    const float fd = __shfl(d, f);
                    if (lane == 0) {
                        const int rival = vnb[fj * 8 + fb];
                        if (rival >= 0 && vnb[rival * 8 + fs] == fj) {                       // unlink j <-> rival
                            vnb[rival * 8 + fs] = -1;
                            vw[rival * 8 + fs] = 0.f;
                            vst[rival * 8 + fs] = -1;
                        }
                        vnb[i * 8 + fs] = fj;
                        vw[i * 8 + fs] = fd;
                        vst[i * 8 + fs] = stamp;
                        vnb[fj * 8 + fb] = i;
                        vw[fj * 8 + fb] = fd;
                        vst[fj * 8 + fb] = stamp + 1;
                    }
                    stamp += 2;
                    wanted &= ~(1u << fs);
                    from = f + 1;
                    if (!wanted) break;
                }
            }
            if (tid == 0) s_m = 0;
        }
        __syncthreads();
    }

    __syncthreads();
    for (int i = tid; i < n * 8; i += PG_THREADS) {
        g_nbr[(size_t)o0 * 8 + i] = nb[i];
        g_w[(size_t)o0 * 8 + i] = w[i];
        g_st[(size_t)o0 * 8 + i] = st[i];
    }
}

extern "C" int cvpce_planogram_graphs(const float* boxes, const int* offsets, const float* thresh, int B, int sumN, int min_n, int max_n,
                                      int* nbr, float* weight, int* stamp, void* stream) {
    if (B < 0 || sumN < 0) return CVPCE_ERR_ARG;
    if (B == 0) return CVPCE_OK;
    if (min_n < 1 || max_n > PG_MAX || min_n > max_n) return CVPCE_ERR_ARG;
    if ((long long)B * min_n > sumN || (long long)B * max_n < sumN) return CVPCE_ERR_ARG;
    if (!boxes || !offsets || !thresh || !nbr || !weight || !stamp || ((uintptr_t)boxes & 15)) return CVPCE_ERR_ARG;
    if (!cvpce_smem_attr_done<planogram_graphs_kernel>((const void*)planogram_graphs_kernel, (int)pg_graphs_lds(PG_MAX))) return CVPCE_ERR_LAUNCH;
    hipLaunchKernelGGL(planogram_graphs_kernel, dim3((unsigned)B), dim3(PG_THREADS), pg_graphs_lds(max_n), (hipStream_t)stream,
                       (const float4*)boxes, offsets, thresh, sumN, max_n, nbr, weight, stamp);
    return cvpce_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------
// common subgraph
// ---------------------------------------------------------------------------------------------------------------------
struct PgMatchLds {
    int nl2, lab1, lab2, ord1, used1, used2, grown, best, un, nb1, nb2, total;
};

// byte offsets of the LDS arrays for graphs of up to n1 / n2 nodes (`un` is first the [9][n1] level counts, then the queue)
__host__ __device__ static inline PgMatchLds pg_match_lds(int n1, int n2) {
    const int mn = n1 < n2 ? n1 : n2;
    const int un = 9 * n1 > 8 * mn + 8 ? 9 * n1 : 8 * mn + 8;
    PgMatchLds l;
    int o = 0;
    l.nl2 = o; o += 4 * 8 * n2;
    l.lab1 = o; o += 4 * n1;
    l.lab2 = o; o += 4 * n2;
    l.ord1 = o; o += 4 * n1;
    l.used1 = o; o += 4 * n1;
    l.used2 = o; o += 4 * n2;
    l.grown = o; o += 4 * mn;
    l.best = o; o += 4 * mn;
    l.un = o; o += 4 * un;
    l.nb1 = o; o += 2 * 8 * n1;
    l.nb2 = o; o += 2 * 8 * n2;
    l.total = o;
    return l;
}

__global__ __launch_bounds__(PG_THREADS) void planogram_match_kernel(
    const int* __restrict__ nbr1, const int* __restrict__ stamp1, const int* __restrict__ label1, const int* __restrict__ off1,
    const int* __restrict__ nbr2, const int* __restrict__ stamp2, const int* __restrict__ label2, const int* __restrict__ off2,
    const int* __restrict__ params, const int* __restrict__ hyp_off, const int* __restrict__ out_off,
    int sumN1, int sumN2, int max_n1, int max_n2, int sum_out, int sum_hyp, int* __restrict__ hyp,
    int* __restrict__ pairs, int* __restrict__ count) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ int s_part[PG_THREADS];
    __shared__ int s_total, s_outc, s_which;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1);
    // every table below is device data: clamped into its array
    const int a0 = min(max(off1[p], 0), sumN1), a1 = min(max(off1[p + 1], a0), sumN1);
    const int b0 = min(max(off2[p], 0), sumN2), b1 = min(max(off2[p + 1], b0), sumN2);
    const int r0 = min(max(out_off[p], 0), sum_out), r1 = min(max(out_off[p + 1], r0), sum_out);
    const int h0 = min(max(hyp_off[p], 0), sum_hyp), h1 = min(max(hyp_off[p + 1], h0), sum_hyp);
    int n1 = a1 - a0, n2 = b1 - b0;
    const int rows = r1 - r0, hcap = h1 - h0;
    if (n1 > max_n1 || n2 > max_n2 || min(n1, n2) > rows) n1 = n2 = 0;           // not a valid input: count 0
    const int mn = min(n1, n2);
    const int min_agree = params[2 * p], enough = params[2 * p + 1];
    const PgMatchLds L = pg_match_lds(max_n1, max_n2);
    int* nl2 = (int*)(smem + L.nl2);
    int* lab1 = (int*)(smem + L.lab1);
    int* lab2 = (int*)(smem + L.lab2);
    int* ord1 = (int*)(smem + L.ord1);
    int* used1 = (int*)(smem + L.used1);
    int* used2 = (int*)(smem + L.used2);
    int* grown = (int*)(smem + L.grown);
    int* best = (int*)(smem + L.best);
    int* un = (int*)(smem + L.un);
    short* nb1 = (short*)(smem + L.nb1);
    short* nb2 = (short*)(smem + L.nb2);

    for (int i = tid; i < n1 * 8; i += PG_THREADS) {
        const int v = nbr1[(size_t)a0 * 8 + i];
        nb1[i] = (short)((v >= 0 && v < n1) ? v : -1);
    }
    for (int i = tid; i < n2 * 8; i += PG_THREADS) {
        const int v = nbr2[(size_t)b0 * 8 + i];
        nb2[i] = (short)((v >= 0 && v < n2) ? v : -1);
    }
    for (int i = tid; i < n1; i += PG_THREADS) {
        lab1[i] = label1[a0 + i] & INT_MAX;
        used1[i] = 0;
    }
    for (int i = tid; i < n2; i += PG_THREADS) {
        lab2[i] = label2[b0 + i] & INT_MAX;
        used2[i] = 0;
    }
    for (int i = tid; i < 9 * n1; i += PG_THREADS) un[i] = 0;
    __syncthreads();
    // adjacency order of the expected graph's nodes: the filled slots by ascending (stamp, slot), one nibble each, 0xF ends the list
    for (int a = tid; a < n1; a += PG_THREADS) {
        int ss[8], sd[8], k = 0;
        for (int d = 0; d < 8; ++d) {
            if (nb1[a * 8 + d] < 0) continue;
            const int sv = stamp1[(size_t)(a0 + a) * 8 + d];
            int q = k++;
            while (q > 0 && ss[q - 1] > sv) {                        // (insertion: q only falls)
                ss[q] = ss[q - 1];
                sd[q] = sd[q - 1];
                --q;
            }
            ss[q] = sv;
            sd[q] = d;
        }
        unsigned o = 0xFFFFFFFFu;
        for (int q = 0; q < k; ++q) o = (o & ~(0xFu << (4 * q))) | ((unsigned)sd[q] << (4 * q));
        ord1[a] = (int)o;
    }
    for (int i = tid; i < n2 * 8; i += PG_THREADS) {
        const int e = nb2[i];
        nl2[i] = e >= 0 ? lab2[e] : -2;
    }
    __syncthreads();

    // ---- hypotheses: count per (level, n1), prefix, place (pg_hypotheses.h) ----
    pg_build_hypotheses(n1, n2, nb1, nb2, lab1, lab2, nl2, un, s_part, &s_total, hyp + h0, hcap);
    const int H = min(s_total, hcap);
    __syncthreads();                                                  // `un` becomes the queue

    // ---- growth: wave 0, one hypothesis after the other ----
    if (tid < WAVE) {
        volatile int* vq = un;
        volatile int* vu1 = used1;
        volatile int* vu2 = used2;
        volatile int* vgrown = grown;
        volatile int* vbest = best;
        const int qcap = 8 * mn + 8;
        int bestc = 0, epoch = 0, outc = 0, which = 0;                // which: 0 = best, 1 = grown
        bool done = false;
        for (int hb = 0; hb < H && !done; hb += WAVE) {
            const int hv = hb + lane < H ? hyp[(size_t)h0 + hb + lane] : 0;
            const int cnt = min(WAVE, H - hb);
            for (int k = 0; k < cnt && !done; ++k) {
                const int h = __shfl(hv, k);
                const int agree = h >> 20;
                int a = (h >> 10) & 1023, b = h & 1023;
                if (a >= n1 || b >= n2) continue;
                if (agree < min_agree && bestc > 0) {
                    done = true;
                    break;
                }
                ++epoch;
                int gc = 0, head = 0, tail = 0;
                for (int it = 0; it <= qcap && gc < mn; ++it) {       // one accepted pair per turn
                    if (lane == 0) {
                        vu1[a] = epoch;
                        vu2[b] = epoch;
                        vgrown[gc] = (a << 16) | b;
                    }
                    ++gc;
                    if (tail + 8 <= qcap) {                           // (always, for well-formed tables)
                        const int dsl = lane < 8 ? (((unsigned)ord1[a] >> (4 * lane)) & 0xF) : 0xF;
                        const int e1 = dsl < 8 ? nb1[a * 8 + dsl] : -1;
                        const int e2 = dsl < 8 ? nb2[b * 8 + dsl] : -1;
                        const bool ok = e1 >= 0 && e2 >= 0 && lab1[e1] == lab2[e2];
                        const u64 bal = __ballot(ok);
                        if (ok) vq[tail + __popcll(bal & ((1ull << lane) - 1))] = (e1 << 16) | e2;
                        tail += __popcll(bal);
                    }
                    bool found = false;
                    while (head < tail) {                             // (tail <= qcap)
                        const int q = vq[head++];
                        a = q >> 16;
                        b = q & 0xFFFF;
                        if (vu1[a] != epoch && vu2[b] != epoch) {
                            found = true;
                            break;
                        }
                    }
                    if (!found) break;
                }
                if (gc > enough) {
                    outc = gc;
                    which = 1;
                    done = true;
                    break;
                }
                if (gc > bestc) {
                    for (int x = lane; x < gc; x += WAVE) vbest[x] = vgrown[x];
                    bestc = gc;
                }
            }
        }
        if (!which) outc = bestc;
        if (lane == 0) {
            s_outc = outc;
            s_which = which;
        }
    }
    __syncthreads();
    const int outc = s_outc;
    const int* src = s_which ? grown : best;
    for (int x = tid; x < rows; x += PG_THREADS) {
        const int v = x < outc ? src[x] : -1;
        pairs[(size_t)(r0 + x) * 2] = x < outc ? (v >> 16) : -1;
        pairs[(size_t)(r0 + x) * 2 + 1] = x < outc ? (v & 0xFFFF) : -1;
    }
    if (tid == 0) count[p] = outc;
}

extern "C" size_t cvpce_planogram_match_workspace_bytes(long long hypotheses) {
    return hypotheses > 0 ? (size_t)hypotheses * sizeof(int) : 0;
}

extern "C" int cvpce_planogram_match(const int* nbr1, const int* stamp1, const int* label1, const int* off1,
                                     const int* nbr2, const int* stamp2, const int* label2, const int* off2,
                                     const int* params, const int* hyp_off, const int* out_off,
                                     int P, int sumN1, int sumN2, int max_n1, int max_n2, int sum_out, long long sum_hyp,
                                     void* workspace, size_t workspace_bytes, int* pairs, int* count, void* stream) {
    if (P < 0 || sumN1 < 0 || sumN2 < 0 || sum_out < 0 || sum_hyp < 0 || sum_hyp > INT_MAX) return CVPCE_ERR_ARG;
    if (P == 0) return CVPCE_OK;
    if (max_n1 < 1 || max_n1 > PG_MAX || max_n2 < 1 || max_n2 > PG_MAX) return CVPCE_ERR_ARG;
    if (!off1 || !off2 || !params || !hyp_off || !out_off || !count) return CVPCE_ERR_ARG;
    if ((sumN1 > 0 && (!nbr1 || !stamp1 || !label1)) || (sumN2 > 0 && (!nbr2 || !stamp2 || !label2)) || (sum_out > 0 && !pairs)) return CVPCE_ERR_ARG;
    if (workspace_bytes < cvpce_planogram_match_workspace_bytes(sum_hyp) || (sum_hyp > 0 && !workspace) || ((uintptr_t)workspace & 3)) return CVPCE_ERR_ARG;
    const int lds = pg_match_lds(max_n1, max_n2).total;
    if (!cvpce_smem_attr_done<planogram_match_kernel>((const void*)planogram_match_kernel, pg_match_lds(PG_MAX, PG_MAX).total)) return CVPCE_ERR_LAUNCH;
    hipLaunchKernelGGL(planogram_match_kernel, dim3((unsigned)P), dim3(PG_THREADS), (size_t)lds, (hipStream_t)stream,
                       nbr1, stamp1, label1, off1, nbr2, stamp2, label2, off2, params, hyp_off, out_off,
                       sumN1, sumN2, max_n1, max_n2, sum_out, (int)sum_hyp, (int*)workspace, pairs, count);
    return cvpce_check_launch();
}
