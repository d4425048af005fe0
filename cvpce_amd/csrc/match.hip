// K11: cosine-distance matrix detections x gallery as ONE MFMA GEMM with a
// fused per-query top-k epilogue -- the (Q,G) matrix is never written to HBM.
// Replaces `distance` (1 - cosine_similarity) and `nearest_neighbors` (argsort[:, :k] of a
// materialised (Q,G,D) x2 gather) of the reference's module cvpce.models.classification.
//
//   dist[q][g] = 1 - <Q[q], G[g]> / (max(|Q[q]|,eps) * max(|G[g]|,eps))
//
// Layout: Q [Qn][D], G [Gn][D] row-major (K contiguous for both operands),
// bf16 storage, fp32 accumulate (v_mfma_f32_32x32x16_bf16); or fp32 storage
// on the exact-f32 matrix pipe (v_mfma_f32_32x32x2_f32) for index-exact parity.
// Two GEMM cores, chosen per launch by match_plan: match_kernel (tile 128 gallery rows x 128 | 64 queries, K-step 64, swizzled LDS,
// register staged double buffer, same pipeline as conv_igemm; bf16 and f32) and match_big_kernel (bf16 only: 128 MG gallery rows x
// 64 NQ queries, both operands by LDS-DMA).  Both find every query's k smallest (distance, index) pairs of the tile lexicographically
// (ties -> lowest index); the partials [Q][tiles_g][k] are merged by a second tiny kernel.  k > 16 (up to the gallery size): match_kernel
// writes its distances to a block in the workspace instead, followed by an exact per-query select and sort (match_select_kernel).
#include "common.h"
#include "../../include/cvpce_amd.h"
#include <math.h>
#include <cstdlib>
#include <type_traits>

#define MT_TG 128
#define MT_TQ 128
#define MT_BK 64
#define MATCH_KMAX 16          // k above this takes the large-k path (distance block + per-query select + sort, below)

struct MatchArgs {
    const void* q; const void* g;
    const float* qn; const float* gn;     // L2 norms (already clamped by eps)
    int Qn, Gn, D, k, tiles_g, tiles_q;
    float* part_d; int* part_i;           // [Qn][tiles_g][k]
    long long* out_idx; float* out_dist;  // large k: the results [Qn][k]
    float* dist; int ldd;                 // large k: the distance block [Qn][ldd] (match_kernel<F32, TQ, true>)
};

// Dynamic LDS of match_kernel<F32, TQ, STORE>, byte offsets.  K loop: two buffers of 128 gallery rows at 0, two of TQ query rows at `q`.
// The epilogue reuses the staging (the last K-step ended on a barrier): the tile's distances as f32 at 0, one gallery row `ldg` floats and
// one query `ldq` floats apart -- selecting: [g][q] (conflict-free both ways); STORE: [q][g], rows padded to 129 floats (the fragment
// writes of a lane half hit 32 different banks) -- then, selecting only, the scan's candidates cd [256] f32 and cix [256] int, then the
// tile's 128 gallery norms.  `bytes` is what a launch asks for: the staging (f32: 128 KiB, 64-query tiles: 48 KiB) or, for the bf16
// 128-query tiles, the larger epilogue image.
struct MatchLds { int q, staging, ldg, ldq, cd, cix, gn, epilogue, bytes; };
constexpr MatchLds match_lds(bool f32, int tq, bool store) {
    const int rowb = MT_BK * (f32 ? 4 : 2), staging = 2 * (MT_TG + tq) * rowb;
    const int ldg = store ? 1 : tq, ldq = store ? MT_TG + 1 : 1;
    const int cd = (store ? tq * (MT_TG + 1) : MT_TG * tq) * 4, cix = cd + 256 * 4;
    const int gn = store ? cd : cix + 256 * 4, epilogue = gn + MT_TG * 4;
    return {2 * MT_TG * rowb, staging, ldg, ldq, cd, cix, gn, epilogue, (f32 || tq == 64) ? staging : epilogue};
}
// Dynamic LDS of match_big_kernel<NQ, MG>: two K-stages of (128 MG gallery + 64 NQ query) rows of 128 bytes.  Epilogue, over the staging: 1 / |g| of
// the tile's rows (1 KiB), the candidates cd, cix [4][TQ] of the four gallery waves, the round's winner wd, wix [TQ].
#define MB_ROWB 128                        // bytes of one row of a K-stage (64 bf16)
struct MatchBigLds { int stage, cd, cix, wd, wix, epilogue, bytes; };
constexpr MatchBigLds match_big_lds(int nq, int mg) {
    const int tq = 64 * nq, stage = (128 * mg + tq) * MB_ROWB;
    const int cd = 1024, cix = cd + 4 * tq * 4, wd = cix + 4 * tq * 4, wix = wd + tq * 4;
    return {stage, cd, cix, wd, wix, wix + tq * 4, 2 * stage};
}

// (distance, row) as ONE unsigned 64-bit key whose integer order is the lexicographic order: the float's bits made monotone
// (negative: all bits flipped, non-negative: sign bit set) above the row index
__device__ __forceinline__ unsigned match_key32(float d) {
    const unsigned b = __float_as_uint(d);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float match_key_distance(unsigned long long key) {
    const unsigned o = (unsigned)(key >> 32);
    return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xFFFFFFFFu));
}

__global__ void row_norm_bf16_kernel(const bf16_t* __restrict__ x, float* __restrict__ out, int rows, int D, float eps) {
    const int row = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int i = lane * 8; i < D; i += 64 * 8) {
        uint4 v = *reinterpret_cast<const uint4*>(x + (size_t)row * D + i);
        bf16x8 b = *reinterpret_cast<bf16x8*>(&v);
#pragma unroll
        for (int j = 0; j < 8; ++j) s += (float)b[j] * (float)b[j];
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[row] = fmaxf(sqrtf(s), eps);
}
__global__ void row_norm_f32_kernel(const float* __restrict__ x, float* __restrict__ out, int rows, int D, float eps) {
    const int row = blockIdx.x * (blockDim.x / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= rows) return;
    float s = 0.f;
    for (int i = lane; i < D; i += 64) { float v = x[(size_t)row * D + i]; s += v * v; }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) out[row] = fmaxf(sqrtf(s), eps);
}

extern "C" int cvpce_row_norms(const void* x, float* out, int rows, int D, int is_f32, float eps, void* stream) {
    if (!x || !out || D <= 0 || (!is_f32 && D % 8 != 0)) return CVPCE_ERR_ARG;
    if (rows <= 0) return CVPCE_OK;
    if (is_f32)
        hipLaunchKernelGGL(row_norm_f32_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const float*)x, out, rows, D, eps);
    else
        hipLaunchKernelGGL(row_norm_bf16_kernel, dim3((rows + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, out, rows, D, eps);
    return cvpce_check_launch();
}

// The distance of one (query, gallery row) pair from its dot product.  bf16 operands: 1 - dot * (1/|q| * 1/|g|), one multiply and one
// fused multiply-add per pair with the two reciprocals formed once per row (a true division per pair is ~10 VALU instructions: in the
// 256 x 320 tile's epilogue that was 160 divisions per lane, a fifth of the kernel).  Every bf16 kernel of this file forms the distance by
// THIS expression from the same reciprocals, so a query's distances do not depend on the kernel that computed them.  f32 operands (the
// reference's arithmetic): the literal 1 - dot / (|q| |g|).  `nq`, `ng`: the norm (F32) or its reciprocal (bf16), see match_norm_term.
template <bool F32>
__device__ __forceinline__ float match_distance(float dot, float nq, float ng) {
    if constexpr (F32) return 1.f - dot / (nq * ng);
    else return __builtin_fmaf(-dot, nq * ng, 1.f);
}
template <bool F32>
__device__ __forceinline__ float match_norm_term(float norm) { return F32 ? norm : 1.f / norm; }

// lexicographic (d, i) < (e, j)
__device__ __forceinline__ bool lex_lt(float d, int i, float e, int j) { return d < e || (d == e && i < j); }
__device__ __forceinline__ void lex_min(float d, int i, float& bd, int& bi) { if (lex_lt(d, i, bd, bi)) { bd = d; bi = i; } }
// one step of a selection round: (d, i) becomes the best so far (bd, bi) if it lies after the previous pick (pd, pi) and before the best
__device__ __forceinline__ void match_take(float d, int i, float pd, int pi, float& bd, int& bi) { if (lex_lt(pd, pi, d, i)) lex_min(d, i, bd, bi); }

// XCD-aware tile order of both GEMM kernels.  Workgroups are dealt to the 8 XCDs round-robin, each with its own 4-MiB L2; with gallery tiles
// fastest over blockIdx every XCD touches EVERY gallery tile (20 MB at 10 000 x 1 024) and the operands stream from beyond L2
// (9.5 TB/s measured at 1 600 queries: 43 FLOP per byte of a 128 x 64 tile = the 400 TFLOP/s the kernel was stuck at).
// Here XCD x gets a contiguous range of the logical order (xcd_remap), and that order is gallery-class major: class c =
// the gallery tiles c, c + 8, ... with all their query tiles -- an eighth of the gallery (2.5 MB) stays resident in the
// XCD's L2 while the query tiles sweep past it.
__device__ __forceinline__ void match_tile_of_block(int tiles_g, int tiles_q, int& tile_g, int& tile_q) {
    int l = xcd_remap((int)blockIdx.x, (int)gridDim.x);
    int cls = 0, ng = (tiles_g + 7) >> 3;
    while (cls < 7 && l >= ng * tiles_q) {       // at most 7 steps, scalar
        l -= ng * tiles_q;
        ++cls;
        ng = (tiles_g - cls + 7) >> 3;
    }
    tile_q = l / ng;
    tile_g = cls + 8 * (l - tile_q * ng);
}

// Distance epilogue of match_kernel: the tile's gallery norms to s_gn (one coalesced load instead of 64 scattered ones per lane), then
// every accumulator as a distance to T[gl * LDG + ql * LDQ] (gl, ql: row and query within the tile).  Rows past the gallery are +inf,
// and so is a NaN distance (non-finite embedding): it sorts last and still yields a valid index.  Ends on the barrier.
template <bool F32, int TQ, int LDG, int LDQ>
__device__ __forceinline__ void match_tile_distances(const MatchArgs& a, int tile_g, int tile_q, const f32x16 (&acc)[2][TQ / 64],
                                                     float* __restrict__ T, float* __restrict__ s_gn) {
    constexpr int NT = TQ / 64;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wc = wid >> 1, wp = wid & 1, lr = lane & 31, lh = lane >> 5;
    if (tid < MT_TG) {
        const int gg = tile_g * MT_TG + tid;
        s_gn[tid] = match_norm_term<F32>((gg < a.Gn) ? a.gn[gg] : 1.f);
    }
    __syncthreads();
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int ql = wp * 32 * NT + nt * 32 + lr;
        const int qg = tile_q * TQ + ql;
        const float qn = match_norm_term<F32>((qg < a.Qn) ? a.qn[qg] : 1.f);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int gl = wc * 64 + mt * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const int gg = tile_g * MT_TG + gl;
                float d = INFINITY;
                if (gg < a.Gn) {
                    d = match_distance<F32>(acc[mt][nt][r], qn, s_gn[gl]);
                    if (!(d == d)) d = INFINITY;
                }
                T[gl * LDG + ql * LDQ] = d;
            }
    }
    __syncthreads();
}

// TQ = queries per tile: 128 (waves 2 x 2, 64 gallery rows x 64 queries each) or 64 (64 x 32 each; 48 KiB of LDS, three
// workgroups per CU).  Which one a launch takes is a question of tile COUNT, not of kernel quality: 1 600 x 10 000 gives
// 13 x 79 = 1 027 tiles of 128 x 128 -- on 512 workgroup slots a third round for three tiles.
// STORE (the large-k path): the epilogue writes the tile's distances to the block a.dist [Qn][a.ldd] instead of selecting.
template <bool F32, int TQ, bool STORE = false>
__global__ __launch_bounds__(256, TQ == 64 ? 3 : 2) void match_kernel(MatchArgs a) {
    static_assert(TQ == 128 || TQ == 64, "query tile");
    constexpr int NT = TQ / 64;                      // 32-query MFMA blocks per wave
    // element size 2 (bf16) or 4 (f32); one LDS row = MT_BK elements
    constexpr int ES = F32 ? 4 : 2;
    constexpr int ROWB = MT_BK * ES;                 // bytes per tile row: 128 / 256
    constexpr int CPR = ROWB / 16;                   // 16-B chunks per row: 8 / 16
    constexpr int RPP = 256 / CPR;                   // 32 / 16
    constexpr int PASS = MT_TG / RPP;                // 4 / 8
    constexpr int PASSQ = TQ / RPP;                  // query rows per thread
    constexpr int RPB = (256 / ROWB) > 0 ? (256 / ROWB) : 1;   // rows per 256-B bank row: 2 / 1
    constexpr MatchLds L = match_lds(F32, TQ, STORE);
    static_assert(L.staging <= L.bytes && L.epilogue <= L.bytes, "the launch's LDS holds the staging and the epilogue image");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* Gs = smem;                                  // [2][128 rows][ROWB]
    unsigned char* Qs = smem + L.q;

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int wc = wid >> 1, wp = wid & 1;
    int tile_g, tile_q;
    match_tile_of_block(a.tiles_g, a.tiles_q, tile_g, tile_q);
    const int c = tid % CPR, r0 = tid / CPR;

    const unsigned char* gbase = (const unsigned char*)a.g;
    const unsigned char* qbase = (const unsigned char*)a.q;
    const size_t rowbytes = (size_t)a.D * ES;
    const __amdgpu_buffer_rsrc_t srd_g = __builtin_amdgcn_make_buffer_rsrc((void*)a.g, 0, (unsigned)((size_t)a.Gn * rowbytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t srd_q = __builtin_amdgcn_make_buffer_rsrc((void*)a.q, 0, (unsigned)((size_t)a.Qn * rowbytes), 0x00020000);

    // register staging, TWO K-steps deep: the loads of step kt + 2 are issued before the MFMAs of step kt, so a load has a
    // whole iteration (and the barrier) to land before it is written to LDS -- one step deep, every iteration waited out most
    // of an L2 / HBM round trip (~2 us per K-step, the whole kernel was that latency times D / 64)
    constexpr int NS = F32 ? 1 : 2;      // staging slots = K-steps a load has to land (the f32 rows are twice as wide: two sets would spill;
                                         // three slots measured the same as two: 67-69 vs 66 us at 1 600 x 10 000 x 1 024)
    u32x4 greg[NS][PASS], qreg[NS][PASSQ];
    auto load_tile = [&](int kt, int slot) {
#pragma unroll
        for (int i = 0; i < PASS; ++i) {
            int gr = tile_g * MT_TG + r0 + i * RPP;
            // buffer loads: rows past the end are out of the descriptor's range and read as zeros -- no branch around the load,
            // so the compiler can count the loads in flight (behind a branch it waits with vmcnt(0): the staging collapses)
            greg[slot][i] = __builtin_amdgcn_raw_buffer_load_b128(srd_g, (unsigned)gr * (unsigned)rowbytes + (unsigned)(kt * ROWB + c * 16), 0, 0);
            if (i < PASSQ) {
                int qr = tile_q * TQ + r0 + i * RPP;
                qreg[slot][i] = __builtin_amdgcn_raw_buffer_load_b128(srd_q, (unsigned)qr * (unsigned)rowbytes + (unsigned)(kt * ROWB + c * 16), 0, 0);
            }
        }
    };
    auto store_tile = [&](int buf, int slot) {
#pragma unroll
        for (int i = 0; i < PASS; ++i) {
            int row = r0 + i * RPP;
            int phys = c ^ ((row / RPB) & (CPR - 1));
            *reinterpret_cast<u32x4*>(Gs + (size_t)buf * MT_TG * ROWB + row * ROWB + phys * 16) = greg[slot][i];
            if (i < PASSQ) *reinterpret_cast<u32x4*>(Qs + (size_t)buf * TQ * ROWB + row * ROWB + phys * 16) = qreg[slot][i];
        }
    };

    f32x16 acc[2][NT];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int nk = a.D / MT_BK;
    const int lr = lane & 31, lh = lane >> 5;
#pragma unroll
    for (int sl = 0; sl < NS; ++sl) load_tile(sl < nk ? sl : nk - 1, sl);
    store_tile(0, 0);
    __syncthreads();
    int cur = 0;
    // (the loop is unrolled by NS so that the staging slot of a step is a compile-time index: registers, not scratch)
    auto k_step = [&](int kt, auto slot_c) {
        constexpr int SLOT = decltype(slot_c)::value % NS;  // slot holding step kt + 1; the loads of step kt + NS go to the slot step kt came from
        // No branch around the loads or the LDS stores (past the last K-step they re-fetch the last tile into buffers nobody
        // reads): with one straight-line path the compiler's vmcnt bookkeeping is exact -- behind `if (kt + 2 < nk)` it waited
        // for the minimum over both paths, i.e. for the newest loads as well.
        const int last = nk - 1;
        load_tile(kt + NS < nk ? kt + NS : last, (SLOT + NS - 1) % NS);
        __builtin_amdgcn_sched_barrier(0);      // keep the loads ahead of the MFMA section (the scheduler otherwise sinks them to the barrier)
        const unsigned char* Gb = Gs + (size_t)cur * MT_TG * ROWB;
        const unsigned char* Qb = Qs + (size_t)cur * TQ * ROWB;
        if constexpr (!F32) {
#pragma unroll
            for (int kk = 0; kk < MT_BK / 16; ++kk) {
                const int chunk = kk * 2 + lh;
                bf16x8 af[2], bfr[NT];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    int row = wc * 64 + mt * 32 + lr;
                    af[mt] = *reinterpret_cast<const bf16x8*>(Gb + row * ROWB + ((chunk ^ ((row / RPB) & (CPR - 1))) * 16));
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    int rowq = wp * 32 * NT + nt * 32 + lr;
                    bfr[nt] = *reinterpret_cast<const bf16x8*>(Qb + rowq * ROWB + ((chunk ^ ((rowq / RPB) & (CPR - 1))) * 16));
                }
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                    for (int nt = 0; nt < NT; ++nt)
                        acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[mt], bfr[nt], acc[mt][nt], 0, 0, 0);
            }
        } else {
            // v_mfma_f32_32x32x2_f32: lane holds A[row lr][k = lh], B[k = lh][col lr]; read 4 k-steps (8 k) per 16-B chunk pair
#pragma unroll
            for (int k4 = 0; k4 < MT_BK / 8; ++k4) {
                // lane half lh reads the 16-B chunk (2*k4 + lh): k = 8*k4 + 4*lh + {0..3}; the 4 MFMAs then pair
                // element e of half 0 with element e of half 1 -- a permutation of k, identical for A and B.
                const int chunk = k4 * 2 + lh;
                f32x4 af[2], bfr[NT];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    int row = wc * 64 + mt * 32 + lr;
                    af[mt] = *reinterpret_cast<const f32x4*>(Gb + row * ROWB + ((chunk ^ ((row / RPB) & (CPR - 1))) * 16));
                }
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    int rowq = wp * 32 * NT + nt * 32 + lr;
                    bfr[nt] = *reinterpret_cast<const f32x4*>(Qb + rowq * ROWB + ((chunk ^ ((rowq / RPB) & (CPR - 1))) * 16));
                }
#pragma unroll
                for (int e = 0; e < 4; ++e)
#pragma unroll
                    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                        for (int nt = 0; nt < NT; ++nt)
                            acc[mt][nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(af[mt][e], bfr[nt][e], acc[mt][nt], 0, 0, 0);
            }
        }
        store_tile(cur ^ 1, SLOT);
        // raw barrier: `__syncthreads()` also waits for vmcnt(0), i.e. for the loads of step kt + 2 issued a moment ago -- every
        // K-step then costs a whole L2 / HBM round trip and the two-deep staging hides nothing.  What the hand-off needs is that
        // this wave's LDS stores have landed (lgkmcnt) and that every wave is past its reads of the other buffer (the barrier).
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        cur ^= 1;
    };
    int kt = 0;
    for (; kt + NS <= nk; kt += NS) {
        k_step(kt, std::integral_constant<int, 1 % NS>{});
        if constexpr (NS > 1) k_step(kt + 1, std::integral_constant<int, 2 % NS>{});
        if constexpr (NS > 2) k_step(kt + 2, std::integral_constant<int, 3 % NS>{});
    }
    if constexpr (NS > 1) {                                         // the K-steps left over
        if (kt < nk) k_step(kt, std::integral_constant<int, 1 % NS>{});
        if constexpr (NS > 2) { if (kt + 1 < nk) k_step(kt + 1, std::integral_constant<int, 2 % NS>{}); }
    }

    // ---- epilogue: the tile's distances to LDS (match_tile_distances), then to the distance block (STORE) or per-query top-k ----
    float* T = reinterpret_cast<float*>(smem);
    match_tile_distances<F32, TQ, L.ldg, L.ldq>(a, tile_g, tile_q, acc, T, reinterpret_cast<float*>(smem + L.gn));
    if constexpr (STORE) {
        // every query's 128 distances to its row of the block, coalesced along g
        const int qv = min(TQ, a.Qn - tile_q * TQ);                   // query rows of this tile inside the block
        float* out = a.dist + (size_t)tile_q * TQ * a.ldd + (size_t)tile_g * MT_TG;
        for (int i = tid; i < qv * MT_TG; i += 256) out[(size_t)(i >> 7) * a.ldd + (i & 127)] = T[(i >> 7) * L.ldq + (i & 127)];
        return;
    }
    constexpr int NH = 256 / TQ;                                      // threads per query in the scan: 2 | 4 parts of the 128 gallery rows
    float* cd = reinterpret_cast<float*>(smem + L.cd);                // [NH][TQ]
    int* cix = reinterpret_cast<int*>(smem + L.cix);
    const int ql = tid & (TQ - 1), part = tid / TQ;
    const int qg = tile_q * TQ + ql;
    float pd = -INFINITY;
    int pi = -1;
    for (int r = 0; r < a.k; ++r) {
        float bd = INFINITY;
        int bi = 0x7FFFFFFF;
        for (int g0 = part * (MT_TG / NH); g0 < (part + 1) * (MT_TG / NH); g0 += 8) {
            float dv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) dv[u] = T[(g0 + u) * TQ + ql];              // 8 LDS reads in flight
#pragma unroll
            for (int u = 0; u < 8; ++u) match_take(dv[u], tile_g * MT_TG + g0 + u, pd, pi, bd, bi);
        }
        cd[part * TQ + ql] = bd;
        cix[part * TQ + ql] = bi;
        __syncthreads();
#pragma unroll
        for (int p = 1; p < NH; ++p)                     // every part learns the tile's minimum: it bounds its next round
            lex_min(cd[((part + p) & (NH - 1)) * TQ + ql], cix[((part + p) & (NH - 1)) * TQ + ql], bd, bi);
        pd = bd; pi = bi;
        if (part == 0 && qg < a.Qn) {
            const size_t o = ((size_t)qg * a.tiles_g + tile_g) * a.k + r;
            a.part_d[o] = bd;
            a.part_i[o] = bi;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Large query batches (round 5; BASELINE configs[3] at 1 600 queries): a 256-gallery-row x (64 NQ)-query tile per workgroup of
// EIGHT waves (4 along the gallery x 2 along the queries: a wave owns 64 gallery rows x 32 NQ queries = 2 x NQ accumulators of
// v_mfma_f32_32x32x16_bf16), both operands brought in by LDS-DMA (`buffer_load_dwordx4 ... lds`: 8 neighbouring lanes fetch one
// whole 128-byte line of a row; the XOR swizzle that makes the ds_read_b128 fragment reads conflict-free is applied to the SOURCE
// address, the LDS image of a piece is lane-linear) into two 64-deep K-stages, ONE raw barrier per K-stage, and the hand-off
// hidden behind MFMAs: the last of a stage's four 16-deep steps is multiplied AFTER the next stage's barrier, while that stage's
// first fragments are on their way from LDS.  The 128 x 128 kernel above re-reads every operand byte twice as often from L2
// (2 x (128 + 128) rows per 2 x 128 x 128 products against (256 + 320) rows per 256 x 320) and stages through registers + ds_write:
// at 1 600 x 10 000 x 1 024 its K-steps are bound by that traffic (477 TFLOP/s).
//
// Every product is accumulated by the SAME instruction in the SAME K order as in `match_kernel` (32x32x16, 16-deep steps in
// ascending K, one accumulator per (gallery row, query)), and the distance is formed by the same expression: a query's distances do
// not depend on which of the kernels -- i.e. on how many queries it was batched with -- computed them.
// The tile's k nearest rows per query are selected IN REGISTERS (a lane holds 32 gallery rows of each of its NQ queries, in
// ascending row order), combined across the two lane halves by a lane exchange and across the four gallery waves through 10 KiB
// of LDS; partials [Q][tiles_g][k] as above, merged by match_merge_kernel.
// ---------------------------------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void lds_void_m;
typedef __attribute__((address_space(3))) char lds_char_m;

// MG = gallery fragments (32 rows) per wave: the tile is TG = 128 MG gallery rows (MG = 2: the throughput form; MG = 1: twice the workgroups
// for launches that would otherwise leave most CUs without a tile -- a few hundred queries, where the time is the per-CU operand intake)
template <int NQ, int MG>
__global__ __launch_bounds__(512, 1) void match_big_kernel(MatchArgs a) {
    constexpr int TQ = 64 * NQ;
    constexpr int TG = 128 * MG;
    constexpr int GP = 2 * MG;                          // gallery DMA pieces per wave and stage (TG / 8 rows per piece / 8 waves)
    constexpr MatchBigLds L = match_big_lds(NQ, MG);
    constexpr int STAGE = L.stage;                      // gallery rows, then query rows
    static_assert(TG * 4 <= L.cd && L.epilogue <= L.bytes, "the epilogue's regions lie within the staging");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wg = wid >> 1, wq = wid & 1;
    const int lr = lane & 31, lh = lane >> 5;
    int tile_g, tile_q;
    match_tile_of_block(a.tiles_g, a.tiles_q, tile_g, tile_q);
    const unsigned rowbytes = (unsigned)a.D * 2u;
    const __amdgpu_buffer_rsrc_t srd_g = __builtin_amdgcn_make_buffer_rsrc((void*)a.g, 0, (unsigned)((size_t)a.Gn * rowbytes), 0x00020000);
    const __amdgpu_buffer_rsrc_t srd_q = __builtin_amdgcn_make_buffer_rsrc((void*)a.q, 0, (unsigned)((size_t)a.Qn * rowbytes), 0x00020000);

    // DMA piece = 8 rows x 128 B; lane = 8 rr + p fills physical chunk p of row 8 piece + rr with the row's logical chunk
    // p ^ ((row >> 1) & 7).  Wave w takes gallery pieces w, w + 8, w + 16, w + 24 and query pieces w + 8 j (j < NQ); rows beyond the
    // matrix lie beyond the descriptor's range and arrive as zeros.
    const int rr = lane >> 3, pch = lane & 7;
    unsigned vg[GP], vq[NQ];
#pragma unroll
    for (int j = 0; j < GP; ++j) {
        const int row = (wid + 8 * j) * 8 + rr;
        vg[j] = (unsigned)(tile_g * TG + row) * rowbytes + (unsigned)((pch ^ ((row >> 1) & 7)) << 4);
    }
#pragma unroll
    for (int j = 0; j < NQ; ++j) {
        const int row = (wid + 8 * j) * 8 + rr;
        vq[j] = (unsigned)(tile_q * TQ + row) * rowbytes + (unsigned)((pch ^ ((row >> 1) & 7)) << 4);
    }
    // fragment addresses: A block mg = gallery rows 64 wg + 32 mg + lr, B block nq = query rows 32 NQ wq + 32 nq + lr; the 16-deep step kk
    // of a stage = logical chunks 2 kk + lh, physical chunk ^ ((row >> 1) & 7) = ^ ((lr >> 1) & 7) (the block bases are multiples of 16)
    const unsigned lds0 = (unsigned)(size_t)(lds_char_m*)smem;
    const unsigned sw = (unsigned)((lr >> 1) & 7);
    unsigned ca[4], cb[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
        const unsigned co = ((unsigned)(2 * kk + lh) ^ sw) << 4;
        ca[kk] = lds0 + (unsigned)((32 * MG * wg + lr) * MB_ROWB) + co;
        cb[kk] = lds0 + (unsigned)(TG * MB_ROWB + (32 * NQ * wq + lr) * MB_ROWB) + co;
    }

    f32x16 acc[MG][NQ];
#pragma unroll
    for (int i = 0; i < MG; ++i)
#pragma unroll
        for (int j = 0; j < NQ; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;
    bf16x8 fa[2][MG], fb[2][NQ];            // two fragment sets: step s in set s & 1

#define MB_READ(SET, KK, SOFF)                                                                                              \
    {                                                                                                                       \
        const unsigned a_ = ca[KK] + (SOFF), b_ = cb[KK] + (SOFF);                                                          \
        _Pragma("unroll") for (int i = 0; i < MG; ++i)                                                                       \
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fa[SET][i]) : "v"(a_), "n"(i * 32 * MB_ROWB));              \
        _Pragma("unroll") for (int j = 0; j < NQ; ++j)                                                                      \
            asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(fb[SET][j]) : "v"(b_), "n"(j * 32 * MB_ROWB));              \
    }
#define MB_MFMA(SET)                                                                                                        \
    {                                                                                                                       \
        __builtin_amdgcn_s_setprio(1);                                                                                      \
        _Pragma("unroll") for (int i = 0; i < MG; ++i)                                                                       \
            _Pragma("unroll") for (int j = 0; j < NQ; ++j)                                                                  \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[SET][i], fb[SET][j], acc[i][j], 0, 0, 0);            \
        __builtin_amdgcn_s_setprio(0);                                                                                      \
    }
    // the wait, then every fragment register of the set tied to it (the compiler must not move the MFMAs that read them above the wait)
#define MB_WAIT(SET)                                                                                                        \
    {                                                                                                                       \
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                                                                  \
        _Pragma("unroll") for (int i = 0; i < MG; ++i) asm volatile("" : "+v"(fa[SET][i]));                                 \
        _Pragma("unroll") for (int j = 0; j < NQ; ++j) asm volatile("" : "+v"(fb[SET][j]));                                 \
    }

    // one DMA piece of stage KT: IDX 0..GP-1 = this wave's gallery pieces, GP.. = its query pieces
    constexpr int NP = GP + NQ;
    auto piece = [&](int kt, int buf, int idx) {
        unsigned char* dst = smem + buf * STAGE;
        const int koff = kt * MB_ROWB;
        if (idx < GP) __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_g, (lds_void_m*)(dst + (wid + 8 * idx) * 1024), 16, (int)vg[idx], koff, 0, 0);
        else __builtin_amdgcn_raw_ptr_buffer_load_lds(srd_q, (lds_void_m*)(dst + TG * MB_ROWB + (wid + 8 * (idx - GP)) * 1024), 16, (int)vq[idx - GP], koff, 0, 0);
    };
    // the MFMAs of one step with DMA pieces FIRST .. FIRST + COUNT - 1 of stage KT issued between them, one behind each MFMA: issuing a piece
    // takes the wave ~60-100 clocks (MI355X_MICROARCH.md), which the matrix pipe spends on the MFMA just queued -- all nine pieces in a row
    // right behind the barrier left the pipe idle for as long, in every wave at once
#define MB_MFMA_DMA(SET, KT, BUF, FIRST, COUNT, MORE)                                                                       \
    {                                                                                                                       \
        _Pragma("unroll") for (int i = 0; i < MG; ++i)                                                                       \
            _Pragma("unroll") for (int j = 0; j < NQ; ++j) {                                                                \
                acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fa[SET][i], fb[SET][j], acc[i][j], 0, 0, 0);            \
                __builtin_amdgcn_sched_barrier(0);                                                                          \
                if (i * NQ + j < (COUNT) && (MORE)) piece(KT, BUF, (FIRST) + i * NQ + j);   /* (a scalar branch around one instruction) */ \
                __builtin_amdgcn_sched_barrier(0);                                                                          \
            }                                                                                                               \
    }
    constexpr int PA = (NP + 1) / 2;       // pieces issued among the deferred MFMAs; the other NP - PA among step 0's
    static_assert(PA <= MG * NQ && NP - PA <= MG * NQ, "one piece per MFMA");

    const int nk = a.D >> 6;
    // two stages are in flight from the start (both buffers are free)
#pragma unroll
    for (int i = 0; i < NP; ++i) piece(0, 0, i);
    if (nk > 1) {
#pragma unroll
        for (int i = 0; i < NP; ++i) piece(1, 1, i);
        asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP) : "memory");      // stage 0 has landed for this wave; stage 1's pieces stay in flight
    } else {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    }
    __builtin_amdgcn_s_barrier();
    __builtin_amdgcn_sched_barrier(0);
    MB_READ(0, 0, 0u)
    MB_WAIT(0)
    MB_READ(1, 1, 0u)
    __builtin_amdgcn_sched_barrier(0);
    MB_MFMA(0)
    __builtin_amdgcn_sched_barrier(0);
    MB_WAIT(1)
    MB_READ(0, 2, 0u)
    __builtin_amdgcn_sched_barrier(0);
    MB_MFMA(1)
    __builtin_amdgcn_sched_barrier(0);
    MB_WAIT(0)
    MB_READ(1, 3, 0u)
    __builtin_amdgcn_sched_barrier(0);
    MB_MFMA(0)
    __builtin_amdgcn_sched_barrier(0);
    MB_WAIT(1)
    for (int kt = 1; kt < nk; ++kt) {
        const unsigned soff = (unsigned)((kt & 1) * STAGE);
        const int nb = (kt + 1) & 1;
        // stage kt has landed for this wave (its only loads in flight), and -- behind the barrier -- for every wave; every wave has
        // also finished its fragment reads of stage kt - 1 (lgkmcnt(0) above), whose buffer the next DMA overwrites
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        __builtin_amdgcn_sched_barrier(0);
        MB_READ(0, 0, soff)
        __builtin_amdgcn_sched_barrier(0);
        // step 3 of stage kt - 1 (its fragments are in registers): covers the barrier skew, the first reads' latency and half of the
        // next stage's DMA issue
        const bool more = kt + 1 < nk;
        MB_MFMA_DMA(1, kt + 1, nb, 0, PA, more)
        __builtin_amdgcn_sched_barrier(0);
        MB_WAIT(0)
        MB_READ(1, 1, soff)
        __builtin_amdgcn_sched_barrier(0);
        MB_MFMA_DMA(0, kt + 1, nb, PA, NP - PA, more)
        __builtin_amdgcn_sched_barrier(0);
        MB_WAIT(1)
        MB_READ(0, 2, soff)
        __builtin_amdgcn_sched_barrier(0);
        MB_MFMA(1)
        __builtin_amdgcn_sched_barrier(0);
        MB_WAIT(0)
        MB_READ(1, 3, soff)
        __builtin_amdgcn_sched_barrier(0);
        MB_MFMA(0)
        __builtin_amdgcn_sched_barrier(0);
        MB_WAIT(1)                                       // step 3's fragments are in registers before the next barrier
    }
    MB_MFMA(1)
#undef MB_MFMA_DMA
#undef MB_READ
#undef MB_MFMA
#undef MB_WAIT

    // ---- epilogue: per-query k smallest (distance, row) of this tile's 256 gallery rows --------------------------------------------
    __builtin_amdgcn_s_barrier();                                   // every wave is past its last fragment read: the staging LDS is free
    float* s_rg = reinterpret_cast<float*>(smem);                   // [256] 1 / |g| (NaN for rows past the gallery: never selected)
    float* cd = reinterpret_cast<float*>(smem + L.cd);              // [4][TQ] candidates of the four gallery waves
    int* cix = reinterpret_cast<int*>(smem + L.cix);
    float* wd = reinterpret_cast<float*>(smem + L.wd);              // [TQ] the round's winner (k > 1: bounds the next round)
    int* wix = reinterpret_cast<int*>(smem + L.wix);
    if (tid < TG) {
        const int gg = tile_g * TG + tid;
        s_rg[tid] = (gg < a.Gn) ? match_norm_term<false>(a.gn[gg]) : __builtin_nanf("");
    }
    __syncthreads();
    float qnv[NQ];
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq) {
        const int qg = tile_q * TQ + 32 * NQ * wq + 32 * nq + lr;
        qnv[nq] = match_norm_term<false>((qg < a.Qn) ? a.qn[qg] : 1.f);
    }
    const int g0 = tile_g * TG + 32 * MG * wg + 4 * lh;               // gallery row of accumulator element (mg, e): g0 + 32 mg + (e & 3) + 8 (e >> 2)
    float pd[NQ];
    int pi[NQ];
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq) { pd[nq] = -INFINITY; pi[nq] = -1; }
    for (int r = 0; r < a.k; ++r) {
        float bd[NQ];
        int bi[NQ];
        if (a.k == 1) {
            // k = 1 (production.py's classify, the bench): one pass, five VALU instructions per pair (multiply, fused multiply-add,
            // compare, two selects).  The candidate starts as (+inf, the lane's first row): a NaN distance (row past the gallery: NaN
            // norm; non-finite embedding) compares false and is never taken, an all-NaN query keeps (+inf, first row) -- after the
            // lexicographic combines below: the tile's first row, what the general scan and the 128-row kernel return for it
#pragma unroll
            for (int nq = 0; nq < NQ; ++nq) { bd[nq] = INFINITY; bi[nq] = g0; }
#pragma unroll
            for (int mg = 0; mg < MG; ++mg)
#pragma unroll
                for (int r4 = 0; r4 < 4; ++r4) {
                    const f32x4 gn4 = *reinterpret_cast<const f32x4*>(s_rg + 32 * MG * wg + 32 * mg + 8 * r4 + 4 * lh);
#pragma unroll
                    for (int e4 = 0; e4 < 4; ++e4) {
                        const int gi = g0 + 32 * mg + e4 + 8 * r4;
#pragma unroll
                        for (int nq = 0; nq < NQ; ++nq) {
                            const float d = match_distance<false>(acc[mg][nq][4 * r4 + e4], qnv[nq], gn4[e4]);
                            const bool take = d < bd[nq];
                            bd[nq] = take ? d : bd[nq];
                            bi[nq] = take ? gi : bi[nq];
                        }
                    }
                }
        } else {
#pragma unroll
        for (int nq = 0; nq < NQ; ++nq) { bd[nq] = INFINITY; bi[nq] = 0x7FFFFFFF; }
        // (gallery rows in ascending order: mg, then e -- a lane keeps the lowest row among equal distances by strict comparison)
#pragma unroll
        for (int mg = 0; mg < MG; ++mg)
#pragma unroll
            for (int r4 = 0; r4 < 4; ++r4) {
                const f32x4 gn4 = *reinterpret_cast<const f32x4*>(s_rg + 32 * MG * wg + 32 * mg + 8 * r4 + 4 * lh);   // this lane's four rows' norms
#pragma unroll
                for (int e4 = 0; e4 < 4; ++e4) {
                    const int gi = g0 + 32 * mg + e4 + 8 * r4;
                    // rows past the gallery (NaN norm) are never candidates; a NaN distance of a real row (non-finite embedding) sorts last
                    const bool real = gn4[e4] == gn4[e4];
#pragma unroll
                    for (int nq = 0; nq < NQ; ++nq) {
                        float d = match_distance<false>(acc[mg][nq][4 * r4 + e4], qnv[nq], gn4[e4]);
                        d = (d == d) ? d : INFINITY;
                        // match_take's rule, branch-free (bitwise, not short-circuit): after the previous pick AND before the best so far.  gi
                        // ascends along the scan, so "before the best" is d < best alone
                        const bool after = (d > pd[nq]) | ((d == pd[nq]) & (gi > pi[nq]));
                        // (equal distances keep the lower row = the earlier one of this ascending scan; an all-infinite query -- non-finite
                        // embedding -- must still pick its first admissible row: `bi` untouched means nothing was taken yet)
                        const bool take = real & after & ((d < bd[nq]) | (bi[nq] == 0x7FFFFFFF));
                        bd[nq] = take ? d : bd[nq];
                        bi[nq] = take ? gi : bi[nq];
                    }
                }
            }
        }
#pragma unroll
        for (int nq = 0; nq < NQ; ++nq) {
            // the other half of the wave holds the other 32 gallery rows of the same query
            lex_min(__shfl_xor(bd[nq], 32), __shfl_xor(bi[nq], 32), bd[nq], bi[nq]);
            if (lh == 0) {
                cd[wg * TQ + 32 * NQ * wq + 32 * nq + lr] = bd[nq];
                cix[wg * TQ + 32 * NQ * wq + 32 * nq + lr] = bi[nq];
            }
        }
        __syncthreads();
        if (tid < TQ) {
            float bd = cd[tid];
            int bi = cix[tid];
#pragma unroll
            for (int w = 1; w < 4; ++w) lex_min(cd[w * TQ + tid], cix[w * TQ + tid], bd, bi);
            wd[tid] = bd;
            wix[tid] = bi;
            const int qg = tile_q * TQ + tid;
            if (qg < a.Qn) {
                const size_t o = ((size_t)qg * a.tiles_g + tile_g) * a.k + r;
                a.part_d[o] = bd;
                a.part_i[o] = bi;
            }
        }
        if (r + 1 < a.k) {
            __syncthreads();
#pragma unroll
            for (int nq = 0; nq < NQ; ++nq) {
                pd[nq] = wd[32 * NQ * wq + 32 * nq + lr];
                pi[nq] = wix[32 * NQ * wq + 32 * nq + lr];
            }
            __syncthreads();
        }
    }
}

// One WAVE per query: the n partial (distance, index) pairs are spread over the lanes (coalesced loads, all in flight at once --
// one thread walking them paid an L2 round trip per entry), each of the k rounds takes the wave-wide lexicographic minimum of
// the entries greater than the previous pick.
__global__ __launch_bounds__(256) void match_merge_kernel(const float* __restrict__ part_d, const int* __restrict__ part_i, int Qn, int n,
                                                          int k, long long* __restrict__ out_idx, float* __restrict__ out_dist) {
    const int q = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (q >= Qn) return;
    const float* d = part_d + (size_t)q * n;
    const int* ix = part_i + (size_t)q * n;
    constexpr int PER = 8;                      // entries per lane held in registers: n <= 512, else the strided loop below
    float dv[PER];
    int iv[PER];
#pragma unroll
    for (int e = 0; e < PER; ++e) {
        const int j = e * 64 + lane;
        dv[e] = (j < n) ? d[j] : INFINITY;
        iv[e] = (j < n) ? ix[j] : 0x7FFFFFFF;
    }
    float pd = -INFINITY;
    int pi = -1;
    for (int r = 0; r < k; ++r) {
        float bd = INFINITY;
        int bi = 0x7FFFFFFF;
#pragma unroll
        for (int e = 0; e < PER; ++e) match_take(dv[e], iv[e], pd, pi, bd, bi);
        for (int j = PER * 64 + lane; j < n; j += 64) match_take(d[j], ix[j], pd, pi, bd, bi);   // (n > 512: the tail straight from memory)
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) lex_min(__shfl_xor(bd, off), __shfl_xor(bi, off), bd, bi);
        if (lane == 0) {
            out_idx[(size_t)q * k + r] = (long long)bi;
            if (out_dist) out_dist[(size_t)q * k + r] = bd;
        }
        pd = bd; pi = bi;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Large k (MATCH_KMAX < k <= Gn).  The fused epilogues above cost O(k) selection rounds per tile and O(k^2 tiles) in the merge,
// so past k = 16 the search changes algorithm, per query chunk of the call:
//   1. match_kernel<F32, TQ, true> writes the chunk's distances [Qc][Gpad] (fp32, Gpad = Gn rounded up to the 128-row tile);
//   2. match_select_kernel, one workgroup per query: an exact radix select of the k smallest (distance, row) pairs, written
//      unordered as 64-bit keys [Qc][k];
//   3. match_sort_kernel sorts them in LDS (bitonic, runs of MATCH_SORT_RUN keys) and writes the results; k above one run:
//      match_merge_runs_kernel merges sorted runs pairwise through the workspace until one run is left.
//
// Keys: the 32-bit monotone image of the distance (match_key32) above the row index.  The epilogue's distances are
// 1 - dot / (|q| |g|) or fma(-dot, 1/|q| 1/|g|, 1): an exact zero of `1 - x` is +0 in round-to-nearest, so -0.0 never occurs,
// and NaN was made +inf -- on these values the integer order of the keys IS the lexicographic order lex_lt, ties to the
// lower row included.  Distances come back from the keys bit for bit (match_key_distance).
// ---------------------------------------------------------------------------------------------------------------------
#define MATCH_LK_BUDGET (256ull << 20)    // workspace of the large-k path: queries are processed in chunks that fit this
#define MATCH_SORT_RUN 16384              // keys sorted in LDS by one workgroup (128 KiB of 64-bit keys)
#define MATCH_SEL_THREADS 512
#define MATCH_SEL_BINS 2048               // histogram of one select pass: 11 bits of the key
#define MATCH_SEL_STAGE 32768             // rows of a query kept in LDS during the select (128 KiB); longer rows stream from L2

struct MatchLargeK {
    int qc;                                // queries per chunk
    size_t gpad;                           // row stride of the distance block
    size_t dist_bytes, surv_bytes;         // distance block, survivor keys (twice when the merge passes need a ping-pong buffer)
    size_t bytes;
};
static MatchLargeK match_large_k_plan(int Qn, int Gn, int k) {
    MatchLargeK p;
    p.gpad = ((size_t)Gn + MT_TG - 1) / MT_TG * MT_TG;
    const int nsurv = k > MATCH_SORT_RUN ? 2 : 1;
    const size_t per = p.gpad * 4 + (size_t)k * 8 * nsurv;
    size_t qc = MATCH_LK_BUDGET / per;
    if (qc >= MT_TQ) qc = qc / MT_TQ * MT_TQ;       // whole query tiles where the budget allows
    if (qc < 1) qc = 1;
    if (qc > (size_t)Qn) qc = Qn;
    p.qc = (int)qc;
    p.dist_bytes = (qc * p.gpad * 4 + 255) / 256 * 256;
    p.surv_bytes = (qc * (size_t)k * 8 + 255) / 256 * 256;
    p.bytes = p.dist_bytes + nsurv * p.surv_bytes;
    return p;
}

// block-wide exclusive prefix sum of one unsigned per thread (MATCH_SEL_THREADS threads) -> (prefix, total); `red` holds 8 + 1 words
__device__ __forceinline__ unsigned sel_block_scan(unsigned v, unsigned* red, unsigned& total) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    unsigned x = v;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const unsigned y = __shfl_up(x, off);
        if (lane >= off) x += y;
    }
    if (lane == 63) red[wid] = x;
    __syncthreads();
    unsigned before = 0, all = 0;
#pragma unroll
    for (int w = 0; w < MATCH_SEL_THREADS / 64; ++w) {
        const unsigned t = red[w];
        before += w < wid ? t : 0u;
        all += t;
    }
    __syncthreads();                       // (red is reused by the next scan)
    total = all;
    return before + x - v;
}

// One workgroup per query row of the distance block: the threshold key T with #(key < T) < k <= #(key <= T) by radix passes
// over the key range [min, max] (11 bits per pass, histogram in LDS), then every row below T and the lowest-index rows equal to T
// (an ordered block scan, no atomics) -> surv[q][0..k) = (key << 32 | row), unordered.
template <bool STAGED>
__global__ __launch_bounds__(MATCH_SEL_THREADS) void match_select_kernel(const float* __restrict__ dist, int ldd, int Gn, int k,
                                                                         unsigned long long* __restrict__ surv) {
    extern __shared__ __attribute__((aligned(16))) unsigned sel_smem[];
    unsigned* hist = sel_smem;                            // [MATCH_SEL_BINS]
    unsigned* red = sel_smem + MATCH_SEL_BINS;            // [64] scan / reduction scratch
    unsigned* keys = sel_smem + MATCH_SEL_BINS + 64;      // [Gn] (STAGED)
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* row = dist + (size_t)blockIdx.x * ldd;
    unsigned long long* out = surv + (size_t)blockIdx.x * k;
    auto key_at = [&](int i) -> unsigned {
        if constexpr (STAGED) return keys[i];
        else return match_key32(row[i]);
    };

    // pass 0: the key range (and the row into LDS)
    unsigned mn = 0xFFFFFFFFu, mx = 0u;
    for (int i = tid; i < Gn; i += MATCH_SEL_THREADS) {
        const unsigned u = match_key32(row[i]);
        if constexpr (STAGED) keys[i] = u;
        mn = min(mn, u);
        mx = max(mx, u);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        mn = min(mn, (unsigned)__shfl_xor(mn, off));
        mx = max(mx, (unsigned)__shfl_xor(mx, off));
    }
    if (lane == 0) { red[wid] = mn; red[16 + wid] = mx; }
    __syncthreads();
    unsigned lo = red[0], hi = red[16];
#pragma unroll
    for (int w = 1; w < MATCH_SEL_THREADS / 64; ++w) { lo = min(lo, red[w]); hi = max(hi, red[16 + w]); }
    __syncthreads();

    // the k-th smallest key lies in [lo, hi]; kk = its rank among the keys in [lo, hi] (invariant: 1 <= kk <= their count)
    unsigned kk = (unsigned)k;
    while (lo != hi) {                                    // (block-uniform: lo, hi, kk live in every thread alike)
        const unsigned width = hi - lo;
        const int bits = 32 - __builtin_clz(width);
        const int shift = bits > 11 ? bits - 11 : 0;      // (width >> shift) < MATCH_SEL_BINS
        for (int b = tid; b < MATCH_SEL_BINS; b += MATCH_SEL_THREADS) hist[b] = 0u;
        __syncthreads();
        for (int i = tid; i < Gn; i += MATCH_SEL_THREADS) {
            const unsigned u = key_at(i);
            if (u >= lo && u <= hi) atomicAdd(&hist[(u - lo) >> shift], 1u);
        }
        __syncthreads();
        constexpr int BPT = MATCH_SEL_BINS / MATCH_SEL_THREADS;   // 4 bins per thread
        unsigned h[BPT], s = 0;
#pragma unroll
        for (int j = 0; j < BPT; ++j) { h[j] = hist[tid * BPT + j]; s += h[j]; }
        unsigned total;
        const unsigned before = sel_block_scan(s, red, total);
        if (before < kk && kk <= before + s) {            // exactly one thread: the bin holding rank kk
            unsigned c = before;
            int b = 0;
#pragma unroll
            for (int j = 0; j < BPT; ++j)
                if (c + h[j] < kk) { c += h[j]; b = j + 1; }
                else break;
            red[32] = (unsigned)(tid * BPT + b);
            red[33] = kk - c;
        }
        __syncthreads();
        const unsigned bin = red[32];
        kk = red[33];
        __syncthreads();
        const unsigned nlo = lo + (bin << shift);
        const unsigned span = shift ? ((1u << shift) - 1u) : 0u;
        hi = (hi - nlo) <= span ? hi : nlo + span;
        lo = nlo;
    }
    const unsigned T = lo, need = kk;                     // take every key < T (k - need of them) and the first `need` keys == T
    const unsigned nlt = (unsigned)k - need;
    unsigned lt_base = 0, eq_base = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < Gn; base += MATCH_SEL_THREADS) {
        const int i = base + tid;
        const unsigned u = i < Gn ? key_at(i) : 0xFFFFFFFFu;
        const bool lt = i < Gn && u < T, eq = i < Gn && u == T;
        const unsigned long long mlt = __ballot(lt), meq = __ballot(eq);
        if (lane == 0) { red[wid] = (unsigned)__popcll(mlt); red[16 + wid] = (unsigned)__popcll(meq); }
        __syncthreads();
        unsigned olt = 0, oeq = 0, tlt = 0, teq = 0;
#pragma unroll
        for (int w = 0; w < MATCH_SEL_THREADS / 64; ++w) {
            const unsigned a = red[w], b = red[16 + w];
            olt += w < wid ? a : 0u;
            oeq += w < wid ? b : 0u;
            tlt += a;
            teq += b;
        }
        const unsigned long long key = ((unsigned long long)u << 32) | (unsigned)i;
        if (lt) {
            const unsigned p = lt_base + olt + (unsigned)__popcll(mlt & below);
            if (p < nlt) out[p] = key;                    // (always: exactly nlt keys lie below T)
        }
        if (eq) {
            const unsigned p = eq_base + oeq + (unsigned)__popcll(meq & below);
            if (p < need) out[nlt + p] = key;
        }
        lt_base += tlt;
        eq_base += teq;
        if (lt_base == nlt && eq_base >= need) break;     // (block-uniform)
        __syncthreads();
    }
}

// Bitonic sort of one run (P keys, a power of two, padded with all-ones keys that sort last) in LDS.  grid (queries, runs): run r of
// query q = keys [r RUN, min(k, (r + 1) RUN)) of surv[q].  One run: the results are written; several: the sorted run goes back in place.
__global__ __launch_bounds__(1024) void match_sort_kernel(unsigned long long* __restrict__ surv, int k, int P,
                                                          long long* __restrict__ out_idx, float* __restrict__ out_dist) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long sk[];
    const int tid = threadIdx.x, nt = blockDim.x;
    const int r0 = blockIdx.y * MATCH_SORT_RUN;
    const int n = min(MATCH_SORT_RUN, k - r0);
    unsigned long long* run = surv + (size_t)blockIdx.x * k + r0;
    for (int i = tid; i < P; i += nt) sk[i] = i < n ? run[i] : ~0ull;
    __syncthreads();
    for (int size = 2; size <= P; size <<= 1)
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int t = tid; t < P / 2; t += nt) {
                const int i = 2 * t - (t & (stride - 1)), j = i + stride;
                const unsigned long long x = sk[i], y = sk[j];
                if ((x > y) == ((i & size) == 0)) { sk[i] = y; sk[j] = x; }
            }
            __syncthreads();
        }
    if (gridDim.y == 1) {
        for (int i = tid; i < n; i += nt) {
            const unsigned long long key = sk[i];
            out_idx[(size_t)blockIdx.x * k + i] = (long long)(unsigned)(key & 0xFFFFFFFFull);
            if (out_dist) out_dist[(size_t)blockIdx.x * k + i] = match_key_distance(key);
        }
    } else {
        for (int i = tid; i < n; i += nt) run[i] = sk[i];
    }
}

// One merge pass over sorted runs of w keys: runs 2j and 2j + 1 become one.  Every key finds its place by its rank in the partner
// run (binary search; keys are distinct: the row index is part of the key).  grid (ceil(k / 256), queries).  out_idx set: the
// last pass, which writes the results instead of dst.
__global__ __launch_bounds__(256) void match_merge_runs_kernel(const unsigned long long* __restrict__ src, unsigned long long* __restrict__ dst,
                                                               int k, int w, long long* __restrict__ out_idx, float* __restrict__ out_dist) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= k) return;
    const size_t qo = (size_t)blockIdx.y * k;
    const unsigned long long* s = src + qo;
    const long long pair = (long long)i / (2ll * w) * (2ll * w);
    const long long off = i - pair;
    const unsigned long long key = s[i];
    long long p0, p1;                                     // the partner run [p0, p1)
    if (off < w) { p0 = pair + w; p1 = pair + 2ll * w; }
    else { p0 = pair; p1 = pair + w; }
    if (p1 > k) p1 = k;
    if (p0 > k) p0 = k;
    long long a = p0, b = p1;                             // first partner key not below `key`
    while (a < b) {
        const long long m = (a + b) >> 1;
        if (s[m] < key) a = m + 1;
        else b = m;
    }
    const long long pos = pair + (off < w ? off : off - w) + (a - p0);
    if (out_idx) {
        out_idx[qo + pos] = (long long)(unsigned)(key & 0xFFFFFFFFull);
        if (out_dist) out_dist[qo + pos] = match_key_distance(key);
    } else {
        dst[qo + pos] = key;
    }
}

// Test / measurement switches of the bf16 path: read once from the environment, core / nq / mg overwritten by cvpce_match_set_core.  Results
// never depend on them.  core (CVPCE_MATCH_CORE = small | big): 0 = by the cost model of match_plan, 1 = always the 128-row kernel, 2 = always
// the LDS-DMA kernel; nq = 2..5 (CVPCE_MATCH_NQ) and mg = 1 | 2 (CVPCE_MATCH_MG) pin that kernel's tile, tq = 64 | 128 (CVPCE_MATCH_TQ) the
// 128-row kernel's query tile; 0 = by the model.
struct MatchForced { int core, nq, mg, tq; };
static MatchForced g_match_forced = []() {
    auto num = [](const char* name) { const char* e = getenv(name); return e ? atoi(e) : 0; };
    const char* c = getenv("CVPCE_MATCH_CORE");
    const int nq = num("CVPCE_MATCH_NQ"), mg = num("CVPCE_MATCH_MG"), tq = num("CVPCE_MATCH_TQ");
    return MatchForced{!c ? 0 : (c[0] == 's' ? 1 : (c[0] == 'b' ? 2 : 0)), (nq >= 2 && nq <= 5) ? nq : 0, (mg == 1 || mg == 2) ? mg : 0,
                       (tq == 64 || tq == 128) ? tq : 0};
}();
extern "C" int cvpce_match_set_core(int core, int nq, int mg) {
    if (core < 0 || core > 2 || !(nq == 0 || (nq >= 2 && nq <= 5)) || mg < 0 || mg > 2 || (mg == 1 && nq == 5)) return CVPCE_ERR_ARG;
    g_match_forced = MatchForced{core, nq, mg, g_match_forced.tq};
    return CVPCE_OK;
}

// Every launch decision of cvpce_match_topk, made on the host without a HIP call (cvpce_match_plan reports it).
enum { MATCH_PATH_SMALL = 0, MATCH_PATH_BIG = 1, MATCH_PATH_LARGE_K = 2 };
struct MatchPlan {
    int rc;                                 // CVPCE_ERR_ARG: the arguments are rejected (only `workspace` is filled in)
    int path;                               // fused top-k on the 128-row core | on the LDS-DMA core | the large-k search
    int tq;                                 // SMALL, LARGE_K: queries per tile of match_kernel
    int nq, mg;                             // BIG: match_big_kernel's tile, 64 nq queries x 128 mg gallery rows
    int tiles_g, tiles_q, lds, threads;     // the GEMM launch (LARGE_K: of a chunk of lk.qc queries)
    size_t part_i;                          // fused paths: byte offset of the partial indices in the workspace
    size_t workspace;                       // bytes cvpce_match_topk needs
    MatchLargeK lk;                         // LARGE_K
};
static MatchPlan match_plan(int Qn, int Gn, int D, int k, int is_f32, const MatchForced& f) {
    MatchPlan p = {};
    p.rc = CVPCE_ERR_ARG;
    const bool large = k > MATCH_KMAX;
    // the workspace depends on (Qn, Gn, k) alone: filled in whatever becomes of the other arguments (cvpce_match_workspace_bytes)
    const int tiles128 = (Gn + MT_TG - 1) / MT_TG;
    if (large && Qn > 0 && Gn > 0) p.lk = match_large_k_plan(Qn, Gn, k);
    p.part_i = ((size_t)Qn * tiles128 * k * 4 + 255) / 256 * 256;          // (laid out for the 128-row tiling: enough for either core)
    p.workspace = (large ? p.lk.bytes : (size_t)Qn * tiles128 * k * 8) + 512;
    if (D <= 0 || D % MT_BK != 0 || k < 1 || Gn < k) return p;
    if (Qn <= 0) { p.rc = CVPCE_OK; return p; }                            // nothing to launch
    // 32-bit buffer offsets: rows rounded up to whole tiles of tg x tq stay below 2^32 bytes
    auto fits = [&](int tg, int tq) {
        const unsigned long long es = is_f32 ? 4 : 2;
        return ((unsigned long long)Gn + tg) * D * es < (1ull << 32) && ((unsigned long long)Qn + tq) * D * es < (1ull << 32);
    };
    if (!fits(MT_TG, MT_TQ)) return p;
    const int qn = large ? p.lk.qc : Qn;                                   // queries of one GEMM launch
    const long long cus = g_cvpce_persistent_wgs;
    const long long t128 = (long long)tiles128 * ((qn + 127) / 128), t64 = (long long)tiles128 * ((qn + 63) / 64);
    const long long r128 = (t128 + 2 * cus - 1) / (2 * cus), r64 = (t64 + 3 * cus - 1) / (3 * cus);
    // query tile of the 128-row bf16 kernel: 64-query tiles cost ~0.6 of a 128-query tile and run three to a CU instead of two; the
    // cheaper schedule in whole rounds of the chip wins
    p.path = large ? MATCH_PATH_LARGE_K : MATCH_PATH_SMALL;
    p.tq = is_f32 ? MT_TQ : (f.tq ? f.tq : ((double)r64 * 0.6 < (double)r128 * 1.0 ? 64 : 128));
    // Which bf16 core and tile: the LDS-DMA kernel (match_big_kernel, 128 MG gallery rows x 64 NQ queries per workgroup) or the 128-row
    // register-staged one, by estimated time.  Model (microseconds; least-squares fit to tools/dev/bench_match.py on MI355X, 63 launches of
    // 200 ... 3 200 queries x 1 000 ... 10 000 rows x 512 | 1 024, rms error 8 %, picks the fastest variant or one within 1 % of it on all nine
    // shapes):  launch = fixed + rounds x (D / 512) x round, where a round's cost grows with the share u of the CUs that hold a tile in it
    // (L2 intake and clocks):
    //   LDS-DMA kernel:   fixed 3.9 + 0.48 NQ,  round (0.74 + 1.97 NQ) x (MG = 1 ? 0.575 : 1) x (1 + 0.75 u)
    //   128-row kernel:   fixed 10.4,           round 5.4 x (1 + 0.75 u) (64-query tiles, three per CU) | 9.0 x (1 + 0.75 u) (128-query, two per CU)
    // Every bf16 kernel forms identical distances, so the choice changes no result (MatchForced pins one: tests and A/B measurements).
    if (!is_f32 && !large) {
        const double dk = (double)D / 512.0;
        const double e128 = 10.4 + (double)r128 * dk * 9.0 * (1.0 + 0.75 * (double)t128 / (double)(r128 * 2 * cus));
        const double e64 = 10.4 + (double)r64 * dk * 5.4 * (1.0 + 0.75 * (double)t64 / (double)(r64 * 3 * cus));
        const double best = e64 < e128 ? e64 : e128;
        double best_big = 1e30;
        int big_nq = 0, big_mg = 2;
        for (int mg = 1; mg <= 2; ++mg)
            for (int nq = 2; nq <= 5; ++nq) {
                if ((f.nq && nq != f.nq) || (f.mg && mg != f.mg) || (mg == 1 && nq == 5)) continue;
                const long long t = (long long)((Gn + 128 * mg - 1) / (128 * mg)) * ((Qn + 64 * nq - 1) / (64 * nq)), rounds = (t + cus - 1) / cus;
                const double u = (double)t / (double)(rounds * cus);
                const double e = 3.9 + 0.48 * nq + (double)rounds * dk * (0.74 + 1.97 * nq) * (mg == 1 ? 0.575 : 1.0) * (1.0 + 0.75 * u);
                if (e < best_big) { best_big = e; big_nq = nq; big_mg = mg; }
            }
        // (a handful of queries against a small gallery is launch latency either way: the 128-row kernel keeps those)
        const bool keep_small = f.core == 1 || (f.core == 0 && (!(best_big < best) || (long long)Qn * Gn < 64 * 1024));
        if (big_nq && !keep_small) { p.path = MATCH_PATH_BIG; p.tq = 0; p.nq = big_nq; p.mg = big_mg; }
    }
    const bool big = p.path == MATCH_PATH_BIG;
    const int tile_g = big ? 128 * p.mg : MT_TG, tile_q = big ? 64 * p.nq : p.tq;
    if (big && !fits(tile_g, tile_q)) return p;
    p.tiles_g = (Gn + tile_g - 1) / tile_g;
    p.tiles_q = (qn + tile_q - 1) / tile_q;
    p.lds = big ? match_big_lds(p.nq, p.mg).bytes : match_lds(is_f32, p.tq, large).bytes;
    p.threads = big ? 512 : 256;
    p.rc = CVPCE_OK;
    return p;
}

extern "C" size_t cvpce_match_workspace_bytes(int Qn, int Gn, int k) { return match_plan(Qn, Gn, MT_BK, k, 0, g_match_forced).workspace; }

extern "C" int cvpce_match_plan(int Qn, int Gn, int D, int k, int is_f32, long long* out) {
    if (!out) return CVPCE_ERR_ARG;
    const MatchPlan p = match_plan(Qn, Gn, D, k, is_f32, g_match_forced);
    const long long v[CVPCE_MATCH_PLAN_FIELDS] = {p.path, p.tq, p.nq, p.mg, p.tiles_g, p.tiles_q, p.lds, p.threads, p.lk.qc, (long long)p.lk.gpad,
                                                  (long long)p.lk.bytes, (long long)p.workspace};
    for (int i = 0; i < CVPCE_MATCH_PLAN_FIELDS; ++i) out[i] = v[i];
    return p.rc;
}

// One GEMM launch of the plan: the shared-memory attribute of the instance it launches, then the launch.
template <auto Kernel>
static bool match_launch(const MatchPlan& p, const MatchArgs& a, hipStream_t s) {
    if (!cvpce_smem_attr_done<Kernel>((const void*)Kernel, p.lds)) return false;
    hipLaunchKernelGGL(Kernel, dim3(p.tiles_g * p.tiles_q), dim3(p.threads), p.lds, s, a);
    return true;
}
template <bool STORE>
static bool match_launch_small(const MatchPlan& p, int is_f32, const MatchArgs& a, hipStream_t s) {
    if (is_f32) return match_launch<match_kernel<true, 128, STORE>>(p, a, s);
    return p.tq == 128 ? match_launch<match_kernel<false, 128, STORE>>(p, a, s) : match_launch<match_kernel<false, 64, STORE>>(p, a, s);
}
static bool match_launch_big(const MatchPlan& p, const MatchArgs& a, hipStream_t s) {
    switch (p.nq * 4 + p.mg) {
#define MB_LAUNCH(NQ_, MG_) case NQ_ * 4 + MG_: return match_launch<match_big_kernel<NQ_, MG_>>(p, a, s);
        MB_LAUNCH(2, 2) MB_LAUNCH(3, 2) MB_LAUNCH(4, 2) MB_LAUNCH(5, 2) MB_LAUNCH(2, 1) MB_LAUNCH(3, 1) MB_LAUNCH(4, 1)
#undef MB_LAUNCH
    }
    return false;
}

// The large-k search (see match_select_kernel): per chunk of p.lk.qc queries, distance block -> select -> sort [-> merge passes], all on
// the caller's stream.  The distances come from match_kernel (the 128-row core; its bf16 instances form the same distances as the
// LDS-DMA core), so a query's first 16 results equal those of the fused path bit for bit.
static int match_large_k(MatchArgs a, const MatchPlan& p, int is_f32, void* workspace, hipStream_t s) {
    const int Qn = a.Qn, Gn = a.Gn, k = a.k;
    const bool staged = Gn <= MATCH_SEL_STAGE;
    const int lds_sel = (MATCH_SEL_BINS + 64 + (staged ? Gn : 0)) * 4;
    if (!cvpce_smem_attr_done<match_select_kernel<true>>((const void*)match_select_kernel<true>, (MATCH_SEL_BINS + 64 + MATCH_SEL_STAGE) * 4) ||
        !cvpce_smem_attr_done<match_sort_kernel>((const void*)match_sort_kernel, MATCH_SORT_RUN * 8))
        return CVPCE_ERR_LAUNCH;
    float* dist = (float*)workspace;
    unsigned long long* surv = (unsigned long long*)((char*)workspace + p.lk.dist_bytes);
    unsigned long long* tmp = (unsigned long long*)((char*)workspace + p.lk.dist_bytes + p.lk.surv_bytes);
    const int runs = (k + MATCH_SORT_RUN - 1) / MATCH_SORT_RUN;
    int P = 64;
    while (P < k && P < MATCH_SORT_RUN) P <<= 1;
    const int sort_threads = P / 2 < 64 ? 64 : (P / 2 > 1024 ? 1024 : P / 2);
    const size_t es = is_f32 ? 4 : 2;
    a.dist = dist;
    a.ldd = (int)p.lk.gpad;
    for (int c0 = 0; c0 < Qn; c0 += p.lk.qc) {
        const int qc = min(p.lk.qc, Qn - c0);
        const MatchPlan cp = match_plan(qc, Gn, a.D, k, is_f32, g_match_forced);    // (a shorter last chunk may take the other query tile)
        MatchArgs c = a;
        c.q = (const char*)a.q + (size_t)c0 * a.D * es;
        c.qn = a.qn + c0;
        c.Qn = qc; c.tiles_g = cp.tiles_g; c.tiles_q = cp.tiles_q;
        long long* oi = a.out_idx + (size_t)c0 * k;
        float* od = a.out_dist ? a.out_dist + (size_t)c0 * k : nullptr;
        if (!match_launch_small<true>(cp, is_f32, c, s)) return CVPCE_ERR_LAUNCH;
        if (staged) hipLaunchKernelGGL(match_select_kernel<true>, dim3(qc), dim3(MATCH_SEL_THREADS), lds_sel, s, (const float*)dist, a.ldd, Gn, k, surv);
        else hipLaunchKernelGGL(match_select_kernel<false>, dim3(qc), dim3(MATCH_SEL_THREADS), lds_sel, s, (const float*)dist, a.ldd, Gn, k, surv);
        hipLaunchKernelGGL(match_sort_kernel, dim3(qc, runs), dim3(sort_threads), (size_t)P * 8, s, surv, k, P, oi, od);
        unsigned long long *src = surv, *dst = tmp;
        for (long long w = MATCH_SORT_RUN; w < k; w *= 2) {
            const bool last = 2 * w >= k;
            hipLaunchKernelGGL(match_merge_runs_kernel, dim3((k + 255) / 256, qc), dim3(256), 0, s, (const unsigned long long*)src, dst, k, (int)w,
                               last ? oi : nullptr, last ? od : nullptr);
            unsigned long long* t = src; src = dst; dst = t;
        }
        const int rc = cvpce_check_launch();
        if (rc != CVPCE_OK) return rc;
    }
    return CVPCE_OK;
}

extern "C" int cvpce_match_topk(const void* queries, const void* gallery, const float* q_norms, const float* g_norms,
                                int Qn, int Gn, int D, int k, int is_f32, void* workspace, size_t workspace_bytes,
                                long long* out_idx, float* out_dist, void* stream) {
    if (!queries || !gallery || !q_norms || !g_norms || !workspace || !out_idx) return CVPCE_ERR_ARG;
    const MatchPlan p = match_plan(Qn, Gn, D, k, is_f32, g_match_forced);
    if (p.rc != CVPCE_OK) return p.rc;
    if (Qn <= 0) return CVPCE_OK;
    if (workspace_bytes < p.workspace) return CVPCE_ERR_ARG;
    MatchArgs a = {};
    a.q = queries; a.g = gallery; a.qn = q_norms; a.gn = g_norms; a.Qn = Qn; a.Gn = Gn; a.D = D; a.k = k;
    a.out_idx = out_idx; a.out_dist = out_dist;
    a.tiles_g = p.tiles_g; a.tiles_q = p.tiles_q;
    hipStream_t s = (hipStream_t)stream;
    if (p.path == MATCH_PATH_LARGE_K) return match_large_k(a, p, is_f32, workspace, s);
    a.part_d = (float*)workspace;
    a.part_i = (int*)((char*)workspace + p.part_i);
    if (!(p.path == MATCH_PATH_BIG ? match_launch_big(p, a, s) : match_launch_small<false>(p, is_f32, a, s))) return CVPCE_ERR_LAUNCH;
    hipLaunchKernelGGL(match_merge_kernel, dim3((Qn + 3) / 4), dim3(256), 0, s, a.part_d, a.part_i, Qn, a.tiles_g * k, k, out_idx, out_dist);
    return cvpce_check_launch();
}

