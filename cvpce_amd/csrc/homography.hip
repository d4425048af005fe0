// The tail of the planogram comparator (include/cvpce_amd_homography.h): RANSAC homography, refit, projection, per-label claim.
//
// homography_ransac_kernel: grid chunks x B, 256 threads, one hypothesis per thread.  The image's points live in LDS as the
// fp32 values they are; every thread draws its four points from a counter hash, solves its 8 x 8 system in registers (the
// elimination is unrolled with compile-time indices: a dynamically indexed 8 x 9 array would live in scratch memory) and walks
// all n points.  The workgroup's best {count, hypothesis} goes to its own workspace slot.
//
// homography_finish_kernel: one workgroup per image.  Reduces the slots, rebuilds the winner from its index, forms its inlier
// mask, accumulates the 45 distinct entries of the refit's 9 x 9 normal matrix (one thread each, points in index order), wave 0
// diagonalises it by cyclic Jacobi in LDS (lane r owns row r of a rotation), and all threads then count the refit's inliers,
// project the expected boxes and claim the detections.
//
// Every sum whose order could change a bit has a fixed order ("the tail rule"; tests/homography_device_cases.py
// restates it): the file is compiled with FMA contraction off (Makefile), the functions repeat it as a pragma, `/` and sqrt on
// doubles are the correctly rounded ones.  Reductions that run in any order are integer maxima and integer sums.
#include "common.h"
#include "../../include/cvpce_amd_homography.h"
#include <float.h>

#define HG_THREADS CVPCE_HOMOGRAPHY_CHUNK
#define HG_MAX_PAIRS CVPCE_HOMOGRAPHY_MAX_PAIRS
#define HG_MAX_NODES 1024
#define HG_SQRT2 1.4142135623730951           // Python's 2 ** 0.5
#define HG_DEGENERATE 1e-12                   // mean distance to the centroid, |h[2][2]|: planograms._dlt's own tests
#define HG_PIVOT_MIN 1e-12                    // the elimination's smallest acceptable pivot (normalised coordinates)
#define HG_THETA_MAX 1e150                    // beyond it theta * theta would overflow
#define HG_SWEEPS 10

struct HgNorm { double cx, cy, k; };          // normalised point = (p - c) * k
struct HgImage { int a0, n1, b0, n2, r0, m, n, status; };

__device__ __forceinline__ unsigned hg_hash(unsigned seed, unsigned t, unsigned draw) {
    unsigned x = seed + 0x9E3779B9u * (t * 4u + draw + 1u);
    x ^= x >> 16; x *= 0x85EBCA6Bu; x ^= x >> 13; x *= 0xC2B2AE35u; x ^= x >> 16;      // (murmur3's finaliser)
    return x;
}

// Floyd's method: four distinct indices below n (n >= 4), in the order they were drawn
__device__ __forceinline__ void hg_sample(unsigned seed, int t, int n, int s[4]) {
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        const int j = n - 4 + d;
        int v = (int)(hg_hash(seed, (unsigned)t, (unsigned)d) % (unsigned)(j + 1));
        bool seen = false;
#pragma unroll
        for (int e = 0; e < d; ++e) seen = seen || s[e] == v;
        s[d] = seen ? j : v;
    }
}

// The image's slices, every offset clamped into its array, and the status the tables alone decide.  (uniform over the workgroup)
__device__ __forceinline__ HgImage hg_image(int p, const int* off1, const int* off2, const int* out_off, const int* count,
                                            int sumN1, int sumN2, int sum_out, int max_n1, int max_n2, int max_pairs) {
    HgImage I;
    const int a0 = min(max(off1[p], 0), sumN1), a1 = min(max(off1[p + 1], a0), sumN1);
    const int b0 = min(max(off2[p], 0), sumN2), b1 = min(max(off2[p + 1], b0), sumN2);
    const int r0 = min(max(out_off[p], 0), sum_out), r1 = min(max(out_off[p + 1], r0), sum_out);
    I.a0 = a0; I.n1 = a1 - a0; I.b0 = b0; I.n2 = b1 - b0; I.r0 = r0;
    const int m = count[p];
    I.status = CVPCE_HOMOGRAPHY_OK;
    if (m < 0 || m > r1 - r0 || m > max_pairs || I.n1 > max_n1 || I.n2 > max_n2) {
        I.status = CVPCE_HOMOGRAPHY_INVALID;
        I.m = 0;
    } else {
        I.m = m;
        if (m == 0) I.status = CVPCE_HOMOGRAPHY_NONE;
    }
    I.n = I.m == 1 ? 5 : 3 * I.m;
    return I;
}

// Range-checks the pairs, then writes the points to LDS: k = top-left corners, m + k = bottom-right corners, 2m + k = centres
// (fp32, as planograms._three_points forms them); m = 1 appends (x2, y1) and (x0, y3).  -> the image's status.  Contains
// barriers: call it from uniform control flow.
__device__ __forceinline__ int hg_points(const HgImage& I, const float4* boxes1, const float4* boxes2, const int* pairs,
                                         float* sx, float* sy, float* du, float* dv, int* s_flag) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x, m = I.m;
    if (tid == 0) *s_flag = 0;
    __syncthreads();
    if (I.status == CVPCE_HOMOGRAPHY_OK) {
        for (int k = tid; k < m; k += HG_THREADS) {
            const int e = pairs[(size_t)(I.r0 + k) * 2], a = pairs[(size_t)(I.r0 + k) * 2 + 1];
            if (e < 0 || e >= I.n1 || a < 0 || a >= I.n2) *s_flag = 1;      // (any writer: they all write 1)
        }
    }
    __syncthreads();
    int status = I.status;
    if (status == CVPCE_HOMOGRAPHY_OK && *s_flag) status = CVPCE_HOMOGRAPHY_INVALID;
    __syncthreads();
    if (status != CVPCE_HOMOGRAPHY_OK) return status;
    for (int k = tid; k < m; k += HG_THREADS) {
        const int e = pairs[(size_t)(I.r0 + k) * 2], a = pairs[(size_t)(I.r0 + k) * 2 + 1];
        const float4 p = boxes1[I.a0 + e], q = boxes2[I.b0 + a];
        const float fin = ((p.x - p.x) + (p.y - p.y)) + ((p.z - p.z) + (p.w - p.w)) + ((q.x - q.x) + (q.y - q.y)) + ((q.z - q.z) + (q.w - q.w));
        if (!(fin == 0.f)) *s_flag = 1;                                     // a non-finite coordinate: x - x is NaN
        sx[k] = p.x; sy[k] = p.y; du[k] = q.x; dv[k] = q.y;
        sx[m + k] = p.z; sy[m + k] = p.w; du[m + k] = q.z; dv[m + k] = q.w;
        sx[2 * m + k] = (p.x + p.z) / 2.f; sy[2 * m + k] = (p.y + p.w) / 2.f;
        du[2 * m + k] = (q.x + q.z) / 2.f; dv[2 * m + k] = (q.y + q.w) / 2.f;
        if (m == 1) {
            sx[3] = p.z; sy[3] = p.y; du[3] = q.z; dv[3] = q.y;
            sx[4] = p.x; sy[4] = p.w; du[4] = q.x; dv[4] = q.w;
        }
    }
    __syncthreads();
    if (*s_flag) status = CVPCE_HOMOGRAPHY_NONE;
    __syncthreads();
    return status;
}

// Hartley normalisation of the points px, py whose `mask` entry is set (mask = nullptr: all n): centroid c, mean distance s to it,
// k = sqrt(2) / s.  Sums: thread j adds its points j, j + 256, ... in that order, the 256 partial sums are then added in index
// order.  `part` is [3][256] doubles of LDS.  -> false if s < 1e-12 (or is no number).  Contains barriers.
__device__ __forceinline__ bool hg_normalise(const float* px, const float* py, const int* mask, int n, int count, double* part, HgNorm& N) {
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    double ax = 0.0, ay = 0.0;
    for (int k = tid; k < n; k += HG_THREADS) {
        if (mask && !mask[k]) continue;
        ax = ax + (double)px[k];
        ay = ay + (double)py[k];
    }
    part[tid] = ax;
    part[HG_THREADS + tid] = ay;
    __syncthreads();
    double tx = 0.0, ty = 0.0;
    for (int j = 0; j < HG_THREADS; ++j) {
        tx = tx + part[j];
        ty = ty + part[HG_THREADS + j];
    }
    const double cnt = (double)count;
    N.cx = tx / cnt;
    N.cy = ty / cnt;
    double ad = 0.0;
    for (int k = tid; k < n; k += HG_THREADS) {
        if (mask && !mask[k]) continue;
        const double dx = (double)px[k] - N.cx, dy = (double)py[k] - N.cy;
        ad = ad + sqrt(dx * dx + dy * dy);
    }
    part[2 * HG_THREADS + tid] = ad;
    __syncthreads();
    double td = 0.0;
    for (int j = 0; j < HG_THREADS; ++j) td = td + part[2 * HG_THREADS + j];
    const double s = td / cnt;
    N.k = HG_SQRT2 / s;
    __syncthreads();                                                         // (`part` may be reused at once)
    return s >= HG_DEGENERATE;
}

// H = T2^-1 * Hn * T1 for Hn between normalised points, divided by its last entry -> false if that entry is below 1e-12 in
// magnitude or some entry of the result is not finite.
__device__ __forceinline__ bool hg_denormalise(const double hn[9], const HgNorm& A, const HgNorm& B, double h[9]) {
#pragma clang fp contract(off)
    const double tx = A.k * A.cx, ty = A.k * A.cy;
    double M[9];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        M[3 * r] = hn[3 * r] * A.k;
        M[3 * r + 1] = hn[3 * r + 1] * A.k;
        M[3 * r + 2] = (hn[3 * r + 2] - hn[3 * r] * tx) - hn[3 * r + 1] * ty;
    }
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        h[j] = M[j] / B.k + B.cx * M[6 + j];
        h[3 + j] = M[3 + j] / B.k + B.cy * M[6 + j];
        h[6 + j] = M[6 + j];
    }
    const double d = h[8];
    if (!(fabs(d) >= HG_DEGENERATE)) return false;
    bool finite = true;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
        h[i] = h[i] / d;
        finite = finite && fabs(h[i]) <= DBL_MAX;
    }
    return finite;
}

// The homography through the four sampled correspondences: h'[2][2] = 1 between normalised points, the 8 x 8 system solved by
// Gaussian elimination.  Pivoting: at column c the rows c+1 .. 7 are compared with row c in turn and swapped into it where
// their entry is larger in magnitude (strictly), so row c ends up with the column's largest.  -> false: no model.
__device__ __forceinline__ bool hg_minimal(const int s[4], const float* sx, const float* sy, const float* du, const float* dv,
                                           const HgNorm& A, const HgNorm& B, double h[9]) {
#pragma clang fp contract(off)
    double a[8][9];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const double x = ((double)sx[s[i]] - A.cx) * A.k, y = ((double)sy[s[i]] - A.cy) * A.k;
        const double u = ((double)du[s[i]] - B.cx) * B.k, v = ((double)dv[s[i]] - B.cy) * B.k;
        a[2 * i][0] = x; a[2 * i][1] = y; a[2 * i][2] = 1.0; a[2 * i][3] = 0.0; a[2 * i][4] = 0.0; a[2 * i][5] = 0.0;
        a[2 * i][6] = -(u * x); a[2 * i][7] = -(u * y); a[2 * i][8] = u;
        a[2 * i + 1][0] = 0.0; a[2 * i + 1][1] = 0.0; a[2 * i + 1][2] = 0.0; a[2 * i + 1][3] = x; a[2 * i + 1][4] = y; a[2 * i + 1][5] = 1.0;
        a[2 * i + 1][6] = -(v * x); a[2 * i + 1][7] = -(v * y); a[2 * i + 1][8] = v;
    }
    bool ok = true;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const bool sw = fabs(a[r][c]) > fabs(a[c][c]);
#pragma unroll
            for (int j = c; j < 9; ++j) {
                const double top = a[c][j], low = a[r][j];
                a[c][j] = sw ? low : top;
                a[r][j] = sw ? top : low;
            }
        }
        ok = ok && fabs(a[c][c]) >= HG_PIVOT_MIN;
#pragma unroll
        for (int r = c + 1; r < 8; ++r) {
            const double f = a[r][c] / a[c][c];
#pragma unroll
            for (int j = c + 1; j < 9; ++j) a[r][j] = a[r][j] - f * a[c][j];
        }
    }
    double hn[9];
#pragma unroll
    for (int i = 7; i >= 0; --i) {
        double acc = a[i][8];
#pragma unroll
        for (int j = i + 1; j < 8; ++j) acc = acc - a[i][j] * hn[j];
        hn[i] = acc / a[i][i];
    }
    hn[8] = 1.0;
    return hg_denormalise(hn, A, B, h) && ok;
}

// reprojection error of point k under h, in pixels
__device__ __forceinline__ double hg_error(const double h[9], float fx, float fy, float fu, float fv) {
#pragma clang fp contract(off)
    const double x = (double)fx, y = (double)fy;
    const double px = (h[0] * x + h[1] * y) + h[2], py = (h[3] * x + h[4] * y) + h[5], pw = (h[6] * x + h[7] * y) + h[8];
    const double ex = px / pw - (double)fu, ey = py / pw - (double)fv;
    return sqrt(ex * ex + ey * ey);
}

static inline size_t hg_points_lds(int max_pairs) { return (size_t)(max_pairs == 1 ? 5 : 3 * max_pairs) * 4 * sizeof(float); }

__global__ __launch_bounds__(HG_THREADS) void homography_ransac_kernel(
    const float4* __restrict__ boxes1, const int* __restrict__ off1, const float4* __restrict__ boxes2, const int* __restrict__ off2,
    const int* __restrict__ pairs, const int* __restrict__ count, const int* __restrict__ out_off, const double* __restrict__ params,
    int sumN1, int sumN2, int sum_out, int max_pairs, unsigned seed, int K, int2* __restrict__ slots) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_part[3 * HG_THREADS];
    __shared__ int s_flag, s_best;
    const int chunk = blockIdx.x, p = blockIdx.y, tid = threadIdx.x;
    const int cap = max_pairs == 1 ? 5 : 3 * max_pairs;
    float* sx = (float*)smem;
    float* sy = sx + cap;
    float* du = sy + cap;
    float* dv = du + cap;
    const HgImage I = hg_image(p, off1, off2, out_off, count, sumN1, sumN2, sum_out, HG_MAX_NODES, HG_MAX_NODES, max_pairs);
    int status = hg_points(I, boxes1, boxes2, pairs, sx, sy, du, dv, &s_flag);
    const int n = I.n;
    if (status == CVPCE_HOMOGRAPHY_OK && n < 4) status = CVPCE_HOMOGRAPHY_NONE;
    int2* slot = slots + (size_t)p * gridDim.x + chunk;
    if (status != CVPCE_HOMOGRAPHY_OK) {                                       // (uniform)
        if (tid == 0) *slot = make_int2(0, chunk * HG_THREADS);
        return;
    }
    HgNorm A, B;
    const bool okA = hg_normalise(sx, sy, nullptr, n, n, s_part, A);
    const bool okB = hg_normalise(du, dv, nullptr, n, n, s_part, B);
    if (tid == 0) s_best = -1;
    __syncthreads();
    const int t = chunk * HG_THREADS + tid;
    if (t < K) {
        int cnt = 0;
        if (okA && okB) {
            int s[4];
            double h[9];
            hg_sample(seed, t, n, s);
            if (hg_minimal(s, sx, sy, du, dv, A, B, h)) {
                const double thr = params[2 * p];
                for (int k = 0; k < n; ++k) cnt += hg_error(h, sx[k], sy[k], du[k], dv[k]) < thr ? 1 : 0;
            }
        }
        atomicMax(&s_best, cnt * 256 + (HG_THREADS - 1 - tid));                // highest count, then lowest hypothesis: any order
    }
    __syncthreads();
    if (tid == 0) {
        const int best = s_best;                                              // (t = chunk * 256 < K: thread 0 always took part)
        *slot = make_int2(best >> 8, chunk * HG_THREADS + (HG_THREADS - 1 - (best & 255)));
    }
}

// entry i of the two DLT rows of a normalised correspondence
__device__ __forceinline__ double hg_pick(const double r[9], int i) {
    return i == 0 ? r[0] : i == 1 ? r[1] : i == 2 ? r[2] : i == 3 ? r[3] : i == 4 ? r[4] : i == 5 ? r[5] : i == 6 ? r[6] : i == 7 ? r[7] : r[8];
}

#include "iou.h"                              // hg_iou: the claim's IoU, shared with report.hip

struct HgFinishLds { int pos, lab1, me, mask, total; };

__host__ __device__ static inline HgFinishLds hg_finish_lds(int max_n1, int max_pairs) {
    const int cap = max_pairs == 1 ? 5 : 3 * max_pairs;
    HgFinishLds L;
    int o = 4 * cap * 4;                                                      // the four point arrays come first
    o = (o + 15) & ~15;
    L.pos = o; o += 16 * max_n1;
    L.lab1 = o; o += 4 * max_n1;
    L.me = o; o += 4 * max_n1;
    L.mask = o; o += 4 * cap;
    L.total = o;
    return L;
}

__global__ __launch_bounds__(HG_THREADS) void homography_finish_kernel(
    const float4* __restrict__ boxes1, const int* __restrict__ label1, const int* __restrict__ off1,
    const float4* __restrict__ boxes2, const int* __restrict__ label2, const int* __restrict__ off2,
    const int* __restrict__ pairs, const int* __restrict__ count, const int* __restrict__ out_off, const double* __restrict__ params,
    int sumN1, int sumN2, int sum_out, int max_n1, int max_n2, int max_pairs, unsigned seed, int K, int chunks,
    const int2* __restrict__ slots, int* __restrict__ g_status, double* __restrict__ g_H, int* __restrict__ g_winner,
    int* __restrict__ g_wcount, int* __restrict__ g_fcount, int* __restrict__ g_me, int* __restrict__ g_ma, float4* __restrict__ g_pos) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    __shared__ double s_part[3 * HG_THREADS];
    __shared__ double s_A[81], s_V[81], s_H[9];
    __shared__ int s_flag, s_best, s_count, s_ok;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1);
    const int cap = max_pairs == 1 ? 5 : 3 * max_pairs;
    const HgFinishLds L = hg_finish_lds(max_n1, max_pairs);
    float* sx = (float*)smem;
    float* sy = sx + cap;
    float* du = sy + cap;
    float* dv = du + cap;
    float4* pos = (float4*)(smem + L.pos);
    int* lab1 = (int*)(smem + L.lab1);
    int* me = (int*)(smem + L.me);
    int* mask = (int*)(smem + L.mask);

    const HgImage I = hg_image(p, off1, off2, out_off, count, sumN1, sumN2, sum_out, max_n1, max_n2, max_pairs);
    int status = hg_points(I, boxes1, boxes2, pairs, sx, sy, du, dv, &s_flag);
    const int n = I.n, n1 = I.n1, n2 = I.n2;
    if (status == CVPCE_HOMOGRAPHY_OK && n < 4) status = CVPCE_HOMOGRAPHY_NONE;

    // a non-finite coordinate anywhere in the image's two box sets: no homography
    if (tid == 0) {
        s_flag = 0;
        s_best = -1;
        s_count = 0;
        s_ok = 0;
    }
    __syncthreads();
    if (status == CVPCE_HOMOGRAPHY_OK) {
        for (int i = tid; i < n1 + n2; i += HG_THREADS) {
            const float4 b = i < n1 ? boxes1[I.a0 + i] : boxes2[I.b0 + (i - n1)];
            if (!(((b.x - b.x) + (b.y - b.y)) + ((b.z - b.z) + (b.w - b.w)) == 0.f)) s_flag = 1;
        }
        // the winner: highest count, lowest hypothesis at equal counts (slot contents are device data: clamped)
        for (int c = tid; c < chunks; c += HG_THREADS) {
            const int2 s = slots[(size_t)p * chunks + c];
            const int cnt = min(max(s.x, 0), n), t = min(max(s.y, 0), K - 1);
            atomicMax(&s_best, cnt * 65536 + (65535 - t));
        }
    }
    __syncthreads();
    if (status == CVPCE_HOMOGRAPHY_OK && s_flag) status = CVPCE_HOMOGRAPHY_NONE;
    const int winner = status == CVPCE_HOMOGRAPHY_OK ? 65535 - (s_best & 65535) : 0;
    __syncthreads();

    double h[9];
    int wcount = 0, fcount = 0;
    if (status == CVPCE_HOMOGRAPHY_OK) {                                       // (uniform from here on: status is)
        HgNorm A, B;
        const bool okA = hg_normalise(sx, sy, nullptr, n, n, s_part, A);
        const bool okB = hg_normalise(du, dv, nullptr, n, n, s_part, B);
        int s[4];
        hg_sample(seed, winner, n, s);
        bool ok = okA && okB;
        ok = hg_minimal(s, sx, sy, du, dv, A, B, h) && ok;
        const double thr = params[2 * p];
        int mine = 0;
        for (int k = tid; k < n; k += HG_THREADS) {
            const int in = ok && hg_error(h, sx[k], sy[k], du[k], dv[k]) < thr ? 1 : 0;
            mask[k] = in;
            mine += in;
        }
        atomicAdd(&s_count, mine);
        __syncthreads();
        wcount = s_count;
        __syncthreads();
        if (wcount < 4) status = CVPCE_HOMOGRAPHY_NONE;
    }
    if (status == CVPCE_HOMOGRAPHY_OK) {
        // refit over the winner's inliers, normalised over the inliers
        HgNorm A, B;
        const bool okA = hg_normalise(sx, sy, mask, n, wcount, s_part, A);
        const bool okB = hg_normalise(du, dv, mask, n, wcount, s_part, B);
        if (tid < 45) {
            int i = 0, j = tid;
            for (int row = 0; row < 8; ++row) {                               // entry tid of the upper triangle, row by row
                if (j >= 9 - i) {
                    j -= 9 - i;
                    ++i;
                }
            }
            j += i;
            double acc = 0.0;
            for (int k = 0; k < n; ++k) {
                if (!mask[k]) continue;
                const double x = ((double)sx[k] - A.cx) * A.k, y = ((double)sy[k] - A.cy) * A.k;
                const double u = ((double)du[k] - B.cx) * B.k, v = ((double)dv[k] - B.cy) * B.k;
                const double r1[9] = {-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u};
                const double r2[9] = {0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v};
                acc = acc + (hg_pick(r1, i) * hg_pick(r1, j) + hg_pick(r2, i) * hg_pick(r2, j));
            }
            s_A[i * 9 + j] = acc;
            s_A[j * 9 + i] = acc;
        }
        for (int e = tid; e < 81; e += HG_THREADS) s_V[e] = e / 9 == e % 9 ? 1.0 : 0.0;
        __syncthreads();
        if (tid < WAVE) {
            // cyclic Jacobi: rotation (p, q) zeroes a_pq; lane r < 9 owns row r of the matrix and of the vectors
            volatile double* Am = s_A;
            volatile double* Vm = s_V;
            for (int sweep = 0; sweep < HG_SWEEPS; ++sweep) {
                for (int pp = 0; pp < 8; ++pp) {
                    for (int q = pp + 1; q < 9; ++q) {
                        const double apq = Am[pp * 9 + q];
                        if (apq == 0.0) continue;                             // (uniform: every lane read the same entry)
                        const double app = Am[pp * 9 + pp], aqq = Am[q * 9 + q];
                        const double theta = (aqq - app) / (2.0 * apq), at = fabs(theta);
                        double t = at > HG_THETA_MAX ? 0.5 / at : 1.0 / (at + sqrt(at * at + 1.0));
                        t = theta < 0.0 ? -t : t;
                        const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                        double arp = 0.0, arq = 0.0, vrp = 0.0, vrq = 0.0;
                        if (lane < 9) {
                            arp = Am[lane * 9 + pp];
                            arq = Am[lane * 9 + q];
                            vrp = Vm[lane * 9 + pp];
                            vrq = Vm[lane * 9 + q];
                        }
                        __builtin_amdgcn_wave_barrier();
                        if (lane < 9) {
                            Vm[lane * 9 + pp] = c * vrp - sn * vrq;
                            Vm[lane * 9 + q] = sn * vrp + c * vrq;
                            if (lane != pp && lane != q) {
                                const double np = c * arp - sn * arq, nq = sn * arp + c * arq;
                                Am[lane * 9 + pp] = np;
                                Am[pp * 9 + lane] = np;
                                Am[lane * 9 + q] = nq;
                                Am[q * 9 + lane] = nq;
                            }
                        }
                        if (lane == 0) {
                            Am[pp * 9 + pp] = app - t * apq;
                            Am[q * 9 + q] = aqq + t * apq;
                            Am[pp * 9 + q] = 0.0;
                            Am[q * 9 + pp] = 0.0;
                        }
                        __builtin_amdgcn_wave_barrier();
                    }
                }
            }
            int imin = 0;
            double least = Am[0];
            for (int i = 1; i < 9; ++i) {
                const double d = Am[i * 9 + i];
                if (d < least) {
                    least = d;
                    imin = i;
                }
            }
            double hn[9], hr[9];
#pragma unroll
            for (int i = 0; i < 9; ++i) hn[i] = Vm[i * 9 + imin];
            const bool ok = hg_denormalise(hn, A, B, hr) && okA && okB;
            if (lane == 0) {
#pragma unroll
                for (int i = 0; i < 9; ++i) s_H[i] = hr[i];
                s_ok = ok ? 1 : 0;
            }
        }
        __syncthreads();
        if (!s_ok) status = CVPCE_HOMOGRAPHY_NONE;
    }
    if (tid == 0) s_count = 0;
    for (int i = tid; i < n1 && i < max_n1; i += HG_THREADS) me[i] = 0;
    __syncthreads();
    if (status == CVPCE_HOMOGRAPHY_OK) {
#pragma unroll
        for (int i = 0; i < 9; ++i) h[i] = s_H[i];
        const double thr = params[2 * p], iou_thr = params[2 * p + 1];
        int mine = 0;
        for (int k = tid; k < n; k += HG_THREADS) mine += hg_error(h, sx[k], sy[k], du[k], dv[k]) < thr ? 1 : 0;
        atomicAdd(&s_count, mine);
        // projection: H rounded to fp32, every corner in fp32
        float f[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) f[i] = (float)h[i];
        for (int i = tid; i < n1; i += HG_THREADS) {
            const float4 b = boxes1[I.a0 + i];
            const float w0 = (f[6] * b.x + f[7] * b.y) + f[8], w1 = (f[6] * b.z + f[7] * b.w) + f[8];
            float4 r;
            r.x = __fdiv_rn((f[0] * b.x + f[1] * b.y) + f[2], w0);
            r.y = __fdiv_rn((f[3] * b.x + f[4] * b.y) + f[5], w0);
            r.z = __fdiv_rn((f[0] * b.z + f[1] * b.w) + f[2], w1);
            r.w = __fdiv_rn((f[3] * b.z + f[4] * b.w) + f[5], w1);
            pos[i] = r;
            g_pos[I.a0 + i] = r;
            lab1[i] = label1[I.a0 + i];
        }
        __syncthreads();
        fcount = s_count;
        // claim: detection j is taken by the lowest expected box of its label at IoU >= threshold
        for (int j = tid; j < n2; j += HG_THREADS) {
            const float4 b = boxes2[I.b0 + j];
            const int lb = label2[I.b0 + j];
            int by = -1;
            for (int i = 0; i < n1; ++i) {
                if (lab1[i] == lb && (double)hg_iou(pos[i], b) >= iou_thr) {
                    by = i;
                    break;
                }
            }
            if (by >= 0) me[by] = 1;                                          // (any writer: they all write 1)
            g_ma[I.b0 + j] = by >= 0 ? 1 : 0;
        }
        __syncthreads();
        for (int i = tid; i < n1; i += HG_THREADS) g_me[I.a0 + i] = me[i];
    } else {
        for (int i = tid; i < n1; i += HG_THREADS) {
            g_me[I.a0 + i] = 0;
            g_pos[I.a0 + i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        for (int j = tid; j < n2; j += HG_THREADS) g_ma[I.b0 + j] = 0;
    }
    if (tid < 9) g_H[(size_t)p * 9 + tid] = status == CVPCE_HOMOGRAPHY_OK ? s_H[tid] : 0.0;
    if (tid == 0) {
        const bool ok = status == CVPCE_HOMOGRAPHY_OK;
        g_status[p] = status;
        g_winner[p] = ok ? winner : 0;
        g_wcount[p] = ok ? wcount : 0;
        g_fcount[p] = ok ? fcount : 0;
    }
}

static inline int hg_chunks(int hypotheses) { return (hypotheses + HG_THREADS - 1) / HG_THREADS; }

extern "C" size_t cvpce_homography_workspace_bytes(int B, int hypotheses) {
    if (B < 0 || hypotheses < 1 || hypotheses > CVPCE_HOMOGRAPHY_MAX_HYPOTHESES) return 0;
    return (size_t)B * hg_chunks(hypotheses) * sizeof(int2);
}

static bool hg_common_ok(const float* boxes1, const int* off1, const float* boxes2, const int* off2, const int* pairs, const int* count,
                         const int* out_off, const double* params, int B, int sumN1, int sumN2, int sum_out, int max_pairs, int hypotheses,
                         const void* workspace, size_t workspace_bytes) {
    if (B < 0 || B > 65535 || sumN1 < 0 || sumN2 < 0 || sum_out < 0) return false;
    if (hypotheses < 1 || hypotheses > CVPCE_HOMOGRAPHY_MAX_HYPOTHESES || max_pairs < 1 || max_pairs > HG_MAX_PAIRS) return false;
    if (B == 0) return true;
    if (!off1 || !off2 || !count || !out_off || !params) return false;
    if ((sumN1 > 0 && !boxes1) || (sumN2 > 0 && !boxes2) || (sum_out > 0 && !pairs)) return false;
    if (((uintptr_t)boxes1 & 15) || ((uintptr_t)boxes2 & 15) || ((uintptr_t)params & 7)) return false;
    if (!workspace || ((uintptr_t)workspace & 7) || workspace_bytes < cvpce_homography_workspace_bytes(B, hypotheses)) return false;
    return true;
}

extern "C" int cvpce_homography_ransac(const float* boxes1, const int* off1, const float* boxes2, const int* off2,
                                       const int* pairs, const int* count, const int* out_off, const double* params,
                                       int B, int sumN1, int sumN2, int sum_out, int max_pairs, unsigned seed, int hypotheses,
                                       void* workspace, size_t workspace_bytes, void* stream) {
    if (!hg_common_ok(boxes1, off1, boxes2, off2, pairs, count, out_off, params, B, sumN1, sumN2, sum_out, max_pairs, hypotheses,
                      workspace, workspace_bytes)) return CVPCE_ERR_ARG;
    if (B == 0) return CVPCE_OK;
    if (!cvpce_smem_attr_done<homography_ransac_kernel>((const void*)homography_ransac_kernel, (int)hg_points_lds(HG_MAX_PAIRS))) return CVPCE_ERR_LAUNCH;
    hipLaunchKernelGGL(homography_ransac_kernel, dim3((unsigned)hg_chunks(hypotheses), (unsigned)B), dim3(HG_THREADS), hg_points_lds(max_pairs),
                       (hipStream_t)stream, (const float4*)boxes1, off1, (const float4*)boxes2, off2, pairs, count, out_off, params,
                       sumN1, sumN2, sum_out, max_pairs, seed, hypotheses, (int2*)workspace);
    return cvpce_check_launch();
}

extern "C" int cvpce_homography_finish(const float* boxes1, const int* label1, const int* off1, const float* boxes2, const int* label2, const int* off2,
                                       const int* pairs, const int* count, const int* out_off, const double* params,
                                       int B, int sumN1, int sumN2, int sum_out, int max_n1, int max_n2, int max_pairs, unsigned seed, int hypotheses,
                                       const void* workspace, size_t workspace_bytes,
                                       int* status, double* H, int* winner, int* winner_count, int* final_count,
                                       int* matched_expected, int* matched_actual, float* expected_positions, void* stream) {
    if (!hg_common_ok(boxes1, off1, boxes2, off2, pairs, count, out_off, params, B, sumN1, sumN2, sum_out, max_pairs, hypotheses,
                      workspace, workspace_bytes)) return CVPCE_ERR_ARG;
    if (max_n1 < 1 || max_n1 > HG_MAX_NODES || max_n2 < 1 || max_n2 > HG_MAX_NODES) return CVPCE_ERR_ARG;
    if (B == 0) return CVPCE_OK;
    if (!status || !H || !winner || !winner_count || !final_count || ((uintptr_t)H & 7)) return CVPCE_ERR_ARG;
    if ((sumN1 > 0 && (!label1 || !matched_expected || !expected_positions)) || (sumN2 > 0 && (!label2 || !matched_actual))) return CVPCE_ERR_ARG;
    if ((uintptr_t)expected_positions & 15) return CVPCE_ERR_ARG;
    if (!cvpce_smem_attr_done<homography_finish_kernel>((const void*)homography_finish_kernel, hg_finish_lds(HG_MAX_NODES, HG_MAX_PAIRS).total)) return CVPCE_ERR_LAUNCH;
    hipLaunchKernelGGL(homography_finish_kernel, dim3((unsigned)B), dim3(HG_THREADS), (size_t)hg_finish_lds(max_n1, max_pairs).total,
                       (hipStream_t)stream, (const float4*)boxes1, label1, off1, (const float4*)boxes2, label2, off2, pairs, count, out_off, params,
                       sumN1, sumN2, sum_out, max_n1, max_n2, max_pairs, seed, hypotheses, hg_chunks(hypotheses), (const int2*)workspace,
                       status, H, winner, winner_count, final_count, matched_expected, matched_actual, (float4*)expected_positions);
    return cvpce_check_launch();
}
