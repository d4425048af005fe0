// Scoring the detector's Gaussian maps (include/cvpce_amd_gaussians.h): the target tensor of a batch rendered from
// the ground-truth boxes and resized in one launch, and the reference's loss by a radix select instead of a sort.
//
//   gauss_kant_table_kernel   the kant method's size x size table
//   gauss_targets_kernel      one workgroup per 16 x 16 output tile of one image.  The image's boxes are visited in chunks of 256: a
//                             thread reduces and clips one box and tests it against the tile's source rectangle, an ORDERED compaction
//                             (wave ballot + wave offsets: a prefix sum, no atomic append) packs the hits into the LDS list in index
//                             order, then every thread joins the list's boxes, in that order, to its source taps -- four with the
//                             resize (two per axis), one without.  `join_box` is the one function that renders a box into a source
//                             pixel in both modes, so the fused output has the bits of render-then-resize by this kernel.
//   gauss_loss_*              pass 0 takes the positive sums, the counts and the histogram of the top 8 bits of the negatives' squared
//                             errors; passes 1-3 histogram the next 8 bits below the prefix found so far (every workgroup re-derives
//                             it from the earlier histograms: 256 bins, one LDS scan each); `tail` sums the errors above the
//                             threshold tau; `finish` adds the workgroups' partial sums in index order.  Histograms and counts are
//                             integers (vector atomics: order cannot change them); float sums never meet an atomic.
//
// Compiled with -ffp-contract=off: every fp32 operation below is rounded on its own, expf is the only library call.
#include "common.h"
#include "../../include/cvpce_amd_gaussians.h"

#define GT CVPCE_GAUSS_TILE
#define GL CVPCE_GAUSS_LIST
#define GT_THREADS (GT * GT)
#define LT CVPCE_GAUSS_LOSS_THREADS
#define LI CVPCE_GAUSS_LOSS_ITEMS
#define L_SPAN (LT * LI)

static_assert(GT_THREADS == GL, "one box per thread and chunk");

__global__ __launch_bounds__(256) void gauss_kant_table_kernel(float* __restrict__ out, int size, int sigma) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= size * size) return;
    const int i = idx / size - size / 2, j = idx % size - size / 2;
    const float c = -4.f * 0.6931472f;
    out[idx] = expf((c * (float)(i * i + j * j)) / (float)(sigma * sigma));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// targets
// ---------------------------------------------------------------------------------------------------------------------------------
struct GaussBox {          // a reduced, clipped box and the constants of its generate method
    int xlo, xhi, ylo, yhi;
    float p[6];
};

__device__ __forceinline__ int floor_div(int a, int r) {
    const int q = a / r;
    return (a % r != 0 && a < 0) ? q - 1 : q;
}

// smallest squared distance of the integers [lo, hi) to c
__device__ __forceinline__ float min_dist2(float c, int lo, int hi) {
    const float f = floorf(c);
    const float a = fminf(fmaxf(f, (float)lo), (float)(hi - 1)), b = fminf(fmaxf(f + 1.f, (float)lo), (float)(hi - 1));
    const float da = a - c, db = b - c;
    return fminf(da * da, db * db);
}

// one axis of F.interpolate(mode='bilinear', align_corners=False): the two taps of output index `dst` and their weights
__device__ __forceinline__ void bilinear_taps(int dst, float scale, int in_size, int& i0, int& i1, float& l0, float& l1) {
    float src = scale * ((float)dst + 0.5f) - 0.5f;
    if (src < 0.f) src = 0.f;
    i0 = min((int)src, in_size - 1);
    i1 = i0 + (i0 < in_size - 1 ? 1 : 0);
    l1 = src - (float)i0;
    l0 = 1.f - l1;
}

// Reduces box (x1, y1, x2, y2) by r, clips it to the (hs, ws) map and prepares its method's constants; false: it contributes nothing.
__device__ __forceinline__ bool prepare_box(int bx1, int by1, int bx2, int by2, int r, int hs, int ws, int method, float a, float b, float c,
                                            int table_size, GaussBox& g) {
    const int x1 = floor_div(bx1, r), y1 = floor_div(by1, r), x2 = floor_div(bx2, r), y2 = floor_div(by2, r);
    g.xlo = max(x1, 0); g.xhi = min(x2, ws); g.ylo = max(y1, 0); g.yhi = min(y2, hs);
    if (x1 == x2 || y1 == y2 || g.xlo >= g.xhi || g.ylo >= g.yhi) return false;
    const float cx = (float)(x1 + x2) * 0.5f, cy = (float)(y1 + y2) * 0.5f;
    const float wd = (float)abs(x2 - x1), ht = (float)abs(y2 - y1);
    if (method == CVPCE_GAUSS_MULTIVARIATE_NORMAL) {          // a = peak, b = variance_scale
        const float sw = wd * b, sh = ht * b;
        g.p[0] = cx; g.p[1] = cy; g.p[2] = sw * sw; g.p[3] = sh * sh;
        g.p[4] = min_dist2(cx, g.xlo, g.xhi); g.p[5] = min_dist2(cy, g.ylo, g.yhi);
    } else if (method == CVPCE_GAUSS_SIMPLE_AND_SCALED) {     // a = minimum, b = maximum, c = sigma_divisor
        const float sx = wd / c, sy = ht / c;
        g.p[0] = cx; g.p[1] = cy; g.p[2] = 2.f * (sx * sx); g.p[3] = 2.f * (sy * sy);
        g.p[4] = 0.f; g.p[5] = 0.f;
    } else {                                                  // kant: the table resampled to the clipped box
        g.p[0] = (float)table_size / (float)(g.xhi - g.xlo); g.p[1] = (float)table_size / (float)(g.yhi - g.ylo);
        g.p[2] = g.p[3] = g.p[4] = g.p[5] = 0.f;
    }
    return true;
}

// Joins box g to the source pixel (sx, sy) whose value so far is v.  THE rendering rule of a source pixel, in both modes.
__device__ __forceinline__ void join_box(float& v, int sx, int sy, int xlo, int xhi, int ylo, int yhi, float p0, float p1, float p2, float p3,
                                         float p4, float p5, int method, int join, float a, float b, const float* __restrict__ table,
                                         int table_size) {
    if (sx < xlo || sx >= xhi || sy < ylo || sy >= yhi) return;
    float val;
    if (method == CVPCE_GAUSS_MULTIVARIATE_NORMAL) {
        const float dx = (float)sx - p0, dy = (float)sy - p1;
        const float ex = (dx * dx - p4) / p2, ey = (dy * dy - p5) / p3;
        val = a * expf(-0.5f * (ey + ex));
    } else if (method == CVPCE_GAUSS_SIMPLE_AND_SCALED) {
        const float dx = (float)sx - p0, dy = (float)sy - p1;
        const float ex = (dx * dx) / p2, ey = (dy * dy) / p3;
        val = (b - a) * expf(-(ex + ey)) + a;
    } else {
        int i0, i1, j0, j1;
        float li0, li1, lj0, lj1;
        bilinear_taps(sx - xlo, p0, table_size, i0, i1, li0, li1);         // x runs along the table's first axis (datautils.py:53)
        bilinear_taps(sy - ylo, p1, table_size, j0, j1, lj0, lj1);
        const float* r0 = table + (size_t)i0 * table_size;
        const float* r1 = table + (size_t)i1 * table_size;
        val = li0 * (lj0 * r0[j0] + lj1 * r0[j1]) + li1 * (lj0 * r1[j0] + lj1 * r1[j1]);
    }
    if (join == CVPCE_GAUSS_JOIN_MAX) v = fmaxf(v, val);
    else if (join == CVPCE_GAUSS_JOIN_ADDITION) v = v + val;
    else v = val;
}

__global__ __launch_bounds__(GT_THREADS) void gauss_targets_kernel(
    const int* __restrict__ boxes, const int* __restrict__ box_offsets, const long long* __restrict__ map_ptrs,
    const int* __restrict__ geom, const float* __restrict__ table, int table_size, int sumB, int Hb, int Wb, int method, int join,
    float pa, float pb, float pc, float background, int resize, float* __restrict__ out) {
    __shared__ int s_rect[4][GL];
    __shared__ float s_p[6][GL];
    __shared__ int s_wave[GT_THREADS / WAVE];

    const int tid = threadIdx.x, n = blockIdx.z;
    const int x = blockIdx.x * GT + (tid & (GT - 1)), y = blockIdx.y * GT + tid / GT;
    const int* gm = geom + (size_t)n * CVPCE_GAUSS_GEOM;
    const int r = max(gm[2], 1);
    const int hs = max(gm[0], 0) / r, ws = max(gm[1], 0) / r;
    int h = min(max(gm[3], 0), Hb), w = min(max(gm[4], 0), Wb);
    if (!resize) { h = min(h, hs); w = min(w, ws); }
    const bool in_tensor = y < Hb && x < Wb;
    float* dst = out + ((size_t)n * Hb + (in_tensor ? y : 0)) * Wb + (in_tensor ? x : 0);
    // (uniform per workgroup: a tile with no pixel inside the extent, or an image without a source pixel, is background)
    if ((int)blockIdx.y * GT >= h || (int)blockIdx.x * GT >= w || hs < 1 || ws < 1) {
        if (in_tensor) *dst = background;
        return;
    }
    const bool inside = y < h && x < w;
    // this thread's taps (x0, x1) x (y0, y1); a thread outside the extent gets taps no box covers
    int x0 = -1, x1 = -1, y0 = -1, y1 = -1;
    float lx0 = 1.f, lx1 = 0.f, ly0 = 1.f, ly1 = 0.f;
    // the tile's source rectangle [rx0, rx1] x [ry0, ry1]
    int rx0, rx1, ry0, ry1;
    const int tx_last = min((int)blockIdx.x * GT + GT - 1, w - 1), ty_last = min((int)blockIdx.y * GT + GT - 1, h - 1);
    if (resize) {
        const float scale_x = (float)ws / (float)w, scale_y = (float)hs / (float)h;
        if (inside) {
            bilinear_taps(x, scale_x, ws, x0, x1, lx0, lx1);
            bilinear_taps(y, scale_y, hs, y0, y1, ly0, ly1);
        }
        int t;
        float f0, f1;
        bilinear_taps((int)blockIdx.x * GT, scale_x, ws, rx0, t, f0, f1);
        bilinear_taps(tx_last, scale_x, ws, t, rx1, f0, f1);
        bilinear_taps((int)blockIdx.y * GT, scale_y, hs, ry0, t, f0, f1);
        bilinear_taps(ty_last, scale_y, hs, t, ry1, f0, f1);
    } else {
        if (inside) { x0 = x1 = x; y0 = y1 = y; }
        rx0 = blockIdx.x * GT; rx1 = tx_last; ry0 = blockIdx.y * GT; ry1 = ty_last;
    }
    float v00 = background, v01 = background, v10 = background, v11 = background;   // v[y tap][x tap]
    if (map_ptrs) {
        if (inside) {
            const float* src = (const float*)(uintptr_t)map_ptrs[n];
            v00 = src[(size_t)y0 * ws + x0];
            if (resize) {
                v01 = src[(size_t)y0 * ws + x1];
                v10 = src[(size_t)y1 * ws + x0];
                v11 = src[(size_t)y1 * ws + x1];
            }
        }
    } else {
        const int b0 = min(max(box_offsets[n], 0), sumB), b1 = min(max(box_offsets[n + 1], b0), sumB);
        const int lane = tid & (WAVE - 1), wave = tid / WAVE;
        for (int base = b0; base < b1; base += GL) {                               // (b0, b1 are uniform: so are the barriers)
            const int b = base + tid;
            GaussBox g;
            bool hit = false;
            if (b < b1) {
                const int* bx = boxes + (size_t)b * 4;
                hit = prepare_box(bx[0], bx[1], bx[2], bx[3], r, hs, ws, method, pa, pb, pc, table_size, g)
                      && g.xlo <= rx1 && g.xhi > rx0 && g.ylo <= ry1 && g.yhi > ry0;
            }
            const unsigned long long ballot = __ballot(hit);
            if (lane == 0) s_wave[wave] = __popcll(ballot);
            __syncthreads();
            int at = __popcll(ballot & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
            for (int i = 0; i < GT_THREADS / WAVE; ++i) {
                if (i < wave) at += s_wave[i];
                total += s_wave[i];
            }
            if (hit) {                                                             // at < total <= GL: index order kept
                s_rect[0][at] = g.xlo; s_rect[1][at] = g.xhi; s_rect[2][at] = g.ylo; s_rect[3][at] = g.yhi;
#pragma unroll
                for (int i = 0; i < 6; ++i) s_p[i][at] = g.p[i];
            }
            __syncthreads();
            for (int i = 0; i < total; ++i) {
                const int xlo = s_rect[0][i], xhi = s_rect[1][i], ylo = s_rect[2][i], yhi = s_rect[3][i];
                const float p0 = s_p[0][i], p1 = s_p[1][i], p2 = s_p[2][i], p3 = s_p[3][i], p4 = s_p[4][i], p5 = s_p[5][i];
                join_box(v00, x0, y0, xlo, xhi, ylo, yhi, p0, p1, p2, p3, p4, p5, method, join, pa, pb, table, table_size);
                if (resize) {
                    join_box(v01, x1, y0, xlo, xhi, ylo, yhi, p0, p1, p2, p3, p4, p5, method, join, pa, pb, table, table_size);
                    join_box(v10, x0, y1, xlo, xhi, ylo, yhi, p0, p1, p2, p3, p4, p5, method, join, pa, pb, table, table_size);
                    join_box(v11, x1, y1, xlo, xhi, ylo, yhi, p0, p1, p2, p3, p4, p5, method, join, pa, pb, table, table_size);
                }
            }
            __syncthreads();                                                       // the list is rewritten by the next chunk
        }
    }
    if (!in_tensor) return;
    if (!inside) *dst = background;
    else if (!resize) *dst = v00;
    else *dst = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
}

extern "C" int cvpce_gauss_kant_table(float* out, int size, int sigma, void* stream) {
    if (!out || size < 1 || size > 4096 || sigma < 1 || sigma > 32768) return CVPCE_ERR_ARG;
    hipLaunchKernelGGL(gauss_kant_table_kernel, dim3((size * size + 255) / 256), dim3(256), 0, (hipStream_t)stream, out, size, sigma);
    return cvpce_check_launch();
}

extern "C" int cvpce_gauss_targets(const int* boxes, const int* box_offsets, const long long* map_ptrs, const int* geom, const float* table,
                                   int table_size, int sumB, int N, int Hb, int Wb, int method, int join, const float* params, int tanh,
                                   int resize, float* out, void* stream) {
    if (N < 0 || Hb < 0 || Wb < 0 || sumB < 0) return CVPCE_ERR_ARG;
    if (method < CVPCE_GAUSS_MULTIVARIATE_NORMAL || method > CVPCE_GAUSS_SIMPLE_AND_SCALED) return CVPCE_ERR_ARG;
    if (join < CVPCE_GAUSS_JOIN_MAX || join > CVPCE_GAUSS_JOIN_REPLACEMENT) return CVPCE_ERR_ARG;
    if (!params) return CVPCE_ERR_ARG;
    if (N == 0 || Hb == 0 || Wb == 0) return CVPCE_OK;
    if (!geom || !out || N > 65535) return CVPCE_ERR_ARG;
    const bool from_maps = map_ptrs != nullptr;
    if (from_maps == (box_offsets != nullptr)) return CVPCE_ERR_ARG;                 // exactly one source
    if (from_maps && boxes) return CVPCE_ERR_ARG;
    if (!from_maps && sumB > 0 && !boxes) return CVPCE_ERR_ARG;
    if (!from_maps && method == CVPCE_GAUSS_KANT && (!table || table_size < 1 || table_size > 4096)) return CVPCE_ERR_ARG;
    if (!from_maps && method == CVPCE_GAUSS_SIMPLE_AND_SCALED && !(params[2] != 0.f)) return CVPCE_ERR_ARG;
    const long long gx = ((long long)Wb + GT - 1) / GT, gy = ((long long)Hb + GT - 1) / GT;
    if (gy > 65535 || gx > 0x7fffffffLL) return CVPCE_ERR_ARG;
    hipLaunchKernelGGL(gauss_targets_kernel, dim3((unsigned)gx, (unsigned)gy, (unsigned)N), dim3(GT_THREADS), 0, (hipStream_t)stream, boxes,
                       box_offsets, map_ptrs, geom, table, table_size, sumB, Hb, Wb, method, join, params[0], params[1], params[2],
                       tanh ? -1.f : 0.f, resize ? 1 : 0, out);
    return cvpce_check_launch();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// loss
// ---------------------------------------------------------------------------------------------------------------------------------
// workspace: int hist[N][4][256], int counts[N][2] (padded to 4 ints), float partial_pos[N * gx], float partial_neg[N * gx]
struct LossSpace {
    int* hist;
    int* counts;
    float* partial_pos;
    float* partial_neg;
    size_t int_bytes, bytes;
    int gx;
};

static bool loss_space(int N, int Hb, int Wb, void* base, LossSpace& s) {
    if (N < 1 || Hb < 1 || Wb < 1) return false;
    const long long hw = (long long)Hb * Wb;
    if (hw * N >= (1LL << 31) || N > 65535) return false;
    s.gx = (int)((hw + L_SPAN - 1) / L_SPAN);
    const size_t ints = (size_t)N * 4 * 256 + (((size_t)N * 2 + 3) & ~(size_t)3);
    s.int_bytes = ints * sizeof(int);
    s.bytes = s.int_bytes + 2 * (size_t)N * s.gx * sizeof(float);
    s.hist = (int*)base;
    s.counts = s.hist + (size_t)N * 4 * 256;
    s.partial_pos = (float*)((char*)base + s.int_bytes);
    s.partial_neg = s.partial_pos + (size_t)N * s.gx;
    return true;
}

struct LossArgs {
    const float* pred;
    const float* target;
    const int* extent;
    int N, Hb, Wb, gx;
    float neg_thr, pos_thr;
    int min_neg, per_pos, per_image;
    int* hist;
    int* counts;
    float* partial_pos;
    float* partial_neg;
};

// fixed-order sum of one value per thread: the same tree on every run
__device__ __forceinline__ float block_sum(float v, float* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int d = LT / 2; d > 0; d >>= 1) {
        if (tid < d) sh[tid] = sh[tid] + sh[tid + d];
        __syncthreads();
    }
    return sh[0];
}

// The select so far, re-derived by every workgroup from the histograms of passes [0, passes): the bits found (`prefix`, 8 per pass),
// m = the number of negatives used, above = how many negatives lie above the prefix's group.  sh: LT + 2 ints.
__device__ __forceinline__ void select_chain(const int* __restrict__ hist_seg, const int* __restrict__ counts_seg, int passes, int min_neg,
                                             int per_pos, int* sh, unsigned& prefix, int& m, int& above) {
    const int tid = threadIdx.x;
    const long long npos = counts_seg[0], nneg = counts_seg[1];
    long long n = (long long)per_pos * npos;
    if (n < (long long)min_neg) n = min_neg;
    m = (int)(n < nneg ? n : nneg);
    prefix = 0u;
    above = 0;
    if (m <= 0) { m = 0; return; }                                                  // (uniform: the counts are the workgroup's)
    int rem = m;
    for (int p = 0; p < passes; ++p) {
        const int c = hist_seg[p * 256 + 255 - tid];                                // bins in descending order
        __syncthreads();
        sh[tid] = c;
        __syncthreads();
        for (int d = 1; d < LT; d <<= 1) {
            const int add = tid >= d ? sh[tid - d] : 0;
            __syncthreads();
            sh[tid] += add;
            __syncthreads();
        }
        const int incl = sh[tid], excl = incl - c;
        if (incl >= rem && excl < rem) { sh[LT] = 255 - tid; sh[LT + 1] = excl; }
        __syncthreads();
        prefix = (prefix << 8) | (unsigned)sh[LT];
        above += sh[LT + 1];
        rem -= sh[LT + 1];
    }
    __syncthreads();
}

static_assert(LT == 256, "one histogram bin per thread");

// pass 0 .. 3: the histograms; pass 4: the sum above tau
__global__ __launch_bounds__(LT) void gauss_loss_pass_kernel(LossArgs a, int pass) {
    __shared__ int s_hist[256];
    __shared__ int s_scan[LT + 2];
    __shared__ float s_sum[LT];
    __shared__ int s_cnt[2];
    const int tid = threadIdx.x, n = blockIdx.y, seg = a.per_image ? n : 0;
    const int hw = a.Hb * a.Wb;
    int eh = a.Hb, ew = a.Wb;
    if (a.per_image) { eh = min(max(a.extent[2 * n], 0), a.Hb); ew = min(max(a.extent[2 * n + 1], 0), a.Wb); }
    unsigned prefix = 0u;
    int m = 1, above = 0;
    if (pass > 0) {
        select_chain(a.hist + (size_t)seg * 1024, a.counts + 2 * seg, min(pass, 4), a.min_neg, a.per_pos, s_scan, prefix, m, above);
        if (m == 0) {                                                               // nothing to select in this segment
            if (pass == 4 && tid == 0) a.partial_neg[(size_t)n * a.gx + blockIdx.x] = 0.f;
            return;
        }
    }
    s_hist[tid] = 0;
    if (tid < 2) s_cnt[tid] = 0;
    __syncthreads();
    const size_t image = (size_t)n * hw;
    const int base = blockIdx.x * L_SPAN;
    float sum = 0.f;
    int npos = 0, nneg = 0;
    const int shift = 24 - 8 * pass;                                                // (passes 0-3)
#pragma unroll
    for (int i = 0; i < LI; ++i) {
        const int idx = base + i * LT + tid;
        if (idx >= hw) break;
        if (a.per_image) {
            const int yy = idx / a.Wb, xx = idx - yy * a.Wb;
            if (yy >= eh || xx >= ew) continue;
        }
        const float t = a.target[image + idx], d = a.pred[image + idx] - t;
        const float se = d * d;
        const unsigned bits = __float_as_uint(se);
        const bool neg = t <= a.neg_thr;
        if (pass == 0) {
            if (t >= a.pos_thr) { sum = sum + se; ++npos; }
            if (neg) { atomicAdd(&s_hist[bits >> 24], 1); ++nneg; }
        } else if (pass < 4) {
            if (neg && (bits >> (shift + 8)) == prefix) atomicAdd(&s_hist[(bits >> shift) & 255u], 1);
        } else if (neg && bits > prefix) {
            sum = sum + se;
        }
    }
    if (pass == 0) {
        if (npos) atomicAdd(&s_cnt[0], npos);
        if (nneg) atomicAdd(&s_cnt[1], nneg);
    }
    if (pass == 0 || pass == 4) {
        const float total = block_sum(sum, s_sum);
        if (tid == 0) (pass == 0 ? a.partial_pos : a.partial_neg)[(size_t)n * a.gx + blockIdx.x] = total;
    }
    __syncthreads();
    if (pass < 4) {
        const int c = s_hist[tid];
        if (c) atomicAdd(a.hist + (size_t)seg * 1024 + pass * 256 + tid, c);
        if (pass == 0 && tid < 2 && s_cnt[tid]) atomicAdd(a.counts + 2 * seg + tid, s_cnt[tid]);
    }
}

__global__ __launch_bounds__(LT) void gauss_loss_finish_kernel(LossArgs a, float* __restrict__ out_f, int* __restrict__ out_i) {
    __shared__ int s_scan[LT + 2];
    __shared__ float s_sum[LT];
    const int tid = threadIdx.x, seg = blockIdx.x;
    unsigned prefix;
    int m, above;
    select_chain(a.hist + (size_t)seg * 1024, a.counts + 2 * seg, 4, a.min_neg, a.per_pos, s_scan, prefix, m, above);
    const size_t first = a.per_image ? (size_t)seg * a.gx : 0, count = a.per_image ? (size_t)a.gx : (size_t)a.N * a.gx;
    float ps = 0.f, ns = 0.f;
    for (size_t i = tid; i < count; i += LT) {                                      // index order per thread, then a fixed tree
        ps = ps + a.partial_pos[first + i];
        ns = ns + a.partial_neg[first + i];
    }
    const float pos_sum = block_sum(ps, s_sum);
    const float gt_sum = block_sum(ns, s_sum);
    if (tid == 0) {
        const int npos = a.counts[2 * seg];
        float neg_sum = 0.f;
        if (m > 0) neg_sum = gt_sum + (float)(m - above) * __uint_as_float(prefix);
        out_f[3 * seg] = (pos_sum + neg_sum) / (float)(npos + m);
        out_f[3 * seg + 1] = pos_sum;
        out_f[3 * seg + 2] = neg_sum;
        out_i[2 * seg] = npos;
        out_i[2 * seg + 1] = m;
    }
}

extern "C" size_t cvpce_gauss_loss_workspace_bytes(int N, int Hb, int Wb) {
    LossSpace s;
    return loss_space(N, Hb, Wb, nullptr, s) ? s.bytes : 0;
}

extern "C" int cvpce_gauss_loss(const float* pred, const float* target, const int* extent, int N, int Hb, int Wb, float negative_threshold,
                                float positive_threshold, int min_negatives, int negatives_per_positive, int per_image, void* workspace,
                                size_t workspace_bytes, float* out_f, int* out_i, void* stream) {
    LossSpace s;
    if (!loss_space(N, Hb, Wb, workspace, s)) return CVPCE_ERR_ARG;
    if (!pred || !target || !out_f || !out_i || !workspace || ((uintptr_t)workspace & 15) || workspace_bytes < s.bytes) return CVPCE_ERR_ARG;
    if (min_negatives < 0 || negatives_per_positive < 0 || (per_image && !extent)) return CVPCE_ERR_ARG;
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(workspace, 0, s.int_bytes, st) != hipSuccess) return CVPCE_ERR_LAUNCH;
    LossArgs a{pred, target, extent, N, Hb, Wb, s.gx, negative_threshold, positive_threshold, min_negatives, negatives_per_positive,
               per_image ? 1 : 0, s.hist, s.counts, s.partial_pos, s.partial_neg};
    for (int pass = 0; pass <= 4; ++pass) {
        hipLaunchKernelGGL(gauss_loss_pass_kernel, dim3((unsigned)s.gx, (unsigned)N), dim3(LT), 0, st, a, pass);
        const int rc = cvpce_check_launch();
        if (rc != CVPCE_OK) return rc;
    }
    hipLaunchKernelGGL(gauss_loss_finish_kernel, dim3(per_image ? (unsigned)N : 1u), dim3(LT), 0, st, a, out_f, out_i);
    return cvpce_check_launch();
}
