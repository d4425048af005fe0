// The compliance pictures' compositor (include/cvpce_amd_render.h; the picture rule of DESIGN.md 4b): one launch paints any number of
// canvases, each from an ordered item list -- a pixel shows the last item that covers it.
//
//   render_canvases_kernel  one workgroup per 64 x 16 tile of a canvas (the grid is the sum of the tiles of all canvases; a block finds
//                           its canvas by a binary search of the table's tile prefix).  A thread owns 4 adjacent pixels of a row: 12
//                           contiguous bytes, three dword stores where the address allows, bytes at row tails and odd offsets.  The
//                           workgroup walks its canvas's items from the LAST chunk of 256 to the first: thread t tests item t of the
//                           chunk against the tile rectangle, the survivors are compacted into LDS in list order (a 64-bit ballot and
//                           a prefix popcount per wave, plus the wave offsets), and every wave scans them from the back -- all lanes
//                           read the same LDS entry, a broadcast -- until each of its pixels has its first hit.  When every pixel of
//                           the tile is resolved the workgroup stops reading chunks: a base item that covers the canvas ends the walk,
//                           and a tile of a 2048^2 shelf with 200 products tests a handful of items per pixel, not 200.
//                           Source bytes are gathered through L2 with byte loads: a product image is re-read by all tiles of its box.
//
// No floating-point arithmetic beyond comparisons, a clamp, floorf and ceilf: nothing to contract, no FLAGS_render in the Makefile.
#include "common.h"
#include "../../include/cvpce_amd_render.h"

#define RN_THREADS CVPCE_RENDER_THREADS
#define RN_WAVES (RN_THREADS / WAVE)
#define RN_TW CVPCE_RENDER_TILE_W
#define RN_TH CVPCE_RENDER_TILE_H
#define RN_CHUNK CVPCE_RENDER_CHUNK
#define RN_SIDE CVPCE_RENDER_MAX_SIDE
#define RN_COLS CVPCE_RENDER_TABLE_COLS
#define RN_PX 4                                  // pixels of a thread
#define RN_ALL ((1u << RN_PX) - 1u)

static_assert(RN_CHUNK == RN_THREADS, "a thread tests one item of a chunk");
static_assert(RN_TW * RN_TH == RN_THREADS * RN_PX && RN_TW % RN_PX == 0, "a thread owns RN_PX pixels of a tile row");

struct RnItem {
    int x1, y1, bw, bh;                          // integer extents: [x1, x1 + bw) x [y1, y1 + bh)
    int colour, thick;
    int sh, sw;                                  // the source, 0 x 0 where there is none
    long long soff;                              // its byte offset in `from`
    const unsigned char* from;                   // atlas or base
};

// One axis of the sampling rule: pixel i of b -> the two source indices and the 8-bit fraction, of a source of s.  All integers; the
// 32-bit division is the 64-bit one wherever the numerator fits (it is below 2 * b * s * 256).
__device__ __forceinline__ void rn_axis(int i, int b, int s, int& p0, int& p1, unsigned& f) {
    long long q;
    if (s == b) {
        q = (long long)(2 * i + 1) * 128;                                               // (exact: the division leaves no rest)
    } else if ((long long)b * s < (1ll << 23)) {
        q = (long long)(((unsigned)(2 * i + 1) * (unsigned)s * 256u) / (2u * (unsigned)b));
    } else {
        q = ((long long)(2 * i + 1) * s * 256) / (2ll * b);
    }
    long long px = q - 128;
    const long long top = (long long)(s - 1) * 256;
    px = px < 0 ? 0 : (px > top ? top : px);
    p0 = (int)(px >> 8);
    f = (unsigned)(px & 255);
    p1 = min(p0 + 1, s - 1);
}

__device__ __forceinline__ unsigned rn_rgb(const unsigned char* p) {
    return (unsigned)p[0] | ((unsigned)p[1] << 8) | ((unsigned)p[2] << 16);
}

__device__ __forceinline__ unsigned rn_sample(const RnItem& it, int i, int y0, int y1, unsigned fy) {
    int x0, x1;
    unsigned fx;
    rn_axis(i, it.bw, it.sw, x0, x1, fx);
    const unsigned char* s = it.from + it.soff;
    const size_t row = (size_t)it.sw * 3;
    const unsigned char* r0 = s + (size_t)y0 * row;
    if ((fx | fy) == 0) return rn_rgb(r0 + (size_t)x0 * 3);                              // (the other three weights are 0)
    const unsigned char* r1 = s + (size_t)y1 * row;
    const unsigned char *a = r0 + (size_t)x0 * 3, *b = r0 + (size_t)x1 * 3, *c = r1 + (size_t)x0 * 3, *d = r1 + (size_t)x1 * 3;
    const unsigned w00 = (256 - fx) * (256 - fy), w01 = fx * (256 - fy), w10 = (256 - fx) * fy, w11 = fx * fy;
    unsigned v = 0;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) {
        const unsigned t = (w00 * a[ch] + w01 * b[ch] + w10 * c[ch] + w11 * d[ch] + 32768u) >> 16;    // (<= 65536 * 255 + 32768)
        v |= t << (8 * ch);
    }
    return v;
}

__device__ __forceinline__ bool rn_finite(float v) { return v == v && v != __builtin_inff() && v != -__builtin_inff(); }
__device__ __forceinline__ float rn_clamp(float v) { return v < -32768.f ? -32768.f : (v > 32767.f ? 32767.f : v); }

__global__ __launch_bounds__(RN_THREADS) void render_canvases_kernel(
    const long long* __restrict__ canvases, int C, unsigned char* __restrict__ out, long long out_bytes,
    const unsigned char* __restrict__ base, long long base_bytes, const float4* __restrict__ box, const int* __restrict__ src,
    const int* __restrict__ colour, const int* __restrict__ thickness, int n_items, const unsigned char* __restrict__ atlas,
    long long atlas_bytes, const int* __restrict__ atlas_rows, int rows, unsigned background) {
    __shared__ RnItem s_item[RN_CHUNK];
    __shared__ int s_wcount[RN_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const long long bid = blockIdx.x;
    // the last canvas whose tile_start is <= bid (uniform)
    int lo = 0, hi = C - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (canvases[(size_t)mid * RN_COLS] <= bid) lo = mid; else hi = mid - 1;
    }
    const long long* cv = canvases + (size_t)lo * RN_COLS;
    const long long tile = bid - cv[0], out_off = cv[1], H64 = cv[2], W64 = cv[3];
    if (H64 < 1 || H64 > RN_SIDE || W64 < 1 || W64 > RN_SIDE) return;                   // (uniform, as every return below)
    const int H = (int)H64, W = (int)W64;
    const long long bytes = (long long)H * W * 3;
    if (out_off < 0 || out_off > out_bytes || bytes > out_bytes - out_off) return;
    const int tiles_x = (W + RN_TW - 1) / RN_TW, tiles_y = (H + RN_TH - 1) / RN_TH;
    if (tile < 0 || tile >= (long long)tiles_x * tiles_y) return;
    const int tx0 = (int)(tile % tiles_x) * RN_TW, ty0 = (int)(tile / tiles_x) * RN_TH;
    const int tx1 = min(tx0 + RN_TW, W), ty1 = min(ty0 + RN_TH, H);                      // the tile rectangle, cut to the canvas
    // the base, if it lies in its buffer
    const long long b_off = cv[4], b_h = cv[5], b_w = cv[6];
    const bool has_base = base && b_off >= 0 && b_h >= 1 && b_h <= RN_SIDE && b_w >= 1 && b_w <= RN_SIDE && b_off <= base_bytes &&
                          b_h * b_w * 3 <= base_bytes - b_off;
    const long long k0 = min(max(cv[7], 0ll), (long long)n_items), k1 = min(max(cv[8], k0), (long long)n_items);

    const int px = tx0 + (tid % (RN_TW / RN_PX)) * RN_PX, py = ty0 + tid / (RN_TW / RN_PX);
    unsigned val[RN_PX], done = 0;
#pragma unroll
    for (int q = 0; q < RN_PX; ++q) {
        val[q] = background;
        if (py >= H || px + q >= W) done |= 1u << q;                                    // not a pixel: nothing to resolve or store
    }

    const long long chunks = (k1 - k0 + RN_CHUNK - 1) / RN_CHUNK;
    for (long long c = chunks - 1; c >= 0; --c) {
        const long long k = k0 + c * RN_CHUNK + tid;
        bool keep = false;
        RnItem it;
        if (k < k1) {
            const float4 b = box[k];
            if (rn_finite(b.x) && rn_finite(b.y) && rn_finite(b.z) && rn_finite(b.w)) {
                const int X1 = (int)floorf(rn_clamp(b.x)), Y1 = (int)floorf(rn_clamp(b.y));
                const int X2 = (int)ceilf(rn_clamp(b.z)), Y2 = (int)ceilf(rn_clamp(b.w));
                it.x1 = X1, it.y1 = Y1, it.bw = X2 - X1, it.bh = Y2 - Y1;
                it.colour = colour[k] & 0xFFFFFF;
                it.thick = thickness[k];
                it.sh = it.sw = 0, it.soff = 0, it.from = nullptr;
                const int s = src[k];
                if (s == CVPCE_RENDER_SRC_BASE) {
                    if (has_base) it.sh = (int)b_h, it.sw = (int)b_w, it.soff = b_off, it.from = base;
                } else if (s >= 0 && s < rows) {
                    const long long o = atlas_rows[3 * (size_t)s], h = atlas_rows[3 * (size_t)s + 1], w = atlas_rows[3 * (size_t)s + 2];
                    if (o >= 0 && h >= 1 && h <= RN_SIDE && w >= 1 && w <= RN_SIDE && o <= atlas_bytes && h * w * 3 <= atlas_bytes - o)
                        it.sh = (int)h, it.sw = (int)w, it.soff = o, it.from = atlas;
                }
                // kept: a box with an extent that meets the tile and paints something
                keep = X2 > X1 && Y2 > Y1 && X1 < tx1 && X2 > tx0 && Y1 < ty1 && Y2 > ty0 && (it.thick >= 1 || it.sw > 0);
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_wcount[wave] = __popcll(mask);
        __syncthreads();
        int at = __popcll(mask & ((1ull << lane) - 1ull)), n = 0;
#pragma unroll
        for (int w = 0; w < RN_WAVES; ++w) {
            const int cnt = s_wcount[w];
            if (w < wave) at += cnt;
            n += cnt;
        }
        if (keep) s_item[at] = it;                                                       // (at < n <= RN_CHUNK)
        __syncthreads();
        for (int s = n - 1; s >= 0; --s) {                                               // (uniform per wave: n and the break below)
            if (__ballot(done != RN_ALL) == 0ull) break;
            const RnItem& e = s_item[s];
            const int j = py - e.y1;
            if (done == RN_ALL || j < 0 || j >= e.bh) continue;
            const int jm = min(j, e.bh - 1 - j);
            int y0 = 0, y1 = 0;
            unsigned fy = 0;
            bool have_y = false;
#pragma unroll
            for (int q = 0; q < RN_PX; ++q) {
                if (done & (1u << q)) continue;
                const int i = px + q - e.x1;
                if (i < 0 || i >= e.bw) continue;
                if (e.thick >= 1 && min(min(i, e.bw - 1 - i), jm) < e.thick) {
                    val[q] = (unsigned)e.colour;
                    done |= 1u << q;
                } else if (e.sw > 0) {
                    if (!have_y) {
                        rn_axis(j, e.bh, e.sh, y0, y1, fy);
                        have_y = true;
                    }
                    val[q] = rn_sample(e, i, y0, y1, fy);
                    done |= 1u << q;
                }
            }
        }
        if (__syncthreads_and(done == RN_ALL)) break;                                    // (also: s_item and s_wcount may be rewritten)
    }

    if (py >= H || px >= W) return;
    unsigned char* p = out + out_off + ((size_t)py * W + px) * 3;                        // (within the canvas's bytes, checked above)
    if (px + RN_PX <= W && ((uintptr_t)p & 3) == 0) {
        unsigned* p4 = (unsigned*)p;
        p4[0] = val[0] | (val[1] << 24);
        p4[1] = (val[1] >> 8) | (val[2] << 16);
        p4[2] = (val[2] >> 16) | (val[3] << 8);
    } else {
#pragma unroll
        for (int q = 0; q < RN_PX; ++q) {
            if (px + q < W) {
                p[3 * q] = (unsigned char)val[q];
                p[3 * q + 1] = (unsigned char)(val[q] >> 8);
                p[3 * q + 2] = (unsigned char)(val[q] >> 16);
            }
        }
    }
}

extern "C" int cvpce_render_canvases(const long long* canvases, int C, long long total_tiles, unsigned char* out, long long out_bytes,
                                     const unsigned char* base, long long base_bytes, const float* box, const int* src, const int* colour,
                                     const int* thickness, int n_items, const unsigned char* atlas, long long atlas_bytes,
                                     const int* atlas_rows, int rows, int background, void* stream) {
    if (C < 0 || total_tiles < 0 || total_tiles > 0x7FFFFFFFll || out_bytes < 0 || base_bytes < 0 || n_items < 0 || atlas_bytes < 0 || rows < 0)
        return CVPCE_ERR_ARG;
    if (C == 0 || total_tiles == 0) return CVPCE_OK;
    if (!canvases || ((uintptr_t)canvases & 7) || (out_bytes > 0 && !out) || (base_bytes > 0 && !base)) return CVPCE_ERR_ARG;
    if (n_items > 0 && (!box || !src || !colour || !thickness || ((uintptr_t)box & 15))) return CVPCE_ERR_ARG;
    if ((atlas_bytes > 0 && !atlas) || (rows > 0 && !atlas_rows)) return CVPCE_ERR_ARG;
    hipLaunchKernelGGL(render_canvases_kernel, dim3((unsigned)total_tiles), dim3(RN_THREADS), 0, (hipStream_t)stream, canvases, C, out,
                       out_bytes, base, base_bytes, (const float4*)box, src, colour, thickness, n_items, atlas, atlas_bytes, atlas_rows, rows,
                       (unsigned)background & 0xFFFFFFu);
    return cvpce_check_launch();
}
