// The step pictures' strokes (include/ext/cvpce_amd_strokes.h; the stroke rule of DESIGN.md 4b): one launch draws straight strokes with
// round caps over any number of canvases that already exist, each from an ordered stroke list -- a covered pixel takes the colour of
// the last stroke that covers it, a pixel no stroke covers is not written.
//
//   strokes_draw_kernel  render.hip's shape: one workgroup per 64 x 16 tile of a canvas (the grid is the sum of the tiles of all
//                        canvases; a block finds its canvas by a binary search of the table's tile prefix), a thread owns 4 adjacent
//                        pixels of a row.  The workgroup walks its canvas's strokes from the LAST chunk of 256 to the first: thread t
//                        turns stroke t of the chunk into integers and tests it against the tile, the survivors' constants (A, d, L2,
//                        R^2, colour) are compacted into LDS in list order (a 64-bit ballot and a prefix popcount per wave, plus the
//                        wave offsets), and every wave scans them from the back -- all lanes read the same LDS entry, a broadcast --
//                        until each of its pixels has its first hit.  When every pixel of the tile is resolved the workgroup stops
//                        reading chunks.
//                        The tile test is the stroke's bounding box grown by the radius: a long diagonal passes it in every tile of
//                        its box, also those it does not touch, and costs them one entry of the scan each.  Graph edges join
//                        neighbouring products, so long diagonals are rare and the box is what a handful of tiles test anyway.
//                        Only covered pixels are stored: three dword stores where a thread's four pixels are all covered and the
//                        address allows, else three byte stores per covered pixel.  No byte is read.
//
// The only floating-point operations are comparisons, a clamp, a doubling and floorf, each exact: nothing to contract, no FLAGS_strokes
// in the Makefile.
#include "common.h"
#include "../../include/ext/cvpce_amd_strokes.h"

#define SK_THREADS CVPCE_STROKES_THREADS
#define SK_WAVES (SK_THREADS / WAVE)
#define SK_TW CVPCE_STROKES_TILE_W
#define SK_TH CVPCE_STROKES_TILE_H
#define SK_CHUNK CVPCE_STROKES_CHUNK
#define SK_SIDE CVPCE_STROKES_MAX_SIDE
#define SK_RADIUS CVPCE_STROKES_MAX_RADIUS
#define SK_COLS CVPCE_STROKES_TABLE_COLS
#define SK_PX 4                                  // pixels of a thread
#define SK_ALL ((1u << SK_PX) - 1u)

static_assert(SK_CHUNK == SK_THREADS, "a thread tests one stroke of a chunk");
static_assert(SK_TW * SK_TH == SK_THREADS * SK_PX && SK_TW % SK_PX == 0, "a thread owns SK_PX pixels of a tile row");

struct SkStroke {                                // in half pixels
    int ax, ay, dx, dy;                          // A and d = B - A: |A| <= 2^16, |d| < 2^17
    long long l2;                                // d.d <= 2^35
    int r2, colour;                              // R^2 <= 4096
};

__device__ __forceinline__ bool sk_finite(float v) { return v == v && v != __builtin_inff() && v != -__builtin_inff(); }
// a coordinate in half pixels: clamp, double (exact: a power of two), floor -> [-65536, 65534]
__device__ __forceinline__ int sk_half(float v) { return (int)floorf(2.f * (v < -32768.f ? -32768.f : (v > 32767.f ? 32767.f : v))); }

// Is the pixel centre at v = P - A covered?  |v| < 2^17 and |d| < 2^17 a component, so s, v.v, L2 and |cross| are at most 2^35: 64-bit
// sums of 32 x 32 -> 64-bit products.
__device__ __forceinline__ bool sk_covers(const SkStroke& e, int vx, int vy) {
    const long long s = (long long)vx * e.dx + (long long)vy * e.dy;
    if (s <= 0) return (long long)vx * vx + (long long)vy * vy <= e.r2;                  // (also L2 = 0: the disc)
    if (s >= e.l2) {
        const int wx = vx - e.dx, wy = vy - e.dy;                                        // P - B, |.| < 2^17
        return (long long)wx * wx + (long long)wy * wy <= e.r2;
    }
    const long long cross = (long long)vx * e.dy - (long long)vy * e.dx;
    const unsigned long long a = (unsigned long long)(cross < 0 ? -cross : cross);
    // R <= 64 and L2 <= 2^35: the right side is below 2^48, so |cross| >= 2^24 is "not covered", and below that the square fits
    return a < (1ull << 24) && a * a <= (unsigned long long)e.r2 * (unsigned long long)e.l2;
}

__global__ __launch_bounds__(SK_THREADS) void strokes_draw_kernel(
    const long long* __restrict__ canvases, int C, unsigned char* __restrict__ out, long long out_bytes,
    const float4* __restrict__ ends, const int* __restrict__ colour, const int* __restrict__ radius, int n_strokes) {
    __shared__ SkStroke s_stroke[SK_CHUNK];
    __shared__ int s_wcount[SK_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const long long bid = blockIdx.x;
    // the last canvas whose tile_start is <= bid (uniform)
    int lo = 0, hi = C - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (canvases[(size_t)mid * SK_COLS] <= bid) lo = mid; else hi = mid - 1;
    }
    const long long* cv = canvases + (size_t)lo * SK_COLS;
    const long long tile = bid - cv[0], out_off = cv[1], H64 = cv[2], W64 = cv[3];
    if (H64 < 1 || H64 > SK_SIDE || W64 < 1 || W64 > SK_SIDE) return;                   // (uniform, as every return below)
    const int H = (int)H64, W = (int)W64;
    const long long bytes = (long long)H * W * 3;
    if (out_off < 0 || out_off > out_bytes || bytes > out_bytes - out_off) return;
    const int tiles_x = (W + SK_TW - 1) / SK_TW, tiles_y = (H + SK_TH - 1) / SK_TH;
    if (tile < 0 || tile >= (long long)tiles_x * tiles_y) return;
    const int tx0 = (int)(tile % tiles_x) * SK_TW, ty0 = (int)(tile / tiles_x) * SK_TH;
    const int tx1 = min(tx0 + SK_TW, W), ty1 = min(ty0 + SK_TH, H);                      // the tile rectangle, cut to the canvas
    // its pixel centres in half pixels: [cx0, cx1] x [cy0, cy1]
    const int cx0 = 2 * tx0 + 1, cx1 = 2 * tx1 - 1, cy0 = 2 * ty0 + 1, cy1 = 2 * ty1 - 1;
    const long long k0 = min(max(cv[4], 0ll), (long long)n_strokes), k1 = min(max(cv[5], k0), (long long)n_strokes);

    const int px = tx0 + (tid % (SK_TW / SK_PX)) * SK_PX, py = ty0 + tid / (SK_TW / SK_PX);
    const int cpx = 2 * px + 1, cpy = 2 * py + 1;
    unsigned val[SK_PX], done = 0, hit = 0;
#pragma unroll
    for (int q = 0; q < SK_PX; ++q) {
        val[q] = 0;
        if (py >= H || px + q >= W) done |= 1u << q;                                    // not a pixel: nothing to resolve or store
    }

    const long long chunks = (k1 - k0 + SK_CHUNK - 1) / SK_CHUNK;
    for (long long c = chunks - 1; c >= 0; --c) {
        const long long k = k0 + c * SK_CHUNK + tid;
        bool keep = false;
        SkStroke st;
        if (k < k1) {
            const float4 e = ends[k];
            const int r = min(radius[k], SK_RADIUS);
            if (r >= 1 && sk_finite(e.x) && sk_finite(e.y) && sk_finite(e.z) && sk_finite(e.w)) {
                const int ax = sk_half(e.x), ay = sk_half(e.y), bx = sk_half(e.z), by = sk_half(e.w);
                st.ax = ax, st.ay = ay, st.dx = bx - ax, st.dy = by - ay;
                st.l2 = (long long)st.dx * st.dx + (long long)st.dy * st.dy;
                st.r2 = r * r;
                st.colour = colour[k] & 0xFFFFFF;
                // kept: the bounding box grown by the radius holds a pixel centre of the tile (a covered centre is within R of the
                // segment, so inside that box)
                keep = min(ax, bx) - r <= cx1 && max(ax, bx) + r >= cx0 && min(ay, by) - r <= cy1 && max(ay, by) + r >= cy0;
            }
        }
        const unsigned long long mask = __ballot(keep);
        if (lane == 0) s_wcount[wave] = __popcll(mask);
        __syncthreads();
        int at = __popcll(mask & ((1ull << lane) - 1ull)), n = 0;
#pragma unroll
        for (int w = 0; w < SK_WAVES; ++w) {
            const int cnt = s_wcount[w];
            if (w < wave) at += cnt;
            n += cnt;
        }
        if (keep) s_stroke[at] = st;                                                     // (at < n <= SK_CHUNK)
        __syncthreads();
        for (int s = n - 1; s >= 0; --s) {                                               // (uniform per wave: n and the break below)
            if (__ballot(done != SK_ALL) == 0ull) break;
            const SkStroke& e = s_stroke[s];
            if (done == SK_ALL) continue;
            const int vy = cpy - e.ay;
#pragma unroll
            for (int q = 0; q < SK_PX; ++q) {
                if (done & (1u << q)) continue;
                if (sk_covers(e, cpx + 2 * q - e.ax, vy)) {
                    val[q] = (unsigned)e.colour;
                    done |= 1u << q;
                    hit |= 1u << q;
                }
            }
        }
        if (__syncthreads_and(done == SK_ALL)) break;                                    // (also: s_stroke and s_wcount may be rewritten)
    }

    if (!hit) return;                                                                    // (hit bits are pixels of the canvas)
    unsigned char* p = out + out_off + ((size_t)py * W + px) * 3;                        // (within the canvas's bytes, checked above)
    if (hit == SK_ALL && ((uintptr_t)p & 3) == 0) {                                      // (all four covered: px + 4 <= W)
        unsigned* p4 = (unsigned*)p;
        p4[0] = val[0] | (val[1] << 24);
        p4[1] = (val[1] >> 8) | (val[2] << 16);
        p4[2] = (val[2] >> 16) | (val[3] << 8);
    } else {
#pragma unroll
        for (int q = 0; q < SK_PX; ++q) {
            if (hit & (1u << q)) {
                p[3 * q] = (unsigned char)val[q];
                p[3 * q + 1] = (unsigned char)(val[q] >> 8);
                p[3 * q + 2] = (unsigned char)(val[q] >> 16);
            }
        }
    }
}

extern "C" int cvpce_strokes_draw(const long long* canvases, int C, long long total_tiles, unsigned char* out, long long out_bytes,
                                  const float* ends, const int* colour, const int* radius, int n_strokes, void* stream) {
    if (C < 0 || total_tiles < 0 || total_tiles > 0x7FFFFFFFll || out_bytes < 0 || n_strokes < 0) return CVPCE_ERR_ARG;
    if (C == 0 || total_tiles == 0 || n_strokes == 0) return CVPCE_OK;
    if (!canvases || ((uintptr_t)canvases & 7) || (out_bytes > 0 && !out)) return CVPCE_ERR_ARG;
    if (!ends || !colour || !radius || ((uintptr_t)ends & 15)) return CVPCE_ERR_ARG;
    hipLaunchKernelGGL(strokes_draw_kernel, dim3((unsigned)total_tiles), dim3(SK_THREADS), 0, (hipStream_t)stream, canvases, C, out,
                       out_bytes, (const float4*)ends, colour, radius, n_strokes);
    return cvpce_check_launch();
}
