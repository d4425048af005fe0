// Gallery build from 8-bit product images (include/cvpce_amd_gallery.h): a ragged batch of (h,w,3) byte images -> the (n,S,S,C) bf16
// pixels the embedder reads, one launch.  No arithmetic on pixel values: a pixel's channels are looked up in the caller's (3,257) bf16
// table (256 codes + the padding), which ops.gallery_table makes with cvpce_pack_embed_input -- the float path's own kernel.
#include "common.h"
#include "../../include/cvpce_amd_gallery.h"

#define GALLERY_THREADS 256
#define GALLERY_ROWS 8          // output rows of one image per workgroup
#define GALLERY_CODES 257       // 256 codes + the padding entry

template <int C> struct GalleryPixel;
template <> struct GalleryPixel<4> { typedef bf16x4 type; };
template <> struct GalleryPixel<8> { typedef bf16x8 type; };

// Memory-bound: per pixel three single-byte loads (neighbouring lanes read neighbouring pixels: a wave's loads cover 192 consecutive
// bytes), three 2-byte LDS reads of the table and ONE 8- (C = 4) or 16-byte (C = 8) store.  A workgroup is GALLERY_ROWS rows of one
// image; its 256 threads are `1 << lane_shift` lanes per row (the power of two >= min(S, 256)) x the rows that fit beside each other, so
// that a small S does not leave a workgroup's lanes idle.  Every index is derived from the CLAMPED h / w: a bad geom row reads inside
// 3 * h' * w' <= 3 * h * w bytes of its image and stores inside its own (S,S,C) slot.
template <int C>
__global__ void __launch_bounds__(GALLERY_THREADS)
gallery_pack_u8_kernel(const unsigned char* __restrict__ bytes, const int* __restrict__ geom, const bf16_t* __restrict__ table,
                       bf16_t* __restrict__ out, int S, int lane_shift, int content_only, int* __restrict__ ext) {
    typedef typename GalleryPixel<C>::type pixel_t;
    __shared__ bf16_t tab[3 * GALLERY_CODES];
    const int img = blockIdx.y, y0 = blockIdx.x * GALLERY_ROWS, tid = threadIdx.x;
    const int off = geom[3 * img];
    int h = geom[3 * img + 1], w = geom[3 * img + 2];
    h = h < 0 ? 0 : (h > S ? S : h);
    w = w < 0 ? 0 : (w > S ? S : w);
    if (off < 0) h = w = 0;                                  // (no image starts before the buffer: read as empty)
    if (blockIdx.x == 0 && tid == 0) {
        ext[2 * img] = h;
        ext[2 * img + 1] = w;
    }
    if (content_only && (y0 >= h || w == 0)) return;         // nothing but padding in these rows: left unwritten
    for (int i = tid; i < 3 * GALLERY_CODES; i += GALLERY_THREADS) tab[i] = table[i];
    __syncthreads();
    pixel_t pad;
#pragma unroll
    for (int j = 0; j < C; ++j) pad[j] = (bf16_t)0.f;
#pragma unroll
    for (int c = 0; c < 3; ++c) pad[c] = tab[c * GALLERY_CODES + 256];
    const unsigned char* src = bytes + off;
    pixel_t* dst = reinterpret_cast<pixel_t*>(out) + (size_t)img * S * S;
    const int lanes = 1 << lane_shift, x_first = tid & (lanes - 1), rows_beside = GALLERY_THREADS >> lane_shift;
    int y_end = y0 + GALLERY_ROWS < S ? y0 + GALLERY_ROWS : S;
    if (content_only) y_end = y_end < h ? y_end : h;
    const int x_end = content_only ? w : S;
    for (int y = y0 + (tid >> lane_shift); y < y_end; y += rows_beside) {
        for (int x = x_first; x < x_end; x += lanes) {
            pixel_t o = pad;
            if (y < h && x < w) {
                const unsigned char* p = src + (y * w + x) * 3;          // (< 3 * S * S: 32-bit)
#pragma unroll
                for (int c = 0; c < 3; ++c) o[c] = tab[c * GALLERY_CODES + p[c]];
            }
            dst[(size_t)y * S + x] = o;
        }
    }
}

extern "C" int cvpce_gallery_pack_u8(const unsigned char* bytes, const int* geom, const void* table, void* out, int n, int S, int C,
                                     int content_only, int* ext_out, void* stream) {
    if (!bytes || !geom || !table || !out || !ext_out || n < 0 || S <= 0 || (C != 4 && C != 8)) return CVPCE_ERR_ARG;
    // (32-bit offsets: of a byte within the batch's buffer, which holds at most n * S * S * 3 bytes)
    if ((long long)n * S * S * 3 >= (1LL << 31)) return CVPCE_ERR_ARG;
    if (n > CVPCE_GALLERY_MAX_IMAGES) return CVPCE_ERR_ARG;
    if (n == 0) return CVPCE_OK;
    int lane_shift = 0;
    while ((1 << lane_shift) < S && (1 << lane_shift) < GALLERY_THREADS) ++lane_shift;
    const dim3 grid((S + GALLERY_ROWS - 1) / GALLERY_ROWS, n);
    if (C == 4)
        hipLaunchKernelGGL(gallery_pack_u8_kernel<4>, grid, dim3(GALLERY_THREADS), 0, (hipStream_t)stream, bytes, geom,
                           (const bf16_t*)table, (bf16_t*)out, S, lane_shift, content_only, ext_out);
    else
        hipLaunchKernelGGL(gallery_pack_u8_kernel<8>, grid, dim3(GALLERY_THREADS), 0, (hipStream_t)stream, bytes, geom,
                           (const bf16_t*)table, (bf16_t*)out, S, lane_shift, content_only, ext_out);
    return cvpce_check_launch();
}
