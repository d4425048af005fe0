// The work-list entry of the embedder's constant-padding tile skipping (skiplist.hip builds the lists; conv3x3_halo2.hip,
// conv3x3_halo3.hip and vgg_stem2.hip walk them): its layout, pack / unpack, and the launch limits that follow from it.
//
//   entry = hi << 32 | lo          lo = n << 16 | ty << 8 | tx          hi = rows << 24 | ey << 12 | ex
//
//   n        image (crop) of the tile; image N - 1 of every tensor is the constant crop
//   ty, tx   tile row / column in the image, in the tile size of the kernel that walks the list
//   rows     how many of the tile's 16 conv-output rows are computed (even, 2 .. 16; the list modes 2 and 3 of skiplist.hip: 4 | 8 | 12 | 16)
//   ey, ex   the crop's content extent on the kernel's INPUT tensor: pixels with y >= ey or x >= ex are read from the constant crop
// The kernels read an entry as its two 32-bit words (one readfirstlane each) and take the fields from those.
#pragma once

constexpr int WL_TILE_BITS = 8;      // tx, ty
constexpr int WL_IMAGE_BITS = 16;    // n
constexpr int WL_EXT_BITS = 12;      // ex, ey
constexpr int WL_ROWS_BITS = 8;      // rows
static_assert(2 * WL_TILE_BITS + WL_IMAGE_BITS == 32 && 2 * WL_EXT_BITS + WL_ROWS_BITS == 32, "an entry is two 32-bit words");

// What a launch that walks a list may be given.  Tile rows / columns and images are bounded as COUNTS (skiplist.hip also keeps a
// crop's tile counts in fields of WL_TILE_BITS), an extent can be the whole height / width of the input tensor.
constexpr int WL_MAX_TILES = (1 << WL_TILE_BITS) - 1;      // 255 tile rows, 255 tile columns
constexpr int WL_MAX_IMAGES = (1 << WL_IMAGE_BITS) - 1;    // 65535 images, the constant crop included
constexpr int WL_MAX_EXTENT = (1 << WL_EXT_BITS) - 1;      // 4095 rows / columns of the input tensor

__host__ __device__ inline unsigned wl_pack_ext(unsigned ey, unsigned ex) { return (ey << WL_EXT_BITS) | ex; }
// ext = wl_pack_ext(ey, ex)
__host__ __device__ inline unsigned long long wl_pack(unsigned rows, unsigned ext, unsigned n, unsigned ty, unsigned tx) {
    return ((unsigned long long)((rows << (2 * WL_EXT_BITS)) | ext) << 32) |
           (unsigned long long)((n << (2 * WL_TILE_BITS)) | (ty << WL_TILE_BITS) | tx);
}

__host__ __device__ inline unsigned wl_lo(unsigned long long e) { return (unsigned)e; }
__host__ __device__ inline unsigned wl_hi(unsigned long long e) { return (unsigned)(e >> 32); }
__host__ __device__ inline int wl_image(unsigned lo) { return (int)(lo >> (2 * WL_TILE_BITS)); }
// The halo kernels keep the low word in a signed register and shift it arithmetically, as they always have: the same image for
// n < 32768 (a pass has a few thousand crops).  Kept so that their code stays what it was; reading it unsigned is a change of its own.
__host__ __device__ inline int wl_image_signed(int lo) { return lo >> (2 * WL_TILE_BITS); }
__host__ __device__ inline int wl_ty(unsigned lo) { return (int)((lo >> WL_TILE_BITS) & ((1u << WL_TILE_BITS) - 1)); }
__host__ __device__ inline int wl_tx(unsigned lo) { return (int)(lo & ((1u << WL_TILE_BITS) - 1)); }
__host__ __device__ inline int wl_rows(unsigned hi) { return (int)((hi >> (2 * WL_EXT_BITS)) & ((1u << WL_ROWS_BITS) - 1)); }
__host__ __device__ inline int wl_ey(unsigned hi) { return (int)((hi >> WL_EXT_BITS) & ((1u << WL_EXT_BITS) - 1)); }
__host__ __device__ inline int wl_ex(unsigned hi) { return (int)(hi & ((1u << WL_EXT_BITS) - 1)); }

// a launch over N images of H x W input pixels in tiles of 16 rows x tile_w columns can be described by entries
static inline bool wl_fits(int N, int H, int W, int tile_w) {
    return N <= WL_MAX_IMAGES && (H + 15) / 16 <= WL_MAX_TILES && (W + tile_w - 1) / tile_w <= WL_MAX_TILES && H <= WL_MAX_EXTENT &&
           W <= WL_MAX_EXTENT;
}
