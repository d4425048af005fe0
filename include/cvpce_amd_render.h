/* cvpce_amd -- the compliance pictures' compositor, NOT part of the inference ABI.
 *
 * One launch paints any number of canvases of different sizes by the picture rule of DESIGN.md 4b: a canvas is a uint8 (H, W, 3)
 * image described by an ordered item list; a pixel shows the LAST item of the list that covers it, else the background colour.  An
 * item is a box with a ring of a colour and, inside it, nothing, a row of the thumbnail atlas or the canvas's base image, resampled
 * to the box by a bilinear rule written in integers.  Declared apart from include/cvpce_amd_report.h.  Same conventions: every
 * pointer is a DEVICE pointer, the call is asynchronous on `stream` (a hipStream_t passed as void*), performs no allocation and no
 * synchronisation, and returns 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad argument, nothing launched) or 2 (CVPCE_ERR_LAUNCH).  Compiled
 * into the same libcvpce_hip.so.  The only floating-point operations are comparisons, a clamp, floorf and ceilf; no atomics; every
 * output byte has one writer, so the output does not depend on scheduling.
 */
#ifndef CVPCE_AMD_RENDER_H
#define CVPCE_AMD_RENDER_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVPCE_RENDER_THREADS 256
#define CVPCE_RENDER_TILE_W 64               /* a workgroup owns TILE_W x TILE_H pixels of one canvas, a thread 4 adjacent ones of a row */
#define CVPCE_RENDER_TILE_H 16
#define CVPCE_RENDER_CHUNK 256               /* items tested against a tile at a time; there is no maximum on the items of a canvas */
#define CVPCE_RENDER_MAX_SIDE 32768          /* of a canvas and of a base image */
#define CVPCE_RENDER_TABLE_COLS 10

#define CVPCE_RENDER_SRC_NONE (-1)           /* nothing inside the ring: earlier items show through */
#define CVPCE_RENDER_SRC_BASE (-2)           /* the canvas's base image */

/* The tiles of an H x W canvas: what the host adds up into `tile_start`. */
#define CVPCE_RENDER_TILES(H, W) ((((long long)(H) + CVPCE_RENDER_TILE_H - 1) / CVPCE_RENDER_TILE_H) * \
                                  (((long long)(W) + CVPCE_RENDER_TILE_W - 1) / CVPCE_RENDER_TILE_W))

/* Paints C canvases.
 *
 *   canvases     [C][10] i64, 8-byte aligned: {tile_start, out_offset, H, W, base_offset, base_h, base_w, item_begin, item_end, 0}
 *                  tile_start   the tiles of the canvases before this one (ascending; the host's prefix sum of CVPCE_RENDER_TILES)
 *                  out_offset   byte offset of the canvas's H*W*3 bytes in `out`
 *                  base_offset  byte offset of its base image's base_h*base_w*3 bytes in `base`; < 0: the canvas has no base
 *                  item_begin, item_end   its items are box[item_begin .. item_end), in list order
 *   total_tiles  the tiles of all canvases = the grid; 0: nothing to do
 *   out [out_bytes] u8;  base [base_bytes] u8 or NULL with base_bytes 0
 *   box [n_items][4] f32 x1 y1 x2 y2 in canvas pixels, 16-byte aligned;  src, colour, thickness [n_items] i32
 *                  src >= 0 an atlas row, CVPCE_RENDER_SRC_NONE, CVPCE_RENDER_SRC_BASE;  colour R | G<<8 | B<<16
 *   atlas [atlas_bytes] u8;  atlas_rows [rows][3] i32 {byte offset, h, w} (production.pack_gallery_bytes' layout)
 *   background   R | G<<8 | B<<16
 * The table and the items are device data.  A canvas whose H or W is not in [1, CVPCE_RENDER_MAX_SIDE] or whose bytes do not lie
 * in `out` is not painted at all; its item range is clamped to [0, n_items]; a base that does not lie in `base`, or has a side
 * outside [1, CVPCE_RENDER_MAX_SIDE], is no base; an atlas row that does not lie in `atlas` (or has h < 1 or w < 1) and a src outside
 * [-2, rows) count as CVPCE_RENDER_SRC_NONE.  Every byte of a painted canvas is written, nothing else is. */
int cvpce_render_canvases(const long long* canvases, int C, long long total_tiles, unsigned char* out, long long out_bytes,
                          const unsigned char* base, long long base_bytes, const float* box, const int* src, const int* colour,
                          const int* thickness, int n_items, const unsigned char* atlas, long long atlas_bytes, const int* atlas_rows,
                          int rows, int background, void* stream);

#ifdef __cplusplus
}
#endif
#endif
