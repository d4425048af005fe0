/* cvpce_amd -- the step pictures' strokes: NOT part of the inference ABI.
 *
 * One launch draws straight strokes with round caps over canvases that already exist -- the flat output of cvpce_render_canvases,
 * drawn on in place -- by the stroke rule of DESIGN.md 4b: a canvas has an ordered stroke list, a pixel some stroke covers takes the
 * colour of the LAST stroke of the list that covers it, and a pixel no stroke covers is NOT WRITTEN.  A node disc is a stroke of
 * length zero.  Same conventions as the headers of include/: every pointer is a DEVICE pointer, the call is asynchronous on `stream`
 * (a hipStream_t passed as void*), performs no allocation and no synchronisation, and returns 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad
 * argument, nothing launched) or 2 (CVPCE_ERR_LAUNCH).  Compiled into the same libcvpce_hip.so.  No atomics; a byte has at most one
 * writer, so the output does not depend on scheduling.
 *
 * This header lies in include/ext/ for the reason include/ext/cvpce_amd_tonioni.h gives: the ABI mirror test pins the set of
 * headers directly under include/ and their entry point counts.
 *
 * The rule, in integers.  Stroke k has `ends` (ax ay bx by, float32, canvas pixels), a colour (R | G<<8 | B<<16) and a radius in HALF
 * pixels: radius <= 0 is skipped, larger values are clamped to CVPCE_STROKES_MAX_RADIUS; thickness t px is radius t.  A stroke with an
 * end that is not finite is skipped.  Each coordinate is clamped to [-32768, 32767] and taken to half pixels as floor(2 * x) -- the
 * only floating-point operations, each exact.  With A, B the integer ends, P = (2x + 1, 2y + 1) the centre of pixel (x, y),
 * d = B - A, v = P - A, L2 = d.d, s = v.d and R the radius, the pixel is covered iff
 *      s <= 0   and  v.v <= R^2,       or
 *      s >= L2  and  |P - B|^2 <= R^2, or
 *      otherwise     (vx * dy - vy * dx)^2 <= R^2 * L2          (L2 = 0 falls under the first case: a disc).
 */
#ifndef CVPCE_AMD_STROKES_H
#define CVPCE_AMD_STROKES_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVPCE_STROKES_THREADS 256
#define CVPCE_STROKES_TILE_W 64              /* the compositor's tile: a workgroup owns TILE_W x TILE_H pixels, a thread 4 of a row */
#define CVPCE_STROKES_TILE_H 16
#define CVPCE_STROKES_CHUNK 256              /* strokes tested against a tile at a time; there is no maximum on the strokes of a canvas */
#define CVPCE_STROKES_MAX_SIDE 32768
#define CVPCE_STROKES_MAX_RADIUS 64          /* half pixels */
#define CVPCE_STROKES_TABLE_COLS 6

/* Draws on C canvases.
 *
 *   canvases     [C][6] i64, 8-byte aligned: {tile_start, out_offset, H, W, stroke_begin, stroke_end}
 *                  tile_start   the tiles of the canvases before this one (ascending; a canvas of H x W has
 *                               ceil(H / TILE_H) * ceil(W / TILE_W) tiles)
 *                  out_offset   byte offset of the canvas's H*W*3 bytes in `out`
 *                  stroke_begin, stroke_end   its strokes are ends[stroke_begin .. stroke_end), in list order
 *   total_tiles  the tiles of all canvases = the grid; 0, as C = 0 or n_strokes = 0: nothing to do, nothing launched
 *   out [out_bytes] u8: the canvases, drawn on in place
 *   ends [n_strokes][4] f32 ax ay bx by, 16-byte aligned;  colour, radius [n_strokes] i32
 * The table and the strokes are device data.  A canvas whose H or W is not in [1, CVPCE_STROKES_MAX_SIDE] or whose bytes do not lie
 * in `out` is not drawn on; its stroke range is clamped to [0, n_strokes].  Only the three bytes of covered pixels are written. */
int cvpce_strokes_draw(const long long* canvases, int C, long long total_tiles, unsigned char* out, long long out_bytes,
                       const float* ends, const int* colour, const int* radius, int n_strokes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
