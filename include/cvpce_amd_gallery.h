/* cvpce_amd -- the gallery kernel that reads 8-bit product images, NOT part of the pinned inference ABI.
 *
 * include/cvpce_amd.h is pinned entry point by entry point, and include/cvpce_amd_input.h holds the shelf side's byte-reading
 * kernels (its symbol list is pinned too).  The entry point here is the gallery side's: a product photo, resized on the host so
 * that its longer side is S and kept as the decoder made it -- (h,w,3) bytes, contiguous, a row is 3*w bytes with no padding and
 * no alignment beyond the byte -- becomes the (S,S,C) bf16 pixels the embedder reads, in one launch for a whole ragged batch.  No
 * float copy of an image exists at any time.  Same conventions as the other headers: every pointer is a DEVICE pointer, every
 * call is asynchronous on `stream` (a hipStream_t passed as void*), performs no allocation and no synchronisation, and returns 0
 * (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad argument) or 2 (CVPCE_ERR_LAUNCH).  All headers are compiled into the same libcvpce_hip.so.
 *
 * Meaning of a byte: channel c of a content pixel is table[c][byte], channels 0-2 of a padding pixel (y >= h or x >= w) are
 * table[c][256], channels 3.. are bf16 zero everywhere.  The kernel does NO arithmetic on pixel values -- the caller's table holds
 * what the float path computes for the 256 codes and for the pad value (cvpce_amd.ops.gallery_table makes it with
 * cvpce_pack_embed_input itself), so the pixels have the float path's bits for any mean / std.
 * The kernel loads single bytes: no load is unaligned or wider than a byte, none touches a byte outside
 * [bytes + off, bytes + off + 3*h*w) of its image.  Offsets are 32-bit.
 */
#ifndef CVPCE_AMD_GALLERY_H
#define CVPCE_AMD_GALLERY_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVPCE_GALLERY_MAX_IMAGES 65535   /* images per launch (the grid's y extent) */

/* n gallery byte images -> out (n,S,S,C) bf16, C = 4 (the 8-byte pixels of cvpce_crop_resize mode 2) or 8 (mode 1).
 *   bytes         the images back to back, no alignment between images or rows
 *   geom          (n,3) int32: byte offset of image i in `bytes`, its h, its w (1 <= h, w <= S)
 *   table         (3,257) bf16: per channel the pixel value of the 256 codes, then of the padding
 *   content_only  != 0: padding pixels are NOT written (valid input only for the work-list embedder, which reads the constant crop
 *                 instead -- cvpce_crop_resize_content's contract)
 *   ext_out       (n,2) int32 = (rows, cols) = (h, w): cvpce_crop_extents' meaning -- every pixel at y >= rows or x >= cols is the
 *                 pad constant
 * h / w are data on the device: the kernel clamps them to [0, S] (and reads an image at a negative offset as empty), so a bad geom
 * row stores nothing outside its image's slot; ext_out reports the clamped values.
 * Errors, decided on the host before anything is launched: a null pointer, n < 0, S <= 0, C not 4 or 8, n * S * S * 3 >= 2^31,
 * n > CVPCE_GALLERY_MAX_IMAGES.  n == 0: CVPCE_OK, nothing is launched. */
int cvpce_gallery_pack_u8(const unsigned char* bytes, const int* geom, const void* table, void* out, int n, int S, int C,
                          int content_only, int* ext_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
