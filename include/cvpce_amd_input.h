/* cvpce_amd -- input kernels that read 8-bit images, NOT part of the pinned inference ABI.
 *
 * include/cvpce_amd.h is pinned entry point by entry point; its transform and crop kernels read an image as float32 planes
 * (3,H,W) in [0,1].  The entry points here are the same kernels (csrc/preproc.hip, one template per kernel) reading the image as
 * the decoder made it: (H,W,3) bytes, contiguous, a row is 3*W bytes with no padding and no alignment beyond the byte.  No float
 * copy of the image exists at any time.  Same conventions as the other two headers: every pointer is a DEVICE pointer unless said
 * otherwise, every call is asynchronous on `stream` (a hipStream_t passed as void*), performs no allocation and no
 * synchronisation, and returns 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad argument) or 2 (CVPCE_ERR_LAUNCH).  All three headers are
 * compiled into the same libcvpce_hip.so.
 *
 * Meaning of a byte: code b is the float32 table[b], and the caller's table holds float32(b) / float32(255), correctly rounded,
 * computed on the host (256 floats on the device; cvpce_amd.ops.uint8_table).  The kernels use the table's values and nothing
 * else -- no multiply by 1/255 (wrong for 126 of the 256 codes), no division -- so with that table every result has the bits the
 * float entry point gives for the float image `bytes.permute(2,0,1).float() / 255`.
 * The kernels load single bytes: no load is unaligned or wider than a pixel, none touches a byte outside [img, img + H*W*3).
 * Byte offsets are 32-bit: an image with H * W * 3 >= 2^31 is CVPCE_ERR_ARG, decided on the host before anything is launched.
 */
#ifndef CVPCE_AMD_INPUT_H
#define CVPCE_AMD_INPUT_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* cvpce_gln_transform_batch (cvpce_amd.h) over a list that may mix the two image forms -- still ONE launch per 32 images.
 *   imgs      [n] HOST array of device pointers: float32 (3,H0,W0) planes, or (H0,W0,3) bytes where is_bytes[i] != 0
 *   is_bytes  [n] HOST array, the form of each image
 *   H0, W0, h, w  [n] HOST arrays: original and resized size of each image; out_nhwc8 (n,Hp,Wp,8) bf16 (fp16: the _f16 twin)
 *   table     [256] float32 on the device
 * Errors: a null pointer, a size <= 0, h > Hp or w > Wp, a byte image with H0 * W0 * 3 >= 2^31. */
int cvpce_gln_transform_batch_u8(const void* const* imgs, const unsigned char* is_bytes, const int* H0, const int* W0,
                                 const int* h, const int* w, int n, void* out_nhwc8, int Hp, int Wp, const float* mean3,
                                 const float* std3, const float* table, void* stream);
int cvpce_gln_transform_batch_u8_f16(const void* const* imgs, const unsigned char* is_bytes, const int* H0, const int* W0,
                                     const int* h, const int* w, int n, void* out_nhwc8, int Hp, int Wp, const float* mean3,
                                     const float* std3, const float* table, void* stream);

/* cvpce_crop_resize (cvpce_amd.h: modes 0 / 1 / 2, the same boxes, count and outputs) from an (H0,W0,3) byte image. */
int cvpce_crop_resize_u8(const unsigned char* img, const float* table, const float* boxes, const int* count_dev,
                         int max_boxes, void* out, int H0, int W0, int S, int mode, const float* mean3, const float* std3,
                         void* stream);

/* cvpce_crop_resize_content (cvpce_amd.h: modes 1 / 2, even S, the crops' content only) from an (H0,W0,3) byte image. */
int cvpce_crop_resize_content_u8(const unsigned char* img, const float* table, const float* boxes, const int* count_dev,
                                 int max_boxes, void* out, int H0, int W0, int S, int mode, const float* mean3,
                                 const float* std3, const int* ext, void* stream);

#ifdef __cplusplus
}
#endif
#endif
