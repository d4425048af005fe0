/* cvpce_amd -- planogram comparator re-classification kernels, NOT part of the inference ABI.
 *
 * The two ends of the comparator's second trip through the crop / embed / match kernels (cvpce/production.py:100-115: the
 * expected-but-undetected positions are cropped, classified and compared with the expected labels) for a batch of shelf images:
 * `cvpce_reclass_plan` turns what cvpce_homography_finish left on the device into the boxes to crop, `cvpce_reclass_verdict`
 * turns the match result into the per-image number of expected boxes found.  Declared apart from
 * include/cvpce_amd_homography.h.  Same conventions: every pointer is a DEVICE pointer, every call is asynchronous on `stream`
 * (a hipStream_t passed as void*), performs no allocation and no synchronisation, and returns 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad
 * argument, nothing launched) or 2 (CVPCE_ERR_LAUNCH).  Compiled into the same libcvpce_hip.so.  The arithmetic is the
 * re-classification rule of DESIGN.md 4b: fp32 comparisons and one fp32 subtraction per side, integers everywhere else; no
 * atomics, so the output does not depend on scheduling.
 *
 * Shared by both calls (B images, one workgroup each; B = 0: nothing to do, 0; B > 65535 is refused):
 *   status            [B] i32, matched_expected [sumN1] i32, off1 [B+1] i32: as cvpce_homography_finish took / wrote them -- image p
 *                     owns the expected boxes off1[p] .. off1[p+1]-1
 *   cap               slots per image, 1 .. CVPCE_RECLASS_MAX_NODES: the host-known bound of the images' box counts
 *   expected_index    [B][cap] i32, count [B] i32: the plan -- image p's count[p] positions to classify, as indices local to the image
 * All tables are device data: offsets are clamped into their arrays and every index read from memory is range-checked before it
 * is used; an image of more than `cap` boxes is treated like an image whose status is not OK.
 */
#ifndef CVPCE_AMD_RECLASS_H
#define CVPCE_AMD_RECLASS_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVPCE_RECLASS_MAX_NODES 1024          /* = CVPCE_PLANOGRAM_MAX_NODES */
#define CVPCE_RECLASS_THREADS 256

/* The positions to re-classify, in order.
 *
 *   expected_positions [sumN1][4] f32 xyxy, 16-byte aligned: every expected box projected into the image
 *   image              [B][3] i32: {h, w, enabled} -- the image's height and width in pixels, enabled = 0: nothing to classify
 *   boxes              [B][cap][4] f32 out, 16-byte aligned; expected_index [B][cap] i32 out; count [B] i32 out
 * For an image with status OK and enabled != 0, the expected boxes i with matched_expected[i] == 0 are walked in ascending i:
 * x0, x2 are clamped to [0, (float)w] and y1, y3 to [0, (float)h] by comparisons (v < lo ? lo : v > hi ? hi : v: a NaN stays a
 * NaN, -0 stays -0); the position is valid iff (x2 - x0 > 1) && (y3 - y1 > 1).  Valid positions are written densely from slot 0:
 * the clamped box and i; count = their number.  Slots at and beyond count are NOT written.  Any other image: count = 0. */
int cvpce_reclass_plan(const int* status, const int* matched_expected, const float* expected_positions, const int* off1, const int* image,
                       int B, int sumN1, int cap, float* boxes, int* expected_index, int* count, void* stream);

/* The verdict's numerator.
 *
 *   slot_row          [B][cap] i32: the row of each valid slot in the match result
 *   indices           [M][k] i64: the match result (nearest gallery rows, nearest first); only column 0 is read; k >= 1
 *   gallery_label_id  [G] i32, expected_label_id [sumN1] i32: label ids in one id space (equal id = equal label; -1 = a label no
 *                     gallery item has)
 *   found             [sumN1] i32 out, found_count [B] i32 out
 * For an image with status OK: found[i] = matched_expected[i] != 0 for every expected box i; then, for every slot s < count with
 * e = expected_index[s] inside the image, found[e] = 1 iff 0 <= row < M, 0 <= j = indices[row][0] < G, and
 * gallery_label_id[j] == expected_label_id[e] >= 0.  found_count = the integer sum of the image's rows of found.  An image whose
 * status is not OK: found_count = -1, its rows of found are NOT written. */
int cvpce_reclass_verdict(const int* expected_index, const int* count, const int* slot_row, const long long* indices,
                          const int* gallery_label_id, const int* expected_label_id, const int* matched_expected, const int* off1,
                          const int* status, int B, int sumN1, int cap, int M, int k, int G, int* found, int* found_count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
