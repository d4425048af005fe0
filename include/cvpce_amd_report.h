/* cvpce_amd -- planogram comparator compliance report kernels, NOT part of the inference ABI.
 *
 * What the comparator's verdict is made of, position by position (the report rule of DESIGN.md 4b): which expected positions were
 * detected, recovered by the re-classification, missing, out of view or never checked, which unclaimed detection sits on a position
 * that was not detected, and which unclaimed detections sit on no position at all.  `cvpce_report_positions` runs behind
 * cvpce_reclass_plan (or behind cvpce_homography_finish where nothing is planned), `cvpce_report_reclass` behind
 * cvpce_reclass_verdict; neither changes what those wrote.  Declared apart from include/cvpce_amd_reclass.h.  Same conventions:
 * every pointer is a DEVICE pointer, every call is asynchronous on `stream` (a hipStream_t passed as void*), performs no allocation
 * and no synchronisation, and returns 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad argument, nothing launched) or 2 (CVPCE_ERR_LAUNCH).
 * Compiled into the same libcvpce_hip.so.  fp32 comparisons, the two fp32 subtractions of the validity test and the IoU of the
 * claim (csrc/iou.h), every operation rounded on its own; no global atomics, and every LDS flag is stored with one value by all
 * its writers, so the output does not depend on scheduling.
 *
 * Shared by both calls (B images, one workgroup of CVPCE_REPORT_THREADS each; B = 0: nothing to do, 0; B > 65535 is refused):
 *   status [B] i32, matched_expected [sumN1] i32, off1 [B+1] i32: as cvpce_homography_finish took / wrote them
 *   outcome [sumN1] i32: one CVPCE_REPORT_* code per expected position
 * All tables are device data: offsets are clamped into their arrays and every index read from memory is range-checked before it
 * is used.  For an image whose status is not OK (or that has more boxes than the call allows) none of its rows are written.
 */
#ifndef CVPCE_AMD_REPORT_H
#define CVPCE_AMD_REPORT_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVPCE_REPORT_MAX_NODES 1024          /* = CVPCE_RECLASS_MAX_NODES */
#define CVPCE_REPORT_THREADS 256

#define CVPCE_REPORT_DETECTED 0              /* matched_expected != 0 */
#define CVPCE_REPORT_RECOVERED 1             /* re-classified as the expected label */
#define CVPCE_REPORT_MISSING 2               /* re-classified as anything else, or not classifiable */
#define CVPCE_REPORT_OUT_OF_VIEW 3           /* the clamped position is not valid (cvpce_reclass_plan's test) */
#define CVPCE_REPORT_UNCHECKED 4             /* the image's `enabled` is 0: no classifier or no image */
#define CVPCE_REPORT_PENDING 5               /* will be re-classified: cvpce_report_reclass decides */

/* Outcomes before the re-classification, occupants and strays.
 *
 *   matched_actual     [sumN2] i32, off2 [B+1] i32: as cvpce_homography_finish wrote / took them
 *   expected_positions [sumN1][4] f32 xyxy, actual_boxes [sumN2][4] f32 xyxy, both 16-byte aligned
 *   image              [B][3] i32: {h, w, enabled}, as cvpce_reclass_plan takes it
 *   actual_row         [sumN2] i32 or NULL: the detections' gallery rows
 *   iou_threshold      the claim's own threshold; the test is (double)iou >= iou_threshold, false on NaN
 *   outcome, occupant, occupant_row [sumN1] i32 out; occupant_iou [sumN1] f32 out; stray [sumN2] i32 out
 * For an image with status OK, n1 <= CVPCE_REPORT_MAX_NODES expected boxes and n2 <= CVPCE_REPORT_MAX_NODES detections:
 *   outcome[e]   DETECTED where matched_expected[e] != 0; else UNCHECKED where enabled == 0; else the position is clamped and tested
 *                exactly as cvpce_reclass_plan does: OUT_OF_VIEW where it is not valid, PENDING where it is
 *   occupant[e]  for matched_expected[e] == 0 (whatever the outcome): the detection j of the image (local index) with
 *                matched_actual[j] == 0 and the largest iou(expected_positions[e], actual_boxes[j]) >= iou_threshold, the lowest j
 *                among equals; -1 where there is none and for a matched position.  occupant_iou[e]: that IoU, else -1.0f.
 *                occupant_row[e]: actual_row[occupant] (0 <= occupant), else -1
 *   stray[j]     1 iff matched_actual[j] == 0 and j is no position's occupant, else 0
 */
int cvpce_report_positions(const int* status, const int* matched_expected, const int* matched_actual, const float* expected_positions,
                           const float* actual_boxes, const int* off1, const int* off2, const int* image, const int* actual_row,
                           double iou_threshold, int B, int sumN1, int sumN2, int* outcome, int* occupant, float* occupant_iou,
                           int* occupant_row, int* stray, void* stream);

/* What the re-classification made of the PENDING positions.
 *
 *   expected_index, count, slot_row, indices, gallery_label_id, expected_label_id, cap, M, k, G: as cvpce_reclass_verdict takes them
 *   distances         [M][k] f32: the match result's distances beside `indices`; only column 0 is read
 *   outcome           [sumN1] i32 in / out; seen_row [sumN1] i32 out; seen_distance [sumN1] f32 out
 * For an image with status OK and at most `cap` boxes: seen_row = -1 and seen_distance = -1.0f for every position; then every
 * position e with outcome[e] == PENDING becomes RECOVERED iff some slot s < count with expected_index[s] == e has 0 <= row < M,
 * 0 <= j = indices[row][0] < G and gallery_label_id[j] == expected_label_id[e] >= 0 (cvpce_reclass_verdict's condition), else
 * MISSING; the LOWEST slot of e with an in-range row and index gives seen_row[e] = j and seen_distance[e] = distances[row][0]
 * (copied, not recomputed).  Every other outcome stays.  So found[e] of cvpce_reclass_verdict == (outcome[e] <= RECOVERED). */
int cvpce_report_reclass(const int* expected_index, const int* count, const int* slot_row, const long long* indices, const float* distances,
                         const int* gallery_label_id, const int* expected_label_id, const int* off1, const int* status, int B, int sumN1,
                         int cap, int M, int k, int G, int* outcome, int* seen_row, float* seen_distance, void* stream);

#ifdef __cplusplus
}
#endif
#endif
