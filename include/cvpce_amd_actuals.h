/* cvpce_amd -- the detections of a window as the planogram comparator's actual side, NOT part of the inference ABI.
 *
 * Between the matcher and the comparator a window's detections need three things done to them (cvpce_amd/production.py,
 * `PlanogramEvaluator.detect_and_classify_batch`): the zero-area boxes are dropped (`_nondegenerate`), every kept box gets the label
 * of its nearest gallery item, and the graph kernel wants one distance threshold per image (`planograms_device.graph_threshold`).
 * `cvpce_actuals_count` tells the host how many boxes each image keeps -- all it needs to know to size the comparator's launches --
 * and `cvpce_actuals_pack` leaves the kept boxes, their gallery rows, their label ids and the thresholds on the device, packed the
 * way cvpce_planogram_graphs, cvpce_planogram_match and the cvpce_homography_* calls read an actual side.  Declared apart from
 * include/cvpce_amd_reclass.h.  Same conventions: every pointer is a DEVICE pointer, every call is asynchronous on `stream` (a
 * hipStream_t passed as void*), performs no allocation and no synchronisation, and returns 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad
 * argument, nothing launched) or 2 (CVPCE_ERR_LAUNCH).  Compiled into the same libcvpce_hip.so, every fp32 operation rounded on its
 * own; no atomics, so the output does not depend on scheduling.
 *
 * Shared by both calls (B images, one workgroup each; B = 0: nothing to do, 0; B > 65535 is refused):
 *   boxes   [B][per][4] f32 xyxy, 16-byte aligned: the detector's kept boxes, `per` slots per image (per >= 1)
 *   count   [B] i32: image i's boxes are its slots j < clamp(count[i], 0, per) -- its prefix.  Slots at and beyond the prefix are
 *           never read.
 * A prefix box is KEPT iff it is non-degenerate by `production._nondegenerate`'s rule: every coordinate is truncated toward zero to
 * an integer (x0, y1, x2, y3), and x2 - x0 > 0 and y3 - y1 > 0.  A box with a coordinate that is not finite or not below 2^62 in
 * magnitude is not kept.
 */
#ifndef CVPCE_AMD_ACTUALS_H
#define CVPCE_AMD_ACTUALS_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVPCE_ACTUALS_THREADS 256

/* kept [B] i32 out: the number of kept boxes of every image. */
int cvpce_actuals_count(const float* boxes, const int* count, int B, int per, int* kept, void* stream);

/* The actual side of a window, packed.
 *
 *   indices            [B][per][k] i64: the match result of every slot (nearest gallery rows, nearest first); only column 0 of the
 *                      kept boxes' slots is read; k >= 1
 *   gallery_label_id   [G] i32: the label id of every gallery row
 *   off2               [B+1] i32: image i owns the output rows off2[i] .. off2[i+1]-1 -- the host's prefix sums of `kept`
 *   thresh_size        the graph threshold as a fraction of the span of the boxes (planograms.build_graph)
 *   out_boxes          [sum2][4] f32 out, 16-byte aligned; out_row [sum2] i32 out; out_label [sum2] i32 out
 *   thresh             [B] f32 out; status [B] i32 out
 * Image i's kept boxes are copied bit for bit, in slot order, to its output rows from the first one on; beside each go the gallery
 * row r = indices[i][j][0] and gallery_label_id[r].  A row outside [0, G) is written as -1 with label 0.  Offsets are clamped into
 * [0, sum2] and a kept box beyond the image's rows is not written, so a stale off2 cannot make the kernel write outside its image's
 * rows.  Output rows beyond an image's kept boxes are NOT written.
 *   thresh[i] = thresh_size * ((((max x2 - min x0) + max y3) - min y1) / 2) over the image's kept boxes, in fp32 in that order --
 * `planograms_device.graph_threshold` of the kept boxes, bit for bit.  NOT written for an image that keeps nothing.
 *   status[i] = 2 if a row read for a kept box lay outside [0, G); else 1 if the number of kept boxes is not off2[i+1] - off2[i];
 * else 0. */
int cvpce_actuals_pack(const float* boxes, const int* count, const long long* indices, int k, const int* gallery_label_id, int G,
                       const int* off2, float thresh_size, int B, int per, int sum2, float* out_boxes, int* out_row, int* out_label,
                       float* thresh, int* status, void* stream);

#ifdef __cplusplus
}
#endif
#endif
