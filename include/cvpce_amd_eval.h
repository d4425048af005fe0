/* cvpce_amd -- evaluation kernels, NOT part of the inference ABI.
 *
 * include/cvpce_amd.h is the layer under the reference's inference API and is pinned entry point by entry point.  What the
 * evaluation harnesses run on the device after the detector (matching detections to ground truth for mAP) is declared here
 * instead, so that a caller who only links the inference path sees an unchanged header.  Same conventions: every pointer is
 * a DEVICE pointer, every call is asynchronous on `stream` (a hipStream_t passed as void*), performs no allocation and no
 * synchronisation, and returns 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad argument) or 2 (CVPCE_ERR_LAUNCH).  Both headers are
 * compiled into the same libcvpce_hip.so.
 */
#ifndef CVPCE_AMD_EVAL_H
#define CVPCE_AMD_EVAL_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Match the detections of N images to their ground truth at K IoU thresholds in one launch -- the per-image loop of
 * cvpce/metrics.py:17-28 (`check_matches`) in closed form.  The reference visits predictions in descending confidence; a
 * prediction is a true positive when some target with IoU >= threshold is still unused, and (its inner loop has no `break`)
 * it then uses up EVERY unused target at or above the threshold.  So the used set after prediction p is the union of the
 * threshold rows of predictions 0..p, and a prediction is a true positive iff it is the FIRST prediction, in confidence
 * order, that covers some target: per target a min-reduction of rank over the covering predictions.
 *
 *   pred      [sumP][4] f32 xyxy, the images' predictions packed back to back, 16-byte aligned
 *   pred_off  [N+1] i32, image n owns predictions pred_off[n] .. pred_off[n+1]-1 (at most 20 480 of them are expected,
 *             the detector's cap; more are legal)
 *   rank      [sumP] i32, position of the prediction in a STABLE descending sort of its image's confidences
 *             (0 = most confident; equal confidences keep input order); a permutation of 0 .. P_n-1 per image
 *   pred_cls  [sumP] i32 or NULL; tgt_cls [sumT] i32 or NULL (both or neither): with class ids a prediction covers a
 *             target only if the two ids are equal
 *   tgt       [sumT][4] f32 xyxy, 16-byte aligned; tgt_off [N+1] i32
 *   thr       [K] f32, 1 <= K <= 16: the thresholds ROUNDED TO float32 (what comparing a float32 tensor with a Python float
 *             does); the test is iou >= thr in fp32
 *   max_targets  an upper bound of the per-image target count (host-known; sizes the grid)
 *   first     [K][sumT] i32 out: rank of the first covering prediction of each target, -1 if none
 *   tp        [K][sumP] u8 in/out, indexed by pred_off[n] + RANK: set to 1 where some target's `first` is that rank.  The
 *             caller zero-fills it; entries that are not true positives are not written.
 *
 * IoU is cvpce_amd.metrics.box_iou bit for bit: area = (x2-x1)*(y2-y1), inter = max(0, .)*max(0, .),
 * iou = inter / (area_a + area_b - inter), every operation an individually rounded fp32 operation (no fused multiply-add)
 * and the division correctly rounded; 0/0 is NaN and never matches.
 * Errors: K < 1 or K > 16, a negative size, one class array without the other (where both sides have boxes; an empty array
 * may be NULL), a misaligned box pointer. */
int cvpce_eval_match_detections(const float* pred, const int* pred_off, const int* rank, const int* pred_cls,
                                const float* tgt, const int* tgt_off, const int* tgt_cls, const float* thr,
                                int N, int sumP, int sumT, int max_targets, int K,
                                int* first, unsigned char* tp, void* stream);

#ifdef __cplusplus
}
#endif
#endif
