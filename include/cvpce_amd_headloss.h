/* cvpce_amd -- scoring the detector's classification and regression heads, NOT part of the inference ABI.
 *
 * The reference's `GaussianLayerNetwork.compute_loss` (cvpce/models/proposals.py:169-175) adds RetinaNet's two training losses to
 * its Gaussian loss: every anchor of an image is matched to the ground-truth boxes by IoU (torchvision's Matcher(0.5, 0.4,
 * allow_low_quality_matches=True)), a sigmoid focal loss runs over the anchors that are not between the thresholds and an L1
 * loss over the encoded boxes of the foreground anchors.  Here the IoU matrix is never stored: the boxes sit in LDS and every
 * anchor is a thread (DESIGN.md 4d is the rule).  Same conventions as the other headers: every pointer is a DEVICE pointer unless
 * it says otherwise, a call is asynchronous on `stream` (a hipStream_t passed as void*), performs no allocation and no
 * synchronisation, and returns 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad argument, nothing launched) or 2 (CVPCE_ERR_LAUNCH).  Compiled
 * into the same libcvpce_hip.so, with every fp32 operation rounded on its own (no contraction); the library functions are expf,
 * log1pf and logf.
 */
#ifndef CVPCE_AMD_HEADLOSS_H
#define CVPCE_AMD_HEADLOSS_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVPCE_HEADLOSS_CHUNK 1024             /* boxes of one image staged in LDS at a time (16 KiB of boxes, 4 KiB of best IoUs) */
#define CVPCE_HEADLOSS_THREADS 256            /* anchors per workgroup: one per thread */
#define CVPCE_HEADLOSS_MAX_LEVELS 8

/* Workspace of cvpce_headloss in bytes (host only, no GPU call); 0 for arguments it would refuse.  gh, gw: HOST arrays [L]. */
size_t cvpce_headloss_workspace_bytes(const int* gh, const int* gw, int L, int A, int N, int sumT);

/* The two head losses of a batch of N images: a memset and three launches (headloss_match, headloss_terms, headloss_finish),
 * whatever the number of boxes.
 *
 *   logits, regs   HOST arrays [L] of device pointers, as cvpce_detect_postprocess takes them: level l's logits
 *                  [N][gh*gw*A*K] f32 and regressions [N][gh*gw*A][4] f32
 *   gh, gw, stride_h, stride_w   HOST arrays [L]: the level's grid and stride = padded size // grid
 *   base_anchors   [L][A][4] f32
 *   boxes          [sumT][4] f32 xyxy in original-image pixels, labels [sumT] i32, box_offsets [N+1] i32 ascending from 0:
 *                  image n's boxes (an offset is clamped to [0, sumT])
 *   scales         [N][2] f32: ratio_h, ratio_w = float(transformed size) / float(original size); a box becomes
 *                  (x1 * ratio_w, y1 * ratio_h, x2 * ratio_w, y2 * ratio_h), one fp32 multiply per coordinate
 *   matched        [N][A_total] i32, A_total = A * sum(gh * gw), anchors level-major, cell-major, then anchor: the box index
 *                  (within its image) an anchor is matched to, -1 background, -2 between the thresholds.  EVERY element is written.
 *   out_f          [N][2] f32: classification, bbox_regression          out_i  [N][3] i32: foreground, between, restored
 * (restored: anchors whose best IoU is below 0.5 that the low-quality rule made foreground).  Sums are fp32 in a fixed order --
 * per thread, a fixed tree per workgroup, the workgroups' partials in index order -- and the only atomics are integer maxima:
 * two runs give the same bits.  Refused: L outside [1, 8], A, K < 1, N < 1 or > 65535, a grid or stride < 1, N * A_total or
 * A_total * K or sumT of 2^31 and more, a null pointer, a workspace smaller than cvpce_headloss_workspace_bytes or not 16-byte
 * aligned. */
int cvpce_headloss(const float* const* logits, const float* const* regs, const int* gh, const int* gw, const int* stride_h,
                   const int* stride_w, const float* base_anchors, const float* boxes, const int* labels, const int* box_offsets,
                   const float* scales, int L, int N, int A, int K, int sumT, void* workspace, size_t workspace_bytes, int* matched,
                   float* out_f, int* out_i, void* stream);

#ifdef __cplusplus
}
#endif
#endif
