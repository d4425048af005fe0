/* cvpce_amd -- planogram comparator tail kernels, NOT part of the inference ABI.
 *
 * What follows the common subgraph in the planogram comparator (cvpce/planograms.py: `find_homography` +
 * `finalize_via_ransac`) for a batch of shelf images: a RANSAC homography over the matched boxes' corners and centres, its
 * refit over the inliers, the projection of every expected box and the per-label IoU claim.  Declared apart from
 * include/cvpce_amd_planogram.h, whose entry points are pinned.  Same conventions: every pointer is a DEVICE pointer, every
 * call is asynchronous on `stream` (a hipStream_t passed as void*), performs no allocation and no synchronisation, and returns
 * 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad argument, nothing launched) or 2 (CVPCE_ERR_LAUNCH).  Compiled into the same
 * libcvpce_hip.so.  The arithmetic is the device rule of DESIGN.md 4b ("the tail rule"): fp64 on points and homographies,
 * + - * / sqrt only, every operation rounded on its own, in a fixed order; fp32 for the projection and the IoU.
 *
 * Inputs shared by both calls (B images):
 *   boxes1   [sumN1][4] f32 xyxy, the expected boxes packed back to back, 16-byte aligned; off1 [B+1] i32: image p owns
 *            boxes1[off1[p]] .. boxes1[off1[p+1]-1]
 *   boxes2, off2  the detections, likewise
 *   pairs    [sum_out][2] i32, count [B] i32, out_off [B+1] i32: the matchings as cvpce_planogram_match wrote them -- image p's
 *            count[p] pairs (expected node, actual node) from row out_off[p], in growth order
 *   params   [B][2] f64: {reproj_threshold (pixels), iou_threshold}
 *   seed, hypotheses   the sampler's seed and the number K of hypotheses per image, 1 .. 65536
 *   max_pairs  host-known bound of count[p], 1 .. 1024; max_n1, max_n2: bounds of the box counts, 1 .. 1024
 * All tables are device data: offsets are clamped into their arrays, a count outside 0 .. min(rows, max_pairs), a box count
 * beyond its bound or a pair whose node lies outside its graph gives the image status 2 (invalid) and is never used as an
 * index.
 */
#ifndef CVPCE_AMD_HOMOGRAPHY_H
#define CVPCE_AMD_HOMOGRAPHY_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVPCE_HOMOGRAPHY_MAX_PAIRS 1024
#define CVPCE_HOMOGRAPHY_MAX_HYPOTHESES 65536
#define CVPCE_HOMOGRAPHY_CHUNK 256            /* hypotheses scored by one workgroup */

#define CVPCE_HOMOGRAPHY_OK 0                 /* per-image status */
#define CVPCE_HOMOGRAPHY_NONE 1               /* no homography (too few points, degenerate, fewer than 4 inliers, a non-finite box) */
#define CVPCE_HOMOGRAPHY_INVALID 2            /* the matching is not a valid input */

/* Bytes of workspace for B images and `hypotheses` hypotheses each: one {inlier count, hypothesis} slot per image and chunk of
 * 256 hypotheses.  0 for arguments out of range. */
size_t cvpce_homography_workspace_bytes(int B, int hypotheses);

/* Scores all hypotheses: grid B x chunks, one hypothesis per thread.  Every slot of the workspace is written (no atomics on
 * global memory, nothing needs zeroing before the call).  B = 0: nothing to do, 0; B > 65535 is refused. */
int cvpce_homography_ransac(const float* boxes1, const int* off1, const float* boxes2, const int* off2,
                            const int* pairs, const int* count, const int* out_off, const double* params,
                            int B, int sumN1, int sumN2, int sum_out, int max_pairs, unsigned seed, int hypotheses,
                            void* workspace, size_t workspace_bytes, void* stream);

/* One workgroup per image: picks the winner (highest count, lowest hypothesis at equal counts) from the workspace that
 * cvpce_homography_ransac filled with the same inputs, rebuilds it, refits over its inliers, projects every expected box and
 * runs the per-label claim.
 *
 *   label1 [sumN1], label2 [sumN2] i32: label ids as cvpce_planogram_match takes them (equal id = equal label)
 *   status        [B] i32 out: CVPCE_HOMOGRAPHY_OK / NONE / INVALID
 *   H             [B][9] f64 out: the refit homography, row-major, H[8] = 1
 *   winner, winner_count, final_count  [B] i32 out: the winning hypothesis, its inlier count, the refit's inlier count
 *   matched_expected [sumN1] i32 out, matched_actual [sumN2] i32 out: 0 / 1
 *   expected_positions [sumN1][4] f32 out: every expected box projected through H (rounded to fp32)
 * Every output element is written on every call; an image whose status is not OK gets zeros everywhere else. */
int cvpce_homography_finish(const float* boxes1, const int* label1, const int* off1, const float* boxes2, const int* label2, const int* off2,
                            const int* pairs, const int* count, const int* out_off, const double* params,
                            int B, int sumN1, int sumN2, int sum_out, int max_n1, int max_n2, int max_pairs, unsigned seed, int hypotheses,
                            const void* workspace, size_t workspace_bytes,
                            int* status, double* H, int* winner, int* winner_count, int* final_count,
                            int* matched_expected, int* matched_actual, float* expected_positions, void* stream);

#ifdef __cplusplus
}
#endif
#endif
