/* cvpce_amd -- classification evaluation kernel, NOT part of the inference ABI.
 *
 * The comparison at the end of the embed + match accuracy harness (cvpce/classification_eval.py:28-42: `a1 in a2[:knn]` and
 * `a1 != a2[0]` over label strings) for a window of ground-truth boxes, on label ids: per box, the rank of the first neighbour
 * that carries the wanted label, and the label of the nearest neighbour.  Every knn's count and the confusion table follow from
 * these two numbers on the host.  Declared apart from include/cvpce_amd_reclass.h, whose verdict reads the nearest neighbour
 * alone.  Same conventions: every pointer is a DEVICE pointer, the call is asynchronous on `stream` (a hipStream_t passed as
 * void*), performs no allocation and no synchronisation, and returns 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad argument, nothing
 * launched) or 2 (CVPCE_ERR_LAUNCH).  Compiled into the same libcvpce_hip.so.  Integers only; no atomics, so the output does not
 * depend on scheduling.
 */
#ifndef CVPCE_AMD_CLASSEVAL_H
#define CVPCE_AMD_CLASSEVAL_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVPCE_CLASSEVAL_THREADS 256           /* four waves: four query rows per workgroup */

/* The first rank of the wanted label, and the nearest neighbour's label.
 *
 *   indices           [Q][K] i64, 8-byte aligned: the match result (gallery rows, nearest first), K = min(k, G) >= 1
 *   gallery_label_id  [G] i32: every gallery row's label id (equal id = equal label), G >= 1
 *   want              [Q] i32: the wanted label id of every query row; negative = a label no gallery item has
 *   records           [Q][2] i32 out, 8-byte aligned (a record is stored as one pair)
 * For every query row q (one wave each: lanes stride over K, then a wave minimum):
 *   records[q][0] = the smallest j in [0, K) with 0 <= indices[q][j] < G and gallery_label_id[indices[q][j]] == want[q] >= 0;
 *                   K where there is none
 *   records[q][1] = gallery_label_id[indices[q][0]]; -1 where indices[q][0] lies outside [0, G)
 * An index outside [0, G) reads nothing and matches nothing.  Every element of `records` is written, nothing else is.
 * Q = 0: nothing to do, 0.  K < 1, Q < 0 and G < 1 are refused, as is a null or misaligned pointer where Q > 0. */
int cvpce_classeval_rank(const long long* indices, const int* gallery_label_id, const int* want, int Q, int K, int G, int* records,
                         void* stream);

#ifdef __cplusplus
}
#endif
#endif
