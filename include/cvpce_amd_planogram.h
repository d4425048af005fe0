/* cvpce_amd -- planogram comparator kernels, NOT part of the inference ABI.
 *
 * The two graph stages of the planogram comparator (cvpce/planograms.py:30-132: `build_graph`, `build_hypotheses` +
 * `large_common_subgraph`) for a batch of shelf images.  Declared apart from include/cvpce_amd.h for the reason
 * include/cvpce_amd_eval.h is.  Same conventions: every pointer is a DEVICE pointer, every call is asynchronous on `stream`
 * (a hipStream_t passed as void*), performs no allocation and no synchronisation, and returns 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG,
 * bad argument, nothing launched) or 2 (CVPCE_ERR_LAUNCH).  Compiled into the same libcvpce_hip.so.
 */
#ifndef CVPCE_AMD_PLANOGRAM_H
#define CVPCE_AMD_PLANOGRAM_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVPCE_PLANOGRAM_MAX_NODES 1024

/* 8-direction nearest-neighbour graphs of B box sets in one launch, one workgroup per graph ("the device rule").
 *
 *   boxes    [sumN][4] f32 xyxy, the graphs' boxes packed back to back, 16-byte aligned
 *   offsets  [B+1] i32, graph b owns boxes offsets[b] .. offsets[b+1]-1
 *   thresh   [B] f32: graph b's distance threshold, `thresh_size * span` computed by the caller with build_graph's own expression
 *   min_n, max_n  host-known bounds of the per-graph node counts: 1 <= min_n <= max_n <= 1024 or the call is refused.  (The
 *            offsets are device data: a graph whose count is outside 1 .. max_n is not a valid input; its workgroup writes nothing.)
 *   nbr      [sumN][8] i32 out: per node and direction slot (E NE N NW W SW S SE; y as given) the neighbour's index LOCAL to its
 *            graph, or -1
 *   weight   [sumN][8] f32 out: the edge's distance, 0 in an empty slot
 *   stamp    [sumN][8] i32 out: insertion stamp from a per-graph counter starting at 0, -1 in an empty slot.  The adjacency
 *            order of a node (networkx: edge insertion order) is its filled slots by ascending stamp; a slot that was emptied
 *            and filled again carries the later stamp.
 *   Every slot of every node is written.
 *
 * The rule: centre = ((x0+x2)/2, (y0+y3)/2) in fp32; d(i,j) = sqrt(dx*dx + dy*dy), every operation rounded on its own, the root
 * correctly rounded; node i = 0 .. n-1 in turn walks the other nodes in ascending (d, j) and stops at d > thresh or when its
 * eight slots are filled; a pair at d = 0 has no direction and is skipped; the 8-way sector of i -> j is decided by comparing
 * |dy| with tan(pi/8)|dx| and tan(3pi/8)|dx| (it equals the host's acos sector except within rounding of a sector boundary);
 * a candidate whose slot at i is filled is skipped; so is one that already has a neighbour on i's side at weight <= d; a
 * farther such neighbour is unlinked in both directions first.  B = 0: nothing to do, 0. */
int cvpce_planogram_graphs(const float* boxes, const int* offsets, const float* thresh, int B, int sumN, int min_n, int max_n,
                           int* nbr, float* weight, int* stamp, void* stream);

/* Bytes of workspace cvpce_planogram_match needs for `hypotheses` seed pairs in all (the sum over the pairs of the number of
 * equal-label node pairs); 0 for a negative count. */
size_t cvpce_planogram_match_workspace_bytes(long long hypotheses);

/* Hypothesis-seeded common subgraph of P (expected, actual) graph pairs in one launch, one workgroup per pair: exactly
 * `build_hypotheses` + `large_common_subgraph` over graphs in the table form above.
 *
 *   nbr1, stamp1 [sumN1][8] i32, label1 [sumN1] i32, off1 [P+1] i32: the expected graphs, packed; pair p's is off1[p] .. off1[p+1]-1
 *   nbr2, stamp2, label2, off2: the actual graphs.  Label ids are >= 0; equal id = equal label.
 *   params   [P][2] i32: {min_agree, enough_floor}.  A hypothesis whose agree count (directions present at both nodes whose
 *            neighbours carry equal labels) is below min_agree has score > min_score; enough_floor = floor(min(n1,n2) * stop_at_fraction).
 *   hyp_off  [P+1] i32: pair p's slice of `workspace`, in hypotheses; its length is at least the number of equal-label node pairs
 *   out_off  [P+1] i32: pair p's rows of `pairs`; at least min(n1, n2) of them
 *   max_n1, max_n2  host-known bounds of the node counts, 1 .. 1024 (a graph outside 0 .. max is not a valid input: count 0)
 *   workspace, workspace_bytes  at least cvpce_planogram_match_workspace_bytes(hyp_off[P]); contents are scratch
 *   pairs    [out_off[P]][2] i32 out: the matching of pair p, (expected node, actual node), in the order it grew, from row
 *            out_off[p]; the rows beyond count[p] are -1.  Every row is written.
 *   count    [P] i32 out
 *
 * Hypotheses are visited by (agree descending, n1, n2); each grows first-in-first-out, steps appended in the order of n1's
 * adjacency (ascending stamp), the partner being n2's neighbour in the same direction if its label is equal; a popped pair with
 * a used side is skipped.  The first hypothesis that grows beyond enough_floor pairs is the result; a hypothesis below
 * min_agree ends the search if some set was kept; otherwise the strictly larger set is kept.  Neighbour indices outside their
 * graph are read as -1, and every loop is bounded by the table sizes.  P = 0: nothing to do, 0. */
int cvpce_planogram_match(const int* nbr1, const int* stamp1, const int* label1, const int* off1,
                          const int* nbr2, const int* stamp2, const int* label2, const int* off2,
                          const int* params, const int* hyp_off, const int* out_off,
                          int P, int sumN1, int sumN2, int max_n1, int max_n2, int sum_out, long long sum_hyp,
                          void* workspace, size_t workspace_bytes, int* pairs, int* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
