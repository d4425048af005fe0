/* cvpce_amd -- planogram comparator, Tonioni's matcher: NOT part of the inference ABI.
 *
 * The second graph matcher of the planogram comparator (cvpce/planograms.py:134-169, `tonioni_mcs`) for a batch of (expected,
 * actual) graph pairs: the opt-in alternative to cvpce_planogram_match, with the same inputs (minus the stamps, which this search
 * never reads) and the same outputs, so everything behind the matching takes it as it is (the Tonioni rule of DESIGN.md 4b).
 * Same conventions as the headers of include/: every pointer is a DEVICE pointer, every call is asynchronous on `stream` (a
 * hipStream_t passed as void*), performs no allocation and no synchronisation, and returns 0 (CVPCE_OK), 1 (CVPCE_ERR_ARG, bad
 * argument, nothing launched) or 2 (CVPCE_ERR_LAUNCH).  Compiled into the same libcvpce_hip.so.  Integers only.
 *
 * This header lies in include/ext/ because the ABI mirror test pins the set of headers directly under include/ and their entry
 * point counts; a later change that is free to edit that test folds it into include/ (with its table in `_lib.HEADERS` and its
 * op module in the test's registry) without touching a declaration.
 *
 * The rule.  The hypotheses of a pair are its equal-label node pairs ordered by (agree descending, n1, n2), exactly
 * cvpce_planogram_match's.  The run from start i plays the suffix i.. to its end: the smallest (score8, n1, n2) is taken, where
 * score8 = -agree - 8 * bumps; the run ends when nothing is left or that score8 is above the pair's limit; every hypothesis
 * sharing n1 or n2 with the taken one dies; every survivor (x1, x2) with nbr1[n1][d] == x1 and nbr2[n2][d] == x2 for some
 * direction slot d is bumped once; bound = pairs taken so far + the number of survivors that are both the first survivor with
 * their x1 and the first with their x2, "first" in the order BEFORE this step's bumps; the next head is chosen AFTER them.
 * F_i is the run's size and M_i the minimum of its bounds (INT_MAX if it took no pair).  The choice: best = 0; for i = 0 ..
 * H-1: stop if best > H - i; if M_i >= best and F_i > best, start i is adopted and best = F_i.  The bound is the size of one
 * greedy matching, not an upper bound, so the test on M cannot be dropped: it changes results.
 */
#ifndef CVPCE_AMD_TONIONI_H
#define CVPCE_AMD_TONIONI_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

/* The most hypotheses one pair may have: a run keeps one 32-bit key per hypothesis in LDS, beside two 32-bit tables of max_n1 and
 * max_n2 entries, and the launch is sized by the call's declared maxima: 4 * (max_hyp + max_n1 + max_n2) bytes and 32 static
 * ones.  At this limit with 1024-node graphs that is 73 760 bytes: two workgroups of 256 threads on a CU's 160 KiB.  A shelf of
 * 200 positions in 3 labels (11 640 hypotheses) takes 48 192 bytes: three workgroups.  The compiler's own figures for the run
 * kernel (-Rpass-analysis=kernel-resource-usage, gfx950): 26 vector and 102 scalar registers, no spill, no scratch, 32 bytes of
 * static LDS, occupancy 7 waves per SIMD by registers -- the LDS decides (2 or 3 workgroups = 2 or 3 waves per SIMD). */
#define CVPCE_TONIONI_MAX_HYPOTHESES 16384

/* Bytes of workspace both calls need for `hypotheses` seed pairs in all (hyp_off[P]) and P pairs: int32 words -- the hypotheses
 * [hypotheses], then (M, F) per start [hypotheses][2], then the pairs' hypothesis counts [P].  0 for a negative argument. */
size_t cvpce_tonioni_workspace_bytes(long long hypotheses, int P);

/* The runs: two launches, the hypotheses (one workgroup per pair) and the runs (one workgroup per pair and start; those beyond a
 * pair's real hypothesis count exit at once).
 *
 *   nbr1 [sumN1][8] i32, label1 [sumN1] i32, off1 [P+1] i32; nbr2, label2, off2: the graphs as cvpce_planogram_match takes them
 *   params   [P] i32: the pair's score8 limit, the largest integer t for which t / 8 is not above min_score
 *   hyp_off  [P+1] i32 ascending: pair p's slice of the workspace's per-hypothesis parts; at least as long as the number of its
 *            equal-label node pairs (a longer slice is a bound: the kernel counts) and at most max_hyp
 *   max_n1, max_n2  host-known bounds of the node counts, 1 .. 1024; max_hyp: of the slice lengths, 0 .. CVPCE_TONIONI_MAX_HYPOTHESES
 *            (more: CVPCE_ERR_ARG).  A pair outside these bounds is not a valid input: no hypotheses, count 0.
 *   workspace, workspace_bytes  at least cvpce_tonioni_workspace_bytes(sum_hyp, P), sum_hyp = hyp_off[P]; written: the hypotheses
 *            and (M, F) of every start below the pair's count, and all P counts.
 * All tables are device data: offsets are clamped into their arrays and every index read from memory is range-checked. */
int cvpce_tonioni_run(const int* nbr1, const int* label1, const int* off1, const int* nbr2, const int* label2, const int* off2,
                      const int* params, const int* hyp_off, int P, int sumN1, int sumN2, int max_n1, int max_n2,
                      int max_hyp, long long sum_hyp, void* workspace, size_t workspace_bytes, void* stream);

/* The choice and the result: one launch, one workgroup per pair, on the workspace as cvpce_tonioni_run left it (the same tables
 * and bounds).
 *
 *   out_off  [P+1] i32: pair p's rows of `pairs`; at least min(n1, n2) of them
 *   pairs    [sum_out][2] i32 out: the adopted run's pairs, (expected node, actual node), in the order they were taken, from row
 *            out_off[p]; the rows beyond count[p] are -1.  Every row is written.
 *   count    [P] i32 out
 * The layout of cvpce_planogram_match's outputs.  The workspace is only read. */
int cvpce_tonioni_select(const int* nbr1, const int* off1, const int* nbr2, const int* off2, const int* params,
                         const int* hyp_off, const int* out_off, int P, int sumN1, int sumN2, int max_n1, int max_n2,
                         int max_hyp, int sum_out, long long sum_hyp, const void* workspace, size_t workspace_bytes,
                         int* pairs, int* count, void* stream);

#ifdef __cplusplus
}
#endif
#endif
