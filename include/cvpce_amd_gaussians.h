/* cvpce_amd -- scoring the detector's Gaussian maps, NOT part of the inference ABI.
 *
 * The reference judges a checkpoint's Gaussian branch by `gaussian_loss` (cvpce/models/proposals.py:141-160) against maps that
 * `generate_gaussians` (cvpce/datautils.py:18-85) renders from the ground-truth boxes.  Here the targets of a whole batch are
 * rendered and resized in one launch and the loss is found with a radix select instead of a sort.  Same
 * conventions as the other headers: every pointer is a DEVICE pointer unless it says otherwise, a call is asynchronous on
 * `stream` (a hipStream_t passed as void*), performs no allocation and no synchronisation, and returns 0 (CVPCE_OK),
 * 1 (CVPCE_ERR_ARG, bad argument, nothing launched) or 2 (CVPCE_ERR_LAUNCH).  Compiled into the same libcvpce_hip.so, with every
 * fp32 operation rounded on its own (no contraction); the only library function is expf.
 */
#ifndef CVPCE_AMD_GAUSSIANS_H
#define CVPCE_AMD_GAUSSIANS_H
#include <stddef.h>
#ifdef __cplusplus
extern "C" {
#endif

#define CVPCE_GAUSS_TILE 16                   /* a workgroup writes a 16 x 16 tile of one image's output: 256 threads */
#define CVPCE_GAUSS_LIST 256                  /* boxes of one chunk = capacity of a tile's box list in LDS */
#define CVPCE_GAUSS_GEOM 5                    /* ints per image in `geom`: H0, W0, r, h, w */
#define CVPCE_GAUSS_LOSS_THREADS 256
#define CVPCE_GAUSS_LOSS_ITEMS 8              /* elements per thread of a loss workgroup */

/* generate methods (datautils.py:27-63); `params` holds three floats */
#define CVPCE_GAUSS_MULTIVARIATE_NORMAL 0     /* params = peak, variance_scale, - */
#define CVPCE_GAUSS_KANT 1                    /* params unused; `table` [size][size] */
#define CVPCE_GAUSS_SIMPLE_AND_SCALED 2       /* params = minimum, maximum, sigma_divisor */
/* join methods (datautils.py:18-25) */
#define CVPCE_GAUSS_JOIN_MAX 0
#define CVPCE_GAUSS_JOIN_ADDITION 1
#define CVPCE_GAUSS_JOIN_REPLACEMENT 2

/* The kant method's table: out[i][j] = expf(((-4 * ln2) * float((i - c)^2 + (j - c)^2)) / float(sigma * sigma)), c = size / 2,
 * ln2 = 0.6931472f.  out [size][size] f32, every element written.  size in [1, 4096], sigma >= 1. */
int cvpce_gauss_kant_table(float* out, int size, int sigma, void* stream);

/* The target tensor of a batch.
 *
 *   boxes        [sumB][4] i32 (x1, y1, x2, y2 in original pixels), box_offsets [N+1] i32 ascending from 0: image n's boxes, in
 *                index order (an offset is clamped to [0, sumB]).  Both null: every image's source is a map instead --
 *   map_ptrs     [N] i64: the device address of image n's source map [H0/r][W0/r] f32 (contiguous).  Null with boxes.
 *   geom         [N][5] i32: H0, W0 (original size), r (size_reduction >= 1), h, w (output extent).  The source map of an image
 *                has hs = H0 / r rows and ws = W0 / r columns.
 *   table        [table_size][table_size] f32 of cvpce_gauss_kant_table for the kant method, null otherwise
 *   out          [N][Hb][Wb] f32 (= (N,1,Hb,Wb)).  EVERY element is written.
 *   resize       1: out[n][y][x] for y < h, x < w is the bilinear resize (align_corners = False, no antialiasing: two taps per
 *                axis, src = scale * (dst + 0.5) - 0.5 clamped at 0, scale = float(in) / float(out)) of the source map to (h, w);
 *                0: h = hs and w = ws are required and out[n][y][x] is the source pixel itself.
 *                Outside (h, w) an element holds the background value: -1 with `tanh`, else 0.
 * A source pixel starts from the background value; every box of the image, in index order, whose coordinates floor-divided by r
 * (towards minus infinity) cover it after clipping to the map joins its generated value to it (DESIGN.md 4c has the arithmetic).
 * A box with zero reduced width or height, or empty after clipping, contributes nothing.
 * N = 0 or Hb * Wb = 0: nothing to do, 0.  Refused: negative sizes, h > Hb or w > Wb cannot be seen here (geom is on the device: an
 * extent is clamped to the tensor), an unknown method or join, kant without a table, both or neither source, a null pointer. */
int cvpce_gauss_targets(const int* boxes, const int* box_offsets, const long long* map_ptrs, const int* geom, const float* table,
                        int table_size, int sumB, int N, int Hb, int Wb, int method, int join, const float* params /* HOST, 3 floats */,
                        int tanh, int resize, float* out, void* stream);

/* Workspace of cvpce_gauss_loss in bytes (host only, no GPU call); 0 for arguments it would refuse. */
size_t cvpce_gauss_loss_workspace_bytes(int N, int Hb, int Wb);

/* The reference's loss over S segments: S = 1 (per_image = 0: the whole tensor, padding included, `extent` unused and may be
 * null) or S = N (per_image = 1: image n over its rows [0, extent[n][0]) and columns [0, extent[n][1]), clamped to the tensor).
 *
 *   pred, target   [N][Hb][Wb] f32
 *   extent         [N][2] i32
 *   out_f          [S][3] f32: loss, pos_sum, neg_sum          out_i  [S][2] i32: pos_count, neg_count_used
 * Per segment: se = (p - t)^2; positives t >= positive_threshold, negatives t <= negative_threshold; npos, nneg their counts;
 * n = max(min_negatives, negatives_per_positive * npos); m = min(n, nneg) = neg_count_used; neg_sum = the sum of the m largest
 * negative se = sum(se > tau) + (m - count(se > tau)) * tau, tau the m-th largest (radix select on the bit pattern);
 * loss = (pos_sum + neg_sum) / float(npos + m) (0 / 0 = NaN).  All float sums: per-workgroup partials in the workspace, then one
 * pass in index order -- the same bits on every run.  A fixed number of stream operations (one memset, six kernels), no host wait.
 * N * Hb * Wb must be in [1, 2^31).  workspace: 16-byte aligned, at least cvpce_gauss_loss_workspace_bytes(N, Hb, Wb). */
int cvpce_gauss_loss(const float* pred, const float* target, const int* extent, int N, int Hb, int Wb, float negative_threshold,
                     float positive_threshold, int min_negatives, int negatives_per_positive, int per_image, void* workspace,
                     size_t workspace_bytes, float* out_f, int* out_i, void* stream);

#ifdef __cplusplus
}
#endif
#endif
