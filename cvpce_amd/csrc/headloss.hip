// Scoring the detector's heads (include/cvpce_amd_headloss.h): RetinaNet's anchor matching, focal loss and L1 box loss
// without the (anchors x boxes) IoU matrix.
//
//   headloss_match    one thread per anchor, grid (anchor tile, image).  The image's boxes are staged in LDS in chunks of
//                     CVPCE_HEADLOSS_CHUNK, scaled on load; a thread walks the chunk with its anchor in registers and keeps the largest
//                     IoU and the LOWEST box index that reaches it (strict >).  best[t], the largest IoU of box t over the anchors, is a
//                     maximum of bit patterns (IoUs are >= 0: the unsigned order is the float order): into LDS first and only for
//                     IoU > 0, then one global atomicMax per non-zero entry and workgroup.  Integer maxima: order cannot change them.
//   headloss_terms    the final match of an anchor -- anchors below 0.5 walk the boxes again: the same function on the same operands
//                     gives the bits `best` holds -- then its K focal terms and 4 L1 terms, the workgroup's partial sums and counts.
//   headloss_finish   one workgroup per image adds the partials in index order and divides.
//
// Compiled with -ffp-contract=off: every fp32 operation below is rounded on its own; expf, log1pf and logf are the library calls.
#include "common.h"
#include "anchors.h"
#include "iou.h"
#include "../../include/cvpce_amd_headloss.h"

#define HC CVPCE_HEADLOSS_CHUNK
#define HT CVPCE_HEADLOSS_THREADS
#define HL CVPCE_HEADLOSS_MAX_LEVELS

struct HeadArgs {
    const float* logits[HL];           // [N][gh*gw*A*K]
    const float* regs[HL];             // [N][gh*gw*A][4]
    int gh[HL], gw[HL], sh[HL], sw[HL];
    int first[HL + 1];                 // first anchor of each level; [L] = A_total
    const float* base_anchors;         // [L][A][4]
    const float* boxes;                // [sumT][4]
    const int* labels;                 // [sumT]
    const int* box_offsets;            // [N+1]
    const float* scales;               // [N][2] ratio_h, ratio_w
    int L, N, A, K, sumT, gx;
    unsigned* best;                    // [sumT] IoU bit patterns, zeroed before headloss_match
    float* val;                        // [N][A_total]
    int* arg;                          // [N][A_total]
    float* partial_f;                  // [N][gx][2]
    int* partial_i;                    // [N][gx][3]
};

struct AnchorAt { int level, idx; float4 box; };   // idx: the anchor's index within its level (cell * A + an)

__device__ __forceinline__ AnchorAt anchor_at(const HeadArgs& a, int i) {
    int level = 0;
    while (level + 1 < a.L && i >= a.first[level + 1]) ++level;
    const int idx = i - a.first[level];
    const int cell = idx / a.A, an = idx - cell * a.A;
    const int y = cell / a.gw[level], x = cell - y * a.gw[level];
    return {level, idx, grid_anchor(a.base_anchors, level, a.A, an, x, y, a.sw[level], a.sh[level])};
}

// box b of the packed list in the transformed image of its owner: resize_boxes, one multiply per coordinate
__device__ __forceinline__ float4 scaled_box(const float* __restrict__ boxes, int b, float rh, float rw) {
    const float4 g = *reinterpret_cast<const float4*>(boxes + (size_t)b * 4);
    return make_float4(g.x * rw, g.y * rh, g.z * rw, g.w * rh);
}

// THE IoU of an anchor with a box, in both walks: hg_iou's expression (a pair that does not overlap skips the division: 0 / uni = +0)
__device__ __forceinline__ float pair_iou(float4 anchor, float4 box) {
    const HgIouTerms t = hg_iou_terms(box, anchor);
    return t.inter > 0.f ? __fdiv_rn(t.inter, t.uni) : 0.f;
}

// Nearly all pairs are disjoint, and a disjoint pair's IoU is +0 (one factor of hg_iou_terms' intersection is clamped to 0): both walks
// test this first and evaluate pair_iou -- the same two differences among its operations -- only for the pairs that may overlap.
__device__ __forceinline__ bool may_overlap(float4 anchor, float4 box) {
    return fminf(box.z, anchor.z) - fmaxf(box.x, anchor.x) > 0.f && fminf(box.w, anchor.w) - fmaxf(box.y, anchor.y) > 0.f;
}

__device__ __forceinline__ void image_boxes(const HeadArgs& a, int n, int& b0, int& b1) {
    b0 = min(max(a.box_offsets[n], 0), a.sumT);
    b1 = min(max(a.box_offsets[n + 1], b0), a.sumT);
}

__global__ __launch_bounds__(HT) void headloss_match_kernel(HeadArgs a) {
    __shared__ float4 s_box[HC];
    __shared__ unsigned s_best[HC];
    const int tid = threadIdx.x, n = blockIdx.y, total = a.first[a.L];
    const int i = blockIdx.x * HT + tid;
    const bool live = i < total;
    float4 anchor = make_float4(0.f, 0.f, 0.f, 0.f);
    if (live) anchor = anchor_at(a, i).box;
    int b0, b1;
    image_boxes(a, n, b0, b1);
    const float rh = a.scales[2 * n], rw = a.scales[2 * n + 1];
    // with boxes: box 0 reaches the IoU 0 first and only a larger IoU replaces it; without: -1, below both thresholds
    float val = b1 > b0 ? 0.f : -1.f;
    int arg = b1 > b0 ? 0 : -1;
    for (int base = b0; base < b1; base += HC) {                                       // (b0, b1 are uniform: so are the barriers)
        const int count = min(HC, b1 - base);
        for (int j = tid; j < count; j += HT) {
            s_box[j] = scaled_box(a.boxes, base + j, rh, rw);
            s_best[j] = 0u;
        }
        __syncthreads();
        if (live) {
#pragma unroll 4
            for (int j = 0; j < count; ++j) {
                const float4 box = s_box[j];
                if (!may_overlap(anchor, box)) continue;
                const float iou = pair_iou(anchor, box);
                if (iou > val) { val = iou; arg = base - b0 + j; }
                if (iou > 0.f) {
                    const unsigned bits = __float_as_uint(iou);
                    if (bits > s_best[j]) atomicMax(&s_best[j], bits);                 // (a stale read only costs an atomic: best grows)
                }
            }
        }
        __syncthreads();
        for (int j = tid; j < count; j += HT)
            if (s_best[j]) atomicMax(a.best + base + j, s_best[j]);
        __syncthreads();                                                               // the chunk is rewritten by the next one
    }
    if (live) {
        a.val[(size_t)n * total + i] = val;
        a.arg[(size_t)n * total + i] = arg;
    }
}

// fixed-order sum of one value per thread: the same tree on every run
template <class T>
__device__ __forceinline__ T block_sum(T v, T* sh) {
    const int tid = threadIdx.x;
    __syncthreads();
    sh[tid] = v;
    __syncthreads();
    for (int d = HT / 2; d > 0; d >>= 1) {
        if (tid < d) sh[tid] = sh[tid] + sh[tid + d];
        __syncthreads();
    }
    return sh[0];
}

// one class of one anchor: torchvision's sigmoid_focal_loss, alpha 0.25, gamma 2 (t is 0 or 1)
__device__ __forceinline__ float focal_term(float x, float t) {
    const float p = 1.f / (1.f + expf(-x));
    const float ce = (fmaxf(x, 0.f) - x * t) + log1pf(expf(-fabsf(x)));
    const float p_t = p * t + (1.f - p) * (1.f - t);
    const float alpha_t = 0.25f * t + 0.75f * (1.f - t);
    const float q = 1.f - p_t;
    return alpha_t * (ce * (q * q));
}

__global__ __launch_bounds__(HT) void headloss_terms_kernel(HeadArgs a, int* __restrict__ matched) {
    __shared__ float4 s_box[HC];
    __shared__ unsigned s_best[HC];
    __shared__ float s_f[HT];
    __shared__ int s_i[HT];
    __shared__ int s_zero;                                                             // some box of the image has best == 0
    const int tid = threadIdx.x, n = blockIdx.y, total = a.first[a.L];
    const int i = blockIdx.x * HT + tid;
    const bool live = i < total;
    if (tid == 0) s_zero = 0;
    __syncthreads();
    AnchorAt at = {0, 0, make_float4(0.f, 0.f, 0.f, 0.f)};
    float val = 1.f;                                                                   // (a dead thread walks nothing)
    int arg = -1;
    if (live) {
        at = anchor_at(a, i);
        val = a.val[(size_t)n * total + i];
        arg = a.arg[(size_t)n * total + i];
    }
    int b0, b1;
    image_boxes(a, n, b0, b1);
    const float rh = a.scales[2 * n], rw = a.scales[2 * n + 1];
    const bool below = val < 0.5f;
    bool restored = false;
    for (int base = b0; base < b1; base += HC) {
        const int count = min(HC, b1 - base);
        for (int j = tid; j < count; j += HT) {
            const unsigned best = a.best[base + j];
            s_box[j] = scaled_box(a.boxes, base + j, rh, rw);
            s_best[j] = best;
            if (best == 0u) s_zero = 1;                                                // (only ever set: it holds for the chunks after it too)
        }
        __syncthreads();
        if (live && below) {
            // a box whose best is 0 is disjoint from every anchor of the image: each of them reaches that best (the rule's quirk), and
            // no other disjoint pair can reach a best, which is > 0 -- so only the pairs that may overlap are evaluated
            restored = restored || s_zero != 0;
#pragma unroll 4
            for (int j = 0; j < count; ++j) {
                const float4 box = s_box[j];
                if (may_overlap(at.box, box)) restored = restored || __float_as_uint(pair_iou(at.box, box)) == s_best[j];
            }
        }
        __syncthreads();
    }
    int m = -1;
    if (live) {
        m = !below || restored ? arg : (val >= 0.4f ? -2 : -1);
        matched[(size_t)n * total + i] = m;
    }
    float cls = 0.f, reg = 0.f;
    if (live && m != -2) {
        const int label = m >= 0 ? a.labels[b0 + m] : -1;
        const float* lg = a.logits[at.level] + ((size_t)n * (a.first[at.level + 1] - a.first[at.level]) + at.idx) * a.K;
        for (int k = 0; k < a.K; ++k) cls = cls + focal_term(lg[k], k == label ? 1.f : 0.f);
    }
    if (live && m >= 0) {
        const float4 g = scaled_box(a.boxes, b0 + m, rh, rw);
        const float4 r = *reinterpret_cast<const float4*>(a.regs[at.level] + ((size_t)n * (a.first[at.level + 1] - a.first[at.level]) + at.idx) * 4);
        const float w = at.box.z - at.box.x, h = at.box.w - at.box.y;
        const float cx = at.box.x + 0.5f * w, cy = at.box.y + 0.5f * h;
        const float gw = g.z - g.x, gh = g.w - g.y;
        const float gcx = g.x + 0.5f * gw, gcy = g.y + 0.5f * gh;
        reg = fabsf(r.x - (gcx - cx) / w);
        reg = reg + fabsf(r.y - (gcy - cy) / h);
        reg = reg + fabsf(r.z - logf(gw / w));
        reg = reg + fabsf(r.w - logf(gh / h));
    }
    const float cls_sum = block_sum(cls, s_f), reg_sum = block_sum(reg, s_f);
    const int fg = block_sum((int)(live && m >= 0), s_i), between = block_sum((int)(live && m == -2), s_i);
    const int rest = block_sum((int)(live && below && restored), s_i);
    if (tid == 0) {
        const size_t o = (size_t)n * a.gx + blockIdx.x;
        a.partial_f[2 * o] = cls_sum;
        a.partial_f[2 * o + 1] = reg_sum;
        a.partial_i[3 * o] = fg;
        a.partial_i[3 * o + 1] = between;
        a.partial_i[3 * o + 2] = rest;
    }
}

__global__ __launch_bounds__(HT) void headloss_finish_kernel(HeadArgs a, float* __restrict__ out_f, int* __restrict__ out_i) {
    __shared__ float s_f[HT];
    __shared__ int s_i[HT];
    const int tid = threadIdx.x, n = blockIdx.x;
    float cls = 0.f, reg = 0.f;
    int fg = 0, between = 0, rest = 0;
    for (int g = tid; g < a.gx; g += HT) {                                             // index order per thread, then a fixed tree
        const size_t o = (size_t)n * a.gx + g;
        cls = cls + a.partial_f[2 * o];
        reg = reg + a.partial_f[2 * o + 1];
        fg += a.partial_i[3 * o];
        between += a.partial_i[3 * o + 1];
        rest += a.partial_i[3 * o + 2];
    }
    cls = block_sum(cls, s_f);
    reg = block_sum(reg, s_f);
    fg = block_sum(fg, s_i);
    between = block_sum(between, s_i);
    rest = block_sum(rest, s_i);
    if (tid == 0) {
        const float den = (float)max(1, fg);
        out_f[2 * n] = cls / den;
        out_f[2 * n + 1] = reg / den;
        out_i[3 * n] = fg;
        out_i[3 * n + 1] = between;
        out_i[3 * n + 2] = rest;
    }
}

// workspace: unsigned best[sumT] (padded to 4), float val[N * A_total], int arg[N * A_total], float partial_f[N * gx * 2],
// int partial_i[N * gx * 3]
struct HeadSpace {
    size_t best_bytes, off_val, off_arg, off_pf, off_pi, bytes;
    int first[HL + 1], gx;
};

static bool head_space(const int* gh, const int* gw, int L, int A, int K, int N, int sumT, HeadSpace& s) {
    if (!gh || !gw || L < 1 || L > HL || A < 1 || K < 1 || N < 1 || N > 65535 || sumT < 0) return false;
    long long total = 0;
    for (int l = 0; l < L; ++l) {
        if (gh[l] < 1 || gw[l] < 1) return false;
        s.first[l] = (int)total;
        total += (long long)gh[l] * gw[l] * A;
        if (total * N >= (1LL << 31) || total * K >= (1LL << 31)) return false;
    }
    for (int l = L; l <= HL; ++l) s.first[l] = (int)total;
    s.gx = (int)((total + HT - 1) / HT);
    const size_t per = (((size_t)N * total + 3) & ~(size_t)3) * 4;
    s.best_bytes = (((size_t)sumT + 3) & ~(size_t)3) * 4;
    s.off_val = s.best_bytes;
    s.off_arg = s.off_val + per;
    s.off_pf = s.off_arg + per;
    s.off_pi = s.off_pf + (size_t)N * s.gx * 2 * 4;
    s.bytes = s.off_pi + (size_t)N * s.gx * 3 * 4;
    return true;
}

extern "C" size_t cvpce_headloss_workspace_bytes(const int* gh, const int* gw, int L, int A, int N, int sumT) {
    HeadSpace s;
    return head_space(gh, gw, L, A, 1, N, sumT, s) ? s.bytes : 0;
}

extern "C" int cvpce_headloss(const float* const* logits, const float* const* regs, const int* gh, const int* gw, const int* stride_h,
                              const int* stride_w, const float* base_anchors, const float* boxes, const int* labels, const int* box_offsets,
                              const float* scales, int L, int N, int A, int K, int sumT, void* workspace, size_t workspace_bytes,
                              int* matched, float* out_f, int* out_i, void* stream) {
    HeadSpace s;
    if (!head_space(gh, gw, L, A, K, N, sumT, s)) return CVPCE_ERR_ARG;
    if (!logits || !regs || !stride_h || !stride_w || !base_anchors || !box_offsets || !scales || !matched || !out_f || !out_i) return CVPCE_ERR_ARG;
    if (sumT > 0 && (!boxes || !labels)) return CVPCE_ERR_ARG;
    if (!workspace || ((uintptr_t)workspace & 15) || workspace_bytes < s.bytes) return CVPCE_ERR_ARG;
    HeadArgs a = {};
    for (int l = 0; l < L; ++l) {
        if (!logits[l] || !regs[l] || stride_h[l] < 1 || stride_w[l] < 1) return CVPCE_ERR_ARG;
        a.logits[l] = logits[l]; a.regs[l] = regs[l];
        a.gh[l] = gh[l]; a.gw[l] = gw[l]; a.sh[l] = stride_h[l]; a.sw[l] = stride_w[l];
    }
    for (int l = 0; l <= HL; ++l) a.first[l] = s.first[l];
    a.base_anchors = base_anchors; a.boxes = boxes; a.labels = labels; a.box_offsets = box_offsets; a.scales = scales;
    a.L = L; a.N = N; a.A = A; a.K = K; a.sumT = sumT; a.gx = s.gx;
    char* w = (char*)workspace;
    a.best = (unsigned*)w; a.val = (float*)(w + s.off_val); a.arg = (int*)(w + s.off_arg);
    a.partial_f = (float*)(w + s.off_pf); a.partial_i = (int*)(w + s.off_pi);
    hipStream_t st = (hipStream_t)stream;
    if (s.best_bytes && hipMemsetAsync(a.best, 0, s.best_bytes, st) != hipSuccess) return CVPCE_ERR_LAUNCH;
    const dim3 grid((unsigned)s.gx, (unsigned)N);
    hipLaunchKernelGGL(headloss_match_kernel, grid, dim3(HT), 0, st, a);
    int rc = cvpce_check_launch();
    if (rc != CVPCE_OK) return rc;
    hipLaunchKernelGGL(headloss_terms_kernel, grid, dim3(HT), 0, st, a, matched);
    rc = cvpce_check_launch();
    if (rc != CVPCE_OK) return rc;
    hipLaunchKernelGGL(headloss_finish_kernel, dim3((unsigned)N), dim3(HT), 0, st, a, out_f, out_i);
    return cvpce_check_launch();
}
