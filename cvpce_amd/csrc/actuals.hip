// A window's detections as the comparator's actual side, on the device (include/cvpce_amd_actuals.h; the rule of DESIGN.md 4b):
// which of the detector's confident boxes are kept, and the kept boxes packed with their gallery rows, label ids and thresholds.
//
//   actuals_count_kernel   one workgroup per image: the number of non-degenerate boxes of the image's prefix, an integer tree
//   actuals_pack_kernel    one workgroup per image: the kept boxes written densely IN SLOT ORDER -- per-wave ballots, a prefix over the
//                          four waves, a running base over the chunks of 256 slots, as reclass_plan_kernel has it -- and the four
//                          extremes of the kept boxes reduced by max / min, whose result does not depend on the order; no atomics
//
// Compiled with -ffp-contract=off like its neighbours: the three additions, the division and the product of the threshold are
// `planograms_device.graph_threshold`'s, each rounded on its own.
#include "common.h"
#include "../../include/cvpce_amd_actuals.h"

#define AC_THREADS CVPCE_ACTUALS_THREADS
#define AC_WAVES (AC_THREADS / WAVE)

// production._nondegenerate on one box: `.to(torch.long)` truncates toward zero; the differences are integer differences
__device__ __forceinline__ bool ac_kept(const float4 b) {
    const float lim = 4611686018427387904.f;                                    // 2^62: the differences below cannot overflow
    if (!(fabsf(b.x) < lim && fabsf(b.y) < lim && fabsf(b.z) < lim && fabsf(b.w) < lim)) return false;       // (false on NaN)
    const long long x0 = (long long)b.x, y1 = (long long)b.y, x2 = (long long)b.z, y3 = (long long)b.w;
    return (x2 - x0 > 0) && (y3 - y1 > 0);
}

__global__ __launch_bounds__(AC_THREADS) void actuals_count_kernel(
    const float4* __restrict__ boxes, const int* __restrict__ count, int per, int* __restrict__ kept) {
    __shared__ int s_sum[AC_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int c = min(max(count[p], 0), per);
    const size_t row0 = (size_t)p * per;
    int sum = 0;
    for (int j = tid; j < c; j += AC_THREADS) sum += ac_kept(boxes[row0 + j]) ? 1 : 0;
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) sum += __shfl_down(sum, d, WAVE);
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (tid == 0) {
        int total = 0;
#pragma unroll
        for (int w = 0; w < AC_WAVES; ++w) total += s_sum[w];
        kept[p] = total;
    }
}

__global__ __launch_bounds__(AC_THREADS) void actuals_pack_kernel(
    const float4* __restrict__ boxes, const int* __restrict__ count, const long long* __restrict__ indices, int k,
    const int* __restrict__ gallery_label_id, int G, const int* __restrict__ off2, float thresh_size, int per, int sum2,
    float4* __restrict__ out_boxes, int* __restrict__ out_row, int* __restrict__ out_label, float* __restrict__ thresh,
    int* __restrict__ status) {
#pragma clang fp contract(off)
    __shared__ int s_wave[AC_WAVES];
    __shared__ int s_bad[AC_WAVES];
    __shared__ float s_ext[4][AC_WAVES];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid / WAVE;
    const int c = min(max(count[p], 0), per);
    // the offsets are device data: clamped into the output, and the image's rows are a capacity
    const int o0 = off2[p], o1 = off2[p + 1];
    const int a0 = min(max(o0, 0), sum2), a1 = min(max(o1, a0), sum2);
    const int cap = a1 - a0;
    const size_t row0 = (size_t)p * per;
    float mx2 = -INFINITY, mn0 = INFINITY, my3 = -INFINITY, mn1 = INFINITY;
    int base = 0, bad = 0;
    for (int c0 = 0; c0 < c; c0 += AC_THREADS) {                               // (uniform: barriers inside)
        const int j = c0 + tid;
        bool valid = false;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j < c) {
            b = boxes[row0 + j];
            valid = ac_kept(b);
        }
        const unsigned long long ballot = __ballot(valid);
        if (lane == 0) s_wave[wave] = __popcll(ballot);
        __syncthreads();
        int before = base, total = 0;
#pragma unroll
        for (int w = 0; w < AC_WAVES; ++w) {
            const int n = s_wave[w];
            before += w < wave ? n : 0;
            total += n;
        }
        if (valid) {
            mx2 = fmaxf(mx2, b.z);
            mn0 = fminf(mn0, b.x);
            my3 = fmaxf(my3, b.w);
            mn1 = fminf(mn1, b.y);
            const long long r = indices[(row0 + j) * (size_t)k];
            const bool in = r >= 0 && r < (long long)G;
            bad |= in ? 0 : 1;
            const int slot = before + __popcll(ballot & ((1ull << lane) - 1ull));
            if (slot < cap) {
                out_boxes[(size_t)a0 + slot] = b;
                out_row[(size_t)a0 + slot] = in ? (int)r : -1;
                out_label[(size_t)a0 + slot] = in ? gallery_label_id[r] : 0;
            }
        }
        base += total;
        __syncthreads();
    }
    // max and min of finite values: any order gives the same value (a kept box is wider and higher than 0, so no extreme is a zero
    // whose sign could differ)
#pragma unroll
    for (int d = WAVE / 2; d > 0; d >>= 1) {
        mx2 = fmaxf(mx2, __shfl_down(mx2, d, WAVE));
        mn0 = fminf(mn0, __shfl_down(mn0, d, WAVE));
        my3 = fmaxf(my3, __shfl_down(my3, d, WAVE));
        mn1 = fminf(mn1, __shfl_down(mn1, d, WAVE));
    }
    const int any_bad = __ballot(bad != 0) != 0ull ? 1 : 0;
    if (lane == 0) {
        s_ext[0][wave] = mx2;
        s_ext[1][wave] = mn0;
        s_ext[2][wave] = my3;
        s_ext[3][wave] = mn1;
        s_bad[wave] = any_bad;
    }
    __syncthreads();
    if (tid == 0) {
        int flag = 0;
#pragma unroll
        for (int w = 0; w < AC_WAVES; ++w) {
            mx2 = fmaxf(mx2, s_ext[0][w]);
            mn0 = fminf(mn0, s_ext[1][w]);
            my3 = fmaxf(my3, s_ext[2][w]);
            mn1 = fminf(mn1, s_ext[3][w]);
            flag |= s_bad[w];
        }
        if (base > 0) {
            const float span = (((mx2 - mn0) + my3) - mn1) / 2.f;
            thresh[p] = thresh_size * span;
        }
        status[p] = flag ? 2 : ((long long)base != (long long)o1 - (long long)o0 ? 1 : 0);
    }
}

static bool ac_common_ok(const float* boxes, const int* count, int B, int per) {
    if (B < 0 || B > 65535 || per < 1) return false;
    if (B == 0) return true;
    return boxes && count && !((uintptr_t)boxes & 15);
}

extern "C" int cvpce_actuals_count(const float* boxes, const int* count, int B, int per, int* kept, void* stream) {
    if (!ac_common_ok(boxes, count, B, per)) return CVPCE_ERR_ARG;
    if (B == 0) return CVPCE_OK;
    if (!kept) return CVPCE_ERR_ARG;
    hipLaunchKernelGGL(actuals_count_kernel, dim3((unsigned)B), dim3(AC_THREADS), 0, (hipStream_t)stream, (const float4*)boxes, count, per, kept);
    return cvpce_check_launch();
}

extern "C" int cvpce_actuals_pack(const float* boxes, const int* count, const long long* indices, int k, const int* gallery_label_id, int G,
                                  const int* off2, float thresh_size, int B, int per, int sum2, float* out_boxes, int* out_row, int* out_label,
                                  float* thresh, int* status, void* stream) {
    if (!ac_common_ok(boxes, count, B, per)) return CVPCE_ERR_ARG;
    if (k < 1 || G < 0 || sum2 < 0) return CVPCE_ERR_ARG;
    if (B == 0) return CVPCE_OK;
    if (!indices || ((uintptr_t)indices & 7) || (G > 0 && !gallery_label_id) || !off2 || !thresh || !status) return CVPCE_ERR_ARG;
    if (sum2 > 0 && (!out_boxes || !out_row || !out_label)) return CVPCE_ERR_ARG;
    if ((uintptr_t)out_boxes & 15) return CVPCE_ERR_ARG;
    hipLaunchKernelGGL(actuals_pack_kernel, dim3((unsigned)B), dim3(AC_THREADS), 0, (hipStream_t)stream, (const float4*)boxes, count, indices, k,
                       gallery_label_id, G, off2, thresh_size, per, sum2, (float4*)out_boxes, out_row, out_label, thresh, status);
    return cvpce_check_launch();
}
