// What the two 3x3 halo kernels share (conv3x3_halo2.hip: 16 x 16-pixel tiles, Cout > 128; conv3x3_halo3.hip: 16 x 32-pixel tiles,
// Cout <= 128 and the thin fp32-output form): the host's plan of a launch -- argument validation, the common kernel arguments, the
// grid rule, the launch itself -- and the few device functions that are the same in both.  The K loops, the row-streaming macros,
// the patch DMA and the store paths differ in geometry and stay in their files.
#pragma once
#include "common.h"
#include "worklist.h"
#include <type_traits>

// ---------------------------------------------------------------- host ----------------------------------------------------------------

struct HaloShape { int N, H, W, Cin, Cout, K_pad, Cout_pad; };

// where the dispatchers differ in what they accept
struct HaloRules {
    int tile_w;             // pixel tile: 16 rows x tile_w columns
    int cout_tile;          // couts per workgroup; 0: one cout tile whatever Cout is (the thin form)
    long long max_chunks;   // (pixel tiles x cout tiles x 64-channel chunks) of the launch stays below this: the kernels count them in an int
    bool cout_mult8;        // 16-byte stores of 8 couts; the thin form stores fp32 element by element where it must
    int cout_max;           // 0: none
};

// the conditions every halo launch shares; tiles_per_image: of a tile map, 0 = all tiles of the image; list: a work-list launch, whose
// shape must fit the entry format (worklist.h)
static inline bool halo_shape_ok(const void* in, const void* wgt, const HaloShape& s, int fuse_pool2, int tiles_per_image, bool list,
                                 const HaloRules& r) {
    if (!in || !wgt) return false;
    if (s.H <= 0 || s.W <= 0 || s.Cin % 64 != 0 || s.Cin <= 0 || s.Cout <= 0) return false;
    if ((r.cout_mult8 && s.Cout % 8 != 0) || (r.cout_max && s.Cout > r.cout_max)) return false;
    if (fuse_pool2 && ((s.H & 1) || (s.W & 1))) return false;
    if (s.K_pad != 9 * s.Cin || s.Cout_pad % 256 != 0 || s.Cout_pad < s.Cout) return false;
    // 32-bit byte offsets into the input (buffer loads), 32-bit element indices of the output, a 31-bit weight buffer
    if ((long long)s.N * s.H * s.W * s.Cin * 2 >= (1LL << 32) || (long long)s.N * s.H * s.W * s.Cout >= (1LL << 31)) return false;
    if ((long long)s.Cout_pad * s.K_pad * 2 >= (1LL << 31)) return false;
    if (list && !wl_fits(s.N, s.H, s.W, r.tile_w)) return false;
    const long long tpi = tiles_per_image ? tiles_per_image : (long long)((s.W + r.tile_w - 1) / r.tile_w) * ((s.H + 15) / 16);
    const long long ctiles = r.cout_tile ? (s.Cout + r.cout_tile - 1) / r.cout_tile : 1;
    return s.N * tpi * ctiles * (s.Cin / 64) < r.max_chunks;
}

// the fields Halo2Args and Halo3Args have in common (ctiles / ntiles are the launch function's)
template <typename Args>
static inline void halo_fill(Args& a, const void* in, const void* wgt, const float* bias, void* out, const HaloShape& s, int relu, int tile_w,
                             const unsigned long long* list, const int* list_count) {
    a.in = (const bf16_t*)in; a.wgt = (const bf16_t*)wgt; a.bias = bias; a.out = (bf16_t*)out;
    a.N = s.N; a.H = s.H; a.W = s.W; a.Cin = s.Cin; a.Cout = s.Cout; a.K_pad = s.K_pad; a.relu = relu; a.cgroups = s.Cout_pad / 32;
    a.tiles_x = (s.W + tile_w - 1) / tile_w; a.tiles_y = (s.H + 15) / 16; a.ptiles = s.N * a.tiles_x * a.tiles_y;
    a.in_bytes = (unsigned)((long long)s.N * s.H * s.W * s.Cin * 2);
    a.wgt_bytes = (unsigned)((long long)s.Cout_pad * s.K_pad * 2);
    a.ctiles = a.ntiles = 0;
    a.list = list; a.list_count = list_count;
}

// persistent grid: a workgroup per tile up to the cap; work-list launches take the same number of workgroups for every cout tile
static inline int halo_grid(int ntiles, int ctiles, bool list) {
    const int grid = ntiles < g_cvpce_persistent_wgs ? ntiles : g_cvpce_persistent_wgs;
    if (!list) return grid;
    return grid < ctiles ? ctiles : grid / ctiles * ctiles;
}

// smem_max: the most dynamic LDS any launch of this instance asks for, where launches differ (the attribute is set once per
// instance and device)
template <auto Kernel, typename Args>
static inline int halo_launch(const Args& a, int grid, int threads, int smem, hipStream_t stream, int smem_max = 0) {
    if (!cvpce_smem_attr_done<Kernel>((const void*)Kernel, smem_max ? smem_max : smem)) return CVPCE_ERR_LAUNCH;
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(threads), smem, stream, a);
    return cvpce_check_launch();
}

// run-time flags -> template arguments: halo_pick(f, b0, b1, ...) calls f(std::bool_constant<b0>{}, std::bool_constant<b1>{}, ...)
template <bool... Bs, typename F>
static inline int halo_pick(F&& f) { return f(std::bool_constant<Bs>{}...); }
template <bool... Bs, typename F, typename... Rest>
static inline int halo_pick(F&& f, bool b, Rest... rest) {
    return b ? halo_pick<Bs..., true>(f, rest...) : halo_pick<Bs..., false>(f, rest...);
}

// --------------------------------------------------------------- device ---------------------------------------------------------------

// pixel column of MFMA pixel lane l16: lanes {0-3, 12-15} hold the even columns, {4-11} the odd ones (conflict-free fragment reads
// under both kernels' patch swizzles; the pooled exchange below relies on it)
__device__ __forceinline__ int halo_col(int l16) { return l16 < 4 ? 2 * l16 : (l16 >= 12 ? 2 * (l16 - 8) : 2 * (l16 - 4) + 1); }

// lane id from the exec mask: 2 VALU ops where it is needed instead of a VGPR held across the K loop; being volatile it also keeps
// what is computed from it inside the loop it is called in
__device__ __forceinline__ int halo_lane_id() {
    int ln;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(ln));
    return ln;
}

// plain launches: workgroup lbid computes tiles lbid, lbid + grid, ... (all tiles cost the same)
__device__ __forceinline__ int halo_plain_tiles(int ntiles, int lbid, int grid) { return (ntiles - lbid + grid - 1) / grid; }

// LIST launches: a CONTIGUOUS block of the list per workgroup -- listed tiles differ in cost when they are cut at `rows`, and the list
// is crop-major with a fixed number of tiles per crop, so a stride that is a multiple of it would hand one workgroup nothing but
// bottom-row (cut) tiles and another nothing but full ones.  The cout tile stays fixed per workgroup (lbid % ctiles: one weight set
// per workgroup, and with an even grid per XCD); the grid / ctiles workgroups of a cout tile (the host launches grid % ctiles == 0)
// split the list among them.  Returns the workgroup's tiles, first = its first.  (conv3x3_halo2.hip spells the same out, with
// three entries to a tile in its STRIP mode: see there)
__device__ __forceinline__ int halo_list_span(int units, int grid, int ctiles, int lbid, int& first) {
    const int groups = grid / ctiles;
    const int per = (units + groups - 1) / groups;
    first = (lbid / ctiles) * per;
    return units - first < per ? units - first : per;
}

// fused MaxPool2d(2,2): r0, r1 are one accumulator element of output rows 2i, 2i+1 of this lane's column.  Columns 2k, 2k+1 are lanes
// A[k], B[k] with A = {0-3,12-15}, B = {4-11} (halo_col): lane A[k] takes its right neighbour by a row rotate (+4 for lanes 0-3, -4 for
// lanes 12-15; bank masks 1 and 8).  The result is valid in the A lanes.  After ReLU the values order like their bit patterns
__device__ __forceinline__ float halo_pool2x2(float r0, float r1, int relu) {
    if (relu) {
        const unsigned v = max(__float_as_uint(relu_bits(r0)), __float_as_uint(relu_bits(r1)));
        unsigned m = max(v, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x12C, 0xF, 0x1, false));   // row_ror:12 -> lane l reads l+4
        m = max(m, (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x124, 0xF, 0x8, false));            // row_ror:4  -> lane l reads l-4
        return __uint_as_float(m);
    }
    const float v = fmaxf(r0, r1);
    const float up = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x12C, 0xF, 0x1, false));
    const float dn = __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x124, 0xF, 0x8, false));
    return fmaxf(v, fmaxf(up, dn));
}
