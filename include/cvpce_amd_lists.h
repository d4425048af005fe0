/* cvpce_amd -- the fine work lists of the embedder: the entry point that walks a layer's THIN strip list.  A header of its own beside
 * the inference header include/cvpce_amd.h, as include/cvpce_amd_eval.h and include/cvpce_amd_input.h are.  Same conventions: every
 * pointer is a DEVICE pointer, every call is asynchronous on `stream` (hipStream_t, NULL = default stream), returns 0 on success,
 * 1 on a bad argument, 2 on a launch failure.
 *
 * The lists themselves are cvpce_embed_worklists' (include/cvpce_amd.h): a layer with cvpce_skip_layer.skip == 5 gets, beside its
 * list and its STRIP list, a THIN strip list -- its last-row tiles of which only the first 2 conv-output rows are not constant. */
#pragma once
#ifdef __cplusplus
extern "C" {
#endif

/* cvpce_conv3x3_halo_list's companion for a layer's THIN strip list (Cout > 128 only): FOUR listed tiles with `rows` == 2 are computed
 * as one tile -- patch rows 4 s .. 4 s + 3 and accumulator rows 2 s, 2 s + 1 belong to strip s, patch rows 16 and 17 to no strip; all
 * four share every weight fragment.  Same operands, argument checks and partial-write contract as cvpce_conv3x3_halo_strips: it writes
 * the strips' 2 rows (with fuse_pool2: their one pooled row) into the same `out` (and `mac`) the layer's other launches write into,
 * and nothing else. */
int cvpce_conv3x3_halo_strips2(const void* in, const void* wgt, const float* bias, void* out, float* mac, int mac_stride,
                               int mac_off, int N, int H, int W, int Cin, int Cout, int K_pad, int Cout_pad, int relu,
                               int fuse_pool2, const unsigned long long* thin_list, const int* count_dev, void* stream);

#ifdef __cplusplus
}
#endif
