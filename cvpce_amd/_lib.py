"""ctypes binding of the C ABI of libcvpce_hip.so: one signature table per header of include/, in `HEADERS` (include/ext/: in
`EXTENSION_HEADERS` and `PICTURE_EXTENSION_HEADERS`).

The HIP library is the product: there is NO CPU fallback.  Importing this
module without a built `libcvpce_hip.so` raises immediately (build it with
`python -c "import __graft_entry__ as g; g.build()"` or `make -C cvpce_amd/csrc`).
"""
import ctypes
import os
from ctypes import c_int, c_float, c_void_p, c_size_t, c_longlong, POINTER

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('CVPCE_LIB') or os.path.join(_HERE, 'libcvpce_hip.so')   # CVPCE_LIB: dev-only A/B builds


class HipLibraryMissing(ImportError):
    pass


if not os.path.exists(LIB_PATH):
    raise HipLibraryMissing(
        f'{LIB_PATH} not found: the cvpce_amd hot path has no CPU fallback. '
        'Build the HIP library first (python -c "import __graft_entry__ as g; g.build()").')

lib = ctypes.CDLL(LIB_PATH)

_vp = c_void_p
_fp = c_void_p   # float* passed as raw device address
_ip = c_void_p

SIGNATURES = {
    'cvpce_conv2d_nhwc_bf16': (c_int, [_vp, _vp, _fp, _vp, _vp] + [c_int] * 21 + [_vp]),
    'cvpce_conv2d_splitk_bf16': (c_int, [_vp, _vp, _fp, _vp, _vp] + [c_int] * 20 + [_vp, c_size_t, _vp]),
    'cvpce_conv2d_splitk_workspace_bytes': (c_size_t, [c_longlong, c_int, c_int]),
    'cvpce_set_persistent_workgroups': (c_int, [c_int]),
    'cvpce_conv1x1_nhwc_bf16': (c_int, [_vp, _vp, _fp, _vp, _vp] + [c_int] * 14 + [_vp]),
    'cvpce_vgg_stem_fused': (c_int, [_vp, c_int, _vp, _fp, _vp, _fp, _vp, c_int, c_int, c_int, _vp]),
    'cvpce_gln_stem_fused': (c_int, [_vp, _vp, _fp, _vp, c_int, c_int, c_int, _vp]),
    'cvpce_atlas_copy': (c_int, [POINTER(_vp), POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, c_int, _vp, c_int, c_int, c_int, c_int, _vp]),
    'cvpce_conv3x3_halo': (c_int, [_vp, _vp, _fp, _vp] + [c_int] * 9 + [_vp]),
    'cvpce_conv3x3_halo_mac': (c_int, [_vp, _vp, _fp, _vp, _fp, c_int, c_int] + [c_int] * 8 + [_vp]),
    'cvpce_conv3x3_halo_wide': (c_int, [_vp, _vp, _fp, _vp] + [c_int] * 9 + [_vp]),
    'cvpce_conv3x3_halo_masked': (c_int, [_vp, _vp, _fp, _vp, _vp, c_int, _vp] + [c_int] * 8 + [_vp]),
    'cvpce_maxpool2d_nhwc_bf16': (c_int, [_vp, _vp] + [c_int] * 9 + [_vp]),
    'cvpce_relu_bf16': (c_int, [_vp, _vp, c_longlong, _vp]),
    'cvpce_pack_halo_weights': (c_int, [_vp, _vp, c_int, c_int]),
    'cvpce_conv3x3_thin_bf16': (c_int, [_vp, _vp, _fp, _vp] + [c_int] * 9 + [_vp]),
    'cvpce_gauss_tail_bf16': (c_int, [_vp, _vp, _fp, _vp, _fp, _fp, c_longlong, c_int, c_int, _vp]),
    'cvpce_gauss_subnet_bf16': (c_int, [_vp, _vp, _fp, _vp, _fp, _vp, _fp, _vp, _fp, c_int, _vp, _fp, c_int, _fp, c_int, c_int, c_int, c_int, _vp]),
    'cvpce_global_max_nhwc_bf16': (c_int, [_vp, _fp, c_int, c_int, c_int, c_int, c_int, _vp]),
    'cvpce_l2_normalize_f32': (c_int, [_fp, _fp, _vp, c_int, c_int, c_float, _vp]),
    'cvpce_gln_transform': (c_int, [_fp, _vp] + [c_int] * 6 + [POINTER(c_float), POINTER(c_float), _vp]),
    'cvpce_gln_transform_batch': (c_int, [POINTER(c_void_p), POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int, _vp, c_int, c_int,
                                          POINTER(c_float), POINTER(c_float), _vp]),
    'cvpce_crop_resize': (c_int, [_fp, _fp, _ip, c_int, _vp, c_int, c_int, c_int, c_int,
                                  POINTER(c_float), POINTER(c_float), _vp]),
    'cvpce_crop_resize_content': (c_int, [_fp, _fp, _ip, c_int, _vp, c_int, c_int, c_int, c_int,
                                          POINTER(c_float), POINTER(c_float), _ip, _vp]),
    'cvpce_pack_embed_input': (c_int, [_fp, _vp, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), _vp]),
    'cvpce_crop_extents': (c_int, [_fp, _ip, c_int, c_int, c_int, c_int, c_int, _ip, _vp]),
    'cvpce_pad_extents': (c_int, [_fp, c_int, c_int, c_float, _ip, _vp]),
    'cvpce_embed_worklists': (c_int, [_ip, c_int, c_int, ctypes.c_uint, _vp, c_int, _vp, c_longlong, _ip, _ip, _vp]),
    'cvpce_mac_init': (c_int, [_fp, c_int, c_int, c_int, c_int, _fp, _fp, c_int, c_int, _ip, _vp]),
    'cvpce_vgg_stem_fused_list': (c_int, [_vp, c_int, _vp, _vp, _fp, _vp, _fp, _vp, c_int, c_int, c_int, _vp, _ip, _vp]),
    'cvpce_bottleneck_fused_fm': (c_int, [_vp, _vp, _vp, _fp, _vp, _fp, _vp, _fp, _vp] + [c_int] * 5 + [_vp]),
    'cvpce_conv3x3_halo_thin_out': (c_int, [_vp, _vp, _fp, _fp] + [c_int] * 7 + [_vp]),
    'cvpce_conv3x3_halo_list': (c_int, [_vp, _vp, _fp, _vp, _fp, c_int, c_int] + [c_int] * 9 + [_vp, _ip, _vp]),
    'cvpce_conv3x3_halo_strips': (c_int, [_vp, _vp, _fp, _vp, _fp, c_int, c_int] + [c_int] * 9 + [_vp, _ip, _vp]),
    'cvpce_detect_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'cvpce_detect_plan': (c_int, [POINTER(c_int), POINTER(c_int)] + [c_int] * 6 + [POINTER(c_longlong)]),
    'cvpce_detect_postprocess': (c_int, [POINTER(c_void_p), POINTER(c_void_p), POINTER(c_int), POINTER(c_int),
                                         POINTER(c_int), POINTER(c_int), _fp, _ip, _fp,
                                         c_int, c_int, c_int, c_int, c_int, c_float, c_float, c_float, c_int, c_float,
                                         _vp, c_size_t, _fp, _fp, _vp, _ip, _ip, _vp]),
    'cvpce_row_norms': (c_int, [_vp, _fp, c_int, c_int, c_int, c_float, _vp]),
    'cvpce_match_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'cvpce_match_set_core': (c_int, [c_int, c_int, c_int]),
    'cvpce_match_plan': (c_int, [c_int, c_int, c_int, c_int, c_int, POINTER(c_longlong)]),
    'cvpce_probe_l2_stream': (c_int, [_vp, c_longlong, c_int, _fp, c_int, _vp]),
    'cvpce_probe_lds_fill': (c_int, [ctypes.c_uint, _ip, c_int, _vp]),
    'cvpce_probe_mfma_bf16': (c_int, [c_int, c_int, _vp, _fp, c_int, _vp]),
    'cvpce_match_topk': (c_int, [_vp, _vp, _fp, _fp, c_int, c_int, c_int, c_int, c_int, _vp, c_size_t, _vp, _fp, _vp]),
}
# fp16 twins of the detector's kernels (the opt-in accuracy mode): same argument lists as the functions they are named after
for _base, _twin in (('cvpce_conv2d_nhwc_bf16', 'cvpce_conv2d_nhwc_f16'), ('cvpce_conv2d_splitk_bf16', 'cvpce_conv2d_splitk_f16'), ('cvpce_conv1x1_nhwc_bf16', 'cvpce_conv1x1_nhwc_f16'),
                     ('cvpce_gln_stem_fused', 'cvpce_gln_stem_fused_f16'), ('cvpce_conv3x3_halo', 'cvpce_conv3x3_halo_f16'),
                     ('cvpce_conv3x3_halo_wide', 'cvpce_conv3x3_halo_wide_f16'), ('cvpce_conv3x3_halo_thin_out', 'cvpce_conv3x3_halo_thin_out_f16'), ('cvpce_conv3x3_halo_masked', 'cvpce_conv3x3_halo_masked_f16'),
                     ('cvpce_bottleneck_fused_fm', 'cvpce_bottleneck_fused_fm_f16'),
                     ('cvpce_maxpool2d_nhwc_bf16', 'cvpce_maxpool2d_nhwc_f16'), ('cvpce_relu_bf16', 'cvpce_relu_f16'), ('cvpce_gauss_tail_bf16', 'cvpce_gauss_tail_f16'), ('cvpce_gauss_subnet_bf16', 'cvpce_gauss_subnet_f16'), ('cvpce_conv3x3_thin_bf16', 'cvpce_conv3x3_thin_f16'),
                     ('cvpce_gln_transform', 'cvpce_gln_transform_f16'), ('cvpce_gln_transform_batch', 'cvpce_gln_transform_batch_f16')):
    SIGNATURES[_twin] = SIGNATURES[_base]

# One header of include/ <-> one table here <-> one op module (torch_ops.py), in the order the features arrived.  SIGNATURES is the
# inference header's table.
HEADERS = {'cvpce_amd.h': SIGNATURES}

# the evaluation kernels.
HEADERS['cvpce_amd_eval.h'] = {
    'cvpce_eval_match_detections': (c_int, [_fp, _ip, _ip, _ip, _fp, _ip, _ip, _fp] + [c_int] * 5 + [_ip, _vp, _vp]),
}

# the transform and the crop kernels reading (H,W,3) bytes.
HEADERS['cvpce_amd_input.h'] = {
    'cvpce_gln_transform_batch_u8': (c_int, [POINTER(c_void_p), POINTER(ctypes.c_ubyte), POINTER(c_int), POINTER(c_int), POINTER(c_int), POINTER(c_int), c_int,
                                             _vp, c_int, c_int, POINTER(c_float), POINTER(c_float), _fp, _vp]),
    'cvpce_crop_resize_u8': (c_int, [_vp, _fp, _fp, _ip, c_int, _vp, c_int, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), _vp]),
    'cvpce_crop_resize_content_u8': (c_int, [_vp, _fp, _fp, _ip, c_int, _vp, c_int, c_int, c_int, c_int, POINTER(c_float), POINTER(c_float), _ip, _vp]),
}
HEADERS['cvpce_amd_input.h']['cvpce_gln_transform_batch_u8_f16'] = HEADERS['cvpce_amd_input.h']['cvpce_gln_transform_batch_u8']

# the comparator's graph stages.
HEADERS['cvpce_amd_planogram.h'] = {
    'cvpce_planogram_graphs': (c_int, [_fp, _ip, _fp] + [c_int] * 4 + [_ip, _fp, _ip, _vp]),
    'cvpce_planogram_match_workspace_bytes': (c_size_t, [c_longlong]),
    'cvpce_planogram_match': (c_int, [_ip] * 11 + [c_int] * 6 + [c_longlong, _vp, c_size_t, _ip, _ip, _vp]),
}

# the comparator's tail (homography, projection, claim).
HEADERS['cvpce_amd_homography.h'] = {
    'cvpce_homography_workspace_bytes': (c_size_t, [c_int, c_int]),
    'cvpce_homography_ransac': (c_int, [_fp, _ip, _fp, _ip, _ip, _ip, _ip, _vp] + [c_int] * 5 + [ctypes.c_uint, c_int, _vp, c_size_t, _vp]),
    'cvpce_homography_finish': (c_int, [_fp, _ip, _ip, _fp, _ip, _ip, _ip, _ip, _ip, _vp] + [c_int] * 7 + [ctypes.c_uint, c_int, _vp, c_size_t,
                                        _ip, _vp, _ip, _ip, _ip, _ip, _ip, _fp, _vp]),
}

# the thin-strip companion of the work-list launches.
HEADERS['cvpce_amd_lists.h'] = {
    'cvpce_conv3x3_halo_strips2': SIGNATURES['cvpce_conv3x3_halo_strips'],
}

# the gallery side's byte-reading kernel.
HEADERS['cvpce_amd_gallery.h'] = {
    'cvpce_gallery_pack_u8': (c_int, [_vp, _ip, _vp, _vp, c_int, c_int, c_int, c_int, _ip, _vp]),
}

# the two ends of the comparator's re-classification.
HEADERS['cvpce_amd_reclass.h'] = {
    'cvpce_reclass_plan': (c_int, [_ip, _ip, _fp, _ip, _ip] + [c_int] * 3 + [_fp, _ip, _ip, _vp]),
    'cvpce_reclass_verdict': (c_int, [_ip, _ip, _ip, _vp, _ip, _ip, _ip, _ip, _ip] + [c_int] * 6 + [_ip, _ip, _vp]),
}

# the classification harness's comparison.
HEADERS['cvpce_amd_classeval.h'] = {
    'cvpce_classeval_rank': (c_int, [_vp, _ip, _ip] + [c_int] * 3 + [_ip, _vp]),
}

# a window's detections as the comparator's actual side.
HEADERS['cvpce_amd_actuals.h'] = {
    'cvpce_actuals_count': (c_int, [_fp, _ip, c_int, c_int, _ip, _vp]),
    'cvpce_actuals_pack': (c_int, [_fp, _ip, _vp, c_int, _ip, c_int, _ip, c_float, c_int, c_int, c_int, _fp, _ip, _ip, _fp, _ip, _vp]),
}

# the comparator's compliance report.
HEADERS['cvpce_amd_report.h'] = {
    'cvpce_report_positions': (c_int, [_ip, _ip, _ip, _fp, _fp, _ip, _ip, _ip, _ip, ctypes.c_double] + [c_int] * 3 + [_ip, _ip, _fp, _ip, _ip, _vp]),
    'cvpce_report_reclass': (c_int, [_ip, _ip, _ip, _vp, _fp, _ip, _ip, _ip, _ip] + [c_int] * 6 + [_ip, _ip, _fp, _vp]),
}

# the compliance pictures' compositor.
HEADERS['cvpce_amd_render.h'] = {
    'cvpce_render_canvases': (c_int, [_vp, c_int, c_longlong, _vp, c_longlong, _vp, c_longlong, _fp, _ip, _ip, _ip, c_int, _vp, c_longlong, _ip, c_int,
                                      c_int, _vp]),
}

# the Gaussian maps' targets and loss.
HEADERS['cvpce_amd_gaussians.h'] = {
    'cvpce_gauss_kant_table': (c_int, [_fp, c_int, c_int, _vp]),
    'cvpce_gauss_targets': (c_int, [_ip, _ip, _vp, _ip, _fp] + [c_int] * 7 + [POINTER(c_float), c_int, c_int, _fp, _vp]),
    'cvpce_gauss_loss_workspace_bytes': (c_size_t, [c_int, c_int, c_int]),
    'cvpce_gauss_loss': (c_int, [_fp, _fp, _ip, c_int, c_int, c_int, c_float, c_float, c_int, c_int, c_int, _vp, c_size_t, _fp, _ip, _vp]),
}

# anchor matching and the two head losses.
HEADERS['cvpce_amd_headloss.h'] = {
    'cvpce_headloss_workspace_bytes': (c_size_t, [POINTER(c_int), POINTER(c_int)] + [c_int] * 4),
    'cvpce_headloss': (c_int, [POINTER(c_void_p), POINTER(c_void_p)] + [POINTER(c_int)] * 4 + [_fp, _fp, _ip, _ip, _fp] + [c_int] * 5
                       + [_vp, c_size_t, _ip, _fp, _ip, _vp]),
}

# Headers of include/ext/: bound by the same loop, kept apart from HEADERS (the registry of the headers directly under include/).
# Tonioni's matcher, the comparator's second one.
EXTENSION_HEADERS = {'ext/cvpce_amd_tonioni.h': {
    'cvpce_tonioni_workspace_bytes': (c_size_t, [c_longlong, c_int]),
    'cvpce_tonioni_run': (c_int, [_ip] * 8 + [c_int] * 6 + [c_longlong, _vp, c_size_t, _vp]),
    'cvpce_tonioni_select': (c_int, [_ip] * 7 + [c_int] * 7 + [c_longlong, _vp, c_size_t, _ip, _ip, _vp]),
}}

# The step pictures' strokes.  A registry of its own beside EXTENSION_HEADERS: tests/test_tonioni_cpu.py pins that one to the
# matcher's header alone, as tests/test_abi_mirror_cpu.py pins HEADERS; a change that is free to edit both folds the three together.
PICTURE_EXTENSION_HEADERS = {'ext/cvpce_amd_strokes.h': {
    'cvpce_strokes_draw': (c_int, [_vp, c_int, c_longlong, _vp, c_longlong, _fp, _ip, _ip, c_int, _vp]),
}}

for _table in list(HEADERS.values()) + list(EXTENSION_HEADERS.values()) + list(PICTURE_EXTENSION_HEADERS.values()):
    for _name, (_res, _args) in _table.items():
        _fn = getattr(lib, _name)   # AttributeError here = header/library mismatch: fail loudly
        _fn.restype = _res
        _fn.argtypes = _args

_ERR = {1: 'bad argument', 2: 'kernel launch failure'}


def check(rc, what):
    if rc != 0:
        raise RuntimeError(f'{what} failed: {_ERR.get(rc, rc)}')


class SkipLayer(ctypes.Structure):
    """`cvpce_skip_layer` of include/cvpce_amd.h."""
    _fields_ = [(k, c_int) for k in ('H', 'W', 'tile_h', 'tile_w', 'out_ops', 'in_H', 'in_W', 'in_ops', 'skip')]


def float3(vals):
    return (c_float * 3)(*[float(v) for v in vals])
