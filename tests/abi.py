"""What the boundary tests share about the C ABI: the headers of include/ as text, as symbols and as declarations, the op module
of each header, and the few names the rules make exceptions for.  tests/test_abi_mirror_cpu.py checks header <-> ctypes table <->
op list for every header with these; the per-feature tests take a header's text or symbols from here."""
import ctypes
import importlib
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, 'include')

# header -> the module of cvpce_amd/ that registers its ops (its NAMES list)
OP_MODULES = {
    'cvpce_amd.h': 'torch_ops',
    'cvpce_amd_eval.h': 'torch_ops_eval',
    'cvpce_amd_input.h': 'torch_ops_input',
    'cvpce_amd_planogram.h': 'torch_ops_planogram',
    'cvpce_amd_homography.h': 'torch_ops_homography',
    'cvpce_amd_lists.h': 'torch_ops_lists',
    'cvpce_amd_gallery.h': 'torch_ops_gallery',
    'cvpce_amd_reclass.h': 'torch_ops_reclass',
    'cvpce_amd_classeval.h': 'torch_ops_classeval',
    'cvpce_amd_actuals.h': 'torch_ops_actuals',
    'cvpce_amd_report.h': 'torch_ops_report',
    'cvpce_amd_render.h': 'torch_ops_render',
    'cvpce_amd_gaussians.h': 'torch_ops_gaussians',
    'cvpce_amd_headloss.h': 'torch_ops_headloss',
}
INFERENCE = 'cvpce_amd.h'
FEATURES = [h for h in OP_MODULES if h != INFERENCE]

# entry points that run on the host alone: no op stands for them
HOST_ONLY = {
    'cvpce_conv2d_splitk_workspace_bytes', 'cvpce_detect_workspace_bytes', 'cvpce_match_workspace_bytes', 'cvpce_planogram_match_workspace_bytes',
    'cvpce_homography_workspace_bytes', 'cvpce_gauss_loss_workspace_bytes', 'cvpce_headloss_workspace_bytes',
    'cvpce_set_persistent_workgroups', 'cvpce_pack_halo_weights', 'cvpce_match_set_core', 'cvpce_match_plan', 'cvpce_detect_plan',
}

# the op lists of the feature headers, in definition order
PINNED_NAMES = {
    'cvpce_amd_eval.h': ['eval_match_detections'],
    'cvpce_amd_input.h': ['gln_transform_batch_u8', 'crop_resize_u8', 'crop_resize_content_u8'],
    'cvpce_amd_planogram.h': ['planogram_graphs', 'planogram_match'],
    'cvpce_amd_homography.h': ['homography_ransac', 'homography_finish'],
    'cvpce_amd_lists.h': ['conv3x3_halo_strips2'],
    'cvpce_amd_gallery.h': ['gallery_pack_u8'],
    'cvpce_amd_reclass.h': ['reclass_plan', 'reclass_verdict'],
    'cvpce_amd_classeval.h': ['classeval_rank'],
    'cvpce_amd_actuals.h': ['actuals_count', 'actuals_pack'],
    'cvpce_amd_report.h': ['report_positions', 'report_reclass'],
    'cvpce_amd_render.h': ['render_canvases'],
    'cvpce_amd_gaussians.h': ['gauss_kant_table', 'gauss_targets', 'gauss_loss'],
    'cvpce_amd_headloss.h': ['headloss'],
}

# A feature header's family word is in the names of no other header, table or op list.  (`gauss` is no family word: the inference
# header owns cvpce_gauss_tail_* and cvpce_gauss_subnet_*.)  The exceptions, by name -- there are no others:
FAMILY_WORDS = {
    'cvpce_amd_eval.h': 'eval', 'cvpce_amd_input.h': 'u8', 'cvpce_amd_planogram.h': 'planogram', 'cvpce_amd_homography.h': 'homography',
    'cvpce_amd_lists.h': 'strips2', 'cvpce_amd_gallery.h': 'gallery', 'cvpce_amd_reclass.h': 'reclass', 'cvpce_amd_classeval.h': 'classeval',
    'cvpce_amd_actuals.h': 'actuals', 'cvpce_amd_report.h': 'report', 'cvpce_amd_render.h': 'render', 'cvpce_amd_headloss.h': 'headloss',
}
FAMILY_EXCEPTIONS = {('eval', 'cvpce_classeval_rank'), ('u8', 'cvpce_gallery_pack_u8'), ('reclass', 'cvpce_report_reclass')}


def header_text(name):
    """The header without its comments."""
    text = open(os.path.join(INCLUDE, name)).read()
    return re.sub(r'//[^\n]*', '', re.sub(r'/\*.*?\*/', '', text, flags=re.S))


def header_symbols(name):
    return sorted(set(re.findall(r'\b(cvpce_[a-z0-9_]+)\s*\(', header_text(name))))


_C_KINDS = {'int': 'int', 'float': 'float', 'double': 'double', 'size_t': 'size_t', 'long long': 'long long', 'unsigned': 'unsigned',
            'unsigned int': 'unsigned'}
_CTYPES_KINDS = {ctypes.c_int: 'int', ctypes.c_float: 'float', ctypes.c_double: 'double', ctypes.c_size_t: 'size_t',
                 ctypes.c_longlong: 'long long', ctypes.c_uint: 'unsigned'}


def _c_kind(text, named):
    """The kind of a C type: 'pointer' for anything with * (or []) and for hipStream_t, else one of the scalar kinds.  named: the text
    may end in a parameter name."""
    if '*' in text or '[' in text or 'hipStream_t' in text:
        return 'pointer'
    words = re.sub(r'\bconst\b', '', text).split()
    if named and len(words) > 1 and ' '.join(words) not in _C_KINDS:
        words = words[:-1]
    return _C_KINDS[' '.join(words)]          # KeyError: a type this parser does not know -- teach it, do not skip the header


def declarations(name):
    """{entry point: (kind of the return value, [kind of each argument])} in declaration order"""
    out = {}
    for ret, fn, args in re.findall(r'([A-Za-z_][A-Za-z0-9_ \t*]*?)\s*\b(cvpce_[a-z0-9_]+)\s*\(([^;{()]*)\)\s*;', header_text(name)):
        args = [] if args.strip() in ('', 'void') else args.split(',')
        out[fn] = (_c_kind(ret, False), [_c_kind(a, True) for a in args])
    return out


def ctypes_kind(t):
    if t is ctypes.c_void_p or (isinstance(t, type) and issubclass(t, ctypes._Pointer)):
        return 'pointer'
    return _CTYPES_KINDS[t]


def twins(symbols):
    """The fp16 twins among a header's symbols: `X_f16` where X or X_bf16 is declared beside it.  An op reaches a twin through its
    base, by the tensors' dtype."""
    symbols = set(symbols)
    return {s for s in symbols if s.endswith('_f16') and (s[:-4] in symbols or s[:-4] + '_bf16' in symbols)}


def op_module(header):
    return importlib.import_module('cvpce_amd.' + OP_MODULES[header])


def op_symbols(header):
    """The symbols of a header that an op stands for: all but the host-only entry points and the twins."""
    symbols = set(header_symbols(header))
    return sorted(symbols - HOST_ONLY - twins(symbols))
