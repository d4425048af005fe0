"""CPU-side checks of the 8-bit input kernels' boundary (no compute on a GPU): include/cvpce_amd_input.h is a header of its own,
with a signature table and an op list of its own, and leaves the pinned inference header as it was."""
import ctypes
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols(name):
    text = open(os.path.join(ROOT, 'include', name)).read()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(cvpce_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_every_input_symbol():
    from cvpce_amd import _lib
    syms = header_symbols('cvpce_amd_input.h')
    assert syms == ['cvpce_crop_resize_content_u8', 'cvpce_crop_resize_u8', 'cvpce_gln_transform_batch_u8', 'cvpce_gln_transform_batch_u8_f16']
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in include/cvpce_amd_input.h but not exported'
    assert sorted(_lib.INPUT_SIGNATURES) == syms, 'ctypes signature table out of sync with the header'
    assert not set(_lib.INPUT_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.EVAL_SIGNATURES))


def test_input_ops_match_the_header_on_the_gpu_only():
    from cvpce_amd import torch_ops, torch_ops_input
    declared = set(header_symbols('cvpce_amd_input.h'))
    twins = {s for s in declared if s.endswith('_f16')}                # reached through the bf16 op, by the batch tensor's dtype
    assert all(t[:-4] in declared for t in twins)
    assert sorted('cvpce_' + n for n in torch_ops_input.NAMES) == sorted(declared - twins)
    assert not set(torch_ops_input.NAMES) & set(torch_ops.NAMES)
    for name in torch_ops_input.NAMES:
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'cvpce_amd::{name}', 'CPU')
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'cvpce_amd::{name}', 'CUDA')
    u = torch.zeros(4, 4, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.crop_resize_u8(u, torch.zeros(256), torch.zeros(1, 4), None, torch.zeros(1, 3, 2, 2), 2, 0, None, None)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.gln_transform_batch_u8([u], torch.zeros(256), torch.zeros(1, 4, 4, 8, dtype=torch.float16), [4], [4], [0.0] * 3, [1.0] * 3)


def test_inference_header_is_what_it_was():
    syms = header_symbols('cvpce_amd.h')
    assert not [s for s in syms if '_u8' in s]
    from cvpce_amd import _lib, torch_ops
    assert sorted(_lib.SIGNATURES) == syms and not [n for n in torch_ops.NAMES if 'u8' in n]
    assert not set(header_symbols('cvpce_amd_input.h')) & set(syms)


def test_host_side_argument_checks():
    """What the entry points refuse before they touch the device: null pointers, and a byte image whose offsets do not fit 32 bits."""
    from cvpce_amd._lib import lib
    one = ctypes.c_void_p(64)        # (never dereferenced: every call below is refused on its arguments)
    assert lib.cvpce_crop_resize_u8(None, one, one, None, 1, one, 4, 4, 8, 0, None, None, None) == 1
    assert lib.cvpce_crop_resize_u8(one, None, one, None, 1, one, 4, 4, 8, 0, None, None, None) == 1
    assert lib.cvpce_crop_resize_u8(one, one, one, None, 1, one, 32768, 21846, 8, 0, None, None, None) == 1
    assert lib.cvpce_crop_resize_u8(one, one, one, None, 1, one, 4, 4, 8, 1, None, None, None) == 1        # modes 1 / 2 need mean / std
    assert lib.cvpce_crop_resize_content_u8(one, one, one, None, 1, one, 4, 4, 8, 2, (ctypes.c_float * 3)(), (ctypes.c_float * 3)(1, 1, 1), None, None) == 1
    assert lib.cvpce_crop_resize_u8(one, one, one, None, 0, one, 4, 4, 8, 0, None, None, None) == 0        # no boxes: nothing to do
    c1 = lambda v: (ctypes.c_int * 1)(v)
    ptrs, form, f3 = (ctypes.c_void_p * 1)(64), (ctypes.c_ubyte * 1)(1), (ctypes.c_float * 3)(1, 1, 1)
    for fn in (lib.cvpce_gln_transform_batch_u8, lib.cvpce_gln_transform_batch_u8_f16):
        assert fn(ptrs, form, c1(32768), c1(21846), c1(8), c1(8), 1, one, 8, 8, f3, f3, one, None) == 1
        assert fn(ptrs, form, c1(4), c1(4), c1(9), c1(8), 1, one, 8, 8, f3, f3, one, None) == 1            # h > Hp
        assert fn(ptrs, form, c1(4), c1(4), c1(8), c1(8), 1, one, 8, 8, f3, f3, None, None) == 1           # no table
        assert fn(ptrs, form, c1(4), c1(4), c1(8), c1(8), 0, one, 8, 8, f3, f3, one, None) == 0            # n = 0
