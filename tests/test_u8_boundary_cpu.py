"""CPU-side checks of the 8-bit input kernels' boundary (no compute on a GPU): include/cvpce_amd_input.h is a header of its own,
with a signature table and an op list of its own, and leaves the pinned inference header as it was."""
import ctypes

import pytest
import torch

import abi


def test_library_exports_every_input_symbol():
    """(exported, bound and disjoint from the other headers: test_abi_mirror_cpu.py)"""
    syms = abi.header_symbols('cvpce_amd_input.h')
    assert syms == ['cvpce_crop_resize_content_u8', 'cvpce_crop_resize_u8', 'cvpce_gln_transform_batch_u8', 'cvpce_gln_transform_batch_u8_f16']


def test_input_ops_match_the_header_on_the_gpu_only():
    from cvpce_amd import torch_ops_input  # noqa: F401  (registers the ops)
    declared = set(abi.header_symbols('cvpce_amd_input.h'))
    twins = {s for s in declared if s.endswith('_f16')}                # reached through the bf16 op, by the batch tensor's dtype
    assert all(t[:-4] in declared for t in twins)
    u = torch.zeros(4, 4, 3, dtype=torch.uint8)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.crop_resize_u8(u, torch.zeros(256), torch.zeros(1, 4), None, torch.zeros(1, 3, 2, 2), 2, 0, None, None)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.gln_transform_batch_u8([u], torch.zeros(256), torch.zeros(1, 4, 4, 8, dtype=torch.float16), [4], [4], [0.0] * 3, [1.0] * 3)


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
