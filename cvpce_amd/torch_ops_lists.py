"""PyTorch-ROCm custom op over the thin-strip launch of include/cvpce_amd_lists.h: `torch.ops.cvpce_amd.conv3x3_halo_strips2`.

Kept apart from torch_ops.py, whose NAMES list mirrors the inference header entry point by entry point.  Same rules as
torch_ops_eval.py: defined on the library torch_ops owns, CUDA (= HIP on ROCm) dispatch key only -- no CPU kernel exists -- an
out-variant that launches on the current stream through ctypes with no allocation and no synchronisation.
"""
from ._lib import lib
from .torch_ops import _L, _halo_list

NAMES = []


def _op(schema):
    def deco(fn):
        name = schema.split('(')[0]
        _L.define(schema)
        _L.impl(name, fn, 'CUDA')
        NAMES.append(name)
        return fn
    return deco


@_op('conv3x3_halo_strips2(Tensor x, Tensor weight, Tensor? bias, Tensor(a!)? out, Tensor(b!)? mac, int mac_off, int cout, int k_pad, '
     'int cout_pad, int relu, int pool, Tensor work, Tensor count) -> ()')
def _conv3x3_halo_strips2(x, weight, bias, out, mac, mac_off, cout, k_pad, cout_pad, relu, pool, work, count):
    _halo_list(lib.cvpce_conv3x3_halo_strips2, 'cvpce_conv3x3_halo_strips2', x, weight, bias, out, mac, mac_off, cout, k_pad, cout_pad, relu, pool, work, count)
