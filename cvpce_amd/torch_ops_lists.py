"""PyTorch-ROCm custom op over the thin-strip launch of include/cvpce_amd_lists.h: `torch.ops.cvpce_amd.conv3x3_halo_strips2`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
from ._lib import lib
from .torch_ops import _halo_list, registrar

NAMES, _op = registrar()


@_op('conv3x3_halo_strips2(Tensor x, Tensor weight, Tensor? bias, Tensor(a!)? out, Tensor(b!)? mac, int mac_off, int cout, int k_pad, '
     'int cout_pad, int relu, int pool, Tensor work, Tensor count) -> ()')
def _conv3x3_halo_strips2(x, weight, bias, out, mac, mac_off, cout, k_pad, cout_pad, relu, pool, work, count):
    _halo_list(lib.cvpce_conv3x3_halo_strips2, 'cvpce_conv3x3_halo_strips2', x, weight, bias, out, mac, mac_off, cout, k_pad, cout_pad, relu, pool, work, count)
