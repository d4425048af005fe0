"""PyTorch-ROCm custom op over the classification harness's kernel of include/cvpce_amd_classeval.h: `torch.ops.cvpce_amd.classeval_rank`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
import torch

from ._lib import lib, check
from .torch_ops import _p, _stream, registrar

NAMES, _op = registrar()


@_op('classeval_rank(Tensor indices, Tensor gallery_label_id, Tensor want, Tensor(a!) records) -> ()')
def _classeval_rank(indices, gallery_label_id, want, records):
    what = 'cvpce_classeval_rank'
    if indices.dtype != torch.int64 or any(t.dtype != torch.int32 for t in (gallery_label_id, want, records)):
        raise RuntimeError(f'{what}: the match indices are int64, everything else int32')
    if not all(t.is_contiguous() for t in (indices, gallery_label_id, want, records)):
        raise RuntimeError(f'{what}: contiguous tensors only')
    if (indices.dim() != 2 or indices.shape[1] < 1 or gallery_label_id.dim() != 1 or gallery_label_id.numel() < 1 or want.dim() != 1
            or want.numel() != indices.shape[0] or tuple(records.shape) != (indices.shape[0], 2)):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_classeval_rank(_p(indices), _p(gallery_label_id), _p(want), indices.shape[0], indices.shape[1], gallery_label_id.numel(),
                                   _p(records), _stream()), what)
