"""PyTorch-ROCm custom op over the classification harness's kernel of include/cvpce_amd_classeval.h: `torch.ops.cvpce_amd.classeval_rank`.

Kept apart from torch_ops_reclass.py and the other op modules, whose NAMES lists are pinned.  Same rules: defined on the library
torch_ops owns, CUDA (= HIP on ROCm) dispatch key only -- no CPU kernel exists -- an out-variant that launches on the current stream
through ctypes with no allocation and no synchronisation.
"""
import torch

from ._lib import lib, check
from .torch_ops import _L, _p, _stream

NAMES = []


def _op(schema):
    def deco(fn):
        name = schema.split('(')[0]
        _L.define(schema)
        _L.impl(name, fn, 'CUDA')
        NAMES.append(name)
        return fn
    return deco


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
