"""PyTorch-ROCm custom ops over the detections kernels of include/cvpce_amd_actuals.h: `torch.ops.cvpce_amd.actuals_*`.

Kept apart from torch_ops_reclass.py, whose NAMES list is pinned.  Same rules: defined on the library torch_ops owns, CUDA (= HIP on
ROCm) dispatch key only -- no CPU kernel exists -- out-variants that launch on the current stream through ctypes with no allocation
and no synchronisation.
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


def _typed(what, f32, i32, i64=()):
    if (any(t.dtype != torch.float32 for t in f32) or any(t.dtype != torch.int32 for t in i32) or any(t.dtype != torch.int64 for t in i64)):
        raise RuntimeError(f'{what}: boxes and thresholds are float32, the match indices int64, everything else int32')
    if not all(t.is_contiguous() for t in tuple(f32) + tuple(i32) + tuple(i64)):
        raise RuntimeError(f'{what}: contiguous tensors only')


def _window(what, boxes, count):
    """-> (B, per) of a launch over boxes [B][per][4] and count [B]"""
    if boxes.dim() != 3 or boxes.shape[2] != 4 or boxes.shape[1] < 1 or count.dim() != 1 or count.numel() != boxes.shape[0]:
        raise RuntimeError(f'{what}: inconsistent shapes')
    return boxes.shape[0], boxes.shape[1]


@_op('actuals_count(Tensor boxes, Tensor count, Tensor(a!) kept) -> ()')
def _actuals_count(boxes, count, kept):
    what = 'cvpce_actuals_count'
    _typed(what, (boxes,), (count, kept))
    b, per = _window(what, boxes, count)
    if kept.dim() != 1 or kept.numel() != b:
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_actuals_count(_p(boxes), _p(count), b, per, _p(kept), _stream()), what)


@_op('actuals_pack(Tensor boxes, Tensor count, Tensor indices, Tensor gallery_label_id, Tensor off2, float thresh_size, Tensor(a!) out_boxes, '
     'Tensor(b!) out_row, Tensor(c!) out_label, Tensor(d!) thresh, Tensor(e!) status) -> ()')
def _actuals_pack(boxes, count, indices, gallery_label_id, off2, thresh_size, out_boxes, out_row, out_label, thresh, status):
    what = 'cvpce_actuals_pack'
    _typed(what, (boxes, out_boxes, thresh), (count, gallery_label_id, off2, out_row, out_label, status), (indices,))
    b, per = _window(what, boxes, count)
    sum2 = out_boxes.shape[0]
    if (indices.dim() != 3 or indices.shape[0] != b or indices.shape[1] != per or indices.shape[2] < 1 or gallery_label_id.dim() != 1
            or off2.numel() != b + 1 or out_boxes.dim() != 2 or out_boxes.shape[1] != 4 or out_row.dim() != 1 or out_row.numel() != sum2
            or out_label.dim() != 1 or out_label.numel() != sum2 or thresh.numel() != b or status.numel() != b):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_actuals_pack(_p(boxes), _p(count), _p(indices), indices.shape[2], _p(gallery_label_id), gallery_label_id.numel(), _p(off2),
                                 float(thresh_size), b, per, sum2, _p(out_boxes), _p(out_row), _p(out_label), _p(thresh), _p(status), _stream()), what)
