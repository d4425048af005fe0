"""PyTorch-ROCm custom ops over the detections kernels of include/cvpce_amd_actuals.h: `torch.ops.cvpce_amd.actuals_*`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
from ._lib import lib, check
from .torch_ops import _p, _stream, registrar, typed

NAMES, _op = registrar()


def _window(what, boxes, count):
    """-> (B, per) of a launch over boxes [B][per][4] and count [B]"""
    if boxes.dim() != 3 or boxes.shape[2] != 4 or boxes.shape[1] < 1 or count.dim() != 1 or count.numel() != boxes.shape[0]:
        raise RuntimeError(f'{what}: inconsistent shapes')
    return boxes.shape[0], boxes.shape[1]


@_op('actuals_count(Tensor boxes, Tensor count, Tensor(a!) kept) -> ()')
def _actuals_count(boxes, count, kept):
    what = 'cvpce_actuals_count'
    typed(what, f32=(boxes,), i32=(count, kept))
    b, per = _window(what, boxes, count)
    if kept.dim() != 1 or kept.numel() != b:
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_actuals_count(_p(boxes), _p(count), b, per, _p(kept), _stream()), what)


@_op('actuals_pack(Tensor boxes, Tensor count, Tensor indices, Tensor gallery_label_id, Tensor off2, float thresh_size, Tensor(a!) out_boxes, '
     'Tensor(b!) out_row, Tensor(c!) out_label, Tensor(d!) thresh, Tensor(e!) status) -> ()')
def _actuals_pack(boxes, count, indices, gallery_label_id, off2, thresh_size, out_boxes, out_row, out_label, thresh, status):
    what = 'cvpce_actuals_pack'
    typed(what, f32=(boxes, out_boxes, thresh), i32=(count, gallery_label_id, off2, out_row, out_label, status), i64=(indices,))
    b, per = _window(what, boxes, count)
    sum2 = out_boxes.shape[0]
    if (indices.dim() != 3 or indices.shape[0] != b or indices.shape[1] != per or indices.shape[2] < 1 or gallery_label_id.dim() != 1
            or off2.numel() != b + 1 or out_boxes.dim() != 2 or out_boxes.shape[1] != 4 or out_row.dim() != 1 or out_row.numel() != sum2
            or out_label.dim() != 1 or out_label.numel() != sum2 or thresh.numel() != b or status.numel() != b):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_actuals_pack(_p(boxes), _p(count), _p(indices), indices.shape[2], _p(gallery_label_id), gallery_label_id.numel(), _p(off2),
                                 float(thresh_size), b, per, sum2, _p(out_boxes), _p(out_row), _p(out_label), _p(thresh), _p(status), _stream()), what)
