"""PyTorch-ROCm custom ops over the comparator's re-classification kernels of include/cvpce_amd_reclass.h: `torch.ops.cvpce_amd.reclass_*`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
from ._lib import lib, check
from .torch_ops import _p, _stream, registrar, typed

NAMES, _op = registrar()
MAX_NODES = 1024          # CVPCE_RECLASS_MAX_NODES


def _window(what, status, matched_expected, off1, slots):
    """-> (B, sumN1, cap) of a launch whose per-slot tables `slots` are [B][cap]"""
    b, sum1 = status.numel(), matched_expected.numel()
    cap = slots[0].shape[1] if slots[0].dim() == 2 else 0
    if off1.numel() != b + 1 or any(t.dim() != 2 or t.shape[0] != b or t.shape[1] != cap for t in slots) or not 1 <= cap <= MAX_NODES:
        raise RuntimeError(f'{what}: inconsistent shapes')
    return b, sum1, cap


@_op('reclass_plan(Tensor status, Tensor matched_expected, Tensor expected_positions, Tensor off1, Tensor image, Tensor(a!) boxes, '
     'Tensor(b!) expected_index, Tensor(c!) count) -> ()')
def _reclass_plan(status, matched_expected, expected_positions, off1, image, boxes, expected_index, count):
    what = 'cvpce_reclass_plan'
    typed(what, f32=(expected_positions, boxes), i32=(status, matched_expected, off1, image, expected_index, count))
    b, sum1, cap = _window(what, status, matched_expected, off1, (expected_index,))
    if (expected_positions.dim() != 2 or tuple(expected_positions.shape) != (sum1, 4) or tuple(boxes.shape) != (b, cap, 4)
            or tuple(image.shape) != (b, 3) or count.numel() != b):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_reclass_plan(_p(status), _p(matched_expected), _p(expected_positions), _p(off1), _p(image), b, sum1, cap,
                                 _p(boxes), _p(expected_index), _p(count), _stream()), what)


@_op('reclass_verdict(Tensor expected_index, Tensor count, Tensor slot_row, Tensor indices, Tensor gallery_label_id, Tensor expected_label_id, '
     'Tensor matched_expected, Tensor off1, Tensor status, Tensor(a!) found, Tensor(b!) found_count) -> ()')
def _reclass_verdict(expected_index, count, slot_row, indices, gallery_label_id, expected_label_id, matched_expected, off1, status, found,
                     found_count):
    what = 'cvpce_reclass_verdict'
    typed(what, i64=(indices,),
          i32=(expected_index, count, slot_row, gallery_label_id, expected_label_id, matched_expected, off1, status, found, found_count))
    b, sum1, cap = _window(what, status, matched_expected, off1, (expected_index, slot_row))
    if (indices.dim() != 2 or indices.shape[1] < 1 or gallery_label_id.dim() != 1 or expected_label_id.numel() != sum1 or found.numel() != sum1
            or count.numel() != b or found_count.numel() != b):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_reclass_verdict(_p(expected_index), _p(count), _p(slot_row), _p(indices), _p(gallery_label_id), _p(expected_label_id),
                                    _p(matched_expected), _p(off1), _p(status), b, sum1, cap, indices.shape[0], indices.shape[1],
                                    gallery_label_id.numel(), _p(found), _p(found_count), _stream()), what)
