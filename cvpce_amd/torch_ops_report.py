"""PyTorch-ROCm custom ops over the comparator's compliance report kernels of include/cvpce_amd_report.h: `torch.ops.cvpce_amd.report_*`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
from ._lib import lib, check
from .torch_ops import _p, _stream, registrar, typed

NAMES, _op = registrar()
MAX_NODES = 1024          # CVPCE_REPORT_MAX_NODES
DETECTED, RECOVERED, MISSING, OUT_OF_VIEW, UNCHECKED, PENDING = range(6)          # CVPCE_REPORT_*
OUTCOMES = ('detected', 'recovered', 'missing', 'out_of_view', 'unchecked', 'pending')


@_op('report_positions(Tensor status, Tensor matched_expected, Tensor matched_actual, Tensor expected_positions, Tensor actual_boxes, '
     'Tensor off1, Tensor off2, Tensor image, Tensor? actual_row, float iou_threshold, Tensor(a!) outcome, Tensor(b!) occupant, '
     'Tensor(c!) occupant_iou, Tensor(d!) occupant_row, Tensor(e!) stray) -> ()')
def _report_positions(status, matched_expected, matched_actual, expected_positions, actual_boxes, off1, off2, image, actual_row, iou_threshold,
                      outcome, occupant, occupant_iou, occupant_row, stray):
    what = 'cvpce_report_positions'
    rows = () if actual_row is None else (actual_row,)
    typed(what, f32=(expected_positions, actual_boxes, occupant_iou),
          i32=(status, matched_expected, matched_actual, off1, off2, image, outcome, occupant, occupant_row, stray) + rows)
    b, sum1, sum2 = status.numel(), matched_expected.numel(), matched_actual.numel()
    if (off1.numel() != b + 1 or off2.numel() != b + 1 or tuple(image.shape) != (b, 3) or tuple(expected_positions.shape) != (sum1, 4)
            or tuple(actual_boxes.shape) != (sum2, 4) or any(t.numel() != sum1 for t in (outcome, occupant, occupant_iou, occupant_row))
            or any(t.numel() != sum2 for t in (stray,) + rows)):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_report_positions(_p(status), _p(matched_expected), _p(matched_actual), _p(expected_positions), _p(actual_boxes), _p(off1),
                                     _p(off2), _p(image), _p(actual_row), float(iou_threshold), b, sum1, sum2,
                                     _p(outcome), _p(occupant), _p(occupant_iou), _p(occupant_row), _p(stray), _stream()), what)


@_op('report_reclass(Tensor expected_index, Tensor count, Tensor slot_row, Tensor indices, Tensor distances, Tensor gallery_label_id, '
     'Tensor expected_label_id, Tensor off1, Tensor status, Tensor(a!) outcome, Tensor(b!) seen_row, Tensor(c!) seen_distance) -> ()')
def _report_reclass(expected_index, count, slot_row, indices, distances, gallery_label_id, expected_label_id, off1, status, outcome, seen_row,
                    seen_distance):
    what = 'cvpce_report_reclass'
    typed(what, f32=(distances, seen_distance), i64=(indices,),
          i32=(expected_index, count, slot_row, gallery_label_id, expected_label_id, off1, status, outcome, seen_row))
    b, sum1 = status.numel(), outcome.numel()
    cap = expected_index.shape[1] if expected_index.dim() == 2 else 0
    if (off1.numel() != b + 1 or any(t.dim() != 2 or t.shape[0] != b or t.shape[1] != cap for t in (expected_index, slot_row))
            or not 1 <= cap <= MAX_NODES or indices.dim() != 2 or indices.shape[1] < 1 or distances.shape != indices.shape
            or gallery_label_id.dim() != 1 or expected_label_id.numel() != sum1 or seen_row.numel() != sum1 or seen_distance.numel() != sum1
            or count.numel() != b):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_report_reclass(_p(expected_index), _p(count), _p(slot_row), _p(indices), _p(distances), _p(gallery_label_id),
                                   _p(expected_label_id), _p(off1), _p(status), b, sum1, cap, indices.shape[0], indices.shape[1],
                                   gallery_label_id.numel(), _p(outcome), _p(seen_row), _p(seen_distance), _stream()), what)
