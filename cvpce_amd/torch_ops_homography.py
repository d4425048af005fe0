"""PyTorch-ROCm custom ops over the comparator-tail kernels of include/cvpce_amd_homography.h: `torch.ops.cvpce_amd.homography_*`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
from ._lib import lib, check
from .torch_ops import _p, _stream, registrar, typed

NAMES, _op = registrar()
MAX_PAIRS = 1024          # CVPCE_HOMOGRAPHY_MAX_PAIRS
MAX_HYPOTHESES = 65536    # CVPCE_HOMOGRAPHY_MAX_HYPOTHESES
OK, NONE, INVALID = 0, 1, 2


def workspace_bytes(b, hypotheses):
    return lib.cvpce_homography_workspace_bytes(b, hypotheses)


def _shapes(what, boxes1, off1, boxes2, off2, pairs, count, out_off, params, workspace):
    b = count.numel()
    if (boxes1.dim() != 2 or boxes1.shape[1] != 4 or boxes2.dim() != 2 or boxes2.shape[1] != 4 or pairs.dim() != 2 or pairs.shape[1] != 2
            or any(t.numel() != b + 1 for t in (off1, off2, out_off)) or params.numel() != 2 * b or not workspace.is_contiguous()):
        raise RuntimeError(f'{what}: inconsistent shapes')
    return b


@_op('homography_ransac(Tensor boxes1, Tensor off1, Tensor boxes2, Tensor off2, Tensor pairs, Tensor count, Tensor out_off, Tensor params, '
     'int max_pairs, int seed, int hypotheses, Tensor(a!) workspace) -> ()')
def _homography_ransac(boxes1, off1, boxes2, off2, pairs, count, out_off, params, max_pairs, seed, hypotheses, workspace):
    what = 'cvpce_homography_ransac'
    typed(what, f32=(boxes1, boxes2), i32=(off1, off2, pairs, count, out_off), f64=(params,))
    b = _shapes(what, boxes1, off1, boxes2, off2, pairs, count, out_off, params, workspace)
    check(lib.cvpce_homography_ransac(_p(boxes1), _p(off1), _p(boxes2), _p(off2), _p(pairs), _p(count), _p(out_off), _p(params),
                                      b, boxes1.shape[0], boxes2.shape[0], pairs.shape[0], max_pairs, seed & 0xFFFFFFFF, hypotheses,
                                      _p(workspace), workspace.numel() * workspace.element_size(), _stream()), what)


@_op('homography_finish(Tensor boxes1, Tensor label1, Tensor off1, Tensor boxes2, Tensor label2, Tensor off2, Tensor pairs, Tensor count, '
     'Tensor out_off, Tensor params, int max_n1, int max_n2, int max_pairs, int seed, int hypotheses, Tensor workspace, Tensor(a!) status, '
     'Tensor(b!) H, Tensor(c!) winner, Tensor(d!) winner_count, Tensor(e!) final_count, Tensor(f!) matched_expected, '
     'Tensor(g!) matched_actual, Tensor(h!) expected_positions) -> ()')
def _homography_finish(boxes1, label1, off1, boxes2, label2, off2, pairs, count, out_off, params, max_n1, max_n2, max_pairs, seed, hypotheses,
                       workspace, status, H, winner, winner_count, final_count, matched_expected, matched_actual, expected_positions):
    what = 'cvpce_homography_finish'
    typed(what, f32=(boxes1, boxes2, expected_positions), f64=(params, H),
          i32=(label1, off1, label2, off2, pairs, count, out_off, status, winner, winner_count, final_count, matched_expected, matched_actual))
    b = _shapes(what, boxes1, off1, boxes2, off2, pairs, count, out_off, params, workspace)
    sum1, sum2 = boxes1.shape[0], boxes2.shape[0]
    if (label1.numel() != sum1 or label2.numel() != sum2 or matched_expected.numel() != sum1 or matched_actual.numel() != sum2
            or expected_positions.numel() != sum1 * 4 or H.numel() != 9 * b or any(t.numel() != b for t in (status, winner, winner_count, final_count))):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_homography_finish(_p(boxes1), _p(label1), _p(off1), _p(boxes2), _p(label2), _p(off2), _p(pairs), _p(count), _p(out_off),
                                      _p(params), b, sum1, sum2, pairs.shape[0], max_n1, max_n2, max_pairs, seed & 0xFFFFFFFF, hypotheses,
                                      _p(workspace), workspace.numel() * workspace.element_size(), _p(status), _p(H), _p(winner),
                                      _p(winner_count), _p(final_count), _p(matched_expected), _p(matched_actual), _p(expected_positions),
                                      _stream()), what)
