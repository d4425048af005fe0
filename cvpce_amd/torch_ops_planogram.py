"""PyTorch-ROCm custom ops over the planogram comparator kernels of include/cvpce_amd_planogram.h: `torch.ops.cvpce_amd.planogram_*`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
from ._lib import lib, check
from .torch_ops import _p, _stream, registrar, typed

NAMES, _op = registrar()
MAX_NODES = 1024          # CVPCE_PLANOGRAM_MAX_NODES


@_op('planogram_graphs(Tensor boxes, Tensor offsets, Tensor thresh, int min_n, int max_n, Tensor(a!) nbr, Tensor(b!) weight, '
     'Tensor(c!) stamp) -> ()')
def _planogram_graphs(boxes, offsets, thresh, min_n, max_n, nbr, weight, stamp):
    what = 'cvpce_planogram_graphs'
    typed(what, f32=(boxes, thresh, weight), i32=(offsets, nbr, stamp))
    b, sum_n = thresh.numel(), boxes.shape[0]
    if boxes.dim() != 2 or boxes.shape[1] != 4 or offsets.numel() != b + 1 or any(t.numel() != sum_n * 8 for t in (nbr, weight, stamp)):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_planogram_graphs(_p(boxes), _p(offsets), _p(thresh), b, sum_n, min_n, max_n, _p(nbr), _p(weight), _p(stamp), _stream()), what)


@_op('planogram_match(Tensor nbr1, Tensor stamp1, Tensor label1, Tensor off1, Tensor nbr2, Tensor stamp2, Tensor label2, Tensor off2, '
     'Tensor params, Tensor hyp_off, Tensor out_off, int max_n1, int max_n2, int hypotheses, Tensor(a!) workspace, Tensor(b!) pairs, '
     'Tensor(c!) count) -> ()')
def _planogram_match(nbr1, stamp1, label1, off1, nbr2, stamp2, label2, off2, params, hyp_off, out_off, max_n1, max_n2, hypotheses,
                     workspace, pairs, count):
    what = 'cvpce_planogram_match'
    typed(what, i32=(nbr1, stamp1, label1, off1, nbr2, stamp2, label2, off2, params, hyp_off, out_off, pairs, count))
    p, sum1, sum2 = count.numel(), label1.numel(), label2.numel()
    if (any(t.numel() != p + 1 for t in (off1, off2, hyp_off, out_off)) or params.numel() != 2 * p or pairs.dim() != 2 or pairs.shape[1] != 2
            or any(t.numel() != sum1 * 8 for t in (nbr1, stamp1)) or any(t.numel() != sum2 * 8 for t in (nbr2, stamp2))
            or not workspace.is_contiguous()):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_planogram_match(_p(nbr1), _p(stamp1), _p(label1), _p(off1), _p(nbr2), _p(stamp2), _p(label2), _p(off2), _p(params),
                                    _p(hyp_off), _p(out_off), p, sum1, sum2, max_n1, max_n2, pairs.shape[0], hypotheses,
                                    _p(workspace), workspace.numel() * workspace.element_size(), _p(pairs), _p(count), _stream()), what)
