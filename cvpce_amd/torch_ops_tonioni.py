"""PyTorch-ROCm custom ops over Tonioni's matcher of include/ext/cvpce_amd_tonioni.h: `torch.ops.cvpce_amd.tonioni_*`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
from ._lib import lib, check
from .torch_ops import _p, _stream, registrar, typed

NAMES, _op = registrar()
MAX_HYPOTHESES = 16384    # CVPCE_TONIONI_MAX_HYPOTHESES


def workspace_words(hypotheses, pairs):
    """int32 words of the workspace of a launch over `pairs` pairs with `hypotheses` hypothesis slots in all"""
    return lib.cvpce_tonioni_workspace_bytes(hypotheses, pairs) // 4


def _shapes(what, p, off, nbr1, sum1, nbr2, sum2, params, workspace, hypotheses):
    if (any(t.numel() != p + 1 for t in off) or params.numel() != p or nbr1.numel() != sum1 * 8 or nbr2.numel() != sum2 * 8
            or not workspace.is_contiguous() or workspace.numel() < workspace_words(hypotheses, p)):
        raise RuntimeError(f'{what}: inconsistent shapes')


@_op('tonioni_run(Tensor nbr1, Tensor label1, Tensor off1, Tensor nbr2, Tensor label2, Tensor off2, Tensor params, Tensor hyp_off, '
     'int max_n1, int max_n2, int max_hyp, int hypotheses, Tensor(a!) workspace) -> ()')
def _tonioni_run(nbr1, label1, off1, nbr2, label2, off2, params, hyp_off, max_n1, max_n2, max_hyp, hypotheses, workspace):
    what = 'cvpce_tonioni_run'
    typed(what, i32=(nbr1, label1, off1, nbr2, label2, off2, params, hyp_off, workspace))
    p, sum1, sum2 = params.numel(), label1.numel(), label2.numel()
    _shapes(what, p, (off1, off2, hyp_off), nbr1, sum1, nbr2, sum2, params, workspace, hypotheses)
    check(lib.cvpce_tonioni_run(_p(nbr1), _p(label1), _p(off1), _p(nbr2), _p(label2), _p(off2), _p(params), _p(hyp_off), p, sum1, sum2,
                                max_n1, max_n2, max_hyp, hypotheses, _p(workspace), workspace.numel() * 4, _stream()), what)


@_op('tonioni_select(Tensor nbr1, Tensor off1, Tensor nbr2, Tensor off2, Tensor params, Tensor hyp_off, Tensor out_off, int max_n1, '
     'int max_n2, int max_hyp, int hypotheses, Tensor workspace, Tensor(a!) pairs, Tensor(b!) count) -> ()')
def _tonioni_select(nbr1, off1, nbr2, off2, params, hyp_off, out_off, max_n1, max_n2, max_hyp, hypotheses, workspace, pairs, count):
    what = 'cvpce_tonioni_select'
    typed(what, i32=(nbr1, off1, nbr2, off2, params, hyp_off, out_off, workspace, pairs, count))
    p = count.numel()
    if pairs.dim() != 2 or pairs.shape[1] != 2 or nbr1.numel() % 8 or nbr2.numel() % 8:
        raise RuntimeError(f'{what}: inconsistent shapes')
    _shapes(what, p, (off1, off2, hyp_off, out_off), nbr1, nbr1.numel() // 8, nbr2, nbr2.numel() // 8, params, workspace, hypotheses)
    check(lib.cvpce_tonioni_select(_p(nbr1), _p(off1), _p(nbr2), _p(off2), _p(params), _p(hyp_off), _p(out_off), p, nbr1.numel() // 8,
                                   nbr2.numel() // 8, max_n1, max_n2, max_hyp, pairs.shape[0], hypotheses, _p(workspace),
                                   workspace.numel() * 4, _p(pairs), _p(count), _stream()), what)
