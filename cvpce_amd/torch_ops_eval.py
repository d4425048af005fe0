"""PyTorch-ROCm custom ops over the evaluation kernels of include/cvpce_amd_eval.h: `torch.ops.cvpce_amd.eval_*`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
import torch

from ._lib import lib, check
from .torch_ops import _p, _stream, registrar

NAMES, _op = registrar()


@_op('eval_match_detections(Tensor pred, Tensor pred_off, Tensor rank, Tensor? pred_cls, Tensor tgt, Tensor tgt_off, '
     'Tensor? tgt_cls, Tensor thr, int max_targets, Tensor(a!) first, Tensor(b!) tp) -> ()')
def _eval_match_detections(pred, pred_off, rank, pred_cls, tgt, tgt_off, tgt_cls, thr, max_targets, first, tp):
    n, sum_p, sum_t, k = pred_off.numel() - 1, pred.shape[0], tgt.shape[0], thr.numel()
    i32 = (pred_off, rank, tgt_off, first) + tuple(t for t in (pred_cls, tgt_cls) if t is not None)
    if any(t.dtype != torch.float32 for t in (pred, tgt, thr)) or any(t.dtype != torch.int32 for t in i32) or tp.dtype != torch.uint8:
        raise RuntimeError('cvpce_eval_match_detections: boxes and thresholds are float32, offsets / ranks / class ids / first int32, tp uint8')
    if not all(t.is_contiguous() for t in (pred, tgt, thr, tp) + i32):
        raise RuntimeError('cvpce_eval_match_detections: contiguous tensors only')
    if (pred.dim() != 2 or pred.shape[1] != 4 or tgt.dim() != 2 or tgt.shape[1] != 4 or tgt_off.numel() != n + 1 or rank.numel() != sum_p
            or first.numel() != k * sum_t or tp.numel() != k * sum_p
            or (pred_cls is not None and pred_cls.numel() != sum_p) or (tgt_cls is not None and tgt_cls.numel() != sum_t)):
        raise RuntimeError('cvpce_eval_match_detections: inconsistent shapes')
    check(lib.cvpce_eval_match_detections(_p(pred), _p(pred_off), _p(rank), _p(pred_cls), _p(tgt), _p(tgt_off), _p(tgt_cls), _p(thr),
                                          n, sum_p, sum_t, max_targets, k, _p(first), _p(tp), _stream()), 'cvpce_eval_match_detections')
