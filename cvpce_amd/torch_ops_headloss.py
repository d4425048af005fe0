"""PyTorch-ROCm custom op over the head-loss kernels of include/cvpce_amd_headloss.h: `torch.ops.cvpce_amd.headloss` issues the memset
and the three launches (headloss_match, headloss_terms, headloss_finish) of one batch.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
import ctypes

from ._lib import lib, check
from .torch_ops import _p, _stream, registrar, typed

NAMES, _op = registrar()
CHUNK, THREADS, MAX_LEVELS = 1024, 256, 8   # CVPCE_HEADLOSS_CHUNK, CVPCE_HEADLOSS_THREADS, CVPCE_HEADLOSS_MAX_LEVELS


def _ints(values):
    return (ctypes.c_int * len(values))(*[int(v) for v in values])


def workspace_bytes(gh, gw, num_anchors, n, sum_t):
    """Host-only size query of `headloss`'s workspace; 0 for a shape it refuses."""
    return int(lib.cvpce_headloss_workspace_bytes(_ints(gh), _ints(gw), len(gh), int(num_anchors), int(n), int(sum_t)))


@_op('headloss(Tensor[] logits, Tensor[] regs, int[] gh, int[] gw, int[] sh, int[] sw, Tensor base_anchors, Tensor boxes, Tensor labels, '
     'Tensor box_offsets, Tensor scales, int num_anchors, int num_classes, Tensor(a!) workspace, Tensor(b!) matched, Tensor(c!) out_f, '
     'Tensor(d!) out_i) -> ()')
def _headloss(logits, regs, gh, gw, sh, sw, base_anchors, boxes, labels, box_offsets, scales, num_anchors, num_classes, workspace, matched,
              out_f, out_i):
    what = 'cvpce_headloss'
    L, n = len(logits), out_f.shape[0]
    typed(what, f32=(*logits, *regs, base_anchors, boxes, scales, out_f), i32=(labels, box_offsets, matched, out_i), u8=(workspace,))
    if not (1 <= L <= MAX_LEVELS and len(regs) == len(gh) == len(gw) == len(sh) == len(sw) == L):
        raise RuntimeError(f'{what}: one logits, regs, grid and stride entry per level, at most {MAX_LEVELS} levels')
    cells = [int(h) * int(w) * num_anchors for h, w in zip(gh, gw)]
    for lg, rg, c in zip(logits, regs, cells):
        if lg.numel() != n * c * num_classes or rg.numel() != n * c * 4:
            raise RuntimeError(f'{what}: a level holds N * gh * gw * A * K logits and N * gh * gw * A * 4 regressions')
    sum_t = labels.numel()
    if tuple(base_anchors.shape) != (L, num_anchors, 4) or boxes.numel() != 4 * sum_t or tuple(box_offsets.shape) != (n + 1,) \
            or tuple(scales.shape) != (n, 2) or tuple(matched.shape) != (n, sum(cells)) or tuple(out_f.shape) != (n, 2) \
            or tuple(out_i.shape) != (n, 3):
        raise RuntimeError(f'{what}: inconsistent shapes')
    lp = (ctypes.c_void_p * L)(*[t.data_ptr() for t in logits])
    rp = (ctypes.c_void_p * L)(*[t.data_ptr() for t in regs])
    check(lib.cvpce_headloss(lp, rp, _ints(gh), _ints(gw), _ints(sh), _ints(sw), _p(base_anchors), _p(boxes) if sum_t else ctypes.c_void_p(0),
                             _p(labels) if sum_t else ctypes.c_void_p(0), _p(box_offsets), _p(scales), L, n, num_anchors, num_classes, sum_t,
                             _p(workspace), workspace.numel(), _p(matched), _p(out_f), _p(out_i), _stream()), what)
