"""PyTorch-ROCm custom ops over the Gaussian-map scoring kernels of include/cvpce_amd_gaussians.h: `torch.ops.cvpce_amd.gauss_kant_table`,
`gauss_targets` and `gauss_loss`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
import ctypes

from ._lib import lib, check
from .torch_ops import _p, _stream, registrar, typed

NAMES, _op = registrar()
GEOM = 5                                    # CVPCE_GAUSS_GEOM: H0, W0, r, h, w per image
TILE, LIST = 16, 256                        # CVPCE_GAUSS_TILE, CVPCE_GAUSS_LIST
METHODS = {'multivariate_normal': 0, 'kant_method': 1, 'simple_and_scaled': 2}
JOINS = {'max': 0, 'addition': 1, 'replacement': 2}


def loss_workspace_bytes(n, hb, wb):
    """Host-only size query of `gauss_loss`'s workspace; 0 for a shape it refuses."""
    return int(lib.cvpce_gauss_loss_workspace_bytes(int(n), int(hb), int(wb)))


@_op('gauss_kant_table(Tensor(a!) out, int sigma) -> ()')
def _gauss_kant_table(out, sigma):
    what = 'cvpce_gauss_kant_table'
    typed(what, f32=(out,))
    if out.dim() != 2 or out.shape[0] != out.shape[1]:
        raise RuntimeError(f'{what}: the table is square')
    check(lib.cvpce_gauss_kant_table(_p(out), out.shape[0], sigma, _stream()), what)


@_op('gauss_targets(Tensor? boxes, Tensor? box_offsets, Tensor? map_ptrs, Tensor geom, Tensor? table, int method, int join, '
     'float p0, float p1, float p2, int tanh, int resize, Tensor(a!) out) -> ()')
def _gauss_targets(boxes, box_offsets, map_ptrs, geom, table, method, join, p0, p1, p2, tanh, resize, out):
    what = 'cvpce_gauss_targets'
    typed(what, i32=(boxes, box_offsets, geom), i64=(map_ptrs,), f32=(table, out))
    if out.dim() != 4 or out.shape[1] != 1:
        raise RuntimeError(f'{what}: the output is (N,1,Hb,Wb)')
    n, _, hb, wb = out.shape
    if tuple(geom.shape) != (n, GEOM):
        raise RuntimeError(f'{what}: geom is (N,{GEOM})')
    if (map_ptrs is None) == (box_offsets is None):
        raise RuntimeError(f'{what}: boxes with offsets, or maps')
    sum_b = 0
    if map_ptrs is not None:
        if boxes is not None or tuple(map_ptrs.shape) != (n,):
            raise RuntimeError(f'{what}: one map address per image and no boxes')
    else:
        if boxes is None or boxes.dim() != 2 or boxes.shape[1] != 4 or tuple(box_offsets.shape) != (n + 1,):
            raise RuntimeError(f'{what}: boxes are (sumB,4), offsets (N+1,)')
        sum_b = boxes.shape[0]
    if table is not None and (table.dim() != 2 or table.shape[0] != table.shape[1]):
        raise RuntimeError(f'{what}: the table is square')
    params = (ctypes.c_float * 3)(p0, p1, p2)
    check(lib.cvpce_gauss_targets(_p(boxes) if sum_b else ctypes.c_void_p(0), _p(box_offsets), _p(map_ptrs), _p(geom), _p(table),
                                  table.shape[0] if table is not None else 0, sum_b, n, hb, wb, method, join, params, tanh, resize, _p(out),
                                  _stream()), what)


@_op('gauss_loss(Tensor pred, Tensor target, Tensor? extent, float negative_threshold, float positive_threshold, int min_negatives, '
     'int negatives_per_positive, int per_image, Tensor(a!) workspace, Tensor(b!) out_f, Tensor(c!) out_i) -> ()')
def _gauss_loss(pred, target, extent, negative_threshold, positive_threshold, min_negatives, negatives_per_positive, per_image, workspace,
                out_f, out_i):
    what = 'cvpce_gauss_loss'
    typed(what, f32=(pred, target, out_f), i32=(extent, out_i), u8=(workspace,))
    if pred.dim() != 4 or pred.shape[1] != 1 or pred.shape != target.shape:
        raise RuntimeError(f'{what}: predictions and targets are (N,1,Hb,Wb)')
    n, _, hb, wb = pred.shape
    segments = n if per_image else 1
    if (per_image and (extent is None or tuple(extent.shape) != (n, 2))) or tuple(out_f.shape) != (segments, 3) \
            or tuple(out_i.shape) != (segments, 2):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_gauss_loss(_p(pred), _p(target), _p(extent), n, hb, wb, negative_threshold, positive_threshold, min_negatives,
                               negatives_per_positive, per_image, _p(workspace), workspace.numel(), _p(out_f), _p(out_i), _stream()), what)
