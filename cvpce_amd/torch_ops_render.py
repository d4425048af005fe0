"""PyTorch-ROCm custom op over the compliance pictures' compositor of include/cvpce_amd_render.h: `torch.ops.cvpce_amd.render_canvases`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.
"""
import torch

from ._lib import lib, check
from .torch_ops import _p, _stream, registrar

NAMES, _op = registrar()
TILE_W, TILE_H = 64, 16           # CVPCE_RENDER_TILE_W, CVPCE_RENDER_TILE_H
MAX_SIDE = 32768                  # CVPCE_RENDER_MAX_SIDE
TABLE_COLS = 10                   # CVPCE_RENDER_TABLE_COLS
SRC_NONE, SRC_BASE = -1, -2       # CVPCE_RENDER_SRC_*


def tiles(h, w):
    """CVPCE_RENDER_TILES: the workgroups an h x w canvas takes"""
    return ((int(h) + TILE_H - 1) // TILE_H) * ((int(w) + TILE_W - 1) // TILE_W)


@_op('render_canvases(Tensor canvases, int total_tiles, Tensor? base, Tensor box, Tensor src, Tensor colour, Tensor thickness, Tensor atlas, '
     'Tensor atlas_rows, int background, Tensor(a!) out) -> ()')
def _render_canvases(canvases, total_tiles, base, box, src, colour, thickness, atlas, atlas_rows, background, out):
    what = 'cvpce_render_canvases'
    u8 = (atlas, out) + (() if base is None else (base,))
    i32 = (src, colour, thickness, atlas_rows)
    if (canvases.dtype != torch.int64 or box.dtype != torch.float32 or any(t.dtype != torch.uint8 for t in u8)
            or any(t.dtype != torch.int32 for t in i32)):
        raise RuntimeError(f'{what}: the canvas table is int64, the boxes float32, the output, the base and the atlas uint8, everything else int32')
    if not all(t.is_contiguous() for t in (canvases, box) + u8 + i32):
        raise RuntimeError(f'{what}: contiguous tensors only')
    n = src.numel()
    if (canvases.dim() != 2 or canvases.shape[1] != TABLE_COLS or tuple(box.shape) != (n, 4) or colour.numel() != n or thickness.numel() != n
            or any(t.dim() != 1 for t in u8 + (src, colour, thickness)) or atlas_rows.dim() != 2 or atlas_rows.shape[1] != 3
            or not 0 <= int(total_tiles) < 2 ** 31):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_render_canvases(_p(canvases), canvases.shape[0], int(total_tiles), _p(out), out.numel(), _p(base),
                                    0 if base is None else base.numel(), _p(box), _p(src), _p(colour), _p(thickness), n, _p(atlas), atlas.numel(),
                                    _p(atlas_rows), atlas_rows.shape[0], int(background) & 0xFFFFFF, _stream()), what)
