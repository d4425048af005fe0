"""PyTorch-ROCm custom op over the step pictures' strokes of include/ext/cvpce_amd_strokes.h: `torch.ops.cvpce_amd.strokes_draw`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, an out-variant on the current stream, no allocation, no
synchronisation.
"""
from ._lib import lib, check
from .torch_ops import _p, _stream, registrar, typed

NAMES, _op = registrar()
TILE_W, TILE_H = 64, 16           # CVPCE_STROKES_TILE_W, CVPCE_STROKES_TILE_H
MAX_SIDE = 32768                  # CVPCE_STROKES_MAX_SIDE
MAX_RADIUS = 64                   # CVPCE_STROKES_MAX_RADIUS, half pixels
TABLE_COLS = 6                    # CVPCE_STROKES_TABLE_COLS


def tiles(h, w):
    """the workgroups an h x w canvas takes"""
    return ((int(h) + TILE_H - 1) // TILE_H) * ((int(w) + TILE_W - 1) // TILE_W)


@_op('strokes_draw(Tensor canvases, int total_tiles, Tensor ends, Tensor colour, Tensor radius, Tensor(a!) out) -> ()')
def _strokes_draw(canvases, total_tiles, ends, colour, radius, out):
    what = 'cvpce_strokes_draw'
    typed(what, i64=(canvases,), f32=(ends,), i32=(colour, radius), u8=(out,))
    n = colour.numel()
    if (canvases.dim() != 2 or canvases.shape[1] != TABLE_COLS or tuple(ends.shape) != (n, 4) or colour.dim() != 1 or tuple(radius.shape) != (n,)
            or out.dim() != 1 or not 0 <= int(total_tiles) < 2 ** 31):
        raise RuntimeError(f'{what}: inconsistent shapes')
    check(lib.cvpce_strokes_draw(_p(canvases), canvases.shape[0], int(total_tiles), _p(out), out.numel(), _p(ends), _p(colour), _p(radius), n,
                                 _stream()), what)
