"""PyTorch-ROCm custom op over the gallery kernel of include/cvpce_amd_gallery.h: `torch.ops.cvpce_amd.gallery_pack_u8`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.  The op checks every tensor itself and raises before the library is called: `data` a flat contiguous uint8
buffer, `geom` (n,3) int32, `table` (3,257) bf16 (ops.gallery_table), `out` (n,S,S,4|8) bf16, `ext` (n,2) int32, all contiguous
and on one device.
"""
import torch

from ._lib import lib, check
from .torch_ops import _p, _stream, registrar

NAMES, _op = registrar()


def _check(data, geom, table, out, ext):
    what = 'gallery_pack_u8'
    for name, t in (('data', data), ('geom', geom), ('table', table), ('out', out), ('ext', ext)):
        if not t.is_cuda:
            raise RuntimeError(f'{what}: {name} is not on the device (no CPU fallback)')
        if t.device != out.device:
            raise RuntimeError(f'{what}: {name} is on {t.device}, out on {out.device}')
        if not t.is_contiguous():
            raise RuntimeError(f'{what}: {name} must be contiguous, got strides {tuple(t.stride())}')
    if data.dtype != torch.uint8 or data.dim() != 1:
        raise RuntimeError(f'{what}: data must be a flat uint8 buffer (the images back to back), got {data.dtype} {tuple(data.shape)}')
    if out.dtype != torch.bfloat16 or out.dim() != 4 or out.shape[1] != out.shape[2] or out.shape[3] not in (4, 8):
        raise RuntimeError(f'{what}: out must be (n,S,S,4) or (n,S,S,8) bfloat16, got {out.dtype} {tuple(out.shape)}')
    n = out.shape[0]
    if geom.dtype != torch.int32 or tuple(geom.shape) != (n, 3):
        raise RuntimeError(f'{what}: geom must be ({n},3) int32 (byte offset, h, w per image), got {geom.dtype} {tuple(geom.shape)}')
    if ext.dtype != torch.int32 or tuple(ext.shape) != (n, 2):
        raise RuntimeError(f'{what}: ext must be ({n},2) int32, got {ext.dtype} {tuple(ext.shape)}')
    if table.dtype != torch.bfloat16 or tuple(table.shape) != (3, 257):
        raise RuntimeError(f'{what}: table must be (3,257) bfloat16 (256 codes + the padding per channel), got {table.dtype} {tuple(table.shape)}')
    if n and data.numel() == 0:
        raise RuntimeError(f'{what}: {n} images but an empty byte buffer')


@_op('gallery_pack_u8(Tensor data, Tensor geom, Tensor table, Tensor(a!) out, int content_only, Tensor(b!) ext) -> ()')
def _gallery_pack_u8(data, geom, table, out, content_only, ext):
    _check(data, geom, table, out, ext)
    n, size, _, channels = out.shape
    if n == 0:
        return
    check(lib.cvpce_gallery_pack_u8(_p(data), _p(geom), _p(table), _p(out), n, size, channels, int(content_only), _p(ext), _stream()),
          'gallery_pack_u8')
