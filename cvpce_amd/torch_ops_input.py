"""PyTorch-ROCm custom ops over the 8-bit input kernels of include/cvpce_amd_input.h: `torch.ops.cvpce_amd.*_u8`.

The rules of torch_ops.py hold: CUDA (= HIP on ROCm) dispatch key only, out-variants on the current stream, no allocation, no
synchronisation.  Every op checks its image arguments itself and raises before the library is called: a byte image is a
contiguous (H,W,3) uint8 tensor on the device, `table` the 256 float32 values of the codes (ops.uint8_table) on the same device.
"""
import ctypes

import torch

from . import _lib
from ._lib import lib, check
from .torch_ops import _p, _stream, _by_dtype, registrar

NAMES, _op = registrar()


def _is_bytes(what, img):
    """True for a byte image, False for float planes; anything else raises."""
    if not img.is_cuda:
        raise RuntimeError(f'{what}: the image is not on the device (no CPU fallback)')
    if img.dtype == torch.uint8:
        if img.dim() != 3 or img.shape[2] != 3 or not img.is_contiguous():
            raise RuntimeError(f'{what}: a byte image is a contiguous (H,W,3) uint8 tensor, got {tuple(img.shape)} strides {tuple(img.stride())}')
        return True
    if img.dtype != torch.float32 or img.dim() != 3 or img.shape[0] != 3 or not img.is_contiguous():
        raise RuntimeError(f'{what}: images must be contiguous (H,W,3) uint8 or (3,H,W) float32 tensors')
    return False


def _check_table(what, table, img):
    if table.dtype != torch.float32 or table.numel() != 256 or not table.is_contiguous() or table.device != img.device:
        raise RuntimeError(f'{what}: table must be the 256 float32 code values on the image\'s device')


@_op('gln_transform_batch_u8(Tensor[] imgs, Tensor table, Tensor(a!) batch, int[] h, int[] w, float[] mean, float[] std) -> ()')
def _gln_transform_batch_u8(imgs, table, batch, h, w, mean, std):
    n, hp, wp, _ = batch.shape
    if len(imgs) != n or len(h) != n or len(w) != n:
        raise RuntimeError('gln_transform_batch_u8: one image and one resized size per batch slot')
    forms = [_is_bytes('gln_transform_batch_u8', t) for t in imgs]
    _check_table('gln_transform_batch_u8', table, batch)
    ci = lambda v: (ctypes.c_int * n)(*[int(x) for x in v])
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in imgs])
    fn = _by_dtype(batch, 'cvpce_gln_transform_batch_u8', 'cvpce_gln_transform_batch_u8_f16')
    check(fn(ptrs, (ctypes.c_ubyte * n)(*[int(f) for f in forms]), ci([t.shape[0] if f else t.shape[1] for t, f in zip(imgs, forms)]),
             ci([t.shape[1] if f else t.shape[2] for t, f in zip(imgs, forms)]), ci(h), ci(w), n, _p(batch), hp, wp,
             _lib.float3(mean), _lib.float3(std), _p(table), _stream()), 'gln_transform_batch_u8')


def _crop_args(what, img, table, boxes):
    if not _is_bytes(what, img):
        raise RuntimeError(f'{what}: the image must be a contiguous (H,W,3) uint8 tensor')
    _check_table(what, table, img)
    if boxes.dtype != torch.float32 or not boxes.is_contiguous():
        raise RuntimeError(f'{what}: boxes must be a contiguous (P,4) float32 tensor')


@_op('crop_resize_u8(Tensor img, Tensor table, Tensor boxes, Tensor? count, Tensor(a!) out, int size, int mode, float[]? mean, float[]? std) -> ()')
def _crop_resize_u8(img, table, boxes, count, out, size, mode, mean, std):
    _crop_args('crop_resize_u8', img, table, boxes)
    check(lib.cvpce_crop_resize_u8(_p(img), _p(table), _p(boxes), _p(count), boxes.shape[0], _p(out), img.shape[0], img.shape[1], size, mode,
                                   _lib.float3(mean) if mean is not None else None, _lib.float3(std) if std is not None else None,
                                   _stream()), 'crop_resize_u8')


@_op('crop_resize_content_u8(Tensor img, Tensor table, Tensor boxes, Tensor? count, Tensor(a!) out, int size, int mode, float[] mean, float[] std, '
     'Tensor ext) -> ()')
def _crop_resize_content_u8(img, table, boxes, count, out, size, mode, mean, std, ext):
    _crop_args('crop_resize_content_u8', img, table, boxes)
    if ext.dtype != torch.int32 or not ext.is_contiguous() or ext.shape != (boxes.shape[0], 2):
        raise RuntimeError('crop_resize_content_u8: ext must be a contiguous (P,2) int32 tensor')
    check(lib.cvpce_crop_resize_content_u8(_p(img), _p(table), _p(boxes), _p(count), boxes.shape[0], _p(out), img.shape[0], img.shape[1], size,
                                           mode, _lib.float3(mean), _lib.float3(std), _p(ext), _stream()), 'crop_resize_content_u8')
