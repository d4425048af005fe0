"""CPU-side checks of the 8-bit gallery path (no compute on a GPU): the readers' uint8 items stand for their float items bit for bit
(`datautils.gallery_float`), include/cvpce_amd_gallery.h is a header of its own with a signature table and an op list of
its own, and the host packing of a byte pass (`production.pack_gallery_bytes`) lays the images out back to back."""
import ctypes
import os

import numpy as np
import pytest
import torch

import abi


# ---------------------------------------------------------------------------------------------------------------------------------
# readers
# ---------------------------------------------------------------------------------------------------------------------------------
def _noise(h, w, c, seed):
    return np.random.RandomState(seed).randint(0, 256, (h, w, c) if c else (h, w), dtype=np.uint8)


@pytest.fixture(scope='module')
def gp_tree(tmp_path_factory):
    """A GP-shaped training tree with one file per case of the reader: tall, wide, square, grey ('L'), RGBA, palette, and an image whose
    resized width is 1."""
    from PIL import Image
    root = tmp_path_factory.mktemp('gallery_u8') / 'Training'
    (root / 'Food' / 'Tea').mkdir(parents=True)
    (root / 'Drinks').mkdir()
    Image.fromarray(_noise(300, 120, 3, 0)).save(root / 'Food/Tea/1_tall.png')
    Image.fromarray(_noise(90, 400, 3, 1)).save(root / 'Food/Tea/2_wide.png')
    Image.fromarray(_noise(200, 200, 3, 2)).save(root / 'Food/Tea/3_square.png')
    Image.fromarray(_noise(130, 77, 0, 3), 'L').save(root / 'Food/4_grey.png')
    Image.fromarray(_noise(64, 150, 4, 4), 'RGBA').save(root / 'Food/5_alpha.png')
    Image.fromarray(_noise(101, 99, 3, 5)).convert('P', palette=Image.ADAPTIVE, colors=64).save(root / 'Drinks/6_palette.png')
    Image.fromarray(_noise(600, 2, 3, 6)).save(root / 'Drinks/7_sliver.png')
    return str(root)


def test_reader_items_stand_for_the_float_items(gp_tree):
    from cvpce_amd import datautils
    data_f = datautils.GroceryProductsDataset([gp_tree], include_annotations=True)
    data_u = datautils.GroceryProductsDataset([gp_tree], include_annotations=True, image_format='uint8')
    assert len(data_f) == len(data_u) == 7
    shapes = {}
    for i in range(len(data_f)):
        f, u = data_f[i], data_u[i]
        assert len(u) == 4 and u[0] is u[1]
        img = u[0]
        assert img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3 and img.is_contiguous()
        assert max(img.shape[:2]) == 256 and min(img.shape[:2]) >= 1
        assert f[0].shape == (3, 256, 256) and f[0].dtype == torch.float32
        assert torch.equal(datautils.gallery_float(img), f[0]), data_f.annotations[i]
        assert u[2] == f[2] and u[3] == f[3]
        shapes[u[3].split('/')[-1]] = tuple(img.shape[:2])
    assert shapes['1_tall'] == (256, 102) and shapes['2_wide'] == (58, 256) and shapes['3_square'] == (256, 256)
    assert shapes['7_sliver'] == (256, 1)
    # without annotations: three fields, the same image
    assert len(datautils.GroceryProductsDataset([gp_tree], image_format='uint8')[0]) == 3


def test_internal_trainset_alpha_to_white_on_bytes(tmp_path):
    from PIL import Image
    from cvpce_amd import datautils
    (tmp_path / 'front').mkdir()
    a = _noise(120, 180, 4, 7)
    a[:40, :, 3] = 0                      # transparent pixels (whatever their colour bytes are) become white
    a[40:80, :, 3] = 255
    Image.fromarray(a, 'RGBA').save(tmp_path / 'front/12345.png')
    Image.fromarray(_noise(50, 30, 3, 8)).save(tmp_path / 'front/777.png')     # (a file without alpha: nothing is transparent)
    data_f = datautils.InternalTrainSet(str(tmp_path), include_annotations=True)
    data_u = datautils.InternalTrainSet(str(tmp_path), include_annotations=True, image_format='uint8')
    assert data_u.annotations == data_f.annotations == ['12345', '777']
    for i in range(2):
        f, u = data_f[i], data_u[i]
        assert u[0].dtype == torch.uint8 and torch.equal(datautils.gallery_float(u[0]), f[0])
        assert u[2:] == f[2:]
    rows = round(256 * 40 / 180)          # the transparent band, resized: white well inside it
    assert bool((data_u[0][0][:rows - 2] == 255).all())


def test_image_format_is_validated(gp_tree, tmp_path):
    from cvpce_amd import datautils
    with pytest.raises(ValueError, match='image_format'):
        datautils.GroceryProductsDataset([gp_tree], image_format='bytes')
    with pytest.raises(ValueError, match='image_format'):
        datautils.InternalTrainSet(gp_tree, image_format='u8')
    with pytest.raises(ValueError, match='resize'):
        datautils.GroceryProductsDataset([gp_tree], image_format='uint8', resize=False)
    with pytest.raises(ValueError, match='resize'):
        datautils.InternalTrainSet(gp_tree, image_format='uint8', resize=False)
    assert datautils.GroceryProductsDataset([gp_tree]).image_format == 'float'          # the default is today's items
    assert datautils.GroceryProductsDataset([gp_tree], resize=False)[0][0].dtype == torch.float32


def test_gallery_float_is_the_contract():
    """content = uint8_table[b] * 2 - 1 in torch float32, 0.0 beyond (h, w); every code, in every channel"""
    from cvpce_amd import datautils, ops
    codes = torch.arange(256, dtype=torch.uint8).view(16, 16, 1).expand(16, 16, 3).contiguous()
    g = datautils.gallery_float(codes, 32)
    want = ops.uint8_table() * 2 - 1
    assert g.shape == (3, 32, 32) and g.dtype == torch.float32
    for c in range(3):
        assert torch.equal(g[c, :16, :16].reshape(-1), want)
    assert bool((g[:, 16:] == 0).all()) and bool((g[:, :, 16:] == 0).all())
    assert float(want[0]) == -1.0 and float(want[255]) == 1.0
    with pytest.raises(ValueError):
        datautils.gallery_float(torch.zeros(33, 4, 3, dtype=torch.uint8), 32)
    with pytest.raises(TypeError):
        datautils.gallery_float(torch.zeros(3, 4, 4), 32)


# ---------------------------------------------------------------------------------------------------------------------------------
# boundary
# ---------------------------------------------------------------------------------------------------------------------------------
def test_library_exports_the_gallery_symbol():
    """(exported, bound and disjoint from the other headers: test_abi_mirror_cpu.py)"""
    assert abi.header_symbols('cvpce_amd_gallery.h') == ['cvpce_gallery_pack_u8']


def test_gallery_op_matches_the_header_on_the_gpu_only():
    from cvpce_amd import torch_ops_gallery  # noqa: F401  (registers the op; name and keys: test_abi_mirror_cpu.py)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.gallery_pack_u8(torch.zeros(48, dtype=torch.uint8), torch.zeros(1, 3, dtype=torch.int32),
                                            torch.zeros(3, 257, dtype=torch.bfloat16), torch.zeros(1, 4, 4, 4, dtype=torch.bfloat16), 0,
                                            torch.zeros(1, 2, dtype=torch.int32))


def test_host_side_argument_checks():
    """What the entry point refuses before it touches the device."""
    from cvpce_amd._lib import lib
    one = ctypes.c_void_p(64)        # (never dereferenced: every call below is refused on its arguments, or has nothing to do)
    f = lib.cvpce_gallery_pack_u8
    for null_at in range(4):
        ptrs = [None if i == null_at else one for i in range(4)]
        assert f(*ptrs, 1, 256, 4, 0, one, None) == 1
    assert f(one, one, one, one, 1, 256, 4, 0, None, None) == 1             # no ext_out
    assert f(one, one, one, one, 1, 0, 4, 0, one, None) == 1                # S <= 0
    assert f(one, one, one, one, 1, -16, 4, 0, one, None) == 1
    for c in (0, 3, 5, 16):
        assert f(one, one, one, one, 1, 256, c, 0, one, None) == 1          # C not 4 or 8
    assert f(one, one, one, one, 10923, 256, 8, 0, one, None) == 1          # n * S * S * 3 = 2^31 + 196 608
    assert f(one, one, one, one, 2, 32768, 4, 1, one, None) == 1
    assert f(one, one, one, one, 65536, 16, 4, 0, one, None) == 1           # n above the grid limit (65 535), 32-bit offsets fine
    assert f(one, one, one, one, -1, 256, 4, 0, one, None) == 1
    for c in (4, 8):
        assert f(one, one, one, one, 0, 256, c, 0, one, None) == 0          # n = 0: nothing to do, nothing launched
        assert f(one, one, one, one, 0, 256, c, 1, one, None) == 0


# ---------------------------------------------------------------------------------------------------------------------------------
# the host side of a byte pass
# ---------------------------------------------------------------------------------------------------------------------------------
def test_pack_gallery_bytes_layout_and_round_trip():
    from cvpce_amd import production
    g = torch.Generator().manual_seed(3)
    sizes = [(1, 256), (256, 1), (5, 7), (256, 255), (33, 64)]
    images = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for h, w in sizes]
    buf = torch.full((6 * 256 * 256 * 3,), 0xEE, dtype=torch.uint8)
    geom = torch.full((6, 3), -7, dtype=torch.int32)
    used = production.pack_gallery_bytes(images, buf, geom)
    assert used == sum(3 * h * w for h, w in sizes)
    off = 0
    for i, (img, (h, w)) in enumerate(zip(images, sizes)):
        assert geom[i].tolist() == [off, h, w]                               # back to back: no alignment between images
        assert torch.equal(buf[off:off + 3 * h * w].view(h, w, 3), img)
        off += 3 * h * w
    assert any(int(o) % 4 for o in geom[:5, 0])                              # (the layout is ragged: image starts are not aligned)
    assert bool((buf[used:] == 0xEE).all()) and geom[5].tolist() == [-7, -7, -7]
    assert production.pack_gallery_bytes([], buf, geom) == 0
    # a non-contiguous image (a view) is copied in its logical order
    view = images[3][:, ::2]
    production.pack_gallery_bytes([view], buf, geom)
    assert geom[0].tolist() == [0, 256, 128] and torch.equal(buf[:view.numel()].view(256, 128, 3), view)


def test_pack_gallery_bytes_refuses_what_is_no_gallery_byte_image():
    from cvpce_amd import production
    buf, geom = torch.zeros(256 * 256 * 3, dtype=torch.uint8), torch.zeros((1, 3), dtype=torch.int32)
    ok = torch.zeros(4, 4, 3, dtype=torch.uint8)
    for bad in (torch.zeros(257, 4, 3, dtype=torch.uint8), torch.zeros(4, 0, 3, dtype=torch.uint8), torch.zeros(3, 4, 4, dtype=torch.uint8),
                torch.zeros(4, 4, 3)):
        with pytest.raises(ValueError):
            production.pack_gallery_bytes([ok, bad], buf, geom)
    with pytest.raises(ValueError, match='fit'):
        production.pack_gallery_bytes([ok, ok], buf, geom)                   # two images, one geom row
    with pytest.raises(ValueError, match='fit'):
        production.pack_gallery_bytes([ok], buf[:47], geom)
    assert production.is_gallery_bytes(ok) and not production.is_gallery_bytes(torch.zeros(3, 4, 4)) and not production.is_gallery_bytes('x')


def test_gallery_switch_defaults_on():
    from cvpce_amd import production
    assert production.GALLERY_U8 is (os.environ.get('CVPCE_GALLERY_U8', '1') != '0')
