"""The 8-bit gallery path on the GPU (csrc/gallery.hip, include/cvpce_amd_gallery.h): the byte kernel's pixels are the float
path's bits, it reads and writes only what it is given, and `Classifier.build_index` over gallery byte images gives the embeddings of the
float items they stand for, bit for bit, on every schedule."""
import os
import subprocess
import sys

import pytest
import torch

import footprint as fp

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RESNET_MEAN, RESNET_STD = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)        # MACResNet.input_mean / input_std
SENTINEL = 0x7FA5                                                 # a bf16 NaN pattern no kernel computes (footprint's prefill)


def _norms():
    from cvpce_amd.models import classification as C
    return {'macvgg': (C.TANH_MEAN, C.TANH_STD), 'macresnet': (RESNET_MEAN, RESNET_STD)}


def _shapes(S):
    """The issue's seven images of one launch: odd widths make rows and image starts unaligned."""
    return [(S, S), (S, 1), (1, S), (S, S - 1), (S - 3, S), (5, 7), (S, S)]


def _images(S, seed=0):
    """Byte images of `_shapes(S)`; the first holds all 256 codes in every channel (a different order per channel)."""
    g = torch.Generator().manual_seed(seed)
    images = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for h, w in _shapes(S)]
    codes = torch.arange(S * S) % 256
    images[0] = torch.stack([codes[torch.randperm(S * S, generator=g)] for _ in range(3)], dim=1).to(torch.uint8).view(S, S, 3).contiguous()
    for c in range(3):
        assert len(set(images[0][:, :, c].reshape(-1).tolist())) == 256
    return images


def _packed_host(images, S):
    """-> (flat uint8 buffer of exactly the bytes used, geom (n,3) int32), on the host: production's own packing"""
    from cvpce_amd import production
    buf = torch.empty(max(1, sum(i.numel() for i in images)), dtype=torch.uint8)
    geom = torch.empty((len(images), 3), dtype=torch.int32)
    used = production.pack_gallery_bytes(images, buf, geom, S)
    return buf[:max(used, 1)], geom


def _reference(images, S, mean, std, dev):
    """what the float path packs for the float images the byte images stand for: (n,S,S,8) bf16"""
    from cvpce_amd import datautils, ops
    return ops.pack_embed_input(torch.stack([datautils.gallery_float(u, S) for u in images]).to(dev), False, mean, std)


def _content_mask(images, S):
    m = torch.zeros(len(images), S, S, 1, dtype=torch.bool)
    for i, u in enumerate(images):
        m[i, :u.shape[0], :u.shape[1]] = True
    return m


@pytest.fixture(scope='module')
def vgg(cuda):
    from cvpce_amd import synthetic
    return synthetic.synthetic_macvgg(seed=1).to(cuda)


@pytest.fixture(scope='module')
def resnet(cuda):
    from cvpce_amd.models import classification as C
    state = torch.random.get_rng_state()
    torch.manual_seed(4)
    try:
        m = C.macresnet_encoder(pretrained=False)
        for mod in m.modules():
            if isinstance(mod, torch.nn.BatchNorm2d):
                mod.running_mean.normal_(0, 0.1); mod.running_var.uniform_(0.5, 1.5)
                mod.weight.data.uniform_(0.4, 0.8); mod.bias.data.normal_(0, 0.1)
    finally:
        torch.random.set_rng_state(state)
    return m.to(cuda)


# ---------------------------------------------------------------------------------------------------------------------------------
# the kernel
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('norm', ['macvgg', 'macresnet'])
@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('S', [16, 256])
def test_kernel_bits(cuda, vgg, S, C, norm):
    from cvpce_amd import ops
    mean, std = _norms()[norm]
    images = _images(S)
    n = len(images)
    buf, geom = _packed_host(images, S)
    assert any(int(o) % 2 for o in geom[:, 0])                               # image starts are unaligned
    data, geom_dev = buf.to(cuda), geom.to(cuda)
    out, ext = ops.gallery_pack_u8(data, geom_dev, n, S, C, mean, std)
    assert out.shape == (n, S, S, C) and out.dtype == torch.bfloat16 and ext.shape == (n, 2) and ext.dtype == torch.int32
    ref = _reference(images, S, mean, std, cuda)
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(out[..., :3]), bits(ref[..., :3]))              # channels 0-2: the float path's bits, content and padding
    assert bool((bits(out[..., 3:]) == 0).all())                             # channels 3..: bf16 zero everywhere
    assert ext.cpu().tolist() == [list(s) for s in _shapes(S)]
    # the padding is the pixel of the all-padding crop the work-list schedule reads instead of it
    const = vgg.engine().const_crop(mean, std, C, S)
    assert const.shape == (S, S, C) and bool((bits(const) == bits(const[0, 0])).all())
    pad = ~_content_mask(images, S).to(cuda).expand(n, S, S, C)
    assert int(pad.sum()) > 0
    assert torch.equal(bits(out)[pad], bits(const[0, 0]).expand(n, S, S, C)[pad])
    # content only: the prefilled padding is untouched, the content identical
    out2 = torch.empty_like(out)
    bits(out2).fill_(SENTINEL)
    ext2 = torch.full_like(ext, -1)
    o, e = ops.gallery_pack_u8(data, geom_dev, n, S, C, mean, std, content_only=True, out=out2, ext=ext2)
    assert o is out2 and e is ext2 and torch.equal(ext2, ext)
    assert bool((bits(out2)[pad] == SENTINEL).all())
    assert torch.equal(bits(out2)[~pad], bits(out)[~pad])


def test_table_is_made_by_the_float_kernel(cuda):
    from cvpce_amd import ops
    for mean, std in _norms().values():
        t = ops.gallery_table(cuda, mean, std)
        assert t.shape == (3, 257) and t.dtype == torch.bfloat16 and t.is_contiguous() and t.is_cuda
        assert ops.gallery_table(cuda, list(mean), list(std)) is t          # cached per (device, mean, std)
        # independently laid out: the 257 values as the first pixels of one 17 x 17 float image through the float path's kernel
        vals = torch.cat((ops.uint8_table() * 2 - 1, torch.zeros(1)))
        img = torch.zeros(1, 3, 17 * 17)
        img[0, :, :257] = vals
        want = ops.pack_embed_input(img.view(1, 3, 17, 17).to(cuda), False, mean, std).view(17 * 17, 8)[:257, :3]
        assert torch.equal(t.view(torch.int16), want.t().contiguous().view(torch.int16))
    assert ops.gallery_table(cuda, *_norms()['macvgg']) is not ops.gallery_table(cuda, *_norms()['macresnet'])


@pytest.mark.parametrize('content_only', [False, True])
@pytest.mark.parametrize('C', [4, 8])
@pytest.mark.parametrize('S', [16, 256])
def test_footprint(cuda, S, C, content_only):
    """Arenas with guard bands: the byte buffer ends unaligned against its guard, every output element that must be written is written
    and nothing else, and a geom row that claims h = S + 9 stores nothing outside its image's slot."""
    from cvpce_amd import ops
    from cvpce_amd.models import classification as Cm
    mean, std = Cm.TANH_MEAN, Cm.TANH_STD
    images = _images(S, seed=1)[1:] if S == 16 else _images(S, seed=1)[3:6]
    images.append(torch.randint(0, 256, (S, 5, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(2)))
    n = len(images)
    buf, geom = _packed_host(images, S)
    assert buf.numel() % 4 != 0                                              # the buffer's end is not even word-aligned
    geom[n - 1, 1] = S + 9                                                   # the last image's row lies about its height
    table = ops.gallery_table(cuda, mean, std)
    p_data, p_geom, p_table = fp.put(buf, cuda), fp.put(geom, cuda), fp.put(table, cuda)
    assert (p_data[0].data_ptr() + p_data[0].numel()) % 4 != 0
    p_out, p_ext = fp.out((n, S, S, C), torch.bfloat16, cuda), fp.out((n, 2), torch.int32, cuda)
    mask = _content_mask(images, S).expand(n, S, S, C) if content_only else None

    def run():
        torch.ops.cvpce_amd.gallery_pack_u8(p_data[0], p_geom[0], p_table[0], p_out[0], int(content_only), p_ext[0])

    out, ext = fp.check(run, [p_data, p_geom, p_table], [p_out, p_ext], written=[mask, None])
    assert ext.cpu().tolist() == [[u.shape[0], u.shape[1]] for u in images]  # the clamped extent: (S, 5) for the last image
    ref = _reference(images, S, mean, std, cuda)
    sel = (lambda t: t[mask.to(cuda)[..., :3]]) if content_only else (lambda t: t)
    assert torch.equal(sel(out[..., :3].contiguous().view(torch.int16)), sel(ref[..., :3].contiguous().view(torch.int16)))


def test_bad_extents_are_clamped(cuda):
    """h / w outside [1, S] and a negative offset are data: clamped (reported clamped), nothing stored outside the image's slot."""
    from cvpce_amd import ops
    from cvpce_amd.models import classification as Cm
    S, C = 16, 4
    g = torch.Generator().manual_seed(5)
    data = torch.randint(0, 256, (4 * S * S * 3,), dtype=torch.uint8, generator=g)
    geom = torch.tensor([[0, -3, 7], [S * S * 3, 9, 0], [-8, 4, 4], [2 * S * S * 3, S + 100, S + 1]], dtype=torch.int32)
    p_out, p_ext = fp.out((4, S, S, C), torch.bfloat16, cuda), fp.out((4, 2), torch.int32, cuda)
    ops.gallery_pack_u8(data.to(cuda), geom.to(cuda), 4, S, C, Cm.TANH_MEAN, Cm.TANH_STD, out=p_out[0], ext=p_ext[0])
    torch.cuda.synchronize()
    assert p_ext[0].cpu().tolist() == [[0, 7], [9, 0], [0, 0], [S, S]]
    for view, whole in (p_out, p_ext):
        off = view.data_ptr() - whole.data_ptr()
        nbytes = view.numel() * view.element_size()
        pre = fp.prefill_value(view.dtype)
        for band in (whole[:off], whole[off + nbytes:]):
            b = band.view(torch.int16 if view.dtype == torch.bfloat16 else torch.int32)
            assert bool((b == pre).all())
    pad = ops.gallery_table(cuda, Cm.TANH_MEAN, Cm.TANH_STD)[:, 256]
    out = p_out[0]
    for i in range(3):                                                       # no content: every pixel is the padding
        assert torch.equal(out[i, :, :, :3].view(torch.int16), pad.view(torch.int16).expand(S, S, 3))
    want = data[2 * S * S * 3:3 * S * S * 3].view(S, S, 3)
    ref = _reference([want], S, Cm.TANH_MEAN, Cm.TANH_STD, cuda)
    assert torch.equal(out[3, :, :, :3].contiguous().view(torch.int16), ref[0, :, :, :3].contiguous().view(torch.int16))


def test_bad_arguments_raise_and_launch_nothing(cuda):
    from cvpce_amd import ops
    from cvpce_amd.models import classification as Cm
    S, n = 16, 2
    data = torch.zeros(n * S * S * 3, dtype=torch.uint8, device=cuda)
    geom = torch.tensor([[0, S, S], [S * S * 3, S, S]], dtype=torch.int32, device=cuda)
    table = ops.gallery_table(cuda, Cm.TANH_MEAN, Cm.TANH_STD)
    out = torch.empty((n, S, S, 4), dtype=torch.bfloat16, device=cuda)
    ext = torch.empty((n, 2), dtype=torch.int32, device=cuda)
    good = dict(data=data, geom=geom, table=table, out=out, ext=ext)
    bad = {
        'float bytes': dict(data=data.float()),
        'bytes not flat': dict(data=data.view(n, -1)),
        'empty bytes': dict(data=data[:0]),
        'geom int64': dict(geom=geom.long()),
        'geom (n,2)': dict(geom=geom[:, :2].contiguous()),
        'geom rows': dict(geom=geom[:1]),
        'geom strided': dict(geom=torch.zeros((n, 6), dtype=torch.int32, device=cuda)[:, ::2]),
        'geom on the host': dict(geom=geom.cpu()),
        'table f32': dict(table=table.float()),
        'table (3,256)': dict(table=table[:, :256].contiguous()),
        'table on the host': dict(table=table.cpu()),
        'out f16': dict(out=out.to(torch.float16)),
        'out C=3': dict(out=torch.empty((n, S, S, 3), dtype=torch.bfloat16, device=cuda)),
        'out not square': dict(out=torch.empty((n, S, S + 1, 4), dtype=torch.bfloat16, device=cuda)),
        'out strided': dict(out=torch.empty((n, S, S, 8), dtype=torch.bfloat16, device=cuda)[..., :4]),
        'ext (n,3)': dict(ext=torch.empty((n, 3), dtype=torch.int32, device=cuda)),
        'ext int64': dict(ext=ext.long()),
    }
    for what, change in bad.items():
        a = dict(good, **change)
        for t in (a['out'], a['ext']):
            t.view(torch.int16 if t.element_size() == 2 else (torch.int32 if t.element_size() == 4 else torch.int64)).fill_(0x5A5A)
        snap = [a['out'].clone(), a['ext'].clone()]
        with pytest.raises(RuntimeError):
            torch.ops.cvpce_amd.gallery_pack_u8(a['data'], a['geom'], a['table'], a['out'], 0, a['ext'])
        torch.cuda.synchronize()
        bits = lambda t: t.contiguous().view(torch.uint8)
        assert torch.equal(bits(a['out']), bits(snap[0])) and torch.equal(bits(a['ext']), bits(snap[1])), what
    torch.ops.cvpce_amd.gallery_pack_u8(data, geom, table, out, 0, ext)      # (the unchanged arguments are fine)
    assert ext.cpu().tolist() == [[S, S], [S, S]]
    with pytest.raises(ValueError):                                         # the host packing refuses an image larger than S
        from cvpce_amd import production
        production.pack_gallery_bytes([torch.zeros(S + 1, 2, 3, dtype=torch.uint8)], torch.zeros(4096, dtype=torch.uint8), torch.zeros((1, 3), dtype=torch.int32), S)


# ---------------------------------------------------------------------------------------------------------------------------------
# Classifier.build_index
# ---------------------------------------------------------------------------------------------------------------------------------
def _gallery_bytes(n, seed=11):
    """n gallery byte images the way the reader makes them: the longer side 256, the other 1 ... 256 (a mix of aspect ratios, thin
    slivers and squares included)."""
    g = torch.Generator().manual_seed(seed)
    out = []
    for i in range(n):
        short = (1, 256, 64, 200, 131)[i] if i < 5 else int(torch.randint(1, 257, (1,), generator=g))
        h, w = (256, short) if i % 2 == 0 else (short, 256)
        out.append(torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g))
    return out


class _Items:
    """sample set of (image, image, categories, annotation) items, like the gallery readers'"""

    def __init__(self, images):
        self.images = images

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return self.images[i], self.images[i], ['Food'], f'Food/{i:04d}'


def _build(enc, dev, images):
    from cvpce_amd import production
    clf = production.Classifier.__new__(production.Classifier)
    clf.batch_size, clf.num_workers, clf.device, clf.emb_device, clf.encoder = 8, 0, dev, dev, enc
    return clf.build_index(_Items(images))


def _profiled(fn):
    """-> (fn(), whether a work-list launch was recorded, the byte kernel's launch records): a work-list launch's record carries its
    list's count"""
    from cvpce_amd import ops
    prof = ops.PROFILE = ops.ConvProfile()
    try:
        res = fn()
        torch.cuda.synchronize()
    finally:
        ops.PROFILE = None
    listed = any(len(r) > 4 for r in prof.records)
    packs = [r for r in prof.byte_records if r[0] == 'gallery_pack_u8_kernel']
    return res, listed, packs


_FLOAT_INDEX = {}


def _float_index(name, enc, dev, n):
    """the float path's index over the float items the first n byte images stand for, computed once per (encoder, n)"""
    from cvpce_amd import datautils
    if (name, n) not in _FLOAT_INDEX:
        _FLOAT_INDEX[(name, n)] = _build(enc, dev, [datautils.gallery_float(u) for u in _gallery_bytes(n)])
    return _FLOAT_INDEX[(name, n)]


@pytest.mark.parametrize('gallery_u8', [True, False])
@pytest.mark.parametrize('skip_padding', [True, False])
@pytest.mark.parametrize('n', [0, 1, 5, 65])
def test_index_is_bit_identical_macvgg(cuda, vgg, monkeypatch, n, skip_padding, gallery_u8):
    from cvpce_amd import production
    from cvpce_amd.models import classification as C
    assert n != 65 or n == production.INDEX_BATCH + 1                        # (more than one pass, the second of one image)
    monkeypatch.setattr(C, 'SKIP_PADDING', skip_padding)
    monkeypatch.setattr(production, 'GALLERY_U8', gallery_u8)
    want_emb, want_ann = _float_index('macvgg', vgg, cuda, n)
    (emb, ann), listed, packs = _profiled(lambda: _build(vgg, cuda, _gallery_bytes(n)))
    assert emb.shape == (n, 1024) and emb.dtype == torch.float32 and emb.device == want_emb.device
    assert torch.equal(emb, want_emb) and ann == want_ann == [f'Food/{i:04d}' for i in range(n)]
    # which path ran: the byte kernel once per pass with the switch on, never with it off; the work-list schedule only with both on
    assert len(packs) == ((n + 63) // 64 if gallery_u8 else 0)
    assert listed == bool(n and gallery_u8 and skip_padding)


@pytest.mark.parametrize('gallery_u8', [True, False])
def test_index_is_bit_identical_macresnet(cuda, resnet, monkeypatch, gallery_u8):
    """an encoder without the work-list schedule: whole crops (C = 8), the plain schedule"""
    from cvpce_amd import production
    monkeypatch.setattr(production, 'GALLERY_U8', gallery_u8)
    assert not hasattr(resnet.engine(), 'skip_plan')
    want_emb, want_ann = _float_index('macresnet', resnet, cuda, 5)
    (emb, ann), listed, packs = _profiled(lambda: _build(resnet, cuda, _gallery_bytes(5)))
    assert torch.equal(emb, want_emb) and ann == want_ann
    assert emb.shape == (5, resnet.engine().embedding_size)
    assert len(packs) == (1 if gallery_u8 else 0) and not listed


def test_mixed_sample_set_keeps_order(cuda, vgg):
    from cvpce_amd import datautils
    images = _gallery_bytes(7)
    want_emb, want_ann = _float_index('macvgg', vgg, cuda, 7)
    mixed = [u if i in (0, 1, 3, 6) else datautils.gallery_float(u) for i, u in enumerate(images)]
    (emb, ann), listed, packs = _profiled(lambda: _build(vgg, cuda, mixed))
    assert torch.equal(emb, want_emb) and ann == want_ann
    assert len(packs) == 3                                                   # byte passes: items 0-1, 3 and 6


def test_cli_prebuild_index_same_bits_with_the_switch_off(cuda, tmp_path):
    """`dihe prebuild-index` in fresh processes, CVPCE_GALLERY_U8=1 and =0: the saved indices are the same bits."""
    from PIL import Image
    from cvpce_amd import synthetic
    torch.save({'model_state_dict': synthetic.synthetic_macvgg(seed=1).state_dict()}, tmp_path / 'dihe.tar')
    g = torch.Generator().manual_seed(8)
    for i, (h, w) in enumerate([(300, 120), (90, 400), (64, 64), (600, 2), (257, 255), (40, 41)]):
        dd = tmp_path / 'Training' / 'Food' / f'Cat{i % 2}'
        dd.mkdir(parents=True, exist_ok=True)
        Image.fromarray(torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).numpy()).save(dd / f'{i}.png')
    indices = []
    for switch in ('1', '0'):
        out_dir = tmp_path / f'out{switch}'
        out_dir.mkdir()
        cmd = [sys.executable, '-m', 'cvpce_amd.cli', 'dihe', 'prebuild-index', '--img-dir', str(tmp_path / 'Training'), '--out-dir', str(out_dir),
               str(tmp_path / 'dihe.tar')]
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600, env=dict(os.environ, CVPCE_GALLERY_U8=switch))
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        indices.append(torch.load(out_dir / 'classifier_index.pkl', map_location='cpu'))
    a, b = indices
    assert a['embedding'].shape == (6, 1024) and torch.equal(a['embedding'], b['embedding'])
    assert a['annotations'] == b['annotations'] and sorted(a['annotations']) == sorted(f'Food/Cat{i % 2}/{i}' for i in range(6))
