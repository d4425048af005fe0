"""Equality, kernel by kernel, for the input side: csrc/preproc.hip against tests/input_cases.py, the fp32 host model of DESIGN.md 4's input
rule -- the detector's transform, the RoI crops in all three modes, their extents, the pack kernel -- and the grid-stride loops of
csrc/elementwise.hip on their second trip.  preproc.hip is built without contraction and divides by IEEE division, the model performs the
same fp32 operations in the same order, so every comparison is torch.equal-strict on the integer view of EVERY element of every output:
outputs are pre-filled, so an element the kernel should have written and did not, or wrote and should not have, differs too."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import exact_cases as ec            # tests/exact_cases.py
import footprint as fp              # tests/footprint.py
import input_cases as ic            # tests/input_cases.py

pytestmark = pytest.mark.gpu

_INT = {2: torch.int16, 4: torch.int32}
PRECISIONS = ['bf16', 'fp16']


@pytest.fixture(autouse=True)
def byte_kernels(monkeypatch):
    from cvpce_amd import ops
    monkeypatch.setattr(ops, 'U8_KERNELS', True)


def bits(t):
    return t if t.dtype in _INT.values() else t.view(_INT[t.element_size()])


def prefilled(shape, dtype, device):
    t = torch.empty(shape, dtype=dtype, device=device)
    bits(t).fill_(fp.prefill_value(dtype))
    return t


def int_view(a):
    return a.view(np.int32) if a.dtype == np.float32 else a


def same_bits(got, want, what=''):
    """the device tensor `got` holds exactly the bits of the host array `want`, element for element"""
    g = bits(got).cpu().numpy()
    w = int_view(np.ascontiguousarray(want))
    assert g.shape == w.shape and g.dtype == w.dtype, (what, g.shape, w.shape, g.dtype, w.dtype)
    if np.array_equal(g, w):
        return
    bad = np.argwhere(g != w)
    first = tuple(bad[0])
    raise AssertionError(f'{what}: {len(bad)} of {g.size} elements differ, first at {first}: kernel {int(g[first]):#x}, model {int(w[first]):#x}')


def dev(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


# ---- the detector's transform --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def transforms():
    """the sources and, per precision, the model's (7,Hp,Wp,8) batch: computed once, never modified"""
    srcs = ic.transform_sources()
    want = {p: np.stack([ic.transform(img, h, w, ic.TRANSFORM_HP, ic.TRANSFORM_WP, ic.IMAGE_MEAN, ic.IMAGE_STD, ic.STORAGE[p])
                         for (_, _, (h, w)), img in zip(ic.TRANSFORMS, srcs)]) for p in PRECISIONS}
    return srcs, want


@pytest.fixture(scope='module')
def tiny():
    srcs = ic.tiny_sources()
    h, w = ic.TINY_DST
    want = {p: np.stack([ic.transform(img, h, w, h, w, ic.IMAGE_MEAN, ic.IMAGE_STD, ic.STORAGE[p]) for img in srcs]) for p in PRECISIONS}
    return srcs, want


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('path', ['into', 'batch_float', 'batch_mixed'])
def test_transform(cuda, transforms, path, precision):
    """one image per launch, the float list and the mixed byte / float list: downscale, upscale, identity, indices on .25 / .5 / .75,
    clamped second taps, in a batch 160 columns wide"""
    from cvpce_amd import ops
    srcs, want = transforms
    sizes = [hw for _, _, hw in ic.TRANSFORMS]
    batch = prefilled((len(srcs), ic.TRANSFORM_HP, ic.TRANSFORM_WP, 8), ops.STORAGE_TYPES[precision], cuda)
    if path == 'into':
        for i, (img, (h, w)) in enumerate(zip(srcs, sizes)):
            ops.gln_transform_into(dev(ic.planes(img), cuda), batch, i, h, w, ic.IMAGE_MEAN, ic.IMAGE_STD)
    elif path == 'batch_float':
        ops.gln_transform_batch([dev(ic.planes(img), cuda) for img in srcs], batch, sizes, ic.IMAGE_MEAN, ic.IMAGE_STD)
    else:
        assert {img.dtype for img in srcs} == {np.dtype(np.uint8), np.dtype(np.float32)}
        ops.gln_transform_batch([dev(img, cuda) for img in srcs], batch, sizes, ic.IMAGE_MEAN, ic.IMAGE_STD)
    same_bits(batch, want[precision], f'transform {path} {precision}')


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('path', ['batch_float', 'batch_mixed'])
def test_transform_second_launch(cuda, tiny, path, precision):
    """33 images in one call: the 33rd goes out in a launch of its own, to its own place in the batch"""
    from cvpce_amd import ops
    srcs, want = tiny
    batch = prefilled((len(srcs),) + ic.TINY_DST + (8,), ops.STORAGE_TYPES[precision], cuda)
    images = [dev(ic.planes(img) if path == 'batch_float' else img, cuda) for img in srcs]
    ops.gln_transform_batch(images, batch, [ic.TINY_DST] * len(srcs), ic.IMAGE_MEAN, ic.IMAGE_STD)
    same_bits(batch, want[precision], f'33 images {path} {precision}')


# ---- the RoI crops ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def crop_model(hw, form, S):
    """-> (image, the 17 boxes, the model's modes 0, 1, 2): computed once per (image, form, size); the tests copy before they change"""
    img = ic.source(form, 600 + hw[0], *hw)
    boxes = ic.crop_boxes(hw[0], hw[1], S, max(ic.CROP_COUNTS))
    c0 = ic.crop(img, boxes, S, 0)
    c1 = ic.pack(c0, True, ic.TANH_MEAN, ic.TANH_STD)          # (test_input_cases_cpu.py: crop mode 1, bit for bit)
    return img, boxes, (c0, c1, np.ascontiguousarray(c1[..., :4]))


def crop_out(p, s, mode, device):
    from cvpce_amd import ops
    return prefilled((p, 3, s, s), torch.float32, device) if mode == 0 else prefilled((p, s, s, 8 if mode == 1 else 4), ops.BF16, device)


@pytest.mark.parametrize('S', ic.CROP_SIZES)
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('form', ['u8', 'f32'])
@pytest.mark.parametrize('hw', ic.CROP_IMAGES, ids=lambda v: 'x'.join(map(str, v)))
def test_crop(cuda, hw, form, mode, S):
    """9 and 17 boxes, with a device count (the slots beyond it keep the prefill) and without"""
    from cvpce_amd import ops
    img, boxes, models = crop_model(hw, form, S)
    dimg = dev(img, cuda)
    kw = dict(mean=ic.TANH_MEAN, std=ic.TANH_STD) if mode else {}
    for n in ic.CROP_COUNTS:
        b = dev(boxes[:n], cuda)
        for live in (None, n - 2):
            out = crop_out(n, S, mode, cuda)
            want = int_view(models[mode][:n]).copy()
            count = None
            if live is not None:
                count = torch.tensor([live], dtype=torch.int32, device=cuda)
                want[live:] = fp.prefill_value(out.dtype)
            ops.crop_resize(dimg, b, S, mode, count=count, out=out, **kw)
            same_bits(out, want, f'crop {hw} {form} mode {mode} S {S}: {n} boxes, count {live}')


@pytest.mark.parametrize('S', [s for s in ic.CROP_SIZES if s % 2 == 0])
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('form', ['u8', 'f32'])
@pytest.mark.parametrize('hw', ic.CROP_IMAGES, ids=lambda v: 'x'.join(map(str, v)))
def test_crop_content_only(cuda, hw, form, mode, S):
    """with content_ext (the MODEL's extents): inside them the model's bits; beyond them the prefill -- but for the column behind an odd
    column extent, which the thread of the last content column writes too (two pixels a thread): the model's bits, the pad constant"""
    from cvpce_amd import ops
    img, boxes, models = crop_model(hw, form, S)
    dimg = dev(img, cuda)
    yy, xx = np.arange(S).reshape(1, S, 1, 1), np.arange(S).reshape(1, 1, S, 1)
    for n in ic.CROP_COUNTS:
        for live in (None, n - 2):
            count = None if live is None else np.array([live], dtype=np.int32)
            ext = ic.extents(boxes[:n], hw[0], hw[1], S, count=count)
            ey, ex = ext[:, 0].reshape(-1, 1, 1, 1), ext[:, 1].reshape(-1, 1, 1, 1)
            written = (yy < ey) & (xx < ex + (ex & 1)) & (np.arange(n).reshape(-1, 1, 1, 1) < (n if live is None else live))
            assert written.any() and not written.all()
            out = crop_out(n, S, mode, cuda)
            want = np.where(written, models[mode][:n], np.int16(fp.prefill_value(out.dtype)))
            ops.crop_resize(dimg, dev(boxes[:n], cuda), S, mode, mean=ic.TANH_MEAN, std=ic.TANH_STD, count=None if live is None else dev(count, cuda),
                            out=out, content_ext=dev(ext, cuda))
            same_bits(out, want, f'content of crop {hw} {form} mode {mode} S {S}: {n} boxes, count {live}')


# ---- extents ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', ic.EXTENT_SIZES)
def test_crop_extents_exhaustive(cuda, S):
    """every integer box with corners in [-2, W0 + 2] x [-2, H0 + 2] of a 12 x 9 image in one launch: the bisection against the scan of
    all S positions; then with one count, and with a count per image"""
    from cvpce_amd import ops
    h, w = ic.EXTENT_IMAGE
    boxes = ic.extent_boxes()
    n = len(boxes)
    dboxes = dev(boxes, cuda)
    out = prefilled((n, 2), torch.int32, cuda)
    ops.crop_extents(dboxes, None, h, w, S, out=out)
    same_bits(out, ic.extents(boxes, h, w, S), f'extents S {S}')
    count = np.array([n // 3], dtype=np.int32)
    out = prefilled((n, 2), torch.int32, cuda)
    ops.crop_extents(dboxes, dev(count, cuda), h, w, S, out=out)
    same_bits(out, ic.extents(boxes, h, w, S, count=count), f'extents S {S} with a count')
    per = 7
    assert n % per == 0
    counts = (np.arange(n // per) % (per + 1)).astype(np.int32)
    out = prefilled((n, 2), torch.int32, cuda)
    ops.crop_extents(dboxes, dev(counts, cuda), h, w, S, out=out, per_image=per)
    same_bits(out, ic.extents(boxes, h, w, S, count=counts, per_image=per), f'extents S {S} per image')


@pytest.mark.parametrize('S', ic.CROP_SIZES)
@pytest.mark.parametrize('hw', ic.CROP_IMAGES, ids=lambda v: 'x'.join(map(str, v)))
def test_crop_extents_of_the_crop_boxes(cuda, hw, S):
    """the boxes of the crop tests (fractional, reversed, outside): the extents the content-only crops were given"""
    from cvpce_amd import ops
    boxes = ic.crop_boxes(hw[0], hw[1], S, max(ic.CROP_COUNTS))
    out = prefilled((len(boxes), 2), torch.int32, cuda)
    ops.crop_extents(dev(boxes, cuda), None, hw[0], hw[1], S, out=out)
    same_bits(out, ic.extents(boxes, hw[0], hw[1], S), f'extents of the crop boxes {hw} S {S}')


@pytest.mark.parametrize('S', ic.CROP_SIZES)
def test_pad_extents(cuda, S):
    """read off the data: the model's crops (17 of each image), a tensor without constant borders, a constant one, another constant"""
    from cvpce_amd import ops
    crops = np.concatenate([crop_model(hw, 'u8', S)[2][0] for hw in ic.CROP_IMAGES])
    noise = np.random.RandomState(7).rand(2, 3, S, S).astype(np.float32)
    noise[1, :, S // 2:, :] = 0.25
    noise[1, :, :, S - 1:] = 0.25
    images = np.concatenate([crops, noise, np.full((1, 3, S, S), 0.5, dtype=np.float32)])
    for pad in (0.5, 0.25):
        want = ic.pad_extents(images, pad)
        assert len({tuple(e) for e in want.tolist()}) > (4 if pad == 0.5 else 1)
        same_bits(ops.pad_extents(dev(images, cuda), pad), want, f'pad_extents S {S} pad {pad}')


# ---- pack ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('to_tanh', [True, False])
def test_pack_embed_input(cuda, to_tanh):
    from cvpce_amd import ops
    mean, std = (ic.TANH_MEAN, ic.TANH_STD) if to_tanh else (ic.IMAGE_MEAN, ic.IMAGE_STD)
    for S in ic.CROP_SIZES:
        crops = np.concatenate([crop_model(hw, 'f32', S)[2][0] for hw in ic.CROP_IMAGES])
        same_bits(ops.pack_embed_input(dev(crops, cuda), to_tanh, mean, std), ic.pack(crops, to_tanh, mean, std), f'pack S {S} to_tanh {to_tanh}')


@pytest.mark.parametrize('to_tanh', [True, False])
def test_pack_embed_input_second_trip(cuda, to_tanh):
    """33 x 256 x 256 pixels: more than 8192 workgroups of 256 -- the grid-stride loop goes round again"""
    from cvpce_amd import ops
    b, s = 33, 256
    assert b * s * s > 8192 * 256 >= (b - 1) * s * s
    images = np.random.RandomState(11).rand(b, 3, s, s).astype(np.float32)
    images[:, :, ::7, ::5] = 0.5
    mean, std = (ic.TANH_MEAN, ic.TANH_STD) if to_tanh else (ic.IMAGE_MEAN, ic.IMAGE_STD)
    same_bits(ops.pack_embed_input(dev(images, cuda), to_tanh, mean, std), ic.pack(images, to_tanh, mean, std), f'pack 33 x 256 x 256 to_tanh {to_tanh}')


# ---- second trips in elementwise.hip -----------------------------------------------------------------------------------------------------
def all_patterns(dtype, device):
    """the 65 536 bit patterns of a 16-bit type as a tensor of that type"""
    return torch.arange(-32768, 32768, dtype=torch.int16, device=device).view(dtype)


INF_CODE = {'bf16': 0x7F80, 'fp16': 0x7C00}
MINUS_ONE = {'bf16': 0xBF80 - 65536, 'fp16': 0xBC00 - 65536}
FIRST_NORMAL = {'bf16': 0x0080, 'fp16': 0x0400}


@pytest.mark.parametrize('precision', PRECISIONS)
@pytest.mark.parametrize('k,stride,pad,size', [(2, 2, 0, 364), (3, 2, 1, 363)], ids=['2-2-0', '3-2-1'])
def test_maxpool_second_trip(cuda, precision, k, stride, pad, size):
    """1 x size x size x 512 -> 182 x 182 x 64 output octets, the smallest square past 8192 x 256.  Input: random bit patterns (infinities
    and 16-bit denormals among them), the top 40 rows negative throughout; NaNs and zeros are replaced (-1 in the top rows, +0 below: which
    zero a maximum of both is, is not defined) -- all of it on the integer view.  Reference: F.max_pool2d on the values widened to float64
    (exact, and no 16-bit denormal is a float64 denormal)."""
    from cvpce_amd import ops
    dt = ops.STORAGE_TYPES[precision]
    c, top = 512, 40
    g = torch.Generator(device=cuda).manual_seed(size)
    raw = torch.randint(-32768, 32768, (1, size, size, c), dtype=torch.int16, device=cuda, generator=g)
    raw[:, :top] |= -32768
    mag = raw & 0x7FFF
    fill = torch.zeros_like(raw)
    fill[:, :top] = MINUS_ONE[precision]
    raw = torch.where((mag > INF_CODE[precision]) | (mag == 0), fill, raw)
    mag = raw & 0x7FFF
    assert bool((mag == INF_CODE[precision]).any()) and bool(((mag > 0) & (mag < FIRST_NORMAL[precision])).any()) and bool((raw[:, :top] < 0).all())
    x = raw.view(dt)
    got = ops.maxpool2d(x, k, stride, pad)
    ho = (size + 2 * pad - k) // stride + 1
    assert tuple(got.shape) == (1, ho, ho, c) and ho * ho * (c // 8) > 8192 * 256 >= (ho - 1) * (ho - 1) * (c // 8)
    ref = F.max_pool2d(x.permute(0, 3, 1, 2).double(), k, stride, pad).permute(0, 2, 3, 1).contiguous()
    want = ref.to(dt)
    assert torch.equal(want.double(), ref) and bool(ref.isinf().any())          # (16-bit values; an infinity won somewhere)
    assert torch.equal(bits(got), bits(want))
    assert bool((bits(got)[:, :10] < 0).all())                                  # the windows that are negative throughout


@pytest.mark.parametrize('precision', PRECISIONS)
def test_relu_second_trip(cuda, precision):
    """129 x 65 536 elements = more than 4096 x 256 octets, every bit pattern 129 times: a positive value that is no NaN passes;
    everything else -- negatives, -0, NaNs of either sign -- becomes +0"""
    from cvpce_amd import ops
    dt = ops.STORAGE_TYPES[precision]
    reps = 129
    assert reps * 65536 // 8 > 4096 * 256 >= (reps - 1) * 65536 // 8
    x = all_patterns(dt, cuda).repeat(reps).roll(3).view(reps, 8192, 8).contiguous()        # (rolled: an octet's patterns differ in the high bits too)
    got = ops.relu(x)
    host = x.cpu()
    want = torch.where(host.float() > 0, bits(host), torch.zeros((), dtype=torch.int16))     # (NaN > 0 and -0 > 0 are false)
    assert int((want != 0).sum()) == reps * INF_CODE[precision]                            # the codes 1 ... +infinity
    assert torch.equal(bits(got).cpu(), want)


@pytest.mark.parametrize('cid', [ec.ids('gauss_tail', dt)[-1] for dt in ec.DTYPES], ids=lambda s: s.split('/')[-1])
def test_gauss_tail_second_trip(cuda, cid):
    """1025 x 1024 pixels, more than 4096 x 256: the one launch equals, bit for bit, two launches over its halves, each under the cap --
    and, the operands being exact_cases' gauss_tail case tiled, the float64 reference of that case, tiled"""
    from cvpce_amd import ops
    c = ec.case(cid)
    ref = c.reference()[0]                                                      # (n,1,h,w) float64
    c4, c5 = [ops.PackedConv(L.w.float(), L.b.float() if L.b is not None else None, L.stride, L.pad, device=cuda, dtype=c.dt) for L in c.layers]
    n, ch, h, w = c.x.shape
    assert ch == 16
    pix = c.x.permute(0, 2, 3, 1).reshape(-1, 16)                               # the case's pixels, in order
    rows, cols = 1025, 1024
    npix = rows * cols
    assert npix > 4096 * 256 and (rows + 1) // 2 * cols <= 4096 * 256
    idx = torch.arange(npix) % pix.shape[0]
    x = pix[idx].to(c.dt)
    assert torch.equal(x.double(), pix[idx])
    x = x.view(1, rows, cols, 16).to(cuda)
    assert ops.can_fuse_gauss_tail(x, c4, c5)
    whole = ops.gauss_tail(x, c4, c5, 1)
    half = (rows + 1) // 2
    parts = torch.cat([ops.gauss_tail(x[:, :half].contiguous(), c4, c5, 1), ops.gauss_tail(x[:, half:].contiguous(), c4, c5, 1)], dim=1)
    assert whole.dtype == torch.float32 and tuple(whole.shape) == (1, rows, cols, 1)
    assert torch.equal(bits(whole), bits(parts))
    tiled = ref.permute(0, 2, 3, 1).reshape(-1)[idx].view(1, rows, cols, 1)
    assert torch.equal(whole.cpu().double(), tiled)
