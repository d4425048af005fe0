"""tests/input_cases.py, the fp32 host model of the input kernels, pinned where it can be without a GPU: against the oracle on the shared
cases (the measured distances are printed; twice their maximum, rounded up, stands in input_cases.py), and against its own rules."""
import numpy as np
import pytest
import torch

import input_cases as ic            # tests/input_cases.py

F = np.float32


# ---- against the oracle ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('form,hw', ic.ORACLE_TRANSFORMS, ids=lambda v: v if isinstance(v, str) else 'x'.join(map(str, v)))
def test_transform_against_oracle(form, hw):
    from oracle import gln as og
    assert og.IMAGE_MEAN == ic.IMAGE_MEAN and og.IMAGE_STD == ic.IMAGE_STD
    img = ic.source(form, 300 + hw[0], *hw)
    ref = og.transform_one(torch.from_numpy(ic.planes(img))).numpy()
    h, w = og.resized_size(*hw)
    assert ref.shape == (3, h, w)
    got = ic.transform_f32(img, h, w, ic.IMAGE_MEAN, ic.IMAGE_STD)
    diff = float(np.abs(got - ref).max())
    print(f'transform {hw[0]}x{hw[1]} -> {h}x{w} ({form}): largest |model - oracle| = {diff:.3e}, bound {ic.T_TRANSFORM_REF[hw]:.1e}')
    assert diff <= ic.T_TRANSFORM_REF[hw]


@pytest.mark.parametrize('form', ['u8', 'f32'])
@pytest.mark.parametrize('hw', ic.CROP_IMAGES, ids=lambda v: 'x'.join(map(str, v)))
def test_crop_against_oracle(hw, form):
    from oracle import crop as ocrop, macvgg as ovgg
    assert tuple(m * 2 - 1 for m in ovgg.IMAGENET_MEAN) == ic.TANH_MEAN and tuple(s * 2 for s in ovgg.IMAGENET_STD) == ic.TANH_STD
    img = ic.source(form, 400 + hw[0], *hw)
    boxes = ic.oracle_boxes(*hw)
    assert len(boxes) >= 8
    ref = ocrop.crop_boxes(torch.from_numpy(ic.planes(img)), torch.from_numpy(boxes))
    refn = ovgg.normalize_tanh(ocrop.scale_to_tanh(ref)).numpy()
    got = ic.crop(img, boxes, ocrop.CLASSIFICATION_IMAGE_SIZE, 0)
    gotn = ic.normalize_tanh_f32(got, ic.TANH_MEAN, ic.TANH_STD)
    d0, d1 = float(np.abs(got - ref.numpy()).max()), float(np.abs(gotn - refn).max())
    print(f'crops of {hw[0]}x{hw[1]} ({form}), {len(boxes)} boxes: largest |model - oracle| = {d0:.3e} (bound {ic.T_CROP_REF:.1e}), '
          f'normalised {d1:.3e} (bound {ic.T_CROP_NORM_REF:.1e})')
    assert d0 <= ic.T_CROP_REF and d1 <= ic.T_CROP_NORM_REF


# ---- the model's own rules -----------------------------------------------------------------------------------------------------------
def test_table():
    t = ic.table()
    assert t.dtype == F and t.shape == (256,) and t[0] == 0 and t[255] == 1
    assert np.array_equal(t, (torch.arange(256, dtype=torch.float32) / 255.0).numpy())
    assert all(t[b] == F(F(b) / F(255)) for b in range(256))


@pytest.mark.parametrize('S', ic.CROP_SIZES)
@pytest.mark.parametrize('hw', ic.CROP_IMAGES, ids=lambda v: 'x'.join(map(str, v)))
def test_beyond_the_extents_is_the_constant(hw, S):
    """every pixel at or beyond `extents` is exactly the pad constant (0.5, or its packed triple), pad_extents of the mode-0 crops is
    `extents`, pack(mode 0) is mode 1 bit for bit and mode 2 its first four channels; bytes and their table values give the same"""
    img = ic.byte_image(500 + S, *hw)
    boxes = ic.crop_boxes(hw[0], hw[1], S, 17)
    ext = ic.extents(boxes, hw[0], hw[1], S)
    c0 = ic.crop(img, boxes, S, 0)
    c1 = ic.crop(img, boxes, S, 1, ic.TANH_MEAN, ic.TANH_STD)
    c2 = ic.crop(img, boxes, S, 2, ic.TANH_MEAN, ic.TANH_STD)
    assert c0.dtype == F and c1.dtype == c2.dtype == np.int16
    yy, xx = np.arange(S)[:, None], np.arange(S)[None, :]
    triple = ic.pack(np.full((1, 3, 1, 1), 0.5, dtype=F), True, ic.TANH_MEAN, ic.TANH_STD)[0, 0, 0]
    seen = set()
    for k, (ey, ex) in enumerate(ext):
        beyond = (yy >= ey) | (xx >= ex)
        assert (c0[k][:, beyond] == F(0.5)).all(), k
        assert (c1[k][beyond] == triple).all() and (c2[k][beyond] == triple[:4]).all(), k
        seen.add(tuple('none' if e == 0 else ('all' if e == S else 'some') for e in (ey, ex)))
    assert {('none', 'none'), ('some', 'all'), ('all', 'some'), ('all', 'all')} <= seen
    # (a crop with no column or no row of content is the constant throughout: read off the data that is (0, 0), whatever the other side)
    assert np.array_equal(ic.pad_extents(c0), np.where(ext.min(axis=1, keepdims=True) > 0, ext, 0))
    assert np.array_equal(ic.pack(c0, True, ic.TANH_MEAN, ic.TANH_STD), c1)
    assert np.array_equal(c2, c1[..., :4]) and not c1[..., 3:].any()
    f = ic.table()[img].transpose(2, 0, 1).copy()
    assert np.array_equal(ic.crop(f, boxes, S, 0), c0) and np.array_equal(ic.crop(f, boxes, S, 1, ic.TANH_MEAN, ic.TANH_STD), c1)


def test_which_normalisation_orders_the_rule_tells_apart():
    """((v * 2 - 1) - mean) / std is the rule.  (v - 0.5) * 2 in the place of v * 2 - 1 is the same fp32 value for every v (a product with 2 is
    exact: both round 2 v - 1 once, onto the same grid), so no test can tell the two apart, and none needs to.  Folding the constants,
    (v * 2 - (1 + mean)) / std, is another function: it changes bf16 results of the shared S = 260 crops, which the GPU tests compare."""
    rng = np.random.RandomState(5)
    v = np.concatenate([rng.rand(1 << 20).astype(F), (rng.rand(1 << 18) * 2.0 ** -rng.randint(0, 120, 1 << 18)).astype(F),
                        np.array([0, 0.125, 0.25, 0.5, 1, np.float32(1e-45), np.float32(1.1754944e-38)], dtype=F)])
    assert np.array_equal(((v - F(0.5)).astype(F) * F(2)).astype(F), ((v * F(2)).astype(F) - F(1)).astype(F))
    hw = ic.CROP_IMAGES[0]
    c0 = ic.crop(ic.byte_image(600 + hw[0], *hw), ic.crop_boxes(hw[0], hw[1], 260, 9), 260, 0)
    folded = (((c0 * F(2)).astype(F) - (F(1) + ic.f3(ic.TANH_MEAN)).astype(F)).astype(F) / ic.f3(ic.TANH_STD)).astype(F)
    rule = ic.normalize_tanh_f32(c0, ic.TANH_MEAN, ic.TANH_STD)
    changed = int((ic.narrow(folded, torch.bfloat16) != ic.narrow(rule, torch.bfloat16)).sum())
    print(f'folded constants: {changed} of {rule.size} bf16 results differ')
    assert changed > 0


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_transform_forms_and_padding(dtype):
    dt = ic.STORAGE[dtype]
    for (form, hw, (h, w)), img in zip(ic.TRANSFORMS, ic.transform_sources()):
        got = ic.transform(img, h, w, ic.TRANSFORM_HP, ic.TRANSFORM_WP, ic.IMAGE_MEAN, ic.IMAGE_STD, dt)
        assert got.shape == (ic.TRANSFORM_HP, ic.TRANSFORM_WP, 8) and got.dtype == np.int16
        assert not got[h:].any() and not got[:, w:].any() and not got[..., 3:].any()
        assert np.array_equal(got, ic.transform(ic.planes(img), h, w, ic.TRANSFORM_HP, ic.TRANSFORM_WP, ic.IMAGE_MEAN, ic.IMAGE_STD, dt))
        if hw == (h, w):          # identity: the normalised source itself
            n = ((ic.planes(img) - ic.f3(ic.IMAGE_MEAN)).astype(F) / ic.f3(ic.IMAGE_STD)).astype(F)
            assert np.array_equal(got[:h, :w, :3], ic.narrow(n, dt).transpose(1, 2, 0))


def test_extents_of_the_exhaustive_boxes():
    """the scan agrees with the closed form where there is one (scale 1: the extent is the side itself), slots beyond a count are (S, S)"""
    h, w = ic.EXTENT_IMAGE
    boxes = ic.extent_boxes()
    assert len(boxes) == (w + 5) ** 2 * (h + 5) ** 2
    x1, y1, cw, ch = ic.box_geometry(boxes, h, w)
    for S in ic.EXTENT_SIZES:
        ext = ic.extents(boxes, h, w, S)
        assert ((ext >= 0) & (ext <= S)).all()
        larger = np.maximum(cw, ch)
        assert (ext[larger == 0] == 0).all()
        assert (ext[cw >= ch, 1] == S)[larger[cw >= ch] > 0].all() and (ext[ch >= cw, 0] == S)[larger[ch >= cw] > 0].all()
        same = larger == S
        assert np.array_equal(ext[same, 0], ch[same]) and np.array_equal(ext[same, 1], cw[same])
    per = 7
    n = len(boxes) // per * per
    counts = np.arange(n // per) % (per + 1)
    ext = ic.extents(boxes[:n], h, w, 8, count=counts, per_image=per)
    whole = ic.extents(boxes[:n], h, w, 8)
    live = (np.arange(n) % per) < counts[np.arange(n) // per]
    assert np.array_equal(ext[live], whole[live]) and (ext[~live] == 8).all() and live.any() and not live.all()


def _rne_bf16(b):
    return ((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF


def _rne_f16(b):
    sign, e, m = (b >> 16) & 0x8000, (b >> 23) & 0xFF, b & 0x7FFFFF
    E = e - 112                                                   # the fp16 exponent field
    # normal results: exponent and the top 10 fraction bits, 13 bits dropped (a carry runs into the exponent, up to infinity)
    q, rem = (np.maximum(E, 0) << 10) | (m >> 13), m & 0x1FFF
    normal = q + ((rem > 0x1000) | ((rem == 0x1000) & (q & 1 == 1)))
    # denormal results: the significand with its hidden bit, 14 - E bits dropped (all of it from 25 on)
    shift = np.clip(14 - E, 14, 25)
    full = np.where(e > 0, m | 0x800000, 0)
    q, rem, half = full >> shift, full & ((1 << shift) - 1), 1 << (shift - 1)
    denormal = q + ((rem > half) | ((rem == half) & (q & 1 == 1)))
    out = np.where(E >= 1, normal, denormal)
    return sign | np.where((E >= 31) | (out > 0x7C00), 0x7C00, out)


@pytest.mark.parametrize('dtype', ['bf16', 'fp16'])
def test_narrow_is_round_to_nearest_even(dtype):
    """all 65 536 upper halves of an fp32, each with the lower halves around both formats' ties (NaNs apart: no kernel here makes one)"""
    lows = [0x0000, 0x0001, 0x0FFF, 0x1000, 0x1001, 0x1FFF, 0x2000, 0x2FFF, 0x3000, 0x3001, 0x7FFF, 0x8000, 0x8001, 0xFFFF]
    b = (np.arange(65536, dtype=np.int64)[:, None] << 16 | np.array(lows, dtype=np.int64)[None, :]).reshape(-1)
    b = b[~(((b >> 23) & 0xFF == 0xFF) & (b & 0x7FFFFF != 0))]
    got = ic.narrow(b.astype(np.uint32).view(F), ic.STORAGE[dtype]).astype(np.int64) & 0xFFFF
    want = _rne_bf16(b) if dtype == 'bf16' else _rne_f16(b)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
