"""The byte-reading input kernels (include/cvpce_amd_input.h): the detector's transform and the RoI crop kernels fed an (H,W,3) uint8
image give the very bits the float kernels give for `ops.uint8_to_float` of it -- the inputs are the same numbers, so every
comparison is bit for bit -- and touch no byte outside the image."""
import ctypes

import pytest
import torch

import footprint as fp            # tests/footprint.py

pytestmark = pytest.mark.gpu

MEAN, STD = [0.485, 0.456, 0.406], [0.229, 0.224, 0.225]
_INT = {2: torch.int16, 4: torch.int32}


@pytest.fixture(autouse=True)
def byte_kernels(monkeypatch):
    from cvpce_amd import ops
    monkeypatch.setattr(ops, 'U8_KERNELS', True)


def bits(t):
    return t.view(_INT[t.element_size()])


def prefilled(shape, dtype, device):
    t = torch.empty(shape, dtype=dtype, device=device)
    bits(t).fill_(fp.prefill_value(dtype))
    return t


def image(seed, h, w):
    return torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


def boxes_for(h, w):
    """The boxes of the crop tests + the live count: the last slot lies beyond the count and must stay unwritten."""
    b = torch.tensor([[0.0, 0.0, w, h],                            # the whole image
                      [w - 1.0, h - 1.0, w, h],                    # 1 x 1 at the bottom-right pixel
                      [w - 9.0, h - 7.0, w + 11.0, h + 5.0],       # hanging over the right and the bottom edge
                      [-4.5, -2.25, 17.75, 20.5],                  # negative and fractional coordinates
                      [3.3, 2.9, 30.6, 33.2],
                      [12.0, 9.0, 12.0, 30.0],                     # zero area
                      [5.0, 2.0, 8.0, 32.0],                       # tall, 3 x 30
                      [4.0, 6.0, 34.0, 9.0],                       # wide, 30 x 3
                      [1.0, 1.0, 20.0, 20.0]], dtype=torch.float32)
    return b, len(b) - 1


def crop_out(p, s, mode, device):
    from cvpce_amd import ops
    return prefilled((p, 3, s, s), torch.float32, device) if mode == 0 else prefilled((p, s, s, 8 if mode == 1 else 4), ops.BF16, device)


# ---- codes --------------------------------------------------------------------------------------------------------------------
def test_every_code_is_its_table_value(cuda):
    from cvpce_amd import ops
    g = torch.Generator().manual_seed(3)
    u = torch.stack([torch.randperm(256, generator=g) for _ in range(3)], dim=1).to(torch.uint8).view(16, 16, 3).to(cuda)
    assert all(sorted(u[:, :, c].flatten().tolist()) == list(range(256)) for c in range(3))
    f = ops.uint8_to_float(u)
    box = torch.tensor([[0.0, 0.0, 16.0, 16.0]], device=cuda)
    got = ops.crop_resize(u, box, 16, mode=0)
    assert torch.equal(bits(got), bits(ops.crop_resize(f, box, 16, mode=0)))
    host = torch.arange(256, dtype=torch.float32) / 255.0              # scale 1: every tap weight is 1 or 0 -> the table itself
    for c in range(3):
        assert torch.equal(bits(got[0, c].cpu()), bits(host[u[:, :, c].cpu().long()]))
    for dt in (ops.BF16, ops.F16):
        a, b = prefilled((1, 16, 16, 8), dt, cuda), prefilled((1, 16, 16, 8), dt, cuda)
        ops.gln_transform_batch([u], a, [(16, 16)], MEAN, STD)
        ops.gln_transform_batch([f], b, [(16, 16)], MEAN, STD)
        assert torch.equal(bits(a), bits(b)) and not bool((bits(a) == fp.prefill_value(dt)).any())


# ---- transform ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['bf16', 'fp16'])
def test_transform_mixed_list_is_one_launch_and_exact(cuda, precision, monkeypatch):
    """[37x53 bytes, 64x48 float, 64x48 bytes] -> (24,35), (80,60), (80,60) in a 96 x 64 batch: odd widths (rows of 159 bytes), a
    downscale, an upscale, padding, and both forms in one list."""
    from cvpce_amd import ops
    dt = ops.STORAGE_TYPES[precision]
    us = [image(11, 37, 53).to(cuda), image(12, 64, 48).to(cuda), image(13, 64, 48).to(cuda)]
    fs = [ops.uint8_to_float(u) for u in us]
    sizes = [(24, 35), (80, 60), (80, 60)]
    want = prefilled((3, 96, 64, 8), dt, cuda)
    ops.gln_transform_batch(fs, want, sizes, MEAN, STD)
    got = prefilled((3, 96, 64, 8), dt, cuda)
    launches = []

    class Spy:                                                         # ops.T with every op call noted
        def __getattr__(self, name):
            def call(*args):
                launches.append(name)
                return getattr(torch.ops.cvpce_amd, name)(*args)
            return call

    with monkeypatch.context() as m:
        m.setattr(ops, 'T', Spy())
        ops.gln_transform_batch([us[0], fs[1], us[2]], got, sizes, MEAN, STD)
    assert launches == ['gln_transform_batch_u8']                      # the mixed list: one op call = one kernel launch (n <= 32)
    assert torch.equal(bits(got), bits(want)) and not bool((bits(got) == fp.prefill_value(dt)).any())
    for u, f, s in zip(us, fs, sizes):                                 # one image alone
        a, b = prefilled((1, 96, 64, 8), dt, cuda), prefilled((1, 96, 64, 8), dt, cuda)
        ops.gln_transform_batch([u], a, [s], MEAN, STD)
        ops.gln_transform_batch([f], b, [s], MEAN, STD)
        assert torch.equal(bits(a), bits(b))


# ---- crop ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def crop_images(cuda):
    from cvpce_amd import ops
    out = {}
    for hw in ((37, 53), (40, 64)):
        u = image(hw[0] * 100 + hw[1], *hw).to(cuda)
        out[hw] = (u, ops.uint8_to_float(u))
    return out


@pytest.mark.parametrize('s', [7, 8, 256])            # odd: the one-pixel kernel; even: two pixels per thread in modes 1 / 2
@pytest.mark.parametrize('mode', [0, 1, 2])
@pytest.mark.parametrize('hw', [(37, 53), (40, 64)])
def test_crop(cuda, crop_images, hw, mode, s):
    from cvpce_amd import ops
    u, f = crop_images[hw]
    boxes, live = boxes_for(hw[0], hw[1])
    boxes = boxes.to(cuda)
    count = torch.tensor([live], dtype=torch.int32, device=cuda)
    kw = dict(mean=MEAN, std=STD) if mode else {}
    for cnt in (count, None):
        got, want = crop_out(len(boxes), s, mode, cuda), crop_out(len(boxes), s, mode, cuda)
        ops.crop_resize(u, boxes, s, mode, count=cnt, out=got, **kw)
        ops.crop_resize(f, boxes, s, mode, count=cnt, out=want, **kw)
        assert torch.equal(bits(got), bits(want))
        stale = (bits(got) == fp.prefill_value(got.dtype)).flatten(1).all(dim=1).tolist()
        assert stale == [False] * live + [cnt is not None]             # the slot beyond the count is unwritten, every other is written


@pytest.mark.parametrize('s', [8, 256])
@pytest.mark.parametrize('mode', [1, 2])
@pytest.mark.parametrize('hw', [(37, 53), (40, 64)])
def test_crop_content_only(cuda, crop_images, hw, mode, s):
    from cvpce_amd import ops
    u, f = crop_images[hw]
    boxes, live = boxes_for(hw[0], hw[1])
    boxes = boxes.to(cuda)
    count = torch.tensor([live], dtype=torch.int32, device=cuda)
    ext = ops.crop_extents(boxes, count, hw[0], hw[1], s)
    got, want = crop_out(len(boxes), s, mode, cuda), crop_out(len(boxes), s, mode, cuda)
    ops.crop_resize(u, boxes, s, mode, mean=MEAN, std=STD, count=count, out=got, content_ext=ext)
    ops.crop_resize(f, boxes, s, mode, mean=MEAN, std=STD, count=count, out=want, content_ext=ext)
    e = ext.cpu().long()
    yy, xx = torch.arange(s).view(1, s, 1, 1), torch.arange(s).view(1, 1, s, 1)
    ey, ex = e[:, 0].view(-1, 1, 1, 1), e[:, 1].view(-1, 1, 1, 1)
    slot = (torch.arange(len(boxes)) < live).view(-1, 1, 1, 1)
    # inside the extents everything is written; a thread writes two pixels, so the column after an odd extent may be written too
    must, may = (yy < ey) & (xx < ex) & slot, (yy < ey) & (xx < ex + (ex & 1)) & slot
    assert must.any() and not may.all()
    must, may = must.expand(got.shape).to(cuda), may.expand(got.shape).to(cuda)
    assert torch.equal(bits(got)[must], bits(want)[must])
    pre = fp.prefill_value(got.dtype)
    for t in (got, want):
        assert not bool((bits(t)[must] == pre).any())
        assert bool((bits(t)[~may] == pre).all())                      # beyond the extents and beyond the count: not written
    assert torch.equal(bits(got), bits(want))                          # (the open column included: the same threads wrote it)
    whole = crop_out(len(boxes), s, mode, cuda)
    ops.crop_resize(u, boxes, s, mode, mean=MEAN, std=STD, count=count, out=whole)
    assert torch.equal(bits(got)[must], bits(whole)[must])


# ---- footprint ----------------------------------------------------------------------------------------------------------------
def byte_arena(u, device, guard):
    """-> (view, whole): `u`'s bytes between two guard bands filled with `guard`; the image ends where its end guard begins, at an
    address that is no multiple of 4.  (fp.arena fills integer guards with one value only: the two fills are made here.)"""
    n, g = u.numel(), fp.GUARD_MIN
    whole = torch.full((g + n + g,), guard, dtype=torch.uint8, device=device)
    view = whole[g:g + n].view(u.shape)
    view.copy_(u)
    return view, whole


def test_footprint(cuda):
    """Transform and crops of a 37 x 53 byte image (5 883 bytes: rows and the image's end are unaligned) in an arena whose guard
    bands hold 0x00, then 0xFF: a byte from outside the image that reached a result would change it between the two runs.  Outputs in
    footprint arenas: guards unchanged, everything that should be written is written."""
    from cvpce_amd import ops
    T = torch.ops.cvpce_amd
    u = image(21, 37, 53)
    f = ops.uint8_to_float(u.to(cuda))
    table = ops.uint8_table(cuda)
    boxes, live = boxes_for(37, 53)
    bx = fp.put(boxes, cuda)
    cnt = fp.put(torch.tensor([live], dtype=torch.int32), cuda)
    mask = (torch.arange(len(boxes)) < live)
    results = []
    for guard in (0x00, 0xFF):
        img, whole = byte_arena(u, cuda, guard)
        snap = whole.clone()
        got = []
        for dt in (ops.BF16, ops.F16):
            batch = fp.out((1, 64, 64, 8), dt, cuda)
            got += fp.check(lambda: T.gln_transform_batch_u8([img], table, batch[0], [48], [61], MEAN, STD), [], [batch], fills=('nan',))
        for mode, s in ((0, 7), (1, 7), (1, 8), (2, 8), (2, 64)):
            out = fp.out((len(boxes), 3, s, s) if mode == 0 else (len(boxes), s, s, 8 if mode == 1 else 4), torch.float32 if mode == 0 else ops.BF16, cuda)
            got += fp.check(lambda: T.crop_resize_u8(img, table, bx[0], cnt[0], out[0], s, mode, MEAN, STD), [bx, cnt], [out],
                            written=mask.view(-1, 1, 1, 1), fills=('nan',))
        assert torch.equal(whole, snap)                                # the image and its guard bands are only read
        results.append(got)
    for a, b in zip(*results):
        assert torch.equal(bits(a), bits(b))
    # ... and they are the float kernels' results
    want = []
    for dt in (ops.BF16, ops.F16):
        batch = torch.empty((1, 64, 64, 8), dtype=dt, device=cuda)
        ops.gln_transform_batch([f], batch, [(48, 61)], MEAN, STD)
        want.append(batch)
    for mode, s in ((0, 7), (1, 7), (1, 8), (2, 8), (2, 64)):
        want.append(ops.crop_resize(f, boxes.to(cuda), s, mode, mean=MEAN, std=STD))
    for a, b in zip(results[0][:2], want[:2]):
        assert torch.equal(bits(a), bits(b))
    for a, b in zip(results[0][2:], want[2:]):
        assert torch.equal(bits(a)[:live], bits(b)[:live])


# ---- bad arguments ------------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(cuda):
    from cvpce_amd import ops
    from cvpce_amd._lib import lib, float3
    T = torch.ops.cvpce_amd
    u = image(31, 20, 24)
    table = ops.uint8_table(cuda)
    boxes = torch.tensor([[0.0, 0.0, 24.0, 20.0]], device=cuda)
    out = prefilled((1, 3, 8, 8), torch.float32, cuda)
    batch = prefilled((1, 32, 32, 8), ops.F16, cuda)
    wide = image(32, 20, 30).to(cuda)[:, :24]                          # (20,24,3) with a row stride of 90 bytes
    assert tuple(wide.shape) == (20, 24, 3) and not wide.is_contiguous()
    planes = u.permute(2, 0, 1).contiguous().to(cuda)                  # (3,H,W) uint8
    bad = [
        lambda: ops.crop_resize(u, boxes, 8, mode=0, out=out),                                       # a CPU tensor
        lambda: ops.gln_transform_batch([u], batch, [(32, 32)], MEAN, STD),
        lambda: T.crop_resize_u8(u, table, boxes, None, out, 8, 0, None, None),
        lambda: T.gln_transform_batch_u8([u], table, batch, [32], [32], MEAN, STD),
        lambda: ops.crop_resize(planes, boxes, 8, mode=0, out=out),                                  # (3,H,W) uint8
        lambda: ops.gln_transform_batch([planes], batch, [(32, 32)], MEAN, STD),
        lambda: ops.device_bytes(planes, cuda),
        lambda: T.crop_resize_u8(planes, table, boxes, None, out, 8, 0, None, None),
        lambda: T.gln_transform_batch_u8([planes], table, batch, [32], [32], MEAN, STD),
        lambda: T.crop_resize_u8(wide, table, boxes, None, out, 8, 0, None, None),                   # not contiguous, to the raw ops
        lambda: T.crop_resize_content_u8(wide, table, boxes, None, out, 8, 1, MEAN, STD, torch.zeros(1, 2, dtype=torch.int32, device=cuda)),
        lambda: T.gln_transform_batch_u8([wide], table, batch, [32], [32], MEAN, STD),
        lambda: T.crop_resize_u8(u.to(cuda), table.cpu(), boxes, None, out, 8, 0, None, None),       # a table that is not on the device
    ]
    for i, call in enumerate(bad):
        with pytest.raises((RuntimeError, TypeError, NotImplementedError)):
            call()
            pytest.fail(f'bad call {i} was accepted')
    # H * W * 3 >= 2^31 through the C entry points, with small dummy allocations: refused on the host, nothing is dereferenced
    dummy = torch.zeros(64, dtype=torch.uint8, device=cuda)
    h0, w0 = 32768, 21846
    assert h0 * w0 * 3 >= 2 ** 31 > h0 * (w0 - 1) * 3
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ext = torch.zeros(1, 2, dtype=torch.int32, device=cuda)
    assert lib.cvpce_crop_resize_u8(p(dummy), p(table), p(boxes), None, 1, p(out), h0, w0, 8, 0, None, None, stream) == 1
    assert lib.cvpce_crop_resize_content_u8(p(dummy), p(table), p(boxes), None, 1, p(out), h0, w0, 8, 2, float3(MEAN), float3(STD), p(ext), stream) == 1
    one = lambda v: (ctypes.c_int * 1)(v)
    for fn in (lib.cvpce_gln_transform_batch_u8, lib.cvpce_gln_transform_batch_u8_f16):
        assert fn((ctypes.c_void_p * 1)(dummy.data_ptr()), (ctypes.c_ubyte * 1)(1), one(h0), one(w0), one(32), one(32), 1, p(batch), 32, 32,
                  float3(MEAN), float3(STD), p(table), stream) == 1
    assert lib.cvpce_crop_resize_u8(p(dummy), None, p(boxes), None, 1, p(out), 4, 4, 8, 0, None, None, stream) == 1      # no table
    torch.cuda.synchronize()
    for t in (out, batch):
        assert bool((bits(t) == fp.prefill_value(t.dtype)).all())      # nothing was launched
    # the good call, for contrast: the same arguments with a byte image on the device are accepted
    ops.crop_resize(u.to(cuda), boxes, 8, mode=0, out=out)
    assert not bool((bits(out) == fp.prefill_value(out.dtype)).any())
