"""Every kernel reads and writes only the tensors it is given.

Each case puts every operand of an entry point of include/cvpce_amd.h -- activations, residuals, masks, boxes, counts, work lists,
weights and biases -- into an input arena of tests/footprint.py and every output and workspace into an output arena, runs the entry
point once per guard fill through `footprint.check` (guards untouched, inputs untouched, every output element written or, under a
partial-write contract, exactly the contracted ones, results bit-identical across the fills and finite) and then compares the result
with a plain fp32 CPU computation on the same 16-bit-rounded operands, at the tolerances tests/test_gpu_kernels.py asserts for the
entry point.  Shapes are the smallest at which a tile edge exists on each side (tests/test_footprint_cpu.py shows that the checker
catches what it is meant to catch).  The views keep the alignment of a fresh allocation: smaller offsets are not tried here.
"""
import math
import zlib

import pytest
import torch
import torch.nn.functional as F

import footprint as fp            # tests/footprint.py
from footprint import listed_pixels as _listed_pixels, worklist_model as _worklist_model, whole

pytestmark = pytest.mark.gpu

BF, H16, F32 = torch.bfloat16, torch.float16, torch.float32
DTYPES = [BF, H16]
IDS = {BF: 'bf16', H16: 'fp16', F32: 'f32'}
TOL16, TOL32 = 1e-2, 2e-4         # rel_err bounds of tests/test_gpu_kernels.py: 16-bit outputs, f32 outputs


def rel_err(a, b):
    return ((a - b).abs().max() / b.abs().max().clamp(min=1e-6)).item()


def seeded(*key):
    return torch.Generator().manual_seed(zlib.crc32('/'.join(str(k) for k in key).encode()))


def to16(t, dt):
    from cvpce_amd import ops
    return ops.to_storage(t, dt)


def nchw(y):
    return y.float().permute(0, 3, 1, 2).cpu()


def packed_conv(wgt, bias, stride, pad, cuda, dt):
    """a PackedConv whose weight, halo-layout weight and bias are arena views of clones -> (pc, the arenas)"""
    from cvpce_amd import ops
    pc = ops.PackedConv(wgt, bias, stride, pad, device=cuda, dtype=dt)
    arenas = []
    for name in ('weight', 'weight_halo', 'bias'):
        t = getattr(pc, name)
        if t is not None:
            pair = fp.put(t, cuda)
            setattr(pc, name, pair[0])
            arenas.append(pair)
    return pc, arenas


def conv_operands(key, n, cin, h, w, cout, k, dt, cin_pad=None):
    """seeded x (n,h,w,cin_pad) of the storage type (channels >= cin zero), weight (cout,cin,k,k) f32, bias"""
    g = seeded(*key)
    cp = cin_pad or (cin + 7) // 8 * 8
    x = torch.zeros(n, h, w, cp)
    x[..., :cin] = torch.randn(n, h, w, cin, generator=g)
    wgt = torch.randn(cout, cin, k, k, generator=g) / math.sqrt(cin * k * k)
    bias = torch.randn(cout, generator=g) * 0.1
    return to16(x, dt), wgt, bias, g


def conv_ref(x16, cin, wgt, bias, dt, stride=1, pad=0, act=0, res=None, pool=False, in_up=0):
    """fp32 on the 16-bit-rounded operands: x16 NHWC storage type -> NCHW f32"""
    x = x16.float().permute(0, 3, 1, 2)[:, :cin]
    if in_up:
        x = F.interpolate(x, scale_factor=2.0, mode='nearest')
    y = F.conv2d(x, to16(wgt, dt).float(), bias, stride=stride, padding=pad)
    if res is not None:
        r = res.float().permute(0, 3, 1, 2)
        y = y + (r if r.shape[-2:] == y.shape[-2:] else F.interpolate(r, size=y.shape[-2:], mode='nearest'))
    if act == 1:
        y = F.relu(y)
    elif act == 2:
        y = torch.tanh(y)
    return F.max_pool2d(y, 2, 2) if pool else y


# ---------------------------------------------------------------------------------------------------------------------------------
# halo 3x3
# ---------------------------------------------------------------------------------------------------------------------------------
HALO_SHAPES = [(15, 17, False), (17, 15, False), (33, 31, False), (13, 13, False), (18, 34, True), (30, 44, True)]


@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('cout', [96, 128, 136, 264])
@pytest.mark.parametrize('cin', [64, 192])
@pytest.mark.parametrize('h,w,pool', HALO_SHAPES)
def test_conv3x3_halo(cuda, h, w, pool, cin, cout, dt):
    """cvpce_conv3x3_halo (16x16 tiles, Cout > 128) and _wide (16x32 tiles, Cout <= 128) through ops.conv2d(out=view): maps that no
    tile covers exactly, a map smaller than a tile, a ragged cout tile on both kernels, the fused pool."""
    from cvpce_amd import ops
    n = 2
    x, wgt, bias, _ = conv_operands(('halo', h, w, cin, cout), n, cin, h, w, cout, 3, dt)
    pc, wa = packed_conv(wgt, bias, 1, 1, cuda, dt)
    xin = fp.put(x, cuda)
    o = fp.out((n, h // 2, w // 2, cout) if pool else (n, h, w, cout), dt, cuda)
    ran = []

    def run():
        before = ops.HALO_RAGGED, ops.PROFILE
        ops.HALO_RAGGED, ops.PROFILE = True, ops.ConvProfile()
        try:
            assert ops.conv2d(xin[0], pc, act=1, pool=pool, out=o[0]) is o[0]
            ran.append(ops.PROFILE.records[-1][0])
        finally:
            ops.HALO_RAGGED, ops.PROFILE = before
    y, = fp.check(run, [xin] + wa, [o])
    assert ran == ['conv3x3_halo3_kernel' if cout <= 128 else 'conv3x3_halo2_kernel'] * 3
    assert rel_err(nchw(y), conv_ref(x, cin, wgt, bias, dt, 1, 1, act=1, pool=pool)) < TOL16


# every map with the plain store and with no store; the fused pool on the two even maps
MAC_CASES = ([(h, w, mode) for mode in ('store', 'no store') for h, w, _ in HALO_SHAPES]
             + [(h, w, 'store+pool') for h, w, pool in HALO_SHAPES if pool])


@pytest.mark.parametrize('cout', [96, 128, 136, 264])
@pytest.mark.parametrize('cin', [64, 192])
@pytest.mark.parametrize('h,w,mode', MAC_CASES)
def test_conv3x3_halo_mac(cuda, h, w, mode, cin, cout):
    """cvpce_conv3x3_halo_mac writing its descriptor at column 40 of a wider row (the caller zero-fills that slice: the kernel takes
    an atomic maximum): the columns outside the slice keep the prefill; with the map stored, stored pooled, and not stored at all.
    Cout <= 128 belongs to the wide-tile kernel, which has no descriptor epilogue: the entry point refuses it, and writes nothing."""
    T = torch.ops.cvpce_amd
    n, off = 2, 40
    x, wgt, bias, _ = conv_operands(('mac', h, w, cin, cout), n, cin, h, w, cout, 3, BF)
    pc, wa = packed_conv(wgt, bias, 1, 1, cuda, BF)
    xin = fp.put(x, cuda)
    mac = fp.out((n, off + cout + 24), F32, cuda)
    pool = mode == 'store+pool'
    o = None if mode == 'no store' else fp.out((n, h // 2, w // 2, cout) if pool else (n, h, w, cout), BF, cuda)
    cols = torch.zeros(1, off + cout + 24, dtype=torch.bool)
    cols[:, off:off + cout] = True

    def launch():
        T.conv3x3_halo_mac(xin[0], pc.weight_halo, pc.bias, o[0] if o else None, mac[0], off, cout, pc.k_pad, pc.cout_pad, int(pool))
    if cout <= 128:
        with pytest.raises(RuntimeError):
            launch()
        torch.cuda.synchronize()
        for view, whole in [mac] + ([o] if o else []):
            b = whole.view(fp._INT_VIEW[view.element_size()])
            assert torch.equal(b, torch.full_like(b, fp.prefill_value(view.dtype)))
        return

    def run():
        mac[0][:, off:off + cout].zero_()                              # the caller's part of the contract
        launch()
    got = fp.check(run, [xin] + wa, [mac] + ([o] if o else []), written=[cols] + ([None] if o else []))
    ref = conv_ref(x, cin, wgt, bias, BF, 1, 1, act=1)
    assert rel_err(got[0][:, off:off + cout].cpu(), ref.to(BF).float().amax(dim=(-2, -1))) < TOL16
    if o:
        assert rel_err(nchw(got[1]), F.max_pool2d(ref, 2, 2) if pool else ref) < TOL16


@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('use_map', [False, True], ids=['mask', 'mask+tile map'])
def test_conv3x3_halo_masked(cuda, use_map, dt):
    """cvpce_conv3x3_halo_masked on a two-level atlas (tests/test_gpu_kernels.py test_conv3x3_atlas_masked): every pixel of a computed
    tile is written, zeros on the gaps; with a tile map the tiles that are not on it are not touched at all."""
    from cvpce_amd import ops
    T = torch.ops.cvpce_amd
    n, cin, cout, hh, ww = 2, 128, 256, 21, 61
    g = seeded('masked', dt)
    a = to16(torch.randn(n, 21, 30, cin, generator=g), dt)
    b = to16(torch.randn(n, 9, 14, cin, generator=g), dt)
    wgt = torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(9 * cin)
    bias = torch.randn(cout, generator=g) * 0.1
    pc, wa = packed_conv(wgt, bias, 1, 1, cuda, dt)
    atlas = torch.zeros(n, hh, ww, cin, dtype=dt)            # columns 45..60: a tile column that lies wholly in the gap
    atlas[:, :, :30] = a
    atlas[:, 5:14, 31:45] = b
    mask = torch.zeros(hh, ww, dtype=torch.uint8)
    mask[:, :30] = 1
    mask[5:14, 31:45] = 1
    xin, min_ = fp.put(atlas, cuda), fp.put(mask, cuda)
    tmap, written = None, None
    if use_map:
        tiles = ops.atlas_tile_map(mask)
        assert tiles.numel() == 5
        tmap = fp.put(tiles, cuda)
        written = torch.zeros(1, hh, ww, 1, dtype=torch.bool)
        for t in tiles.tolist():
            written[:, (t >> 16) * 16:(t >> 16) * 16 + 16, (t & 0xFFFF) * 16:(t & 0xFFFF) * 16 + 16] = True
        assert not bool(written[:, :, 48:].any()) and not bool(written[:, 16:, 32:].any())
    o = fp.out((n, hh, ww, cout), dt, cuda)

    def run():
        T.conv3x3_halo_masked(xin[0], pc.weight_halo, pc.bias, min_[0], tmap[0] if tmap else None, o[0], cout, pc.k_pad, pc.cout_pad, 1)
    y, = fp.check(run, [xin, min_, tmap] + wa, [o], written=written)
    y = y.cpu()
    assert rel_err(nchw(y[:, :, :30]), conv_ref(a, cin, wgt, bias, dt, 1, 1, act=1)) < TOL16
    assert rel_err(nchw(y[:, 5:14, 31:45]), conv_ref(b, cin, wgt, bias, dt, 1, 1, act=1)) < TOL16
    gap = (mask == 0)[None, :, :, None] & (written if use_map else torch.ones(1, hh, ww, 1, dtype=torch.bool))
    assert float(y.float()[gap.expand_as(y)].abs().max()) == 0.0


@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('cout', [9, 36, 1])
@pytest.mark.parametrize('cin', [64, 192])
def test_conv3x3_halo_thin_out(cuda, cin, cout, dt):
    """cvpce_conv3x3_halo_thin_out at 48 x 50, the smallest map ops.conv2d sends to it: 16 x 32 tiles ragged on the right, a Cout that
    is not a multiple of 4, Cout = 1, fp32 stores."""
    T = torch.ops.cvpce_amd
    n, h, w = 2, 48, 50
    x, wgt, bias, _ = conv_operands(('thin_out', cin, cout), n, cin, h, w, cout, 3, dt)
    pc, wa = packed_conv(wgt, bias, 1, 1, cuda, dt)
    xin, o = fp.put(x, cuda), fp.out((n, h, w, cout), F32, cuda)
    y, = fp.check(lambda: T.conv3x3_halo_thin_out(xin[0], pc.weight_halo, pc.bias, o[0], cout, pc.k_pad, pc.cout_pad), [xin] + wa, [o])
    assert rel_err(nchw(y), conv_ref(x, cin, wgt, bias, dt, 1, 1)) < TOL32


# ---------------------------------------------------------------------------------------------------------------------------------
# work-list and strip launches of the embedder
# ---------------------------------------------------------------------------------------------------------------------------------
def test_list_and_strip_launches(cuda):
    """cvpce_crop_extents -> cvpce_embed_worklists -> cvpce_vgg_stem_fused_list -> cvpce_conv3x3_halo_list (wide tiles; 16x16 tiles with
    the fused pool; with the MAC descriptor and no store) + cvpce_conv3x3_halo_strips + cvpce_mac_init, on three crops (a wide box, a
    very thin one, a box without any content column) plus the constant crop at S = 64.  Every launch writes exactly the tiles -- and of
    a cut tile the rows -- on its list; pixels of tiles that are not listed keep the prefill bit for bit, and are never read: the next
    layer's input arena holds them as NaNs."""
    from cvpce_amd import ops
    from cvpce_amd.models.classification import TANH_MEAN, TANH_STD
    T = torch.ops.cvpce_amd
    S, n = 64, 4
    g = seeded('lists')
    img = torch.rand(3, 48, 64, generator=g)
    boxes = torch.tensor([[2., 3., 38., 20.], [1., 10., 41., 12.], [10., 10., 10.5, 30.]])
    imgin, bxin = fp.put(img, cuda), fp.put(boxes, cuda)
    ext = fp.out((3, 2), torch.int32, cuda)
    e, = fp.check(lambda: T.crop_extents(bxin[0], None, 0, 48, 64, S, ext[0]), [bxin], [ext])
    e = e.cpu()
    assert 27 <= int(e[0, 0]) <= 34 and int(e[0, 1]) == S and 1 <= int(e[1, 0]) <= 6 and int(e[2, 1]) == 0, e
    # op chain: conv1_1 conv1_2 pool1 | convA (64 -> 128, wide tiles) | convB (128 -> 256) poolB | convC (256 -> 264, MAC, not stored)
    pool_mask = 0b0100100
    layers = [ops.skip_layer(32, 32, 8, 8, 3, 64, 64, 0, 1), ops.skip_layer(32, 32, 16, 32, 4, 32, 32, 3, 2),
              ops.skip_layer(16, 16, 8, 8, 6, 32, 32, 4, 3), ops.skip_layer(16, 16, 16, 16, 7, 16, 16, 6, 3)]
    nl, max_tiles = len(layers), (S // 16) ** 2
    extin = fp.put(e, cuda)
    # sized exactly as ops.embed_worklists sizes them
    lists, counts, computed = fp.out((2 * nl, n * max_tiles), torch.int64, cuda), fp.out((3 * nl,), torch.int32, cuda), fp.out((nl, n, 2), torch.int32, cuda)
    # what the lists must hold comes from the Python model, not from the kernel: a wrong count cannot move the mask with it
    model = _worklist_model(e.tolist() + [[S, S]], S, pool_mask, layers)
    cnt = [len(m[0]) for m in model] + [m[2] for m in model] + [len(m[1]) for m in model]
    ref_l = torch.zeros(2 * nl, n * max_tiles, dtype=torch.int64)
    lmask = torch.zeros(2 * nl, n * max_tiles, dtype=torch.bool)
    for l, (want, swant, _, _) in enumerate(model):
        for row, ent in ((l, want), (nl + l, swant)):
            ref_l[row, :len(ent)] = torch.tensor(ent, dtype=torch.int64)
            lmask[row, :len(ent)] = True
    flat = [v for l in layers for v in l]
    L, C, K = fp.check(lambda: T.embed_worklists(extin[0], n, S, pool_mask, flat, lists[0], counts[0], computed[0]), [extin],
                       [lists, counts, computed], written=[lmask, None, None])
    assert C.cpu().tolist() == cnt and torch.equal(L.cpu()[lmask], ref_l[lmask])
    assert K.cpu().tolist() == [m[3] for m in model]
    assert cnt[2 * nl + 2] > 0 and cnt[2 * nl + 3] > 0 and cnt[2 * nl] == cnt[2 * nl + 1] == 0, cnt          # both halo2 layers have strips
    L = L.cpu()
    lin, cin_ = fp.put(L.to(cuda), cuda), fp.put(C, cuda)
    entries = lambda row, k: L[row, :k].tolist()

    # the crops: content only (what the work-list embedder is given), the padding stays unwritten
    crops = fp.out((3, S, S, 4), BF, cuda)
    yy, xx = torch.arange(S).view(1, S, 1, 1), torch.arange(S).view(1, 1, S, 1)
    ey, ex = e[:, 0].view(-1, 1, 1, 1), e[:, 1].view(-1, 1, 1, 1)
    must, may = (yy < ey) & (xx < ex), (yy < ey) & (xx < ex + (ex & 1))            # (a thread writes two pixels)
    x0, = fp.check(lambda: T.crop_resize_content(imgin[0], bxin[0], None, crops[0], S, 2, list(TANH_MEAN), list(TANH_STD), extin[0]),
                   [imgin, bxin, extin], [crops], written=(must, may))
    const = ops.crop_resize(torch.zeros(3, 1, 1, device=cuda), torch.zeros(1, 4, device=cuda), S, mode=2, mean=TANH_MEAN, std=TANH_STD)[0]
    full = ops.crop_resize(img.to(cuda), boxes.to(cuda), S, mode=2, mean=TANH_MEAN, std=TANH_STD)
    assert torch.equal(x0.cpu()[must.expand_as(x0)], full.cpu()[must.expand_as(full)])
    x0in, cstin = fp.put(x0, cuda), fp.put(const, cuda)                              # x0's padding: the prefill NaNs

    # stem over its list
    w1, b1 = torch.randn(64, 3, 3, 3, generator=g) / math.sqrt(27), torch.randn(64, generator=g) * 0.1
    w2, b2 = torch.randn(64, 64, 3, 3, generator=g) / math.sqrt(576), torch.randn(64, generator=g) * 0.1
    ps = ops.PackedStem(w1, b1, w2, b2, device=cuda)
    sa = [fp.put(t, cuda) for t in (ps.w1, ps.b1, ps.w2, ps.b2)]
    t0 = fp.out((n, 32, 32, 64), BF, cuda)
    m0 = _listed_pixels(entries(0, cnt[0]), n, 32, 32, 8, 8)
    assert bool(m0[3].all()) and not bool(m0[2, :, 8:].any()) and 0 < int(m0[0].sum()) < 32 * 32
    y0, = fp.check(lambda: T.vgg_stem_fused_list(x0in[0], cstin[0], sa[0][0], sa[1][0], sa[2][0], sa[3][0], t0[0], lin[0][0], cin_[0][0:1]),
                   [x0in, cstin, lin, cin_] + sa, [t0], written=m0)
    xfull = torch.cat((full.cpu(), const.cpu()[None]))
    mid = F.relu(F.conv2d(xfull.float().permute(0, 3, 1, 2)[:, :3], w1.to(BF).float(), b1, padding=1)).to(BF).float()
    ref0 = F.max_pool2d(F.relu(F.conv2d(mid, w2.to(BF).float(), b2, padding=1)), 2, 2).permute(0, 2, 3, 1)
    sel = m0.expand_as(ref0)
    assert rel_err(y0.cpu().float()[sel], ref0[sel]) < TOL16

    def list_layer(li, prev, prev_mask, cin, cout, pool, th, tw, mac_off=None):
        """layer li over its list (+ its strip list) on the previous layer's output AS IT WAS LEFT -> (output, its pixel mask)"""
        hin = prev.shape[1]
        gl = seeded('lists', li)
        wgt = torch.randn(cout, cin, 3, 3, generator=gl) / math.sqrt(9 * cin)
        bias = torch.randn(cout, generator=gl) * 0.1
        pc, wa = packed_conv(wgt, bias, 1, 1, cuda, BF)
        pin = fp.put(prev, cuda)
        ho = hin // 2 if pool else hin
        strips = cout > 128
        ent = entries(li, cnt[li]) + (entries(nl + li, cnt[2 * nl + li]) if strips else [])
        ref = conv_ref(whole(prev, prev_mask), cin, wgt, bias, BF, 1, 1, act=1)
        if mac_off is None:
            o = fp.out((n, ho, ho, cout), BF, cuda)
            m = _listed_pixels(ent, n, ho, ho, th, tw)

            def run():
                T.conv3x3_halo_list(pin[0], pc.weight_halo, pc.bias, o[0], None, 0, cout, pc.k_pad, pc.cout_pad, 1, int(pool), lin[0][li], cin_[0][li:li + 1])
                if strips:
                    T.conv3x3_halo_strips(pin[0], pc.weight_halo, pc.bias, o[0], None, 0, cout, pc.k_pad, pc.cout_pad, 1, int(pool), lin[0][nl + li],
                                          cin_[0][2 * nl + li:2 * nl + li + 1])
            y, = fp.check(run, [pin, lin, cin_] + wa, [o], written=m)
            ref = (F.max_pool2d(ref, 2, 2) if pool else ref).permute(0, 2, 3, 1)
            s_ = m.expand_as(ref)
            assert 0 < int(m.sum()) < m.numel() and rel_err(y.cpu().float()[s_], ref[s_]) < TOL16
            return y, m
        # MAC layer, nothing stored: cvpce_mac_init starts the descriptor slice from the constant crop's suffix maxima
        pf = whole(prev, prev_mask)
        const_map = ops.conv2d(pf[-1:].to(cuda), pc, act=1)[0].float()                                    # (H, W, C) >= 0
        zero = torch.zeros((1, cout), device=cuda)
        rows = fp.put(torch.cat((torch.cummax(const_map.amax(dim=1).flip(0), 0).values.flip(0), zero)), cuda)
        cols = fp.put(torch.cat((torch.cummax(const_map.amax(dim=0).flip(0), 0).values.flip(0), zero)), cuda)
        kin = fp.put(K[li].contiguous(), cuda)
        desc = fp.out((n, mac_off + cout + 24), F32, cuda)
        dm = torch.zeros(1, mac_off + cout + 24, dtype=torch.bool)
        dm[:, mac_off:mac_off + cout] = True

        def run():
            T.mac_init(desc[0], mac_off, rows[0], cols[0], kin[0])
            T.conv3x3_halo_list(pin[0], pc.weight_halo, pc.bias, None, desc[0], mac_off, cout, pc.k_pad, pc.cout_pad, 1, 0, lin[0][li], cin_[0][li:li + 1])
            T.conv3x3_halo_strips(pin[0], pc.weight_halo, pc.bias, None, desc[0], mac_off, cout, pc.k_pad, pc.cout_pad, 1, 0, lin[0][nl + li],
                                  cin_[0][2 * nl + li:2 * nl + li + 1])
        d, = fp.check(run, [pin, lin, cin_, rows, cols, kin] + wa, [desc], written=dm)
        assert rel_err(d[:, mac_off:mac_off + cout].cpu(), ref.to(BF).float().amax(dim=(-2, -1))) < TOL16
        return d, dm

    y1, m1 = list_layer(1, y0, m0, 64, 128, False, 16, 32)
    y2, m2 = list_layer(2, y1, m1, 128, 256, True, 8, 8)
    list_layer(3, y2, m2, 256, 264, False, 16, 16, mac_off=40)


# ---------------------------------------------------------------------------------------------------------------------------------
# implicit GEMM
# ---------------------------------------------------------------------------------------------------------------------------------
IGEMM_CASES = [  # name, n, cin, h, w, cout, k, stride, pad, options
    ('ragged_m', 3, 64, 5, 3, 192, 3, 1, 1, {}),
    ('stem7x7_s2', 1, 3, 19, 13, 64, 7, 2, 3, {}),
    ('3x3_s2', 2, 64, 7, 9, 64, 3, 2, 1, {}),
    ('f32_cout9', 2, 256, 7, 7, 9, 3, 1, 1, {'f32': True, 'act': 0}),
    ('f32_cout36', 2, 256, 7, 7, 36, 3, 1, 1, {'f32': True, 'act': 0}),
    ('f32_cout1', 2, 256, 7, 7, 1, 3, 1, 1, {'f32': True, 'act': 0}),
    ('in_up', 2, 64, 5, 7, 32, 3, 1, 1, {'in_up': 1}),
    ('residual', 2, 64, 9, 11, 256, 1, 1, 0, {'res': 'same'}),
    ('res_resampled', 2, 64, 25, 25, 256, 1, 1, 0, {'res': (13, 13), 'act': 0}),
    ('pool_7x9', 2, 32, 7, 9, 64, 3, 1, 1, {'pool': True, 'rejected': True}),          # odd map: the entry point refuses a fused pool
    ('pool_20x24', 2, 32, 20, 24, 64, 3, 1, 1, {'pool': True}),
]


def _conv2d_case(cuda, dt, name, n, cin, h, w, cout, k, stride, pad, o, splitk=0):
    from cvpce_amd import ops
    from cvpce_amd._lib import lib
    T = torch.ops.cvpce_amd
    x, wgt, bias, g = conv_operands(('igemm', name), n, cin, h, w, cout, k, dt)
    pc, wa = packed_conv(wgt, bias, stride, pad, cuda, dt)
    act, in_up, f32, pool = o.get('act', 1), o.get('in_up', 0), o.get('f32', False), o.get('pool', False)
    ho, wo = pc.out_hw(h, w, in_up)
    res, res_mode = None, 0
    if o.get('res') == 'same':
        res, res_mode = to16(torch.randn(n, ho, wo, cout, generator=g), dt), 1
    elif o.get('res'):
        res, res_mode = to16(torch.randn(n, *o['res'], cout, generator=g), dt), 2
    xin, rin = fp.put(x, cuda), fp.put(res, cuda)
    out = fp.out((n, ho // 2, wo // 2, cout) if pool else (n, ho, wo, cout), F32 if f32 else dt, cuda)
    if splitk:
        ws = fp.out((int(lib.cvpce_conv2d_splitk_workspace_bytes(n * ho * wo, cout, splitk)),), torch.uint8, cuda)
        run = lambda: T.conv2d_splitk(xin[0], pc.weight, pc.bias, rin[0] if rin else None, out[0], cout, k, k, stride, pad, ho, wo, pc.k_pad,
                                      pc.cout_pad, act, int(f32), in_up, res_mode, splitk, ws[0])
    else:
        ws = None
        run = lambda: T.conv2d_nhwc(xin[0], pc.weight, pc.bias, rin[0] if rin else None, out[0], cout, k, k, stride, pad, ho, wo, pc.k_pad,
                                    pc.cout_pad, act, int(f32), in_up, res_mode, int(pool), 0)
    if o.get('rejected'):
        with pytest.raises(RuntimeError):
            run()
        return
    if o.get('variant'):
        assert ops.ConvProfile.variant(pc, n * ho * wo, in_up) == o['variant']
    got = fp.check(run, [xin, rin] + wa, [out] + ([ws] if ws else []), written=[None] + ([fp.SCRATCH] if ws else []))
    ref = conv_ref(x, cin, wgt, bias, dt, stride, pad, act=act, res=res, pool=pool, in_up=in_up)
    assert rel_err(nchw(got[0]), ref) < (TOL32 if f32 else TOL16)


@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('case', IGEMM_CASES, ids=[c[0] for c in IGEMM_CASES])
def test_conv2d_nhwc_generic(cuda, case, dt):
    """cvpce_conv2d_nhwc_*: the register-staged kernels (128-, 64- and 32-cout tiles, K-steps 64 and 32) on maps far below one pixel
    tile, every epilogue: fp32 stores with Cout 9 / 36 / 1, the upsampled input, both residual forms, the fused pool."""
    _conv2d_case(cuda, dt, *case)


DMA_CASES = [  # M = 13 * 41 * 61 = 127 * 256 + 1: the smallest M that selects each LDS-DMA tile form, ragged in Cout
    ('dma256', 13, 64, 41, 61, 192, 3, 1, 1, {'variant': 'conv_dma16_kernel<256,256,2,4,2,4>'}),
    # the same form on an upsampled input goes to the 2-buffer kernel; an upsampled map is even, M = 13 * 42 * 62 = 132 * 256 + 60
    ('dma256_in_up', 13, 64, 21, 31, 192, 3, 1, 1, {'in_up': 1, 'variant': 'conv_dma_kernel<256,256,2,4,2>'}),
    ('dma128', 13, 64, 41, 61, 96, 3, 1, 1, {'variant': 'conv_dma_kernel<128,128,2,2,2>'}),
    ('dma64', 13, 64, 41, 61, 40, 3, 1, 1, {'variant': 'conv_dma_kernel<64,128,2,2,2>'}),
]


@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('case', DMA_CASES, ids=[c[0] for c in DMA_CASES])
def test_conv2d_nhwc_lds_dma(cuda, case, dt):
    """cvpce_conv2d_nhwc_* on the LDS-DMA kernels: the dispatch takes them from 128 pixel tiles of 256 up, so M = 32 513 pixels -- 127
    full tiles and a last one that holds a single pixel, with image boundaries inside the tiles -- is the smallest M for each form;
    one M below it `variant` names a register-staged kernel (dma256_in_up: the 2-buffer 256 x 256 kernel on an upsampled input, at
    M = 33 852, 133 tiles with a ragged last one).  Which kernel ran is read from ops.ConvProfile.variant, the Python
    mirror of the dispatch in csrc/conv_igemm.hip (conv2d_dispatch): the library does not report the kernel it launched, so this
    confirms the case against the mirror, and the mirror is held to the C++ only by reading the two side by side."""
    from cvpce_amd import ops
    name, n, cin, h, w, cout = case[:6]
    pc = ops.PackedConv(torch.zeros(cout, cin, 3, 3), None, 1, 1, device=cuda, dtype=dt)
    in_up = case[9].get('in_up', 0)
    if in_up:
        assert n * (2 * h) * (2 * w) == 132 * 256 + 60          # (upsampled maps are even: no batch of them has 127 * 256 + 1 pixels)
    else:
        assert n * h * w == 127 * 256 + 1
    assert 'conv_igemm_kernel' in ops.ConvProfile.variant(pc, 127 * 256, in_up)
    _conv2d_case(cuda, dt, *case)


SPLITK_CASES = [
    ('splitk_s2', 4, 256, 13, 13, 256, 3, 2, 1, {'act': 0}),
    ('splitk_f32', 2, 320, 9, 11, 200, 3, 1, 1, {'f32': True}),
    ('splitk_res', 1, 256, 25, 25, 256, 3, 1, 1, {'res': 'same', 'act': 0}),
]


@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('case', SPLITK_CASES, ids=[c[0] for c in SPLITK_CASES])
def test_conv2d_splitk(cuda, case, dt):
    """cvpce_conv2d_splitk_*: the workspace is an arena of exactly cvpce_conv2d_splitk_workspace_bytes -- the partial tiles of the ragged
    last pixel tile and cout tile must fit the formula."""
    _conv2d_case(cuda, dt, *case, splitk=4)


C1X1_CASES = [  # name, n, cin, h, w, cout, stride, residual
    ('3_cout_tiles_res', 1, 128, 5, 7, 192, 1, 'same'),
    ('k512', 2, 512, 7, 9, 256, 1, None),
    ('stride2', 2, 256, 9, 11, 512, 2, None),
    ('res_resampled', 1, 1024, 25, 33, 256, 1, (13, 17)),
    ('k64_res_up', 1, 64, 30, 31, 128, 1, (15, 16)),
]


@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('name,n,cin,h,w,cout,stride,res', C1X1_CASES, ids=[c[0] for c in C1X1_CASES])
def test_conv1x1_nhwc(cuda, name, n, cin, h, w, cout, stride, res, dt):
    """cvpce_conv1x1_nhwc_*: the streaming kernels (weights in registers / staged through LDS) and the strided form on a few dozen
    pixels, with the same-size and the nearest-resampled residual."""
    T = torch.ops.cvpce_amd
    x, wgt, bias, g = conv_operands(('1x1', name), n, cin, h, w, cout, 1, dt)
    pc, wa = packed_conv(wgt, bias, stride, 0, cuda, dt)
    ho, wo = pc.out_hw(h, w)
    r, mode = None, 0
    if res == 'same':
        r, mode = to16(torch.randn(n, ho, wo, cout, generator=g), dt), 1
    elif res:
        r, mode = to16(torch.randn(n, *res, cout, generator=g), dt), 2
    xin, rin, o = fp.put(x, cuda), fp.put(r, cuda), fp.out((n, ho, wo, cout), dt, cuda)
    y, = fp.check(lambda: T.conv1x1_nhwc(xin[0], pc.weight, pc.bias, rin[0] if rin else None, o[0], cout, stride, ho, wo, pc.k_pad, pc.cout_pad, 1, mode),
                  [xin, rin] + wa, [o])
    assert rel_err(nchw(y), conv_ref(x, cin, wgt, bias, dt, stride, 0, act=1, res=r)) < TOL16


# ---------------------------------------------------------------------------------------------------------------------------------
# thin and Gaussian layers
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('n,h,w,cout,up', [(1, 7, 70, 32, 0), (1, 51, 33, 16, 0), (1, 3, 5, 32, 1)])
def test_conv3x3_thin(cuda, n, h, w, cout, up, dt):
    """cvpce_conv3x3_thin_*: ragged 16-pixel column strips, fewer / more rows than a task, the upsampled-input form on a 3 x 5 stored map."""
    T = torch.ops.cvpce_amd
    cin = 64 if up else 32
    x, wgt, bias, _ = conv_operands(('thin', h, w, cout), n, cin, h, w, cout, 3, dt)
    pc, wa = packed_conv(wgt, bias, 1, 1, cuda, dt)
    xin, o = fp.put(x, cuda), fp.out((n, h << up, w << up, cout), dt, cuda)
    y, = fp.check(lambda: T.conv3x3_thin(xin[0], pc.weight, pc.bias, o[0], cout, pc.k_pad, pc.cout_pad, 1, up), [xin] + wa, [o])
    assert rel_err(nchw(y), conv_ref(x, cin, wgt, bias, dt, 1, 1, act=1, in_up=up)) < TOL16


@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('act', [1, 2], ids=['relu', 'tanh'])
@pytest.mark.parametrize('n,hs,ws_', [(1, 1, 1), (1, 3, 57), (2, 7, 29)])
def test_gauss_subnet(cuda, n, hs, ws_, act, dt):
    """cvpce_gauss_subnet_*: a 2 x 2 output, a map wider than it is high with a ragged last strip, two images.  Reference and bounds:
    tests/test_gpu_kernels.py test_gauss_subnet_parity (every layer rounded where the per-layer kernels store it)."""
    from cvpce_amd import ops
    T = torch.ops.cvpce_amd
    g = seeded('subnet', hs, ws_, act)
    rd = lambda t: t.to(dt).to(F32)
    shapes = [(32, 64, 3), (32, 32, 3), (16, 32, 3), (16, 16, 1), (1, 16, 1)]
    wts = [torch.randn(co, ci, k, k, generator=g) * math.sqrt(2.0 / (k * k * ci)) for co, ci, k in shapes]
    bs = [torch.randn(co, generator=g) * 0.1 for co, _, _ in shapes]
    convs = [ops.PackedConv(w_, b_, 1, 1 if w_.shape[-1] == 3 else 0, device=cuda, dtype=dt) for w_, b_ in zip(wts, bs)]
    wa = []
    for c in convs:
        for name in ('weight', 'bias'):
            pair = fp.put(getattr(c, name), cuda)
            setattr(c, name, pair[0])
            wa.append(pair)
    x = rd(torch.randn(n, 64, hs, ws_, generator=g).relu())
    xin = fp.put(x.permute(0, 2, 3, 1).contiguous().to(dt), cuda)
    o = fp.out((n, 2 * hs, 2 * ws_, 1), F32, cuda)
    c1, c2, c3, c4, c5 = convs
    y, = fp.check(lambda: T.gauss_subnet(xin[0], c1.weight, c1.bias, c2.weight, c2.bias, c3.weight, c3.bias, c4.weight, c4.bias, c4.k_pad,
                                         c5.weight, c5.bias, c5.k_pad, o[0], act), [xin] + wa, [o])
    t = F.interpolate(x, scale_factor=2.0, mode='nearest')
    for i in range(3):
        t = rd(F.relu(F.conv2d(t, rd(wts[i]), bs[i], padding=1)))
    t = rd(F.relu(F.conv2d(t, rd(wts[3]), bs[3])))
    z = F.conv2d(t, rd(wts[4]), bs[4])[:, 0]
    ref = torch.tanh(z) if act == 2 else F.relu(z)
    atol, mtol = (3e-2, 1.5e-3) if dt == BF else (4e-3, 2e-4)
    scale = max(1.0, float(ref.abs().max()))
    d = (y.cpu()[..., 0] - ref).abs()
    assert d.max() <= atol * scale and d.mean() <= mtol * scale, (d.max(), d.mean(), scale)


@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('act', [1, 2], ids=['relu', 'tanh'])
@pytest.mark.parametrize('npix', [1, 63, 65 * 3])
def test_gauss_tail(cuda, npix, act, dt):
    """cvpce_gauss_tail_*: one pixel, one short of a wave, a ragged last block.  Bounds: tests/test_gpu_kernels.py test_gauss_tail_parity."""
    from cvpce_amd import ops
    T = torch.ops.cvpce_amd
    g = seeded('tail', npix, act)
    rd = lambda t: t.to(dt).to(F32)
    x = torch.randn(npix, 16, generator=g).relu()
    w4, b4 = torch.randn(16, 16, 1, 1, generator=g) / 4, torch.randn(16, generator=g) * 0.1
    w5, b5 = torch.randn(1, 16, 1, 1, generator=g) / 4, torch.randn(1, generator=g) * 0.1
    c4, a4 = packed_conv(w4, b4, 1, 0, cuda, dt)
    c5, a5 = packed_conv(w5, b5, 1, 0, cuda, dt)
    xin, o = fp.put(x.to(dt), cuda), fp.out((npix,), F32, cuda)
    y, = fp.check(lambda: T.gauss_tail(xin[0], c4.weight, c4.bias, c5.weight, c5.bias, o[0], c4.k_pad, act), [xin] + a4 + a5, [o])
    hid = rd(F.relu(rd(x) @ rd(w4[:, :, 0, 0]).t() + b4))
    ref = hid @ rd(w5[0, :, 0, 0]) + b5
    ref = torch.tanh(ref) if act == 2 else F.relu(ref)
    torch.testing.assert_close(y.cpu(), ref, rtol=0, atol=2e-2 if dt == BF else 3e-3)


# ---------------------------------------------------------------------------------------------------------------------------------
# fused blocks
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('n,cin,p,h,w,sep', [(1, 512, 128, 5, 9, False), (1, 1024, 256, 15, 29, False), (1, 64, 64, 13, 15, True)])
def test_bottleneck_fused_fm(cuda, n, cin, p, h, w, sep, dt):
    """cvpce_bottleneck_fused_fm*: a map smaller than the 14 x 14 tile, one pixel past a tile edge both ways, and the projection-shortcut
    form with the residual in a tensor of its own.  Bounds: tests/test_gpu_kernels.py test_bottleneck_fused_parity."""
    from cvpce_amd import ops
    T = torch.ops.cvpce_amd
    rd = lambda t: t.to(dt).to(F32)
    g = seeded('bneck', n, cin, p, h, w)
    x = rd(torch.randn(n, cin, h, w, generator=g))
    mk = lambda co, ci, k: (torch.randn(co, ci, k, k, generator=g) / math.sqrt(ci * k * k), torch.randn(co, generator=g) * 0.1)
    (w1, b1), (w2, b2), (w3, b3) = mk(p, cin, 1), mk(p, p, 3), mk(4 * p, p, 1)
    res = rd(torch.randn(n, 4 * p, h, w, generator=g)) if sep else x
    pcs = [ops.PackedConv(w_, b_, 1, pad, device=cuda, dtype=dt) for (w_, b_, pad) in ((w1, b1, 0), (w2, b2, 1), (w3, b3, 0))]
    wa = [fp.put(t, cuda) for t in ops.pack_bottleneck_weights(*pcs)] + [fp.put(c.bias, cuda) for c in pcs]
    to_dev = lambda t: t.permute(0, 2, 3, 1).contiguous().to(dt)
    xin = fp.put(to_dev(x), cuda)
    rin = fp.put(to_dev(res), cuda) if sep else xin
    o = fp.out((n, h, w, 4 * p), dt, cuda)
    y, = fp.check(lambda: T.bottleneck_fused_fm(xin[0], rin[0], wa[0][0], wa[3][0], wa[1][0], wa[4][0], wa[2][0], wa[5][0], o[0], p),
                  [xin] + ([rin] if sep else []) + wa, [o])
    t1 = rd(F.relu(F.conv2d(x, rd(w1), b1)))
    t2 = rd(F.relu(F.conv2d(t1, rd(w2), b2, padding=1)))
    ref = F.relu(F.conv2d(t2, rd(w3), b3) + res)
    assert rel_err(nchw(y), ref) < (1.5e-2 if dt == BF else 3e-3)


@pytest.mark.parametrize('c', [4, 8], ids=['nhwc4', 'nhwc8'])
@pytest.mark.parametrize('n,h,w', [(1, 16, 16), (2, 16, 32)])
def test_vgg_stem_fused(cuda, n, h, w, c):
    """cvpce_vgg_stem_fused: one 16 x 16 tile, and two tiles in each of two images; 8-byte and 16-byte input pixels."""
    from cvpce_amd import ops
    T = torch.ops.cvpce_amd
    g = seeded('vggstem', n, h, w)
    x = torch.zeros(n, h, w, c)
    x[..., :3] = torch.randn(n, h, w, 3, generator=g)
    x = x.to(BF)
    w1, b1 = torch.randn(64, 3, 3, 3, generator=g) / math.sqrt(27), torch.randn(64, generator=g) * 0.1
    w2, b2 = torch.randn(64, 64, 3, 3, generator=g) / math.sqrt(576), torch.randn(64, generator=g) * 0.1
    ps = ops.PackedStem(w1, b1, w2, b2, device=cuda)
    sa = [fp.put(t, cuda) for t in (ps.w1, ps.b1, ps.w2, ps.b2)]
    xin, o = fp.put(x, cuda), fp.out((n, h // 2, w // 2, 64), BF, cuda)
    y, = fp.check(lambda: T.vgg_stem_fused(xin[0], sa[0][0], sa[1][0], sa[2][0], sa[3][0], o[0]), [xin] + sa, [o])
    mid = F.relu(F.conv2d(x.float().permute(0, 3, 1, 2)[:, :3], w1.to(BF).float(), b1, padding=1)).to(BF).float()
    ref = F.max_pool2d(F.relu(F.conv2d(mid, w2.to(BF).float(), b2, padding=1)), 2, 2)
    assert rel_err(nchw(y), ref) < TOL16


@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('n,h,w', [(1, 1, 1), (1, 7, 9), (2, 37, 51)])
def test_gln_stem_fused(cuda, n, h, w, dt):
    """cvpce_gln_stem_fused*: one pixel, a map below one 8 x 8 pooled tile, ragged tiles both ways in two images."""
    from cvpce_amd import ops
    T = torch.ops.cvpce_amd
    g = seeded('glnstem', n, h, w)
    rd = lambda t: t.to(dt).to(F32)
    x = torch.zeros(n, h, w, 8)
    x[..., :3] = torch.randn(n, h, w, 3, generator=g)
    x = x.to(dt)
    wt = torch.randn(64, 3, 7, 7, generator=g) / math.sqrt(147)
    scale, shift = torch.rand(64, generator=g) + 0.5, torch.randn(64, generator=g) * 0.2
    ps = ops.PackedGlnStem(wt, scale, shift, device=cuda, dtype=dt)
    sa = [fp.put(ps.w_frag, cuda), fp.put(ps.bias, cuda)]
    hc, wc = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    xin, o = fp.put(x, cuda), fp.out((n, (hc - 1) // 2 + 1, (wc - 1) // 2 + 1, 64), dt, cuda)
    y, = fp.check(lambda: T.gln_stem_fused(xin[0], sa[0][0], sa[1][0], o[0]), [xin] + sa, [o])
    conv = F.relu(F.conv2d(x.float().permute(0, 3, 1, 2)[:, :3], rd(wt * scale[:, None, None, None]), shift, stride=2, padding=3))
    assert rel_err(nchw(y), F.max_pool2d(rd(conv), 3, 2, 1)) < TOL16


# ---------------------------------------------------------------------------------------------------------------------------------
# elementwise kernels and reductions
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
def test_relu(cuda, dt):
    T = torch.ops.cvpce_amd
    x = torch.randn(8 * 13, generator=seeded('relu')).to(dt)
    xin, o = fp.put(x, cuda), fp.out((8 * 13,), dt, cuda)
    y, = fp.check(lambda: T.relu(xin[0], o[0]), [xin], [o])
    assert torch.equal(y.cpu(), F.relu(x))


@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('k,stride,pad,h,w', [(3, 2, 1, 17, 23), (2, 2, 0, 7, 9)])
def test_maxpool2d_nhwc(cuda, k, stride, pad, h, w, dt):
    """cvpce_maxpool2d_nhwc_*: windows that hang over every border (3/2/1) and an odd map whose last row and column are dropped (2/2/0)."""
    T = torch.ops.cvpce_amd
    x = torch.randn(2, h, w, 24, generator=seeded('pool', h, w)).to(dt)
    ho, wo = (h + 2 * pad - k) // stride + 1, (w + 2 * pad - k) // stride + 1
    xin, o = fp.put(x, cuda), fp.out((2, ho, wo, 24), dt, cuda)
    y, = fp.check(lambda: T.maxpool2d_nhwc(xin[0], o[0], k, stride, pad), [xin], [o])
    assert torch.equal(nchw(y), F.max_pool2d(x.float().permute(0, 3, 1, 2), k, stride, pad))


def test_global_max_nhwc(cuda):
    """cvpce_global_max_nhwc_bf16 into columns 20..91 of a 100-column row: the other columns keep the prefill."""
    T = torch.ops.cvpce_amd
    x = torch.randn(3, 9, 11, 72, generator=seeded('gmax')).to(BF)
    xin, o = fp.put(x, cuda), fp.out((3, 100), F32, cuda)
    cols = torch.zeros(1, 100, dtype=torch.bool)
    cols[:, 20:92] = True
    y, = fp.check(lambda: T.global_max_nhwc(xin[0], o[0], 20), [xin], [o], written=cols)
    assert torch.equal(y[:, 20:92].cpu(), x.float().amax(dim=(1, 2)))


@pytest.mark.parametrize('want_bf16', [False, True])
@pytest.mark.parametrize('b,d', [(1, 1024), (3, 8), (5, 1000)])
def test_l2_normalize(cuda, b, d, want_bf16):
    T = torch.ops.cvpce_amd
    x = torch.rand(b, d, generator=seeded('l2', b, d))
    x[b // 2] = x[b // 2] * (b > 1)                          # a zero row where there is more than one
    xin, o = fp.put(x, cuda), fp.out((b, d), F32, cuda)
    ob = fp.out((b, d), BF, cuda) if want_bf16 else None
    got = fp.check(lambda: T.l2_normalize(xin[0], o[0], ob[0] if ob else None, 1e-8), [xin], [o] + ([ob] if ob else []))
    torch.testing.assert_close(got[0].cpu(), x / torch.linalg.norm(x, dim=1, keepdim=True).clamp(min=1e-8), rtol=1e-5, atol=1e-7)
    if want_bf16:
        assert torch.equal(got[1].cpu(), got[0].cpu().to(BF))


@pytest.mark.parametrize('dt,rows,d', [(BF, 5, 64), (BF, 130, 512), (F32, 3, 1000), (F32, 5, 64)], ids=lambda v: IDS.get(v, str(v)))
def test_row_norms(cuda, dt, rows, d):
    T = torch.ops.cvpce_amd
    x = torch.rand(rows, d, generator=seeded('norms', rows, d)).to(dt)
    xin, o = fp.put(x, cuda), fp.out((rows,), F32, cuda)
    y, = fp.check(lambda: T.row_norms(xin[0], o[0], 1e-8), [xin], [o])
    torch.testing.assert_close(y.cpu(), torch.linalg.norm(x.float(), dim=1).clamp(min=1e-8), rtol=1e-5, atol=1e-7)


@pytest.mark.parametrize('dt,c', [(BF, 256), (F32, 9), (H16, 8)], ids=lambda v: IDS.get(v, str(v)))
def test_atlas_copy(cuda, dt, c):
    """cvpce_atlas_copy both ways: packing writes the levels' pixels and nothing else (the gaps keep the prefill), unpacking writes
    every pixel of every level."""
    from cvpce_amd.models.proposals import GLNEngine
    T = torch.ops.cvpce_amd
    shapes = [(7, 9), (4, 5), (2, 3), (1, 2), (1, 1)]
    hc, wc, offs = GLNEngine.atlas_layout(shapes)
    oy, ox = [int(o[0]) for o in offs], [int(o[1]) for o in offs]
    g = seeded('atlas', c)
    levels = [torch.randn(2, h, w, c, generator=g).to(dt) for h, w in shapes]
    lin = [fp.put(t, cuda) for t in levels]
    atlas = fp.out((2, hc, wc, c), dt, cuda)
    m = torch.zeros(1, hc, wc, 1, dtype=torch.bool)
    for (h, w), y0, x0 in zip(shapes, oy, ox):
        m[:, y0:y0 + h, x0:x0 + w] = True
    assert 0 < int(m.sum()) < hc * wc
    a, = fp.check(lambda: T.atlas_pack([p[0] for p in lin], atlas[0], oy, ox), lin, [atlas], written=m)
    for t, (h, w), y0, x0 in zip(levels, shapes, oy, ox):
        assert torch.equal(a[:, y0:y0 + h, x0:x0 + w].cpu(), t)
    junk = torch.randn(2, hc, wc, c, generator=g).to(dt)
    ain = fp.put(junk, cuda)
    louts = [fp.out((2, h, w, c), dt, cuda) for h, w in shapes]
    back = fp.check(lambda: T.atlas_unpack(ain[0], [p[0] for p in louts], oy, ox), [ain], louts, written=[None] * len(louts))
    for t, (h, w), y0, x0 in zip(back, shapes, oy, ox):
        assert torch.equal(t.cpu(), junk[:, y0:y0 + h, x0:x0 + w])


# ---------------------------------------------------------------------------------------------------------------------------------
# input side
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('dt', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('batched', [False, True], ids=['per image', 'batch'])
def test_gln_transform(cuda, batched, dt):
    """cvpce_gln_transform* / _batch*: a 37 x 53 image enlarged to 44 x 63 and a 64 x 40 image kept, into one (2, 64, 64, 8) batch: the
    whole batch is written, zeros beyond each image's resized size and in channels 3..7 (tests/test_gpu_kernels.py test_transform_parity)."""
    from cvpce_amd.models import proposals as P
    T = torch.ops.cvpce_amd
    g = seeded('transform')
    imgs = [torch.rand(3, 37, 53, generator=g), torch.rand(3, 64, 40, generator=g)]
    sizes = [(44, 63), (64, 40)]
    iin = [fp.put(t, cuda) for t in imgs]
    batch = fp.out((2, 64, 64, 8), dt, cuda)
    mean, std = [float(v) for v in P.IMAGE_MEAN], [float(v) for v in P.IMAGE_STD]

    def run():
        if batched:
            T.gln_transform_batch([p[0] for p in iin], batch[0], [s[0] for s in sizes], [s[1] for s in sizes], mean, std)
        else:
            for i, (h, w) in enumerate(sizes):
                T.gln_transform(iin[i][0], batch[0], i, h, w, mean, std)
    y, = fp.check(run, iin, [batch])
    y = y.float().cpu()
    for i, (img, (h, w)) in enumerate(zip(imgs, sizes)):
        nrm = (img - torch.tensor(mean)[:, None, None]) / torch.tensor(std)[:, None, None]
        ref = F.interpolate(nrm[None], size=(h, w), mode='bilinear', align_corners=False)[0]
        assert (y[i, ..., 3:] == 0).all() and (y[i, h:] == 0).all() and (y[i, :, w:] == 0).all()
        assert (y[i, :h, :w, :3].permute(2, 0, 1) - ref).abs().max() < 2e-2          # one bf16 ulp at |x| <= 2.7 is 1.6e-2


def _crop_reference(img, boxes, size):
    """production.py:20 + datautils.py:232-239: truncate the box, slice (clamped), pad to a square with 0.5, bilinear resize"""
    out = []
    for x1, y1, x2, y2 in boxes.to(torch.long).tolist():
        crop = img[:, y1:y2, x1:x2]
        larger = max(crop.shape[1], crop.shape[2])
        sq = torch.full((3, larger, larger), 0.5)
        sq[:, :crop.shape[1], :crop.shape[2]] = crop
        out.append(F.interpolate(sq[None], size=(size, size), mode='bilinear', align_corners=False)[0])
    return torch.stack(out)


CROP_BOXES = [[0., 0., 40., 30.],          # the whole image
              [25.3, 18.9, 40., 30.],      # right and bottom edges exactly W and H
              [30.2, 20.7, 50., 45.],      # extends past both
              [5., 6., 6.9, 7.2]]          # 1 x 1 pixel


@pytest.mark.parametrize('limited', [False, True], ids=['all boxes', 'count 3'])
@pytest.mark.parametrize('mode', [0, 1, 2])
def test_crop_resize(cuda, mode, limited):
    """cvpce_crop_resize from a 30 x 40 image in an arena, S = 16: bilinear taps at x = W - 1 / y = H - 1 and boxes that reach or pass
    the border must not read beyond the image; with a device-side count below the box count the rows >= count keep the prefill."""
    from cvpce_amd.models.classification import TANH_MEAN, TANH_STD
    T = torch.ops.cvpce_amd
    S = 16
    img = torch.rand(3, 30, 40, generator=seeded('crop'))
    boxes = torch.tensor(CROP_BOXES)
    iin, bin_ = fp.put(img, cuda), fp.put(boxes, cuda)
    cnt = fp.put(torch.tensor([3], dtype=torch.int32), cuda) if limited else None
    shape, dt = ((4, 3, S, S), F32) if mode == 0 else ((4, S, S, 8 if mode == 1 else 4), BF)
    o = fp.out(shape, dt, cuda)
    rows = torch.arange(4).view(4, 1, 1, 1) < (3 if limited else 4)
    mean, std = (list(TANH_MEAN), list(TANH_STD)) if mode else (None, None)
    y, = fp.check(lambda: T.crop_resize(iin[0], bin_[0], cnt[0] if cnt else None, o[0], S, mode, mean, std), [iin, bin_, cnt], [o], written=rows)
    v = 3 if limited else 4
    ref = _crop_reference(img, boxes, S)[:v]
    if mode == 0:
        torch.testing.assert_close(y[:v].cpu(), ref, rtol=0, atol=2e-6)
    else:
        refp = ((ref * 2 - 1 - torch.tensor(TANH_MEAN)[None, :, None, None]) / torch.tensor(TANH_STD)[None, :, None, None]).permute(0, 2, 3, 1)
        got = y[:v].float().cpu()
        assert (got[..., 3:] == 0).all() and (got[..., :3] - refp).abs().max() < 2e-2


@pytest.mark.parametrize('mode', [1, 2])
def test_crop_extents_and_content(cuda, mode):
    """cvpce_crop_extents (with a count: the slots beyond it get the full extent) and cvpce_crop_resize_content: only the content
    inside the extents is written (a thread writes two pixels: a row may run one pixel past an odd column extent), slots beyond the
    count not at all."""
    from cvpce_amd.models.classification import TANH_MEAN, TANH_STD
    T = torch.ops.cvpce_amd
    S = 16
    img = torch.rand(3, 30, 40, generator=seeded('crop'))
    boxes = torch.tensor(CROP_BOXES + [[3., 4., 33., 9.], [7., 2., 12., 28.]])       # + a wide and a tall box: padding below / right
    iin, bin_ = fp.put(img, cuda), fp.put(boxes, cuda)
    cnt = fp.put(torch.tensor([5], dtype=torch.int32), cuda)
    ext = fp.out((6, 2), torch.int32, cuda)
    e, = fp.check(lambda: T.crop_extents(bin_[0], cnt[0], 0, 30, 40, S, ext[0]), [bin_, cnt], [ext])
    e = e.cpu()
    ref = _crop_reference(img, boxes, S)
    const = (ref == 0.5).all(dim=1)                                                       # (6, S, S)
    for p in range(5):
        ey, ex = e[p].tolist()
        assert bool(const[p, ey:].all()) and bool(const[p, :, ex:].all()), (p, ey, ex)    # beyond the extents: exactly the pad constant
    assert e[4].tolist()[0] < S and e[5].tolist() == [S, S] and e[0].tolist() == [12, 16]
    ein = fp.put(e, cuda)
    o = fp.out((6, S, S, 8 if mode == 1 else 4), BF, cuda)
    yy, xx = torch.arange(S).view(1, S, 1, 1), torch.arange(S).view(1, 1, S, 1)
    ey, ex = e[:, 0].view(-1, 1, 1, 1), e[:, 1].view(-1, 1, 1, 1)
    slot = torch.arange(6).view(6, 1, 1, 1) < 5
    must, may = slot & (yy < ey) & (xx < ex), slot & (yy < ey) & (xx < ex + (ex & 1))
    y, = fp.check(lambda: T.crop_resize_content(iin[0], bin_[0], cnt[0], o[0], S, mode, list(TANH_MEAN), list(TANH_STD), ein[0]),
                  [iin, bin_, cnt, ein], [o], written=(must, may))
    refp = ((ref * 2 - 1 - torch.tensor(TANH_MEAN)[None, :, None, None]) / torch.tensor(TANH_STD)[None, :, None, None]).permute(0, 2, 3, 1)
    sel = must.expand(6, S, S, 3)
    assert (y.float().cpu()[..., :3][sel] - refp[sel]).abs().max() < 2e-2


def test_pad_extents_and_pack_embed_input(cuda):
    """cvpce_pad_extents reads (B,3,S,S) crops to their last pixel; cvpce_pack_embed_input writes every channel of every pixel."""
    from cvpce_amd.models.classification import TANH_MEAN, TANH_STD
    T = torch.ops.cvpce_amd
    S = 16
    img = torch.rand(3, 30, 40, generator=seeded('crop'))
    crops = torch.cat((_crop_reference(img, torch.tensor(CROP_BOXES + [[3., 4., 33., 9.], [7., 2., 12., 28.]]), S),
                       torch.rand(1, 3, S, S, generator=seeded('noise'))))
    cin_ = fp.put(crops, cuda)
    ext = fp.out((7, 2), torch.int32, cuda)
    e, = fp.check(lambda: T.pad_extents(cin_[0], 0.5, ext[0]), [cin_], [ext])
    const = (crops == 0.5).all(dim=1)
    for p, (ey, ex) in enumerate(e.cpu().tolist()):
        assert bool(const[p, ey:].all()) and bool(const[p, :, ex:].all())
    assert e[6].tolist() == [S, S] and e[4].tolist()[0] < S and e[5].tolist()[1] < S
    o = fp.out((7, S, S, 8), BF, cuda)
    y, = fp.check(lambda: T.pack_embed_input(cin_[0], o[0], 1, list(TANH_MEAN), list(TANH_STD)), [cin_], [o])
    refp = ((crops * 2 - 1 - torch.tensor(TANH_MEAN)[None, :, None, None]) / torch.tensor(TANH_STD)[None, :, None, None]).permute(0, 2, 3, 1)
    got = y.float().cpu()
    assert (got[..., 3:] == 0).all() and torch.equal(got[..., :3], refp.to(BF).float())


# ---------------------------------------------------------------------------------------------------------------------------------
# detector post-processing
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thresh', [0.05, 0.999999], ids=['candidates', 'no candidates'])
def test_detect_postprocess(cuda, thresh):
    """cvpce_detect_postprocess on five tiny levels (7x9 .. 1x1, 9 anchors, two images, top-k above every level's candidate count),
    every logits and regression tensor in an arena of its own, the outputs views of one block as ops.detect_postprocess lays them
    out.  That wrapper hands the kernels a ZERO-FILLED block ("the five zero-padded outputs"): rows beyond an image's detection count are
    the caller's zeros, so here, without the fill, they must keep the prefill; the rows below the count and both counts are written."""
    from cvpce_amd._lib import lib
    from cvpce_amd.models import proposals as P
    from oracle import gln as og
    T = torch.ops.cvpce_amd
    n, a, dpi, topk = 2, 9, 1000, og.TOPK_CANDIDATES
    padded = (56, 72)
    grids = [(7, 9), (4, 5), (2, 3), (1, 2), (1, 1)]
    g = seeded('detect')
    cls = [torch.randn(n, gh * gw * a, generator=g) * 2.0 - 1.0 for gh, gw in grids]
    reg = [torch.randn(n, gh * gw * a, 4, generator=g) * 0.5 for gh, gw in grids]
    resized, original = [(56, 70), (50, 72)], [(112, 140), (100, 144)]
    anchors = og.grid_anchors(padded, grids)
    strides = [(padded[0] // gh, padded[1] // gw) for gh, gw in grids]
    ratios = torch.stack([torch.tensor(o, dtype=F32) / torch.tensor(r, dtype=F32) for o, r in zip(original, resized)])
    cin_, rin = [fp.put(t, cuda) for t in cls], [fp.put(t, cuda) for t in reg]
    base, hw, rat = fp.put(P._base_anchors(), cuda), fp.put(torch.tensor(resized, dtype=torch.int32), cuda), fp.put(ratios, cuda)
    ws = fp.out((int(lib.cvpce_detect_workspace_bytes(n, len(grids), topk)),), torch.uint8, cuda)
    nd = n * dpi
    block = fp.out((nd * 7 + n * 2,), torch.int32, cuda)             # labels i64 | boxes f32 x 4 | scores f32 | count i32 | conf i32, in 4-byte words
    b = block[0]
    labels, boxes = b[:nd * 2].view(torch.int64).view(n, dpi), b[nd * 2:nd * 6].view(F32).view(n, dpi, 4)
    scores, count, conf = b[nd * 6:nd * 7].view(F32).view(n, dpi), b[nd * 7:nd * 7 + n], b[nd * 7 + n:]

    def run():
        T.detect_postprocess([p[0] for p in cin_], [p[0] for p in rin], [g_[0] for g_ in grids], [g_[1] for g_ in grids], [s[0] for s in strides],
                             [s[1] for s in strides], base[0], hw[0], rat[0], a, 1, topk, float(thresh), float(og.NMS_THRESH), float(og.BBOX_XFORM_CLIP),
                             dpi, 0.5, ws[0], boxes, scores, labels, count, conf)
    want = []
    for i in range(n):
        bx, sc, lb = og.postprocess_image([c[i].view(-1, 1) for c in cls], [r[i] for r in reg], anchors, resized[i], dpi, score_thresh=thresh)
        want.append((og.resize_boxes(bx, resized[i], original[i]), sc, lb))
    counts = [len(w[0]) for w in want]
    assert (counts == [0, 0]) if thresh > 0.5 else (0 < min(counts) and max(counts) < dpi), counts
    row = torch.arange(dpi)[None, :] < torch.tensor(counts)[:, None]                               # (n, dpi): rows below the count
    wm = torch.cat((row.repeat_interleave(2, dim=1).reshape(-1), row.repeat_interleave(4, dim=1).reshape(-1), row.reshape(-1),
                    torch.ones(2 * n, dtype=torch.bool)))
    got, _ = fp.check(run, cin_ + rin + [base, hw, rat], [block, ws], written=[wm, fp.SCRATCH])
    got = got.cpu()
    glabels, gboxes = got[:nd * 2].view(torch.int64).view(n, dpi), got[nd * 2:nd * 6].view(F32).view(n, dpi, 4)
    gscores, gcount, gconf = got[nd * 6:nd * 7].view(F32).view(n, dpi), got[nd * 7:nd * 7 + n], got[nd * 7 + n:]
    for i, (bx, sc, lb) in enumerate(want):
        c = int(gcount[i])
        assert c == len(bx), (c, len(bx))
        torch.testing.assert_close(gscores[i, :c], sc, rtol=0, atol=1e-6)
        torch.testing.assert_close(gboxes[i, :c], bx, rtol=1e-5, atol=2e-3)
        assert torch.equal(glabels[i, :c], lb) and int(gconf[i]) == int((sc > 0.5).sum())


# ---------------------------------------------------------------------------------------------------------------------------------
# matching
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['f32', 'bf16 core 1', 'bf16 core 2'])
@pytest.mark.parametrize('qn,gn,d,k', [(5, 40, 64, 1), (130, 129, 512, 3), (5, 40, 64, 40)])
def test_match_topk(cuda, qn, gn, d, k, variant):
    """cvpce_match_topk: fewer rows than one tile, one row past a 128-row tile in both operands, and k > 16 (the large-k path, here a
    full ranking), on both bf16 cores and the f32 path; the workspace is an arena of exactly cvpce_match_workspace_bytes."""
    from cvpce_amd import ops
    from cvpce_amd._lib import lib
    from oracle import match as omatch
    T = torch.ops.cvpce_amd
    dt = F32 if variant == 'f32' else BF
    g = seeded('match', qn, gn)
    G = F.normalize(torch.rand(gn, d, generator=g), dim=1).to(dt)
    Q = F.normalize(torch.rand(qn, d, generator=g), dim=1).to(dt)
    qin, gin = fp.put(Q, cuda), fp.put(G, cuda)
    qn_, gn_ = fp.put(ops.row_norms(Q.to(cuda)), cuda), fp.put(ops.row_norms(G.to(cuda)), cuda)
    ws = fp.out((int(lib.cvpce_match_workspace_bytes(qn, gn, k)),), torch.uint8, cuda)
    idx, dist = fp.out((qn, k), torch.int64, cuda), fp.out((qn, k), F32, cuda)
    assert ops.match_set_core(int(variant[-1]) if dt == BF else 0, 0, 0) == 0
    try:
        gi, gd, _ = fp.check(lambda: T.match_topk(qin[0], gin[0], qn_[0], gn_[0], k, ws[0], idx[0], dist[0]), [qin, gin, qn_, gn_], [idx, dist, ws],
                             written=[None, None, fp.SCRATCH])
    finally:
        ops.match_set_core(0, 0, 0)
    gi, gd = gi.cpu(), gd.cpu()
    ref_d = omatch.cosine_distance_matrix(G.float(), Q.float())
    ref_idx = torch.sort(ref_d, dim=-1, stable=True).indices[:, :k]
    srt = ref_d.sort(dim=-1).values[:, :min(k + 1, gn)]
    safe = (srt[:, 1:] - srt[:, :-1]).min(dim=1).values > 2e-6 if srt.shape[1] > 1 else torch.ones(qn, dtype=torch.bool)
    assert int(gi.min()) >= 0 and int(gi.max()) < gn and gi[safe].equal(ref_idx[safe])
    torch.testing.assert_close(gd, ref_d.gather(1, gi), rtol=0, atol=2e-6)


@pytest.mark.parametrize('k', [3, 16])
def test_eval_match_detections(cuda, k):
    """cvpce_eval_match_detections (what device_metrics.match_detections launches) on two images -- 65 targets x 1 prediction and
    3 targets x 130 predictions -- at K thresholds: `first` is written for every target; of `tp`, which the caller zero-fills, only the
    true positives are written (include/cvpce_amd_eval.h), every other byte keeps the prefill."""
    import device_metrics_cases as cases          # tests/device_metrics_cases.py
    from cvpce_amd import device_metrics  # noqa: F401  (registers the op)
    g = seeded('evalmatch')

    def rand_boxes(m):
        xy = torch.rand(m, 2, generator=g) * 20
        return torch.cat((xy, xy + 2 + torch.rand(m, 2, generator=g) * 6), dim=1)
    tgts = [rand_boxes(65), rand_boxes(3)]
    preds = [tgts[0][7:8] + 0.3, torch.cat([tgts[1] + 0.2 * torch.randn(3, 4, generator=g) for _ in range(43)] + [rand_boxes(1)])]
    confs = [torch.rand(len(p), generator=g) for p in preds]
    thr = torch.linspace(0.3, 0.9, k)
    n_p, n_t = [len(p) for p in preds], [len(t) for t in tgts]
    assert n_p == [1, 130]
    flags, firsts, rank = [], [], []
    for t, p, c in zip(tgts, preds, confs):
        fl, fi, _, order = cases.closed_form(t, p, c, [float(v) for v in thr])
        r = torch.empty(len(p), dtype=torch.int32)
        r[order] = torch.arange(len(p), dtype=torch.int32)
        flags.append(fl); firsts.append(fi); rank.append(r)
    off = lambda v: torch.tensor([0, v[0], v[0] + v[1]], dtype=torch.int32)
    ins = [fp.put(t, cuda) for t in (torch.cat(preds), off(n_p), torch.cat(rank), torch.cat(tgts), off(n_t), thr)]
    first, tp = fp.out((k, sum(n_t)), torch.int32, cuda), fp.out((k, sum(n_p)), torch.uint8, cuda)
    want_tp = torch.cat(flags, dim=1)
    assert 0 < int(want_tp.sum()) < want_tp.numel()
    gf, gt = fp.check(lambda: torch.ops.cvpce_amd.eval_match_detections(ins[0][0], ins[1][0], ins[2][0], None, ins[3][0], ins[4][0], None, ins[5][0],
                                                                        max(n_t), first[0], tp[0]), ins, [first, tp], written=[None, want_tp == 1])
    assert torch.equal(gf.cpu().long(), torch.cat(firsts, dim=1))
    assert bool((gt.cpu()[want_tp == 1] == 1).all())


# ---------------------------------------------------------------------------------------------------------------------------------
# ops.conv2d(out=...)
# ---------------------------------------------------------------------------------------------------------------------------------
def test_conv2d_out_is_checked(cuda):
    """ops.conv2d refuses an `out` of the wrong shape, type or layout instead of handing its pointer to a kernel."""
    from cvpce_amd import ops
    pc = ops.PackedConv(torch.randn(64, 64, 3, 3), None, 1, 1, device=cuda)
    x = torch.zeros(1, 8, 8, 64, dtype=BF, device=cuda)
    for bad in (torch.empty(1, 8, 8, 32, dtype=BF, device=cuda), torch.empty(1, 8, 8, 64, dtype=H16, device=cuda),
                torch.empty(1, 8, 8, 64, dtype=F32, device=cuda), torch.empty(1, 8, 8, 128, dtype=BF, device=cuda)[..., ::2],
                torch.empty(1, 4, 4, 64, dtype=BF, device=cuda)):
        with pytest.raises(AssertionError):
            ops.conv2d(x, pc, out=bad)
    assert ops.conv2d(x, pc, pool=True, out=torch.empty(1, 4, 4, 64, dtype=BF, device=cuda)).shape == (1, 4, 4, 64)
    assert ops.conv2d(x, pc, out_f32=True, out=torch.empty(1, 8, 8, 64, dtype=F32, device=cuda)).dtype == F32
