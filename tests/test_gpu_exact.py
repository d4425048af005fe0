"""Equality, kernel by kernel: every convolution kernel on the exactly representable operands of tests/exact_cases.py against the float64
reference with one round-to-nearest-even at each place the kernel stores a 16-bit value.

On these operands every partial sum is exact in fp32 in any order (tests/test_exact_cases_cpu.py shows it for every case on the host), so
a kernel that drops or repeats one K element, loses or doubles a split-K partial, truncates instead of rounding, rounds twice, or rounds
an intermediate layer at another place than the per-layer schedule it replaces gives another result -- and none of it hides inside a
tolerance.  Comparisons are torch.equal on the widened values (a sum of negative zeros may come out with either sign).  Each test shows
through ops.conv_route / ops.PROFILE which kernel ran.  The first two tests are the anchor: a pointwise 64 -> 64 conv with fp32 output
through one kernel on v_mfma_f32_32x32x16 (the register-staged implicit GEMM, 8 x 8 map) and one on v_mfma_f32_16x16x32 (the thin-output
form of the wide halo kernel: it only runs 3 x 3 layers on maps of 48 x 48 and more, so the conv is a 3 x 3 whose off-centre taps are
zero, on a 48 x 48 map) -- if the matrix units rounded sums of exactly representable values, these two would show it before any other test.

The families' edge cases (exact_cases.EDGE_IDS: `_big`, `_subw`, `_subx`, `_sub`) run in the same family tests, on the same routes: fp16
stores that saturate at +-65504 where bf16 and fp32 stores keep the value, and fp16 subnormal weights, activations, residuals and stored
values -- a kernel that forgot a clamp on an intermediate store, clamped a bf16 store, flushed a subnormal or cut it instead of rounding
differs from the reference (tests/test_exact_cases_cpu.py test_edge_mutants_differ shows it for every case on the host).
"""
import contextlib

import pytest
import torch

import exact_cases as ec            # tests/exact_cases.py
import footprint as fp              # tests/footprint.py

pytestmark = pytest.mark.gpu

BF, H16, F32 = torch.bfloat16, torch.float16, torch.float32


def to_nhwc(t, dt, cpad=8):
    """(N,C,H,W) float64 on a grid the type holds -> NHWC of the storage type, C padded with zeros to a multiple of cpad"""
    n, c, h, w = t.shape
    cp = (c + cpad - 1) // cpad * cpad
    out = torch.zeros(n, h, w, cp, dtype=dt)
    out[..., :c] = t.permute(0, 2, 3, 1).to(dt)
    assert torch.equal(out[..., :c].double(), t.permute(0, 2, 3, 1))
    return out


def widen(y, keep=None):
    """NHWC device tensor -> (keep last images,C,H,W) float64 on the host"""
    y = y.double().permute(0, 3, 1, 2).cpu()
    return y if keep is None else y[y.shape[0] - keep:]


def same(got, ref, what=''):
    """torch.equal with the differing element in the message: (image, channel, row, column), both values, how many differ"""
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    if torch.equal(got, ref):
        return
    bad = (got != ref) | (got.isnan() != ref.isnan())
    first = bad.nonzero()[0].tolist()
    raise AssertionError(f'{what}: {int(bad.sum())} of {bad.numel()} values differ, first at (n, c, y, x) = {first}: kernel {got[tuple(first)].item()!r}, '
                         f'reference {ref[tuple(first)].item()!r}; largest difference {float((got - ref)[bad].abs().max())!r}')


@contextlib.contextmanager
def switches(**kw):
    """ops switches for one block, a fresh ConvProfile in ops.PROFILE; restored afterwards"""
    from cvpce_amd import ops
    saved = {k: getattr(ops, k) for k in kw}
    saved['PROFILE'] = ops.PROFILE
    for k, v in kw.items():
        setattr(ops, k, v)
    ops.PROFILE = ops.ConvProfile()
    try:
        yield ops.PROFILE
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)


def packed(L, dt, cuda):
    from cvpce_amd import ops
    return ops.PackedConv(L.w.float(), L.b.float() if L.b is not None else None, L.stride, L.pad, device=cuda, dtype=dt)


def launch_conv(cuda, c, **sw):
    """the single-layer case c through ops.conv2d under the switches sw -> (output, route, kernel record, layer record)"""
    from cvpce_amd import ops
    L = c.layers[0]
    pc = packed(L, c.dt, cuda)
    x = to_nhwc(c.x, c.dt).to(cuda)
    r = to_nhwc(L.res, c.dt).to(cuda) if L.res is not None else None
    n, h, w, _ = x.shape
    with switches(**sw) as prof:
        route, _ = ops.conv_route(pc, n, h, w, L.act, L.f32, r is not None, L.in_up, bool(L.pool))
        y = ops.conv2d(x, pc, act=L.act, out_f32=L.f32, residual=r, in_up_shift=L.in_up, pool=bool(L.pool))
        rec, layer = prof.records[-1][0], prof.layer_records[-1][0]
    torch.cuda.synchronize()
    assert y.dtype == (F32 if L.f32 else c.dt)
    return y, route, rec, layer


# family -> (the ops switches its single-layer cases run under, what (case, route, kernel record, layer record) must satisfy)
SINGLE = {
    'igemm': (dict(FORCE_GENERIC_CONV=True), lambda c, route, rec, layer: route == 'igemm' and rec.startswith('conv_igemm_kernel')),
    'dma': (dict(USE_HALO_3X3=False, USE_CONV1X1=False), lambda c, route, rec, layer: route == 'igemm' and rec.startswith('conv_dma')),
    'splitk': ({}, lambda c, route, rec, layer: route == 'splitk' and 'split-K 4' in layer and rec.startswith('conv_igemm_kernel<128')),
    'conv1x1': (dict(CONV1X1_ANY_SHAPE=True), lambda c, route, rec, layer: route == 'conv1x1' and rec == 'conv1x1_kernel'),
    'halo': (dict(HALO_RAGGED=True), lambda c, route, rec, layer: route == 'halo' and rec == ('conv3x3_halo3_kernel' if c.layers[0].w.shape[0] <= 128 else 'conv3x3_halo2_kernel')),
    'thin_out': ({}, lambda c, route, rec, layer: route == 'halo_thin_out' and layer.startswith('conv3x3_halo3 thin out')),
    'thin3x3': ({}, lambda c, route, rec, layer: route == 'thin3x3' and rec == 'thin3x3_kernel'),
}


def run_single(cuda, c):
    """a single-layer case through ops.conv2d under its family's switches, on the route and kernel the family is about -> output"""
    sw, intended = SINGLE[c.family]
    y, route, rec, layer = launch_conv(cuda, c, **sw)
    assert intended(c, route, rec, layer), (c.id, route, rec, layer)
    return y, rec


@pytest.fixture(scope='module')
def refs():
    """float64 references, computed once per case and shared by the tests that need them; never modified"""
    cache = {}

    def get(cid):
        if cid not in cache:
            c = ec.case(cid)
            cache[cid] = (c, c.reference()[0])
        return cache[cid]
    return get


# ---------------------------------------------------------------------------------------------------------------------------------
# the anchor
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', [f'anchor/pointwise_8x8/{t}' for t in ('bf16', 'fp16')], ids=lambda s: s.split('/')[-1])
def test_anchor_mfma32(cuda, refs, cid):
    """pointwise 64 -> 64, 8 x 8 map, fp32 out through conv_igemm_kernel (E::mfma32, csrc/conv_igemm.hip mma step): 64 exact products per
    output, no store rounding at all"""
    c, ref = refs(cid)
    y, route, rec, _ = launch_conv(cuda, c, FORCE_GENERIC_CONV=True)
    assert route == 'igemm' and rec.startswith('conv_igemm_kernel'), (route, rec)
    same(widen(y), ref, cid)


@pytest.mark.parametrize('cid', [f'anchor/centre_tap_48x48/{t}' for t in ('bf16', 'fp16')], ids=lambda s: s.split('/')[-1])
def test_anchor_mfma16(cuda, refs, cid):
    """the same pointwise conv as the centre tap of a 3 x 3 layer on a 48 x 48 map, fp32 out through the thin-output form of
    conv3x3_halo3_kernel (E::mfma16, csrc/conv3x3_halo3.hip): no other kernel on the 16 x 16 x 32 instruction has an fp32 output"""
    c, ref = refs(cid)
    y, route, rec, layer = launch_conv(cuda, c)
    assert route == 'halo_thin_out' and rec == 'conv3x3_halo3_kernel' and layer.startswith('conv3x3_halo3 thin out'), (route, rec, layer)
    same(widen(y), ref, cid)


# ---------------------------------------------------------------------------------------------------------------------------------
# single layers through ops.conv2d
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('cid', ec.ids('igemm'))
def test_igemm_generic(cuda, refs, cid):
    """the register-staged implicit GEMM (every tile shape, K-step 32 and 64, stride 2, 7 x 7, residual same-size and upsampled, upsampled
    input, fp32 out, fused pool)"""
    c, ref = refs(cid)
    same(widen(run_single(cuda, c)[0], c.keep), ref, cid)


@pytest.mark.parametrize('cid', ec.ids('dma'))
def test_lds_dma_ring(cuda, refs, cid):
    """the LDS-DMA ring kernels (256 x 256, 128 x 128 and 64 x 128 tiles); the whole batch runs (they need 128 pixel tiles), the last image is compared.
    dma_in_up: the 2-buffer 256 x 256 kernel, which takes the ring kernel's shapes on an upsampled input (its padding test runs on
    upsampled coordinates) -- no model has such a layer, so this is the only launch of that instance"""
    c, ref = refs(cid)
    y, rec = run_single(cuda, c)
    if c.name == 'dma_in_up':
        assert rec == 'conv_dma_kernel<256,256,2,4,2>', rec
    same(widen(y, c.keep), ref, cid)


@pytest.mark.parametrize('cid', ec.ids('splitk'))
def test_splitk(cuda, refs, cid):
    """split-K launches: a partial sum lost or added twice in one tile moves that tile by whole quanta; 16-bit and fp32 out, with and
    without a residual"""
    c, ref = refs(cid)
    same(widen(run_single(cuda, c)[0], c.keep), ref, cid)


@pytest.mark.parametrize('cid', ec.ids('conv1x1'))
def test_conv1x1(cuda, refs, cid):
    """the pointwise GEMM kernel: stride 2, both residual modes, K from 64 (one stage) to 2048, weights in registers and in LDS"""
    c, ref = refs(cid)
    same(widen(run_single(cuda, c)[0], c.keep), ref, cid)


@pytest.mark.parametrize('cid', ec.ids('halo'))
def test_halo(cuda, refs, cid):
    """the halo-patch kernels (16 x 16 tiles above 128 couts, 16 x 32 below): ragged tiles, ragged cout tiles (136, 264), the fused pool;
    and, both being exact, equal to the implicit-GEMM kernel on the same inputs"""
    c, ref = refs(cid)
    y, _ = run_single(cuda, c)
    same(widen(y, c.keep), ref, cid)
    y2, route2, rec2, _ = launch_conv(cuda, c, USE_HALO_3X3=False)
    assert route2 != 'halo' and not rec2.startswith('conv3x3_halo'), (route2, rec2)
    same(widen(y), widen(y2), cid + ' against ' + rec2)


@pytest.mark.parametrize('cid', ec.ids('thin_out'))
def test_halo_thin_out(cuda, refs, cid):
    """the thin-output form of the wide halo kernel: Cout 1, 9, 36, fp32 out, no activation, 48 x 48 and a ragged 50 x 77"""
    c, ref = refs(cid)
    same(widen(run_single(cuda, c)[0], c.keep), ref, cid)


@pytest.mark.parametrize('cid', ec.ids('thin3x3'))
def test_thin3x3(cuda, refs, cid):
    """the thin 3 x 3 kernel (32 -> 16 | 32, and 64 -> 32 over the 2x upsampled input), with and without ReLU"""
    c, ref = refs(cid)
    same(widen(run_single(cuda, c)[0], c.keep), ref, cid)


def run_mac(cuda, c):
    """-> (the stored map or None, the descriptor rows with the layer's maxima from column 40)"""
    from cvpce_amd import ops
    L = c.layers[0]
    pool, store = '_pool' in c.name, '_nostore' not in c.name
    n, cout = c.x.shape[0], L.w.shape[0]
    pc = packed(L, BF, cuda)
    x = to_nhwc(c.x, BF).to(cuda)
    mac = torch.zeros(n, 40 + cout, device=cuda)
    with switches(HALO_RAGGED=True) as prof:
        got = ops.conv2d_relu_mac(x, pc, mac, 40, store=store, pool=pool)
        assert prof.records[-1][0] == 'conv3x3_halo2_kernel'
    torch.cuda.synchronize()
    return got, mac


@pytest.mark.parametrize('cid', ec.ids('mac'))
def test_conv2d_relu_mac(cuda, refs, cid):
    """conv + ReLU with the MAC descriptor taken in the epilogue (stored, stored pooled, not stored): the descriptor is the maximum of
    what the unfused schedule would have stored -- the 16-bit values (rounding is monotone, so also the rounded maximum of the sums)"""
    c, ref = refs(cid)
    pool, store = '_pool' in c.name, '_nostore' not in c.name
    got, mac = run_mac(cuda, c)
    assert float(mac[:, :40].abs().max()) == 0.0
    assert torch.equal(mac[:, 40:].double().cpu(), ref.amax(dim=(-2, -1))), cid
    if not store:
        assert got is None
    else:
        same(widen(got), torch.nn.functional.max_pool2d(ref, 2, 2) if pool else ref, cid)


@pytest.mark.parametrize('dt', ec.DTYPES, ids=ec.IDS.get)
@pytest.mark.parametrize('use_map', [False, True], ids=['mask', 'mask+tile map'])
def test_atlas_masked(cuda, refs, use_map, dt):
    """the masked atlas conv on two maps packed with a one-pixel zero gap (tests/test_gpu_kernels.py test_conv3x3_atlas_masked, n = 3):
    level pixels equal the conv of each map alone, gap pixels of computed tiles are exact zeros"""
    check_atlas(cuda, refs, use_map, dt, '')


def check_atlas(cuda, refs, use_map, dt, suffix):
    """test_atlas_masked on the case atlas/a<suffix>: map b takes a's layer, and its x on a's grid"""
    from cvpce_amd import ops
    ca, ra = refs(f'atlas/a{suffix}/{ec.IDS[dt]}')
    cb, rb = refs(f'atlas/b/{ec.IDS[dt]}')
    cb = cb.with_(x=cb.x * (ca.xq / cb.xq), layers=ca.layers)        # one layer over both maps
    rb = cb.reference()[0]
    n = 3
    pc = packed(ca.layers[0], dt, cuda)
    atlas = torch.zeros(n, 21, 61, 128, dtype=dt)                    # columns 45..60: a tile column that lies wholly in the gap
    atlas[:, :, :30] = to_nhwc(ca.x, dt)
    atlas[:, 5:14, 31:45] = to_nhwc(cb.x, dt)
    mask = torch.zeros(21, 61, dtype=torch.uint8)
    mask[:, :30] = 1
    mask[5:14, 31:45] = 1
    with switches() as prof:
        if use_map:
            tile_map = ops.atlas_tile_map(mask.to(cuda))
            assert tile_map.numel() == 5
            out = torch.zeros(n, 21, 61, 256, dtype=dt, device=cuda)
            y = ops.conv3x3_atlas(atlas.to(cuda), pc, mask.to(cuda), act=1, tile_map=tile_map, out=out)
        else:
            y = ops.conv3x3_atlas(atlas.to(cuda), pc, mask.to(cuda), act=1)
        assert prof.records[-1][0] == 'conv3x3_halo2_kernel'
    torch.cuda.synchronize()
    same(widen(y[:, :, :30]), ra, 'level a')
    same(widen(y[:, 5:14, 31:45]), rb, 'level b')
    computed = torch.ones(21, 61, dtype=torch.bool)
    if use_map:
        computed[:] = False
        for t in tile_map.tolist():
            computed[(t >> 16) * 16:(t >> 16) * 16 + 16, (t & 0xFFFF) * 16:(t & 0xFFFF) * 16 + 16] = True
    gap = (computed & (mask == 0))[None, :, :, None].expand(n, 21, 61, 256)
    assert int(gap.sum()) > 0 and float(y.cpu().double()[gap].abs().max()) == 0.0
    return y[:, :, :30]


ATLAS_EDGES = [c.split('/')[1][1:] + '/' + c.split('/')[2] for c in ec.ids('atlas') if c in ec.EDGE_IDS]


@pytest.mark.parametrize('edge', ATLAS_EDGES)
@pytest.mark.parametrize('use_map', [False, True], ids=['mask', 'mask+tile map'])
def test_atlas_masked_edges(cuda, refs, use_map, edge):
    """test_atlas_masked on the edge cases of map a (saturated stores in both types, subnormal weights, subnormal activations)"""
    suffix, dt = edge.split('/')
    check_atlas(cuda, refs, use_map, {v: k for k, v in ec.IDS.items()}[dt], suffix)


# ---------------------------------------------------------------------------------------------------------------------------------
# fused chains: one rounding at each place the per-layer schedule stores
# ---------------------------------------------------------------------------------------------------------------------------------
def run_vgg_stem(cuda, c, cstride=4):
    from cvpce_amd import ops
    l1, l2 = c.layers
    ps = ops.PackedStem(l1.w.float(), l1.b.float(), l2.w.float(), l2.b.float(), device=cuda)
    with switches() as prof:
        y = ops.vgg_stem(to_nhwc(c.x, BF, cstride).to(cuda), ps)
        assert prof.records[-1][0] == 'vgg_stem2_kernel'
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize('cstride', [4, 8])
@pytest.mark.parametrize('cid', ec.ids('vgg_stem'))
def test_vgg_stem(cuda, refs, cid, cstride):
    """conv1_1 + ReLU + conv1_2 + ReLU + pool in one launch: conv1_1's output is rounded to bf16 before conv1_2 reads it, as the
    unfused schedule stores it (tests/test_gpu_kernels.py test_vgg_stem_fused_parity); channel strides 4 and 8"""
    c, ref = refs(cid)
    same(widen(run_vgg_stem(cuda, c, cstride)), ref, cid)


def run_gln_stem(cuda, c):
    from cvpce_amd import ops
    L = c.layers[0]
    ps = ops.PackedGlnStem(c.wt.float(), c.scale.float(), L.b.float(), device=cuda, dtype=c.dt)
    with switches() as prof:
        y = ops.gln_stem(to_nhwc(c.x, c.dt).to(cuda), ps)
        assert prof.records[-1][0] == 'gln_stem_kernel'
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize('cid', ec.ids('gln_stem'))
def test_gln_stem(cuda, refs, cid):
    """conv 7 x 7 / 2 + frozen batch norm (power-of-two scales: the fold is exact) + ReLU + max-pool 3 x 3 / 2 in one launch: the conv
    output is rounded before the pool, as the unfused schedule stores it (test_gln_stem_fused_parity); the pool is exact"""
    c, ref = refs(cid)
    same(widen(run_gln_stem(cuda, c)), ref, cid)


def _chain_convs(c, cuda):
    return [packed(L, c.dt, cuda) for L in c.layers]


def run_gauss_tail(cuda, c):
    from cvpce_amd import ops
    c4, c5 = _chain_convs(c, cuda)
    x = to_nhwc(c.x, c.dt).to(cuda)
    with switches() as prof:
        assert ops.can_fuse_gauss_tail(x, c4, c5)
        y = ops.gauss_tail(x, c4, c5, 1)
        assert prof.records[-1][0] == 'gauss_tail_kernel'
    torch.cuda.synchronize()
    return y


@pytest.mark.parametrize('cid', ec.ids('gauss_tail'))
def test_gauss_tail(cuda, refs, cid):
    """the Gaussian subnet's two pointwise layers in one launch, ReLU: the hidden layer is rounded where the two-launch form stores it
    (test_gauss_tail_parity)"""
    c, ref = refs(cid)
    same(widen(run_gauss_tail(cuda, c)), ref, cid)


def run_gauss_subnet(cuda, c, per_layer=False):
    """-> the fused kernel's output (and that of the per-layer launches: three thin 3 x 3 layers and the fused tail)"""
    from cvpce_amd import ops
    act = c.layers[-1].act
    convs = _chain_convs(c, cuda)
    x = to_nhwc(c.x, c.dt).to(cuda)
    y2 = None
    with switches() as prof:
        assert ops.can_fuse_gauss_subnet(x, convs)
        y = ops.gauss_subnet(x, convs, act)
        assert prof.records[-1][0] == 'gauss_subnet_kernel'
        if per_layer:
            t = ops.conv2d(x, convs[0], act=1, in_up_shift=1)
            t = ops.conv2d(ops.conv2d(t, convs[1], act=1), convs[2], act=1)
            assert [r[0] for r in prof.records[-3:]] == ['thin3x3_kernel'] * 3
            y2 = ops.gauss_tail(t, convs[3], convs[4], act)
    torch.cuda.synchronize()
    return y, y2


@pytest.mark.parametrize('cid', ec.ids('gauss_subnet'))
def test_gauss_subnet(cuda, refs, cid):
    """the whole Gaussian subnet in one launch, no activation and ReLU behind the last layer: rounded at the four places _subnet_reference
    (tests/test_gpu_kernels.py) rounds -- and equal to the per-layer launches, of which the tolerance test can only demand atol"""
    c, ref = refs(cid)
    y, per_layer = run_gauss_subnet(cuda, c, per_layer=True)
    same(widen(y), ref, cid)
    same(widen(per_layer), ref, cid + ' per-layer launches')


STALE_LDS = ['gauss_subnet/2x64x15_act0/bf16', 'gauss_subnet/2x19x23_act1/fp16', 'gauss_tail/1x37x41/fp16', 'bneck/512-128x5x9/fp16', 'bneck/64-64x37x51_sep/bf16']


@pytest.mark.parametrize('cid', STALE_LDS)
def test_fused_chains_ignore_stale_lds(cuda, refs, cid):
    """LDS is not cleared between kernels.  The fused chains keep rings and intermediate layers there and read slots beside the ones they
    wrote (the subnet's unused columns X + 28 .. read pixel slots 32 and 33 of its rings, which no one stores to); what they read there
    is dropped -- unless it is not finite: in the subnet's 16 -> 1 layer a dropped column shares an MFMA column with a kept one under a
    weight row of zeros, and 0 x NaN is NaN.  So: every compute unit's LDS full of 0xFFFFFFFF (ops.probe_lds_fill), then the kernel, and
    the result is the reference all the same."""
    from cvpce_amd import ops
    c, ref = refs(cid)
    assert ops.probe_lds_fill(0xFFFFFFFF) == 2048
    y = run_case(cuda, refs, c) if c.family != 'gauss_subnet' else run_gauss_subnet(cuda, c)[0]
    same(widen(y, c.keep), ref, cid)


def run_bottleneck(cuda, c, three_launches=False):
    """-> the fused kernel's output (and the three-launch schedule's)"""
    from cvpce_amd import ops
    pcs = _chain_convs(c, cuda)
    x = to_nhwc(c.x, c.dt).to(cuda)
    res = c.layers[-1].res
    r = x if res is c.x else to_nhwc(res, c.dt).to(cuda)
    with switches(FUSED_BOTTLENECK_MAX_PLANES=256) as prof:
        assert ops.can_fuse_bottleneck(x, *pcs, r)
        y = ops.bottleneck(x, *pcs, r)
        assert prof.records[-1][0] == 'bneck_kernel'
    y3 = None
    if three_launches:
        with switches(USE_FUSED_BOTTLENECK=False):
            y3 = ops.conv2d(ops.conv2d(ops.conv2d(x, pcs[0], act=1), pcs[1], act=1), pcs[2], act=1, residual=r)
    torch.cuda.synchronize()
    return y, y3


@pytest.mark.parametrize('cid', ec.ids('bneck'))
def test_bottleneck(cuda, refs, cid):
    """the fused bottleneck (1 x 1 -> 3 x 3 -> 1 x 1 + residual, intermediates in LDS) against the reference with the two intermediate
    layers rounded where the three-launch schedule stores them, and against that schedule; identity residual, and a separate residual
    tensor for the projection-shortcut block.  The whole batch runs, the last image is compared with the reference."""
    c, ref = refs(cid)
    y, y3 = run_bottleneck(cuda, c, three_launches=True)
    same(widen(y, c.keep), ref, cid)
    same(widen(y), widen(y3), cid + ' against the three-launch schedule')


# ---------------------------------------------------------------------------------------------------------------------------------
# the edges of fp16, over every kernel at once
# ---------------------------------------------------------------------------------------------------------------------------------
def run_case(cuda, refs, c):
    """the case's kernel, as its family's test launches it -> the output on the device"""
    if c.family in SINGLE:
        return run_single(cuda, c)[0]
    if c.family == 'atlas':
        return check_atlas(cuda, refs, False, c.dt, c.name[1:])
    return {'mac': lambda: run_mac(cuda, c)[0], 'vgg_stem': lambda: run_vgg_stem(cuda, c), 'gln_stem': lambda: run_gln_stem(cuda, c),
            'gauss_tail': lambda: run_gauss_tail(cuda, c), 'bneck': lambda: run_bottleneck(cuda, c)[0]}[c.family]()


BIG_16BIT = [cid for cid in ec.EDGE_IDS if '_big/' in cid and cid.split('/')[0] not in ('gauss_tail', 'gauss_subnet', 'thin_out') and 'cls_f32' not in cid]
BIG_F32 = [cid for cid in ec.EDGE_IDS if '_big/' in cid and (cid.split('/')[0] in ('gauss_tail', 'thin_out') or 'cls_f32' in cid)]


@pytest.mark.parametrize('cid', [c for c in BIG_16BIT if c.endswith('/fp16')])
def test_big_fp16_outputs_saturate(cuda, refs, cid):
    """every `big` case with an fp16 output: the kernel's output is finite, and its largest magnitude is exactly 65504"""
    c, _ = refs(cid)
    y = run_case(cuda, refs, c)
    assert y.dtype == H16 and bool(torch.isfinite(y).all()) and float(y.float().abs().max()) == ec.F16_MAX, cid


@pytest.mark.parametrize('cid', [c for c in BIG_16BIT if c.endswith('/bf16')])
def test_big_bf16_outputs_exceed_fp16(cuda, refs, cid):
    """every `big` case with a bf16 output: the kernel's output is finite and exceeds 65504 somewhere -- no fp16 clamp in a bf16 instance"""
    c, _ = refs(cid)
    y = run_case(cuda, refs, c)
    assert y.dtype == BF and bool(torch.isfinite(y).all()) and float(y.float().abs().max()) > ec.F16_MAX, cid


@pytest.mark.parametrize('cid', BIG_F32)
def test_big_f32_outputs_are_not_clamped(cuda, refs, cid):
    """a `big` case with an fp32 output, in either storage type: values above 65504 arrive (the Gaussian tail's output lies behind a
    layer that scales back down: there only finite)"""
    c, ref = refs(cid)
    y = run_case(cuda, refs, c)
    assert y.dtype == F32 and bool(torch.isfinite(y).all()), cid
    assert c.family == 'gauss_tail' or float(y.abs().max()) == float(ref.abs().max()) > ec.F16_MAX, cid


# ---------------------------------------------------------------------------------------------------------------------------------
# work-list and strip launches of the embedder
# ---------------------------------------------------------------------------------------------------------------------------------
def test_list_and_strip_launches(cuda, refs):
    """The S = 64 construction of tests/test_gpu_footprint.py test_list_and_strip_launches -- three crops (a wide one, a very thin one, one
    without any content column) plus the constant crop, four layers, both strip lists non-empty -- on the exact operands of
    exact_cases.worklist_case: crop content on a grid, the constant crop one grid value per channel.  What is sent to the kernels holds
    NaN outside a crop's extent (the stem) and outside the pixels the previous layer's list covers (the conv layers); listed pixels beyond
    a crop's extent hold the constant crop's values, as a real pass leaves them.  On every listed pixel, and on the listed rows of a cut
    tile, the stem over its list, the wide-tile list launch, the 16 x 16-tile list + strip launches with the fused pool and the MAC list +
    strip launches without a store equal the float64 reference of the tensor with its padding filled in from the constant crop; pixels
    off the lists are not written; the descriptor after mac_init equals the reference's maximum."""
    from cvpce_amd import ops
    S, n, pool_mask = ec.WL_S, ec.WL_N, ec.WL_POOL_MASK
    layers = [ops.skip_layer(*l) for l in ec.WL_LAYERS]
    nl, max_tiles = len(layers), (S // 16) ** 2
    model = ec.worklist_model()
    e = torch.tensor(ec.WL_EXT, dtype=torch.int32)
    wl = ops.embed_worklists(e.to(cuda), n, S, pool_mask, layers, max_tiles, want_computed=True)
    lists, counts, computed = wl      # (the raw tensors are checked against the model by hand, the launches take `wl`'s views)
    L, cnt = lists.cpu(), counts.cpu().tolist()
    assert cnt == [len(m[0]) for m in model] + [m[2] for m in model] + [len(m[1]) for m in model]
    for l, (want, swant, _, _) in enumerate(model):
        assert L[l, :len(want)].tolist() == want and L[nl + l, :len(swant)].tolist() == swant
    assert computed.cpu().tolist() == [m[3] for m in model]
    assert cnt[2 * nl + 2] > 0 and cnt[2 * nl + 3] > 0 and cnt[2 * nl] == cnt[2 * nl + 1] == 0, cnt          # both halo2 layers have strips
    entries = lambda l: L[l, :cnt[l]].tolist() + L[nl + l, :cnt[2 * nl + l]].tolist()
    nan = float('nan')

    def holed(t, mask):
        """NHWC storage tensor -> the same with NaN on the pixels of the crops (not of the constant crop) outside mask"""
        m = mask.clone()
        m[-1] = True
        return torch.where(m.expand_as(t), t, torch.full_like(t, nan))

    # the stem over its list
    c, ref0 = refs('worklist/stem/bf16')
    ref0 = ref0.permute(0, 2, 3, 1)
    yy, xx = torch.arange(S).view(1, S, 1, 1), torch.arange(S).view(1, 1, S, 1)
    content = torch.cat(((yy < e[:, 0].view(-1, 1, 1, 1)) & (xx < e[:, 1].view(-1, 1, 1, 1)), torch.ones(1, S, S, 1, dtype=torch.bool)))
    x_sent = holed(to_nhwc(c.x, BF, 4), content)
    l1, l2 = c.layers
    ps = ops.PackedStem(l1.w.float(), l1.b.float(), l2.w.float(), l2.b.float(), device=cuda)
    with switches() as prof:
        y0 = ops.vgg_stem_list(x_sent[:-1].contiguous().to(cuda), x_sent[-1].contiguous().to(cuda), ps, *wl.main(0))
        assert prof.records[-1][0] == 'vgg_stem2_kernel'
    m0 = fp.listed_pixels(entries(0), n, 32, 32, 8, 8)
    assert bool(m0[3].all()) and 0 < int(m0[0].sum()) < 32 * 32
    sel = m0.expand_as(ref0)
    assert torch.equal(y0.cpu().double()[sel], ref0[sel]), 'vgg_stem_list'

    def list_layer(li, in_mask, th, tw, mac_off=None):
        """layer li over its list (+ its strip list) on its exact input, sent with values only where in_mask says the previous list put
        some -> the pixel mask of its own output"""
        sc, ref = refs(f'worklist/layer{li}/bf16')                    # ref (n, cout, h, w): what an unlisted run stores (pooled for layer 2)
        cin, cout, hin, pool = ec.WL_CONVS[li]
        pc = packed(sc.layers[0], BF, cuda)
        sent = holed(to_nhwc(sc.x, BF), in_mask).to(cuda)
        ho = hin // 2 if pool else hin
        strips = wl.strips(li, layers[li].mode)
        assert (strips is not None) == (cout > 128) and (strips is None or (strips[0].data_ptr(), strips[1].data_ptr()) == (lists[nl + li].data_ptr(), counts[2 * nl + li:].data_ptr()))
        m = fp.listed_pixels(entries(li), n, ho, ho, th, tw)
        with switches() as prof:
            if mac_off is None:
                y = ops.conv2d_list(sent, pc, *wl.main(li), act=1, pool=pool, strips=strips,
                                    out=torch.full((n, ho, ho, cout), nan, dtype=BF, device=cuda))
            else:
                const_map = ref[-1].permute(1, 2, 0).float()                                     # (H, W, C) >= 0: the constant crop's own map
                zero = torch.zeros(1, cout)
                rows = torch.cat((torch.cummax(const_map.amax(dim=1).flip(0), 0).values.flip(0), zero)).to(cuda)
                cols = torch.cat((torch.cummax(const_map.amax(dim=0).flip(0), 0).values.flip(0), zero)).to(cuda)
                desc = torch.full((n, mac_off + cout + 24), -7.0, device=cuda)
                ops.mac_init(desc, mac_off, rows, cols, wl.computed_of(li).contiguous())
                assert ops.conv2d_list(sent, pc, *wl.main(li), act=1, mac=desc, mac_off=mac_off, store=False, strips=strips) is None
            names = [r[0] for r in prof.records]
        assert names[0] == ('conv3x3_halo3_kernel' if cout <= 128 else 'conv3x3_halo2_kernel') and (strips is None or names[-1] == 'conv3x3_halo2_kernel[strips]'), names
        torch.cuda.synchronize()
        if mac_off is not None:
            d = desc.cpu()
            assert torch.equal(d[:, mac_off:mac_off + cout].double(), ref.amax(dim=(-2, -1))), f'layer {li}: descriptor'
            assert bool((d[:, :mac_off] == -7).all()) and bool((d[:, mac_off + cout:] == -7).all())
            return None
        want = ref.permute(0, 2, 3, 1)
        s_ = m.expand_as(want)
        got = y.cpu().double()
        assert 0 < int(m.sum()) < m.numel()
        bad = s_ & (got != want)
        assert not bool(bad.any()), f'layer {li}: {int(bad.sum())} listed values differ, first at (n, y, x, c) = {bad.nonzero()[0].tolist()}'
        assert bool(got[~s_].isnan().all()), f'layer {li}: a pixel outside the list was written'
        return m

    m1 = list_layer(1, m0, 16, 32)
    m2 = list_layer(2, m1, 8, 8)
    list_layer(3, m2, 16, 16, mac_off=40)
