"""The fine work lists of the embedder (`cvpce_skip_layer.skip` 4 and 5, cvpce_conv3x3_halo_strips2, classification.SKIP_FINE): listed
tiles cut at their last non-constant row PAIR, and last-row tiles with only 2 useful rows computed four to a pass.

  1. cvpce_embed_worklists in the fine modes against the plain-Python model of tests/fine_lists.py;
  2. single layers at S = 64 on the construction of tests/fine_lists.py (every even `rows` 2 .. 16 per layer, both strip classes, a
     ragged last thin pass, thin strips of different crops in one pass) through the footprint harness, on exactly representable
     operands: listed pixels and the MAC descriptor equal the plain kernels' output AND the float64 reference, nothing else is written;
  3. the whole embedder with SKIP_FINE on and off against the plain schedule, bit for bit."""
import pytest
import torch

import exact_cases as ec            # tests/exact_cases.py
import fine_lists as fl             # tests/fine_lists.py
import footprint as fp              # tests/footprint.py
from test_gpu_skip import _boxes    # the mixed boxes of tests/test_gpu_skip.py

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
FINE = {2: 4, 3: 5}


@pytest.fixture
def fine_switch():
    """classification.SKIP_FINE, restored afterwards"""
    from cvpce_amd.models import classification as C
    old = (C.SKIP_FINE, C.SKIP_FINE_PARTS)
    yield C
    C.SKIP_FINE, C.SKIP_FINE_PARTS = old


# ---------------------------------------------------------------------------------------------------------------------------------
# 1. the list builder
# ---------------------------------------------------------------------------------------------------------------------------------
def test_fine_worklists_match_python_model(cuda):
    from cvpce_amd import ops, synthetic
    S = 256
    enc = synthetic.synthetic_macvgg(seed=1).cuda()
    steps, layers, pool_mask = enc.engine().skip_plan(S)
    assert [l[-1] for l in layers] == [1] + [2] * 2 + [3] * 9        # `skip_plan` itself is unchanged
    fine = [l._replace(skip=FINE.get(l[-1], l[-1])) for l in layers]
    g = torch.Generator().manual_seed(3)
    n = 131
    ext = torch.stack((torch.randint(1, S + 1, (n,), generator=g), torch.full((n,), S)), dim=1).to(torch.int32)
    ext[::3] = ext[::3].flip(1)                                  # tall boxes: columns
    ext[5] = torch.tensor([S, S]); ext[6] = torch.tensor([0, 0]); ext[7] = torch.tensor([1, S]); ext[8] = torch.tensor([S, 255])
    nl = len(fine)
    model = fl.model(ext.tolist() + [[S, S]], S, pool_mask, fine)
    lists, counts, computed = ops.embed_worklists(ext.cuda(), n + 1, S, pool_mask, fine, 256, want_computed=True)
    assert lists.shape[0] == 3 * nl and counts.numel() == 4 * nl
    lists, counts = lists.cpu(), counts.cpu().tolist()
    assert counts == [len(m[0]) for m in model] + [m[3] for m in model] + [len(m[1]) for m in model] + [len(m[2]) for m in model]
    for li, (want, swant, twant, _, comp) in enumerate(model):
        for row, ent in ((li, want), (nl + li, swant), (2 * nl + li, twant)):
            assert lists[row, :len(ent)].tolist() == ent, (li, row)
    assert computed.cpu().tolist() == [m[4] for m in model]
    assert sum(len(m[1]) for m in model) > 0 and sum(len(m[2]) for m in model) > 0     # the random extents produce both strip classes
    # mode 4 alone keeps the shapes of modes 0 .. 3, and gives the same main lists where no tile goes to a strip list
    only4 = [l._replace(skip=4 if l[-1] >= 2 else l[-1]) for l in layers]
    l4, c4, _ = ops.embed_worklists(ext.cuda(), n + 1, S, pool_mask, only4, 256)
    assert l4.shape[0] == 2 * nl and c4.numel() == 3 * nl
    m4 = fl.model(ext.tolist() + [[S, S]], S, pool_mask, only4)
    assert c4.cpu().tolist() == [len(m[0]) for m in m4] + [m[3] for m in m4] + [0] * nl
    for li, m in enumerate(m4):
        assert l4[li, :len(m[0])].cpu().tolist() == m[0], li


# ---------------------------------------------------------------------------------------------------------------------------------
# 2. single layers at S = 64
# ---------------------------------------------------------------------------------------------------------------------------------
def to_nhwc(t, dt):
    out = t.permute(0, 2, 3, 1).to(dt).contiguous()
    assert torch.equal(out.double(), t.permute(0, 2, 3, 1))
    return out


@pytest.fixture(scope='module')
def s64(cuda):
    """the lists of the construction, built by the kernel and checked against the model once; never modified"""
    from cvpce_amd import ops
    layers = [ops.skip_layer(*l) for l in fl.LAYERS]
    nl = len(layers)
    model = fl.construction()
    e = torch.tensor(fl.EXT, dtype=torch.int32)
    lists, counts, computed = ops.embed_worklists(e.to(cuda), fl.N, fl.S, fl.POOL_MASK, layers, (fl.S // 16) ** 2, want_computed=True)
    assert lists.shape[0] == 3 * nl
    cnt = counts.cpu().tolist()
    assert cnt == [len(m[0]) for m in model] + [m[3] for m in model] + [len(m[1]) for m in model] + [len(m[2]) for m in model]
    L = lists.cpu()
    for l, (want, swant, twant, _, _) in enumerate(model):
        assert L[l, :len(want)].tolist() == want and L[nl + l, :len(swant)].tolist() == swant and L[2 * nl + l, :len(twant)].tolist() == twant
    assert computed.cpu().tolist() == [m[4] for m in model]
    return dict(nl=nl, model=model, lists=lists, counts=counts, computed=computed)


_CASES = {}


def fine_case(li):
    """The exact operands of layer li of the construction, the `worklist/*` recipe of tests/exact_cases.py: the coarse grid, image
    N - 1 the constant crop, and beyond a crop's input extent (bits 32 .. 55 of its entries) the constant crop's own pixels -- what a
    list launch reads there.  -> (case, float64 reference of what an unlisted run stores, the mask of the crops' own pixels)"""
    if li not in _CASES:
        cin, cout, hin, pool = fl.CONVS[li]
        c = ec.single('finelist', f'layer{li}', BF, fl.N, cin, hin, hin, cout, 3, 1, 1, pool=pool)
        inside = torch.zeros(fl.N, 1, hin, hin, dtype=torch.bool)
        want, swant, twant, _, _ = fl.construction()[li]
        for en in want + swant + twant:
            inside[(en >> 16) & 0xFFFF, :, :(en >> 44) & 0xFFF, :(en >> 32) & 0xFFF] = True
        inside[-1] = True
        c.x = torch.where(inside, c.x, c.x[-1:])
        assert c.budget()[0] <= ec.BUDGET_LOG2
        _CASES[li] = (c, c.reference()[0], inside)
    return _CASES[li]


def _arena_conv(L, cuda):
    from cvpce_amd import ops
    pc = ops.PackedConv(L.w.float(), L.b.float(), 1, 1, device=cuda, dtype=BF)
    arenas = []
    for name in ('weight', 'weight_halo', 'bias'):
        pair = fp.put(getattr(pc, name), cuda)
        setattr(pc, name, pair[0])
        arenas.append(pair)
    return pc, arenas


@pytest.mark.parametrize('li, th, tw, mac_off', [(1, 16, 32, None), (2, 8, 8, None), (3, 16, 16, None), (3, 16, 16, 40)],
                         ids=['halo3-list', 'halo2-list-pool', 'halo2-list-strips-thin', 'halo2-mac-no-store'])
def test_single_layers_on_fine_lists(cuda, s64, li, th, tw, mac_off):
    from cvpce_amd import ops
    T = torch.ops.cvpce_amd
    nl, n = s64['nl'], fl.N
    c, ref, inside = fine_case(li)
    cin, cout, hin, pool = fl.CONVS[li]
    want, swant, twant, _, _ = s64['model'][li]
    wide = cout <= 128
    assert wide or (swant and twant)
    pc, wa = _arena_conv(c.layers[0], cuda)
    x = to_nhwc(c.x, BF)
    # what is sent: a crop's own pixels, NaN beyond its extent (read from the constant crop instead)
    sent = torch.where(inside.permute(0, 2, 3, 1).expand_as(x), x, torch.full_like(x, float('nan')))
    pin, lin, cin_ = fp.put(sent, cuda), fp.put(s64['lists'], cuda), fp.put(s64['counts'], cuda)
    ho = hin // 2 if pool else hin
    m = fp.listed_pixels(want + swant + twant, n, ho, ho, th, tw)                 # from the NEW lists, as the model states them
    plain = ops.conv2d(x.to(cuda), pc, act=1, pool=pool)                          # the plain kernel on the whole input
    torch.cuda.synchronize()
    assert torch.equal(plain.double().permute(0, 3, 1, 2).cpu(), ref)
    # list class k (0 main, 1 strips, 2 thin strips): row k nl + li of `lists`; its count sits behind the work figures, at (k + 1) nl + li
    row = lambda k: (lin[0][k * nl + li], cin_[0][(k + 1 if k else 0) * nl + li:][:1])

    def launches(out, mac, off):
        a = (pin[0], pc.weight_halo, pc.bias, out, mac, off, cout, pc.k_pad, pc.cout_pad, 1, int(pool and out is not None))
        T.conv3x3_halo_list(*a, *row(0))
        if not wide:
            T.conv3x3_halo_strips(*a, *row(1))
            T.conv3x3_halo_strips2(*a, *row(2))

    if mac_off is None:
        o = fp.out((n, ho, ho, cout), BF, cuda)
        y, = fp.check(lambda: launches(o[0], None, 0), [pin, lin, cin_] + wa, [o], written=m)     # unlisted pixels keep the prefill
        s_ = m.expand_as(y)
        assert 0 < int(m.sum()) < m.numel()
        got, pl = y.cpu().double(), plain.cpu().double()
        bad = s_ & (got != pl)
        assert not bool(bad.any()), f'layer {li}: {int(bad.sum())} listed values differ from the plain kernel, first at (n, y, x, c) = {bad.nonzero()[0].tolist()}'
        assert torch.equal(got[s_], ref.permute(0, 2, 3, 1)[s_])
        return
    # the MAC form, nothing stored: cvpce_mac_init starts the descriptor from the constant crop's suffix maxima
    const_map = ref[-1].permute(1, 2, 0).float()                                   # (H, W, C) >= 0
    zero = torch.zeros(1, cout)
    rows = fp.put(torch.cat((torch.cummax(const_map.amax(dim=1).flip(0), 0).values.flip(0), zero)), cuda)
    cols = fp.put(torch.cat((torch.cummax(const_map.amax(dim=0).flip(0), 0).values.flip(0), zero)), cuda)
    kin = fp.put(s64['computed'][li].contiguous(), cuda)
    desc = fp.out((n, mac_off + cout + 24), F32, cuda)
    dm = torch.zeros(1, mac_off + cout + 24, dtype=torch.bool)
    dm[:, mac_off:mac_off + cout] = True

    def run():
        T.mac_init(desc[0], mac_off, rows[0], cols[0], kin[0])
        launches(None, desc[0], mac_off)
    d, = fp.check(run, [pin, lin, cin_, rows, cols, kin] + wa, [desc], written=dm)
    d = d.cpu()[:, mac_off:mac_off + cout].double()
    assert torch.equal(d, plain.cpu().double().amax(dim=(1, 2))), 'descriptor against the plain kernel'
    assert torch.equal(d, ref.amax(dim=(-2, -1))), 'descriptor against the float64 reference'


# ---------------------------------------------------------------------------------------------------------------------------------
# 3. the whole embedder
# ---------------------------------------------------------------------------------------------------------------------------------
def _profiled(eng, crops, ext, const):
    from cvpce_amd import ops
    prof = ops.PROFILE = ops.ConvProfile()
    try:
        out = eng.embed_packed(crops, ext=ext, const_in=const)
        summ = prof.summary()
    finally:
        ops.PROFILE = None
    names = [r[0] for r in prof.records]
    return out, sum(v['flops_executed'] for v in summ.values()), sum(v['flops'] for v in summ.values()), names


@pytest.mark.parametrize('batch_norm', [False, True])
def test_embedding_is_bit_identical_with_fine_lists(cuda, fine_switch, batch_norm):
    from cvpce_amd import ops, synthetic
    C = fine_switch
    S = 256
    enc = synthetic.synthetic_macvgg(seed=1, batch_norm=batch_norm).cuda()
    eng = enc.engine()
    h0, w0 = 700, 900
    img = torch.rand(3, h0, w0, generator=torch.Generator().manual_seed(9)).cuda()
    boxes = _boxes(83, h0, w0, seed=21).cuda()
    crops = ops.crop_resize(img, boxes, S, mode=2, mean=C.TANH_MEAN, std=C.TANH_STD)
    ext = ops.crop_extents(boxes, None, h0, w0, S)
    const = eng.const_crop(C.TANH_MEAN, C.TANH_STD, 4, S)
    plain = eng.embed_packed(crops)
    C.SKIP_FINE, C.SKIP_FINE_PARTS = True, ('halo3', 'halo2', 'thin')
    # (the first work-list run of an engine also tabulates the constant crop's MAC maxima, through the plain kernels: keep those
    # launches out of the two profiles that are compared)
    assert torch.equal(plain, eng.embed_packed(crops, ext=ext, const_in=const))
    on, done_on, alg_on, names_on = _profiled(eng, crops, ext, const)
    assert torch.equal(plain, on)
    C.SKIP_FINE = False
    off, done_off, alg_off, names_off = _profiled(eng, crops, ext, const)
    assert torch.equal(plain, off)
    print(f'executed / algorithmic FLOPs: fine {done_on / alg_on:.4f}, coarse {done_off / alg_off:.4f}')
    assert alg_on == alg_off and done_on <= done_off < 0.9 * alg_off, (done_on, done_off, alg_off)
    # the schedule with the switch off is today's, launch for launch; with it on every wide layer has one launch more (its thin list)
    strips = sum(1 for nm in names_off if nm == 'conv3x3_halo2_kernel[strips]')
    assert strips == 9 and len(names_on) == len(names_off) + 9 and sum(1 for nm in names_on if nm == 'conv3x3_halo2_kernel[strips]') == 18
    assert [nm for nm in names_on if not nm.endswith('[strips]')] == [nm for nm in names_off if not nm.endswith('[strips]')]
    # each part on its own
    for parts in (('halo3',), ('halo2',), ('halo2', 'thin')):
        C.SKIP_FINE, C.SKIP_FINE_PARTS = True, parts
        assert torch.equal(plain, eng.embed_packed(crops, ext=ext, const_in=const)), parts


def test_multi_pass_with_fine_lists(cuda, fine_switch):
    """838 crops of one shape (two early passes, the constant crop at the end of each), and the late layers in two passes as well"""
    from cvpce_amd import ops, synthetic
    C = fine_switch
    S = 256
    enc = synthetic.synthetic_macvgg(seed=1).cuda()
    eng = enc.engine()
    h0 = w0 = 512
    img = torch.rand(3, h0, w0, generator=torch.Generator().manual_seed(2)).cuda()
    g = torch.Generator().manual_seed(4)
    n = 838
    assert n > C.FUSED_EMBED_BATCH
    x1 = torch.rand(n, generator=g) * 200; y1 = torch.rand(n, generator=g) * 300
    boxes = torch.stack((x1, y1, x1 + 260, y1 + 100), dim=1)
    boxes[3] = torch.tensor([10.0, 10.0, 10.5, 90.0])            # zero width after .to(long)
    boxes = boxes.cuda()
    crops = ops.crop_resize(img, boxes, S, mode=2, mean=C.TANH_MEAN, std=C.TANH_STD)
    ext = ops.crop_extents(boxes, None, h0, w0, S)
    const = eng.const_crop(C.TANH_MEAN, C.TANH_STD, 4, S)
    plain = eng.embed_packed(crops)
    C.SKIP_FINE, C.SKIP_FINE_PARTS = True, ('halo3', 'halo2', 'thin')
    assert torch.equal(plain, eng.embed_packed(crops, ext=ext, const_in=const))
    old, C.LATE_EMBED_MAX = C.LATE_EMBED_MAX, 500
    try:
        assert torch.equal(plain, eng.embed_packed(crops, ext=ext, const_in=const))
    finally:
        C.LATE_EMBED_MAX = old
