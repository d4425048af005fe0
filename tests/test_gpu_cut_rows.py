"""Cut tiles of the work-list convs (conv3x3_halo2.hip LIST without strips, conv3x3_halo3.hip LIST): a tile with `rows` < 16 fetches
patch rows 0 .. rows + 1 only, streams them, and issues in its last row pair only the taps of rows it stores.  The patch rows it
leaves out keep in LDS what an EARLIER tile of the same workgroup put there, so the kernel can go wrong at a tile-to-tile hand-over
inside one workgroup, at the first row pair (rows = 2) and at the last stored row.  Hence

  * a grid of 1 x ctiles and 2 x ctiles workgroups (cvpce_set_persistent_workgroups): one workgroup walks the whole list;
  * HAND-WRITTEN lists (the 64-bit entries of csrc/worklist.h, not the list builder's output) whose `rows` sequence puts every even cut
    2 .. 14 directly behind a full tile, behind a taller cut and behind a shorter cut, each time on another tile than its predecessor's;
  * Cin = 64 (one chunk: every step 5 is also the hand-off step) and Cin = 128;
  * NaN sent beyond every crop's extent (as test_gpu_skip_fine.py fine_case does): a fetch that should have gone to the constant crop
    poisons a stored value; the footprint harness (tests/footprint.py) sees a row that should not have been written.

Listed pixels equal the plain kernel on the whole input AND the float64 reference on exactly representable operands
(tests/exact_cases.py); unlisted pixels keep the prefill; MAC descriptors equal the plain kernel's maxima; and the same list with every
`rows` raised to 16 gives the same values on the pixels listed originally."""
import pytest
import torch

import exact_cases as ec            # tests/exact_cases.py
import footprint as fp              # tests/footprint.py

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
N = 6                               # five crops and the constant crop (image N - 1)
TILES = 2                           # tile rows and tile columns of a map: 32 x 32 in 16 x 16 tiles (halo2), 32 x 64 in 16 x 32 tiles (halo3)
H = 32
# content rows of crops 0 .. 4 on the conv's INPUT (every crop is wide: all columns are content); a 3x3 conv makes rows 0 .. ey of its
# output non-constant, ey + 1 rows
EY = [1, 5, 9, 12, 19]
# the list: (rows, crop, tile row, tile column) in the order one workgroup walks it
LIST = [
    (16, 4, 0, 0), (2, 0, 0, 0), (4, 4, 1, 0), (6, 1, 0, 0), (8, 1, 0, 1), (10, 2, 0, 0), (12, 2, 0, 1), (14, 3, 0, 0),       # a full tile, then every cut behind a shorter one
    (12, 2, 0, 0), (10, 2, 0, 1), (8, 1, 0, 0), (6, 1, 0, 1), (4, 4, 1, 1), (2, 0, 0, 1),                                     # every cut behind a taller one
    (16, 4, 0, 1), (4, 0, 0, 0), (16, 5, 0, 0), (6, 4, 1, 0), (16, 5, 0, 1), (8, 0, 0, 1), (16, 5, 1, 0), (10, 4, 1, 1),     # every cut behind a full tile
    (16, 5, 1, 1), (12, 1, 0, 0), (16, 3, 0, 1), (14, 3, 0, 0), (16, 4, 0, 0),
]
CUTS = range(2, 16, 2)


def needed(n, ty):
    """the non-constant conv-output rows of tile row ty of crop n, rounded up to even (what the list builder's finest mode lists)"""
    eo = H if n == N - 1 else EY[n] + 1
    return max(0, min(16, (eo - 16 * ty + 1) // 2 * 2))


def rows_computed(n):
    """conv-output rows [0, rc) of crop n are computed by the list, the rest is the constant crop's (cvpce_mac_init's `computed`)"""
    return sum(needed(n, ty) for ty in range(TILES))


def test_the_list_is_what_the_docstring_says():
    """host only, but it belongs to this file: the adjacencies, and that the list is one the kernels' contract allows"""
    rows = [e[0] for e in LIST]
    follows = {(a, b) for a, b in zip(rows, rows[1:])}
    for c in CUTS:
        assert (16, c) in follows, c
        assert c == 14 or any((t, c) in follows for t in CUTS if t > c), c
        assert c == 2 or any((s, c) in follows for s in CUTS if s < c), c
    assert any((c, 16) in follows for c in CUTS)
    for (_, n0, ty0, tx0), (_, n1, ty1, tx1) in zip(LIST, LIST[1:]):
        assert (n0, ty0, tx0) != (n1, ty1, tx1)                              # a cut tile's predecessor left another tile's patch in LDS
    listed = {}
    for r, n, ty, tx in LIST:
        assert 0 < needed(n, ty) <= r <= 16 and r % 2 == 0                   # every non-constant row of a listed tile is computed
        listed[(n, ty, tx)] = max(r, listed.get((n, ty, tx), 0))
    for n in range(N):                                                       # every tile with a non-constant row is listed (the MAC form needs it)
        for ty in range(TILES):
            for tx in range(TILES):
                assert (needed(n, ty) > 0) == ((n, ty, tx) in listed)


def entries(w_in, raised=False):
    """the 64-bit entries (csrc/worklist.h): hi = rows << 24 | ey << 12 | ex, lo = n << 16 | ty << 8 | tx"""
    out = []
    for r, n, ty, tx in LIST:
        ey = H if n == N - 1 else EY[n]
        out.append((((((16 if raised else r) << 24) | (ey << 12) | w_in) << 32) | (n << 16) | (ty << 8) | tx))
    return out


def to_nhwc(t, dt):
    out = t.permute(0, 2, 3, 1).to(dt).contiguous()
    assert torch.equal(out.double(), t.permute(0, 2, 3, 1))
    return out


_CASES = {}


def cut_case(kernel, cin, pool, cuda):
    """exact operands of one layer, computed once and never modified: -> dict(case, whole input, what is sent, float64 references, the
    plain kernel's output on the whole input, the packed weights in arenas)"""
    key = (kernel, cin, pool)
    if key not in _CASES:
        from cvpce_amd import ops
        w_in, cout = (32, 256) if kernel == 'halo2' else (64, 128)
        c = ec.single('cutrows', f'{kernel}-{cin}', BF, N, cin, H, w_in, cout, 3, 1, 1, pool=pool)
        inside = torch.zeros(N, 1, H, w_in, dtype=torch.bool)
        for n, ey in enumerate(EY):
            inside[n, :, :ey] = True
        inside[-1] = True
        c.x = torch.where(inside, c.x, c.x[-1:])
        assert c.budget()[0] <= ec.BUDGET_LOG2
        ref, stored = c.reference()
        L = c.layers[0]
        pc = ops.PackedConv(L.w.float(), L.b.float(), 1, 1, device=cuda, dtype=BF)
        arenas = []
        for name in ('weight', 'weight_halo', 'bias'):
            pair = fp.put(getattr(pc, name), cuda)
            setattr(pc, name, pair[0])
            arenas.append(pair)
        x = to_nhwc(c.x, BF)
        sent = torch.where(inside.permute(0, 2, 3, 1).expand_as(x), x, torch.full_like(x, float('nan')))
        plain = ops.conv2d(x.to(cuda), pc, act=1, pool=pool)                  # the plain kernel on the whole input, at the default grid
        torch.cuda.synchronize()
        assert torch.equal(plain.double().permute(0, 3, 1, 2).cpu(), ref)
        _CASES[key] = dict(c=c, x=x, sent=sent, ref=ref, unpooled=stored[0], plain=plain.cpu(), pc=pc, arenas=arenas, w_in=w_in, cout=cout)
    return _CASES[key]


@pytest.fixture
def small_grid():
    """cvpce_set_persistent_workgroups, 256 again afterwards"""
    from cvpce_amd import _lib
    try:
        yield lambda n: _lib.lib.cvpce_set_persistent_workgroups(n)
    finally:
        assert _lib.lib.cvpce_set_persistent_workgroups(256) == 0


def tile_shape(kernel, pool):
    th, tw = (16, 16) if kernel == 'halo2' else (16, 32)
    return (th // 2, tw // 2) if pool else (th, tw)


def run_list(cuda, k, kernel, pool, ent, x_sent, mode, grid, small_grid):
    """one list launch through the footprint harness -> the stored map (or None) and the descriptor (or None), on the host"""
    T = torch.ops.cvpce_amd
    pc, cout = k['pc'], k['cout']
    pin = fp.put(x_sent, cuda)
    lin = fp.put(torch.tensor(ent, dtype=torch.int64), cuda)
    cnt = fp.put(torch.tensor([len(ent)], dtype=torch.int32), cuda)
    ho, wo = (H // 2, k['w_in'] // 2) if pool else (H, k['w_in'])
    th, tw = tile_shape(kernel, pool)
    m = fp.listed_pixels(ent, N, ho, wo, th, tw)
    assert 0 < int(m.sum()) < m.numel()
    store = mode != 'mac-no-store'
    o = fp.out((N, ho, wo, cout), BF, cuda) if store else None
    ins, outs, written = [pin, lin, cnt] + k['arenas'], [], []
    if store:
        outs.append(o); written.append(m)
    desc = None
    if mode.startswith('mac'):
        off = 40
        const_map = k['unpooled'][-1].permute(1, 2, 0).float()                # the constant crop's stored map before the pool, (H, W, C) >= 0
        zero = torch.zeros(1, cout)
        rtab = fp.put(torch.cat((torch.cummax(const_map.amax(dim=1).flip(0), 0).values.flip(0), zero)), cuda)
        ctab = fp.put(torch.cat((torch.cummax(const_map.amax(dim=0).flip(0), 0).values.flip(0), zero)), cuda)
        kin = fp.put(torch.tensor([[rows_computed(n), k['w_in'] // 16] for n in range(N)], dtype=torch.int32), cuda)
        desc = fp.out((N, off + cout + 24), F32, cuda)
        dm = torch.zeros(1, off + cout + 24, dtype=torch.bool)
        dm[:, off:off + cout] = True
        ins += [rtab, ctab, kin]
        outs.append(desc); written.append(dm)

    def run():
        if desc is not None:
            T.mac_init(desc[0], 40, rtab[0], ctab[0], kin[0])
        T.conv3x3_halo_list(pin[0], pc.weight_halo, pc.bias, o[0] if store else None, desc[0] if desc is not None else None, 40 if desc is not None else 0,
                            cout, pc.k_pad, pc.cout_pad, 1, int(pool and store), lin[0], cnt[0])
    ctiles = 1                                                                # 256 couts in 256-cout tiles, 128 in 128-cout tiles
    assert small_grid(grid * ctiles) == 0
    res = fp.check(run, ins, outs, written=written)
    assert small_grid(256) == 0
    y = res[0].cpu() if store else None
    d = res[-1].cpu()[:, 40:40 + cout].double() if desc is not None else None
    return y, d, m


def check_listed(k, y, m, pool):
    s_ = m.expand_as(y)
    got, pl = y.double(), k['plain'].double()
    bad = s_ & (got != pl)
    assert not bool(bad.any()), f'{int(bad.sum())} listed values differ from the plain kernel, first at (n, y, x, c) = {bad.nonzero()[0].tolist()}'
    assert torch.equal(got[s_], k['ref'].permute(0, 2, 3, 1)[s_])


HALO2 = [(cin, mode, grid) for cin in (64, 128) for mode in ('plain', 'pool', 'mac-pool', 'mac-no-store') for grid in (1, 2)]
HALO3 = [(cin, mode, grid) for cin in (64, 128) for mode in ('plain', 'pool') for grid in (1, 2)]


@pytest.mark.parametrize('kernel, cin, mode, grid', [('halo2',) + p for p in HALO2] + [('halo3',) + p for p in HALO3],
                         ids=lambda v: str(v))
def test_cut_tiles_on_hand_written_lists(cuda, small_grid, kernel, cin, mode, grid):
    pool = mode in ('pool', 'mac-pool')
    k = cut_case(kernel, cin, pool, cuda)
    y, d, m = run_list(cuda, k, kernel, pool, entries(k['w_in']), k['sent'], mode, grid, small_grid)
    if y is not None:
        check_listed(k, y, m, pool)
    if d is not None:
        # with what cvpce_mac_init starts from, the listed tiles' maxima are the maxima of the whole map
        assert torch.equal(d, k['plain'].double().amax(dim=(1, 2))), 'descriptor against the plain kernel'
        assert torch.equal(d, k['unpooled'].amax(dim=(-2, -1))), 'descriptor against the float64 reference'


@pytest.mark.parametrize('kernel', ['halo2', 'halo3'])
def test_cut_and_uncut_paths_agree(cuda, small_grid, kernel):
    """the same list with every `rows` raised to 16, on the NaN-free whole input: the pixels listed originally take the same values"""
    k = cut_case(kernel, 128, False, cuda)
    y_cut, _, m = run_list(cuda, k, kernel, False, entries(k['w_in']), k['x'], 'plain', 1, small_grid)
    y_all, _, m_all = run_list(cuda, k, kernel, False, entries(k['w_in'], raised=True), k['x'], 'plain', 1, small_grid)
    assert bool((m_all | ~m).all())
    s_ = m.expand_as(y_cut)
    assert torch.equal(y_cut.view(torch.int16)[s_], y_all.view(torch.int16)[s_])
    check_listed(k, y_all, m_all, False)
