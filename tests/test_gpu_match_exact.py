"""Bit-exact tests of the matcher (csrc/match.hip) and of l2_normalize on exactly representable operands (tests/exact_match_cases.py;
test_exact_match_cases_cpu.py shows that the cases are sound).  Every distance of a case is a multiple of 2^-8 that fp32 forms without
rounding in any summation order, so the reference is float64 and every comparison is `torch.equal` over ALL queries and ALL positions:
indices as int64 against the stable sort of the reference, distances bit for bit as int32 against the reference cast to fp32.  No
mask of well-separated rows, no tolerance -- the operands are full of ties (at the cut of every k, across gallery tiles, across sort
runs), of negative dot products, of distances 0, 1 (zero rows through the eps clamp) and 2, and of rows whose norms differ 256-fold.
Every kernel variant is compared with the reference, never with another variant.  The launch each search takes is read from
cvpce_match_plan, asserted where the test is about a path, and printed (`pytest -s`)."""
import ctypes

import pytest
import torch

import exact_match_cases as mc            # tests/exact_match_cases.py

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
DTYPES = [torch.float32, BF]
IDS = {torch.float32: 'f32', BF: 'bf16'}
# the pinned variants of the bf16 search, as test_match_cores_and_tiles_give_identical_results enumerates them: the 128-row core, and the
# LDS-DMA core with tiles of 128 mg gallery rows x 64 nq queries
VARIANTS = [(1, 0, 0)] + [(2, nq, mg) for mg in (1, 2) for nq in (2, 3, 4, 5) if not (mg == 1 and nq == 5)]
PATHS = {0: 'fused, 128-row core', 1: 'fused, LDS-DMA core', 2: 'large k'}


def _plan(qn, gn, d, k, dtype):
    from cvpce_amd._lib import lib
    out = (ctypes.c_longlong * 12)()
    assert lib.cvpce_match_plan(qn, gn, d, k, int(dtype == torch.float32), out) == 0
    names = ('path', 'tq', 'nq', 'mg', 'tiles_g', 'tiles_q', 'lds', 'threads', 'chunk')
    return dict(zip(names, out))


def _describe(p):
    tile = f"128 x {p['tq']}" if p['path'] != 1 else f"{128 * p['mg']} x {64 * p['nq']}"
    return f"{PATHS[p['path']]}, tile {tile} (gallery x queries), {p['tiles_g']} x {p['tiles_q']} tiles" + (f", chunk {p['chunk']}" if p['path'] == 2 else '')


def _bits(x):
    return x.contiguous().view(torch.int32)


def _check(got, ref, k, what):
    """all rows, all positions: indices and distance bits equal the float64 reference's first k"""
    idx, dist = got[0].cpu(), got[1].cpu()
    want_i, want_d = ref.indices[:, :k], ref.values[:, :k].float()
    assert idx.dtype == torch.int64 and dist.dtype == torch.float32 and idx.shape == want_i.shape == dist.shape, what
    bad = (_bits(dist) != _bits(want_d)) | (idx != want_i)
    where = ''
    if bool(bad.any()):                                      # the first wrong (query, position): narrows the cause down (tile, merge, select, sort)
        q, j = (int(v) for v in bad.nonzero()[0])
        where = (f'{what}: {int(bad.sum())} of {bad.numel()} wrong, first at query {q} position {j}: got row {int(idx[q, j])} at '
                 f'{float(dist[q, j])!r}, want row {int(want_i[q, j])} at {float(want_d[q, j])!r}')
    assert torch.equal(_bits(dist), _bits(want_d)), where
    assert torch.equal(idx, want_i), where


def _operands(case, dtype, cuda):
    return case.Q.to(dtype).to(cuda), case.G.to(dtype).to(cuda)


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('name', [n for n in mc.SPECS if n != mc.PADDED_CASE])
def test_row_norms_equal_the_reference(cuda, name, dtype):
    """First and apart from the searches, so that a wrong norm is not taken for a wrong GEMM.  The zero rows give eps.  (The case of 100
    features reaches row_norms through pad_features: the next test.)"""
    from cvpce_amd import ops
    c = mc.case(name)
    Q, G = _operands(c, dtype, cuda)
    for x, want in ((Q, c.ref.q_norms), (G, c.ref.g_norms)):
        assert torch.equal(_bits(ops.row_norms(x).cpu()), _bits(want.float()))
    assert float(ops.row_norms(G)[c.planted['g_zero']]) == mc.EPS


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
def test_row_norms_of_padded_rows(cuda, dtype):
    from cvpce_amd import ops
    c = mc.case(mc.PADDED_CASE)
    for x, want in ((c.Q, c.ref.q_norms), (c.G, c.ref.g_norms)):
        padded = ops.pad_features(x.to(dtype).to(cuda))
        assert padded.shape[1] == 128 and not padded[:, c.shape[2]:].any()
        assert torch.equal(_bits(ops.row_norms(padded).cpu()), _bits(want.float()))


@pytest.mark.parametrize('name', mc.FUSED_CASES)
def test_fused_path_f32(cuda, name):
    from cvpce_amd import ops
    c = mc.case(name)
    Q, G = _operands(c, torch.float32, cuda)
    for k in mc.FUSED_KS:
        p = _plan(*c.shape, k, torch.float32)
        print(f'\n{name} f32 k = {k}: {_describe(p)}', end='')
        assert (p['path'], p['tq']) == (0, 128)
        _check(ops.match_topk(Q, G, k, return_distance=True), c.ref, k, (name, 'f32', k))


@pytest.mark.parametrize('name', mc.FUSED_CASES)
def test_fused_path_bf16_every_core_and_tile(cuda, name):
    """The cost model's own choice and every pinned variant, each against the reference."""
    from cvpce_amd import ops
    c = mc.case(name)
    Q, G = _operands(c, BF, cuda)
    try:
        for core, nq, mg in [(0, 0, 0)] + VARIANTS:
            assert ops.match_set_core(core, nq, mg) == 0
            for k in mc.FUSED_KS:
                p = _plan(*c.shape, k, BF)
                print(f'\n{name} bf16 k = {k} pin {(core, nq, mg)}: {_describe(p)}', end='')
                if core == 1:
                    assert p['path'] == 0 and p['tq'] in (64, 128)
                if core == 2:
                    assert (p['path'], p['nq'], p['mg']) == (1, nq, mg)
                _check(ops.match_topk(Q, G, k, return_distance=True), c.ref, k, (name, 'bf16', k, (core, nq, mg)))
    finally:
        ops.match_set_core(0, 0, 0)


@pytest.mark.parametrize('k', [4, 17])
def test_128_query_tiles_bf16(cuda, k):
    """The bf16 128-query instances of the 128-row core (selecting: k = 4, storing: k = 17) run only where whole rounds of the chip favour
    them: the shape the other tests pin them at, the plan asserted."""
    from cvpce_amd import ops
    c = mc.case(mc.TQ128_CASE)
    assert c.shape == (768, 10000, 64) and k in c.ks
    Q, G = _operands(c, BF, cuda)
    try:
        assert ops.match_set_core(1, 0, 0) == 0
        p = _plan(*c.shape, k, BF)
        assert (p['path'], p['tq']) == (2 if k > 16 else 0, 128)
        print(f'\n{c.name} bf16 k = {k} pin (1, 0, 0): {_describe(_plan(*c.shape, k, BF))}', end='')
        got = ops.match_topk(Q, G, k, return_distance=True)
    finally:
        ops.match_set_core(0, 0, 0)
    _check(got, c.ref, k, (c.name, 'bf16', k))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
@pytest.mark.parametrize('name', mc.LARGE_K_CASES)
def test_large_k_path(cuda, name, dtype):
    """k = 17, 100 and the whole gallery: distance block, radix select (whose cut falls inside a tie for nearly every query), LDS sort."""
    from cvpce_amd import ops
    c = mc.case(name)
    Q, G = _operands(c, dtype, cuda)
    gn = c.shape[1]
    for k in mc.LARGE_KS + (gn,):
        assert k in c.ks
        p = _plan(*c.shape, k, dtype)
        print(f'\n{name} {IDS[dtype]} k = {k}: {_describe(p)}', end='')
        assert p['path'] == 2 and p['chunk'] == c.shape[0]
        _check(ops.match_topk(Q, G, k, return_distance=True), c.ref, k, (name, IDS[dtype], k))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
def test_full_ranking_above_one_sort_run(cuda, dtype):
    """k = G = 16 500: two sorted runs merged through the workspace.  The duplicated rows leave the select in different runs (shown on the
    host), so the merge pass decides their order; the whole ranking must be the reference's stable sort."""
    from cvpce_amd import ops
    c = mc.case(mc.SORT_RUNS_CASE)
    gn = c.shape[1]
    assert gn > mc.SORT_RUN
    Q, G = _operands(c, dtype, cuda)
    p = _plan(*c.shape, gn, dtype)
    print(f'\n{c.name} {IDS[dtype]} k = {gn}: {_describe(p)}', end='')
    assert p['path'] == 2
    _check(ops.match_topk(Q, G, gn, return_distance=True), c.ref, gn, (c.name, IDS[dtype], gn))


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
def test_nearest_neighbors_pads_the_features(cuda, dtype):
    """models.classification.nearest_neighbors with 100 features: zero-padded to 128 by pad_features, same neighbours."""
    from cvpce_amd.models.classification import nearest_neighbors
    c = mc.case(mc.PADDED_CASE)
    assert c.shape[2] == 100 and c.ks == (3,)
    got = nearest_neighbors(c.G.float().to(cuda), c.Q.float().to(cuda), k=3, dtype=dtype).cpu()
    assert got.dtype == torch.int64 and torch.equal(got, c.ref.indices[:, :3])


@pytest.mark.parametrize('dtype', DTYPES, ids=IDS.get)
def test_supplied_norms_give_the_same_bits(cuda, dtype):
    """The product path passes the gallery's stored norms: with q_norms / g_norms supplied (the reference's, as fp32) the result is the
    same as with the norms the search computes itself -- the reference -- on the fused and on the large-k path."""
    from cvpce_amd import ops
    c = mc.case('ties_65x129x64')
    Q, G = _operands(c, dtype, cuda)
    qn, gn = c.ref.q_norms.float().to(cuda), c.ref.g_norms.float().to(cuda)
    for k in (4, 17):
        _check(ops.match_topk(Q, G, k, q_norms=qn, g_norms=gn, return_distance=True), c.ref, k, ('both norms', IDS[dtype], k))
        _check(ops.match_topk(Q, G, k, g_norms=gn, return_distance=True), c.ref, k, ('gallery norms', IDS[dtype], k))


@pytest.mark.parametrize('b,d', mc.L2_SHAPES)
def test_l2_normalize_exact(cuda, b, d):
    """x / max(|x|, eps) on recipe rows: the quotient by a power-of-two norm is exact, a zero row stays zero; widths below, at and off the
    64 lanes of a row's wave, row counts that do not fill a block of four rows."""
    from cvpce_amd import ops
    x, want = mc.l2_case(b, d)
    xd = x.float().to(cuda)
    out, out_bf = ops.l2_normalize(xd, 1e-8, want_bf16=True)
    assert torch.equal(_bits(out.cpu()), _bits(want.float()))
    assert out_bf.dtype == BF and torch.equal(out_bf.cpu(), out.cpu().to(BF))
    assert torch.equal(_bits(ops.l2_normalize(xd, 1e-8).cpu()), _bits(want.float()))       # without the bf16 copy
