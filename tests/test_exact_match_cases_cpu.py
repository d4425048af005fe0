"""The cases of tests/exact_match_cases.py are sound before a GPU sees them: every operand is a bf16 value, every reference distance an fp32
value on the 2^-8 grid (so float64, the f32 kernels and the bf16 kernels must agree to the bit, in any summation order), the plain fp32
matmul already equals the float64 one, and the operands put the matcher's decisions where a wrong one shows: `ties` cases tie at the cut of
every k they are searched with and inside the top k across gallery tiles, `dense` cases have a unique first place for most queries and
let no feature column drop out of any query's distances.  The shares of every case are printed (`pytest -s`)."""
import pytest
import torch

import exact_match_cases as mc            # tests/exact_match_cases.py

MIN_CUT_TIES = 1 / 3            # ties: share of queries whose rank-k and rank-(k + 1) distances are equal
MIN_STRADDLES = 1 / 2           # ties, G >= 512 and k >= 4: share of queries with a tie pair across two 128-row tiles inside the top k
MIN_UNIQUE_FIRST = 1 / 2        # dense: share of queries whose nearest row is alone at its distance


@pytest.mark.parametrize('name', list(mc.SPECS))
def test_operands_are_recipe_rows(name):
    c = mc.case(name)
    recipe, qn, gn, d, ks, _ = mc.SPECS[name]
    assert c.shape == (qn, gn, d) and c.recipe == recipe and c.ks == tuple(ks) and max(ks) <= gn
    for x in (c.Q, c.G):
        assert torch.equal(x.to(torch.bfloat16).double(), x) and bool(torch.isfinite(x).all())
        nz = x != 0
        assert not bool(torch.signbit(x[~nz]).any())                          # no negative zeros
        s, top = nz.sum(dim=1), x.abs().amax(dim=1)
        assert all(int(v) in (0,) + mc.SIZES for v in s.unique())
        assert bool(((x.abs() == top[:, None]) | ~nz).all())                 # one magnitude per row ...
        live = top[top > 0]
        assert torch.equal(live.log2(), live.log2().round()) and 2.0 ** -4 <= float(live.min()) and float(live.max()) <= 2.0 ** 4    # ... a power of two in range
    if recipe == 'dense':
        assert bool((c.Q != 0).all())                                        # every query meets every column
    # the planted rows are what they are called
    p, ref = c.planted, c.ref
    assert p['g_twin'] // mc.TILE_G != p['g_duplicate'] // mc.TILE_G and torch.equal(c.G[p['g_twin']], c.G[p['g_duplicate']])
    assert not c.G[p['g_zero']].any() and float(ref.g_norms[p['g_zero']]) == mc.EPS
    assert bool((ref.dist[:, p['g_zero']] == 1.0).all())
    if 'q_positive_multiple' in p:
        q = p['q_positive_multiple']
        assert float(ref.dist[q, p['g_twin']]) == 0.0 and float(ref.dist[q, p['g_duplicate']]) == 0.0
        first = ref.indices[q, :int((ref.dist[q] == 0.0).sum())].tolist()       # (other rows may be multiples of the twin as well)
        assert first == sorted(first) and p['g_twin'] in first and p['g_duplicate'] in first
        assert float(ref.dist[p['q_negative_multiple'], p['g_negated']]) == 2.0
    if 'q_zero' in p:
        assert float(ref.q_norms[p['q_zero']]) == mc.EPS and bool((ref.dist[p['q_zero']] == 1.0).all())
        assert ref.indices[p['q_zero']].equal(torch.arange(gn))                # every row ties: the ranking is the row order
        assert int((c.Q[p['q_one_hot']] != 0).sum()) == 1
    assert ('q_zero' in p) == (recipe == 'ties' and qn >= 6) and ('q_positive_multiple' in p) == (qn >= 3)


@pytest.mark.parametrize('name', list(mc.SPECS))
def test_reference_is_exact_in_fp32(name):
    c, ref = mc.case(name), mc.case(name).ref
    for v in (ref.dist, ref.q_norms, ref.g_norms):
        assert torch.equal(v.float().double(), v)
    assert torch.equal((ref.dist / mc.GRID).round() * mc.GRID, ref.dist)
    assert float(ref.dist.min()) >= 0.0 and float(ref.dist.max()) <= 2.0
    # the norms are powers of two (or eps), so their reciprocals and products are exact
    for n in (ref.q_norms, ref.g_norms):
        live = n[n > mc.EPS]
        assert torch.equal(live.log2(), live.log2().round())
    # the fp32 computation in both of the kernels' forms, with whatever summation order this host's matmul has, is the reference
    Q, G = c.Q.float(), c.G.float()
    qn, gn = Q.square().sum(dim=1).sqrt().clamp(min=mc.EPS), G.square().sum(dim=1).sqrt().clamp(min=mc.EPS)
    assert torch.equal(qn.double(), ref.q_norms) and torch.equal(gn.double(), ref.g_norms)
    dot = Q @ G.T
    assert torch.equal(dot.double(), c.Q @ c.G.T)
    assert torch.equal((1.0 - dot / (qn[:, None] * gn[None, :])).double(), ref.dist)
    rq, rg = 1.0 / qn, 1.0 / gn
    assert torch.equal(torch.addcmul(torch.ones_like(dot), -dot, rq[:, None] * rg[None, :]).double(), ref.dist)
    # the ranking: distances ascending, equal ones by ascending row, every row once
    assert bool((ref.values[:, 1:] >= ref.values[:, :-1]).all())
    tie = ref.values[:, 1:] == ref.values[:, :-1]
    assert bool((ref.indices[:, 1:][tie] > ref.indices[:, :-1][tie]).all())
    assert torch.equal(ref.dist.gather(1, ref.indices), ref.values)


@pytest.mark.parametrize('name', [n for n in mc.SPECS if mc.SPECS[n][0] == 'ties'])
def test_ties_cases_tie_where_the_matcher_decides(name):
    c, ref = mc.case(name), mc.case(name).ref
    gn = c.shape[1]
    vals = ref.dist.unique()
    print(f'\n{name}: {len(vals)} distinct distances in [{float(vals.min())}, {float(vals.max())}], {float((ref.dist > 1).double().mean()):.0%} above 1')
    for k in c.ks:
        line = f'  k = {k}:'
        if k < gn:                                                   # (k = G has no cut)
            cut = float(mc.cut_ties(ref, k).double().mean())
            line += f' tie at the cut {cut:.0%}'
            assert cut >= MIN_CUT_TIES, (name, k, cut)
        if k >= 2:
            share = float(mc.straddles(ref, k).double().mean())
            line += f' tie pair across 128-row tiles {share:.0%}'
            if gn >= 512 and k >= 4:
                assert share >= MIN_STRADDLES, (name, k, share)
        print(line)


@pytest.mark.parametrize('name', [n for n in mc.SPECS if mc.SPECS[n][0] == 'dense'])
def test_dense_cases_single_out_a_winner_and_use_every_column(name):
    c, ref = mc.case(name), mc.case(name).ref
    unique = float((ref.values[:, 0] < ref.values[:, 1]).double().mean())
    print(f'\n{name}: unique first place {unique:.0%}; tie at the cut ' + ', '.join(f'k = {k}: {float(mc.cut_ties(ref, k).double().mean()):.0%}' for k in c.ks))
    assert unique >= MIN_UNIQUE_FIRST, (name, unique)
    # a GEMM that drops feature column j forms dot - Q[:, j] G[:, j]^T under the same norms: every query's distance row must change
    dot, scale = c.Q @ c.G.T, ref.q_norms[:, None] * ref.g_norms[None, :]
    for j in range(c.shape[2]):
        without = 1.0 - (dot - torch.outer(c.Q[:, j], c.G[:, j])) / scale
        assert bool((without != ref.dist).any(dim=1).all()), (name, j)


def test_twins_of_the_long_case_sort_in_different_runs():
    """k = G = 16 500: the select hands the sort 16 384 keys in the first run and the rest in the second.  The duplicated rows must come
    out of the select in different runs for every query, so that their tie is resolved by the merge of the runs."""
    c, ref = mc.case(mc.SORT_RUNS_CASE), mc.case(mc.SORT_RUNS_CASE).ref
    gn = c.shape[1]
    assert gn > mc.SORT_RUN and c.ks == (gn,)
    pos = mc.select_positions(ref, gn)
    assert pos.sort(dim=1).values.equal(torch.arange(gn).expand_as(pos))      # k = G: every row survives, each at its own place
    twin, dup = pos[:, c.planted['g_twin']], pos[:, c.planted['g_duplicate']]
    assert bool((twin < mc.SORT_RUN).all()) and bool((dup >= mc.SORT_RUN).all())
    # ... and ends up behind its twin in the ranking, with nothing but rows of the same distance between them
    rank = ref.indices.argsort(dim=1)
    for q in range(c.shape[0]):
        a, b = int(rank[q, c.planted['g_twin']]), int(rank[q, c.planted['g_duplicate']])
        assert a < b and float(ref.values[q, a]) == float(ref.values[q, b])
    # select_positions itself, on a small k: the survivors are the top k, each placed once
    small = mc.case('ties_65x129x64')
    for k in (17, 100):
        p = mc.select_positions(small.ref, k)
        assert bool(((p >= 0).sum(dim=1) == k).all())
        assert torch.equal((p >= 0).nonzero()[:, 1].reshape(-1, k), small.ref.indices[:, :k].sort(dim=1).values)
        assert p.masked_fill(p < 0, 10 ** 6).sort(dim=1).values[:, :k].equal(torch.arange(k).expand(p.shape[0], k))


@pytest.mark.parametrize('b,d', mc.L2_SHAPES)
def test_l2_cases_divide_exactly(b, d):
    x, want = mc.l2_case(b, d)
    assert x.shape == (b, d) and torch.equal(x.float().double(), x)
    assert torch.equal(want.to(torch.bfloat16).double(), want)                # (so the bf16 copy is exact as well)
    assert torch.equal((x.float() / x.float().square().sum(dim=1, keepdim=True).sqrt().clamp(min=mc.EPS)).double(), want)
    norms = want.square().sum(dim=1)
    assert all(float(v) in (0.0, 1.0) for v in norms)
    assert (b > 3) == bool((norms == 0).any())                                # the zero row of the five-row cases
