"""The cases of tests/exact_cases.py are sound before a GPU sees them: every accumulation stays inside the exactness budget, fp32
F.conv2d equals the float64 reference bit for bit (so no summation order can matter), the large cases put enough of their outputs on
roundings and on exact ties for a store that is not round-to-nearest-even to show, and one operand element changed by one quantum changes
the expected output (so equality would notice a single wrong element).  For every case the budget (log2 quanta) and the three shares of
every 16-bit store are printed (`pytest -s`).  The edge cases (Case.regime: saturated fp16 stores, subnormal operands and stores) meet
their regime's conditions instead of the rounded / tie shares, and test_edge_mutants_differ shows for each that a store without the
clamp, a bf16 store with it, a flushed subnormal result or operand, or a store that cuts instead of rounding would change the expected
output."""
import pytest
import torch

import exact_cases as ec            # tests/exact_cases.py

MIN_OUTPUTS = 10_000                 # smaller cases are exempt from the share conditions (their shares are printed)
MIN_NONZERO, MIN_ROUNDED, MIN_TIES = 0.40, 0.10, 0.02
BIG_SATURATED, BIG_EACH_SIGN, BIG_BETWEEN = (0.10, 0.70), 0.03, 0.20          # shares of a `big` store: |sum| > 65504; each sign without a ReLU; neither zero nor saturated
SUB_OPERANDS, SUB_NONZERO, SUB_ROUNDED, SUB_TIES = 0.9, 0.30, 0.10, 0.02      # of the non-zero named operands subnormal; of a store subnormal and non-zero | and rounded | and an exact tie


def _stored_layers(case):
    """the layer index of each 16-bit store"""
    return [i for i, L in enumerate(case.layers) if not L.f32]


def _edge_shares(case, stored, sums):
    """per 16-bit store of an edge case, the shares its regime's conditions are about -- of the reference alone"""
    out = []
    for s, y in zip(stored, sums):
        mean = lambda m: float(m.double().mean())
        if case.regime == 'big':
            out.append({'saturated': mean(y.abs() > ec.F16_MAX), 'saturated+': mean(y > ec.F16_MAX), 'saturated-': mean(y < -ec.F16_MAX),
                        'between': mean((s != 0) & (y.abs() <= ec.F16_MAX))})
        else:
            sub = (s != 0) & (s.abs() < ec.F16_MIN_NORMAL)
            mirror = 2 * y - s
            tie = (s != y) & (ec.r16(mirror, case.dt) == mirror)
            out.append({'subnormal': mean(sub), 'subnormal rounded': mean(sub & (s != y)), 'subnormal ties': mean(sub & tie),
                        'of the non-zero subnormal': float(sub.sum()) / max(float((s != 0).sum()), 1.0)})
    return out


def _window(case):
    """The case on the top-left window of its last image (all channels): everything one changed element near the origin reaches, and
    the window's outputs away from its cut edges are the case's own.  The window's output size is even (a half-size residual fits)."""
    x = case.x[:1] if case.family == 'worklist' else case.x[-1:]          # (a work-list case's last image is the constant crop)
    L0 = case.layers[0]
    k, up = L0.w.shape[2], L0.in_up
    size = 20 if len(case.layers) > 1 else 2 * k + 6
    out_len = lambda n: ((n << up) + 2 * L0.pad - k) // L0.stride + 1
    cut = []
    for full in x.shape[2:]:
        n = min(full, size)
        if n < full and len(case.layers) == 1 and out_len(n) % 2:
            n += 1
        cut.append(n)
    x = x[:, :, :cut[0], :cut[1]]
    layers = []
    for L in case.layers:
        r = L.res
        if r is not None:
            ho, wo = (out_len(cut[0]), out_len(cut[1])) if len(case.layers) == 1 else cut
            half = r.shape[2] < (out_len(case.x.shape[2]) if len(case.layers) == 1 else case.x.shape[2])
            r = r[-1:, :, :(ho + 1) // 2, :(wo + 1) // 2] if half else r[-1:, :, :ho, :wo]
        layers.append(L.but(res=r))
    return case.with_(x=x, layers=layers)


def _alive(t):
    """the channels of an NCHW tensor that are not zero everywhere"""
    return (t != 0).any(dim=3).any(dim=2).any(dim=0).nonzero().flatten()


def _pick(choices, g):
    return int(choices[int(torch.randint(0, len(choices), (1,), generator=g))])


def _perturbed(base, what, g, outputs):
    """-> the window case `base` with one element changed by one quantum.  The changed weight sits at a seeded random position among
    those an output can show at all: its output channel and (behind the first layer) its input channel are alive -- with a bias of -1
    and a short K the ReLU leaves some channels zero everywhere -- and on a map smaller than the kernel it is the centre tap (the
    others may only ever meet padding).  outputs: per layer, what the base case's layer produces."""
    x2, layers2 = base.x.clone(), list(base.layers)
    if what == 'weight':
        li = int(torch.randint(0, len(layers2), (1,), generator=g))
        L = layers2[li]
        w2 = L.w.clone()
        co = _pick(_alive(outputs[li]), g)
        ci = _pick(_alive(outputs[li - 1]), g) if li else int(torch.randint(0, w2.shape[1], (1,), generator=g))
        kh, kw = (int(torch.randint(0, s, (1,), generator=g)) for s in w2.shape[2:])
        if base.name.startswith('centre_tap') or min(base.x.shape[2:]) << L.in_up < w2.shape[2]:
            kh, kw = w2.shape[2] // 2, w2.shape[3] // 2
        w2[co, ci, kh, kw] += L.wq
        layers2[li] = L.but(w=w2)
    elif what == 'border pixel':
        x2[0, int(torch.randint(0, x2.shape[1], (1,), generator=g)), 0, 0] += base.xq
    else:                                        # a pixel in the last 64-channel chunk (the last channel), away from the window's cut edges
        yy, xx = (int(torch.randint(0, max(s - 8, 1), (1,), generator=g)) for s in x2.shape[2:])
        x2[0, -1, yy, xx] += base.xq
    return base.with_(x=x2, layers=layers2)


# Cases in which one changed element reaches a handful of outputs only, so that one quantum can fall into the dead zone of a ReLU or of a
# rounding at some positions: maps of at most 64 pixels, and cases of pointwise layers only (one pixel reaches Cout outputs; the Gaussian
# tail's one output channel sits behind 16 -> 16 -> 1).
def _few_outputs(case):
    hw = case.x.shape[2] * case.x.shape[3]
    pointwise = all(L.w.shape[2] == 1 for L in case.layers)
    return hw <= 64 or pointwise


@pytest.mark.parametrize('cid', ec.IDS_ALL)
def test_case_is_sound(cid):
    case = ec.case(cid)
    macs = sum(L.w.numel() for L in case.layers) * case.x.shape[2] * case.x.shape[3] * (4 if case.layers[0].in_up else 1) // case.layers[0].stride ** 2
    if macs * case.keep > 3e8:                   # a float64 conv of seconds: one image of the batch (the last)
        case = case.with_()
        case.keep = 1
    # 1. the budget (operands on their grids are checked on the way)
    log2q, q = case.budget()
    ref, stored, sums = case.reference(sums=True)
    per_layer = ec.shares(case, stored, sums)
    cov = ec.covered(case)
    print(f'\n{cid}: budget 2^{log2q:.1f} quanta of {q:g}' + ('' if per_layer else '; no 16-bit store'))
    for i, sh in enumerate(per_layer):
        print(f'  store {i}{" (covered)" if i in cov else ""}: non-zero {sh[0]:.3f} rounded {sh[1]:.3f} ties {sh[2]:.3f} of {sh[3]} values')
    nonzero = float((ref != 0).double().mean())
    print(f'  final output: {ref.numel()} values, non-zero {nonzero:.3f}')
    assert log2q <= ec.BUDGET_LOG2, (cid, log2q)
    if ref.numel() >= MIN_OUTPUTS:
        assert nonzero >= MIN_NONZERO, (cid, nonzero)
    # 2. fp32 equals float64: no partial sum needed a rounding in the order F.conv2d takes, and by the budget in no other order
    ref32, _ = case.reference(torch.float32)
    assert torch.equal(ref32.double(), ref)
    assert bool(torch.isfinite(ref).all())
    # 3. conditions on the inputs, for every store the case answers for ON ITS OWN (a fused case names them in Case.covers; test_every_
    #    fused_store_is_exercised shows that the variants of a chain leave no store out): enough of its values are non-zero, need a
    #    rounding, sit on an exact tie
    #    An edge case (Case.regime) answers for an edge of fp16 instead: the regime conditions of _edge_shares
    assert cov <= set(range(len(per_layer)))
    edge = _edge_shares(case, stored, sums) if case.regime else None
    for i in sorted(cov):
        sh = per_layer[i]
        if edge is not None:
            print(f'  store {i} {case.regime}: ' + ' '.join(f'{k} {v:.3f}' for k, v in edge[i].items()))
        if sh[3] < MIN_OUTPUTS:
            continue
        if edge is None:
            assert sh[0] >= MIN_NONZERO and sh[1] >= MIN_ROUNDED and sh[2] >= MIN_TIES, (cid, i, sh)
        elif case.regime == 'big':
            e = edge[i]
            assert BIG_SATURATED[0] <= e['saturated'] <= BIG_SATURATED[1] and e['between'] >= BIG_BETWEEN, (cid, i, e)
            if not case.layers[_stored_layers(case)[i]].act:
                assert min(e['saturated+'], e['saturated-']) >= BIG_EACH_SIGN, (cid, i, e)
        else:
            e = edge[i]
            assert e['subnormal'] >= SUB_NONZERO and e['subnormal rounded'] >= SUB_ROUNDED and e['subnormal ties'] >= SUB_TIES, (cid, i, e)
            if _stored_layers(case)[i] + 1 < len(case.layers):          # what the next layer reads from this store
                assert e['of the non-zero subnormal'] >= SUB_OPERANDS, (cid, i, e)
    if case.regime and case.regime != 'big':
        named = case.named_operands()
        assert named
        for t in named:
            share = float((t[t != 0].abs() < ec.F16_MIN_NORMAL).double().mean())
            print(f'  named operand: of the non-zero values subnormal {share:.3f}')
            assert share >= SUB_OPERANDS, (cid, share)
    # 4. one element changed by one quantum changes the expected output: at four seeded positions of each kind, every one of them --
    #    except in the cases of FEW_OUTPUTS, where at least one must (the count is printed)
    g = ec.seeded('perturb', cid)
    base = _window(case)
    a, mids = base.reference()
    outputs = mids + ([a] if base.layers[-1].f32 else [])
    assert len(outputs) == len(base.layers)
    for what in ('weight', 'border pixel', 'last-chunk pixel'):
        shown = sum(not torch.equal(a, _perturbed(base, what, g, outputs).reference()[0]) for _ in range(4))
        print(f'  one {what} changed by a quantum: visible in {shown} of 4')
        assert shown >= (1 if _few_outputs(case) else 4), (cid, what, shown)


def test_every_fused_store_is_exercised():
    """Per fused chain (family, shape, storage type): the stores its variants answer for are all of its stores, except those of
    exact_cases.NOT_EXERCISED, which no case can exercise inside the budget."""
    groups = {}
    for cid in ec.IDS_ALL:
        family, name, dt = cid.split('/')
        if cid in ec.EDGE_IDS:
            continue                    # (test_every_fused_store_meets_both_edges)
        if family not in ('vgg_stem', 'gauss_tail', 'gauss_subnet', 'bneck') or (family == 'gauss_subnet' and name.startswith('1x1x1_')):
            continue                    # (the subnet on one pixel stores 128 values a layer: far below what a share means anything for)
        base = name[:-len('_early')] if name.endswith('_early') else name
        groups.setdefault((family, base, dt), []).append(cid)
    assert len(groups) > 20
    for (family, base, dt), cids in groups.items():
        cases = [ec.BUILDERS[c]() for c in cids] if family != 'bneck' else None
        if family == 'bneck':                                   # (their tensors are large: the variants' declarations are enough here)
            cin, p = (int(v) for v in base.split('x')[0].split('-'))
            got = set().union(*[set(cov) for _, _, cov in ec.bneck_variants(ec.H16 if dt == 'fp16' else ec.BF, cin, p)])
            stores, planes = 3, p
        else:
            got = set().union(*[ec.covered(c) for c in cases])
            stores, planes = sum(1 for L in cases[0].layers if not L.f32), None
        missing = set(range(stores)) - got
        allowed = ec.NOT_EXERCISED.get((family, ec.H16 if dt == 'fp16' else ec.BF, planes), set())
        assert missing == allowed, (family, base, dt, missing)


def test_every_fused_store_meets_both_edges():
    """Per fused chain shape among the edge cases: its `big` cases together cover every 16-bit store, and in fp16 its `sub` cases do
    too -- except the stores that exact_cases.NOT_EXERCISED_EDGE names with their measured budget (none: the table is empty)."""
    groups = {}
    for cid in ec.EDGE_IDS:
        family, name, dt = cid.split('/')
        if family in ('vgg_stem', 'gauss_tail', 'gauss_subnet', 'bneck'):
            base, regime = name.rsplit('_', 1)
            groups.setdefault((family, base, dt, regime), []).append(cid)
    shapes = {k[:3] for k in groups}
    assert len(shapes) == 11 and all((*s, 'big') in groups for s in shapes) and all((*s, 'sub') in groups for s in shapes if s[2] == 'fp16')
    for (family, base, dt, regime), cids in groups.items():
        cases = [ec.BUILDERS[c]() for c in cids]
        assert all(c.regime == regime for c in cases)
        stores = len(_stored_layers(cases[0]))
        planes = int(base.split('x')[0].split('-')[1]) if family == 'bneck' else None
        allowed = ec.NOT_EXERCISED_EDGE.get((family, ec.H16 if dt == 'fp16' else ec.BF, planes, regime), (set(), None))[0]
        assert set(range(stores)) - set().union(*[ec.covered(c) for c in cases]) == set(allowed), (family, base, dt, regime)


@pytest.mark.parametrize('cid', ec.EDGE_IDS)
def test_edge_mutants_differ(cid):
    """A wrong model of the store or of the multiply changes the expected output of every edge case -- so the equality of test_gpu_exact.py
    can fail on a kernel that does the same: (a) big, fp16: a store without the clamp (infinity); (b) big, bf16: a store with fp16's clamp
    (an fp32 output: that output clamped, in both types); (c) sub: a subnormal stored value flushed to zero; (d) sub: subnormal operands
    flushed to zero before the multiply; (e) sub: a store that cuts towards zero below 2^-14 instead of rounding.  In a chain the wrong
    store stands at one covered store at a time, and (d) at the layer that reads it (and at the first layer); each must show in the
    final output."""
    case = ec.case(cid).with_()
    case.keep = 1
    ref = case.reference()[0]
    layers = _stored_layers(case)
    differs = lambda *mutant: not torch.equal(case.reference(mutant=mutant)[0], ref)
    tried = 0
    if case.regime == 'big':
        if case.layers[-1].f32 and len(case.layers) == 1:
            assert float(ref.abs().max()) > ec.F16_MAX and differs(0, 'clamp'), cid
            tried += 1
        for i in sorted(ec.covered(case)):
            assert differs(layers[i], 'noclamp' if case.dt == ec.H16 else 'clamp'), (cid, i)
            tried += 1
    else:
        assert case.dt == ec.H16
        assert differs(0, 'operands'), cid
        tried += 1
        for i in sorted(ec.covered(case)):
            assert differs(layers[i], 'flush'), (cid, i, 'flush')
            assert differs(layers[i], 'trunc'), (cid, i, 'trunc')
            if layers[i] + 1 < len(case.layers):
                assert differs(layers[i] + 1, 'input'), (cid, i, 'input')
            tried += 1
    assert tried
    if case.regime == 'big' and case.dt == ec.H16 and layers and layers[-1] == len(case.layers) - 1:
        assert not bool(torch.isfinite(case.reference(mutant=(layers[-1], 'noclamp'))[0]).all()), cid
