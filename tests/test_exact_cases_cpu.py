"""The cases of tests/exact_cases.py are sound before a GPU sees them: every accumulation stays inside the exactness budget, fp32
F.conv2d equals the float64 reference bit for bit (so no summation order can matter), the large cases put enough of their outputs on
roundings and on exact ties for a store that is not round-to-nearest-even to show, and one operand element changed by one quantum changes
the expected output (so equality would notice a single wrong element).  For every case the budget (log2 quanta) and the three shares of
every 16-bit store are printed (`pytest -s`)."""
import pytest
import torch

import exact_cases as ec            # tests/exact_cases.py

MIN_OUTPUTS = 10_000                 # smaller cases are exempt from the share conditions (their shares are printed)
MIN_NONZERO, MIN_ROUNDED, MIN_TIES = 0.40, 0.10, 0.02


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
        layers.append(ec.Layer(L.w, L.b, L.wq, L.stride, L.pad, L.act, L.f32, L.in_up, L.pool, r))
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
        layers2[li] = ec.Layer(w2, L.b, L.wq, L.stride, L.pad, L.act, L.f32, L.in_up, L.pool, L.res)
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
    assert cov <= set(range(len(per_layer)))
    for i in sorted(cov):
        sh = per_layer[i]
        if sh[3] >= MIN_OUTPUTS:
            assert sh[0] >= MIN_NONZERO and sh[1] >= MIN_ROUNDED and sh[2] >= MIN_TIES, (cid, i, sh)
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
