"""The embedder's schedule, launch by launch, checked on the host against the committed table tests/embed_schedule.json
(tests/embed_schedule.py: the recorder that notes which tensor every op got, the cases, `--write`).  The table was written from the
code that preceded the typed schedule of cvpce_amd/ops.py (`SkipMode`, `SkipLayer`, `WorkLists`) and models/classification.py
(`SkipSchedule`, `SkipStep`); it changes only with a change that means to change a launch, a list row or a record."""
import pytest

import embed_schedule as es


@pytest.fixture(scope='module')
def table():
    return es.load_table()


@pytest.fixture(scope='module')
def got():
    return es.replay(profile=True)


def test_schedule_matches_the_table(table, got):
    assert list(got) == list(table)
    for name, want in table.items():
        assert set(got[name]) == set(want), name
        for part in ('plan', 'modes', 'calls', 'records'):
            assert got[name][part] == want[part], (name, part)


def test_same_launches_without_a_profile(table):
    got = es.replay(profile=False)
    for name, want in table.items():
        assert got[name]['calls'] == want['calls'] and got[name]['plan'] == want['plan'] and got[name]['modes'] == want['modes'], name


def test_table_has_every_case(table):
    assert len(table[es.DEFAULT]['calls']) == 95
    assert list(table) == [c['name'] for c in es.CASES]
    names = ' | '.join(table)
    for word in ('N = 37', 'N = 1', 'N = 5', 'N = 0', 'want_bf16', 'vgg16_bn', 'SKIP_ROWS off', 'SKIP_MAC off', 'SKIP_STRIPS off', 'SKIP_FINE off',
                 'SKIP_FINE_PARTS ()', "SKIP_FINE_PARTS ('halo2',)", "SKIP_FINE_PARTS ('halo3',)", "SKIP_FINE_PARTS ('halo3', 'halo2', 'thin')",
                 'SKIP_PADDING off', 'USE_FUSED_MAC off', 'USE_FUSED_STEM off', 'partial', 'wide after 16x16', 'early 1', 'second call'):
        assert word in names, word
    ops_of = lambda name: {c[0] for c in table[name]['calls']}
    # what each case is there for
    assert table['cfg: wide after 16x16']['plan'] is not None and 'copy_' not in ops_of('cfg: wide after 16x16')
    assert sum(c[0] == 'embed_worklists' for c in table['cfg: wide after 16x16']['calls']) == 5           # everything in passes: no late pass
    assert sum(c[0] == 'embed_worklists' for c in table[es.DEFAULT]['calls']) == 5 + 2
    assert table['ops.USE_FUSED_MAC off']['plan'] is None and 'global_max_nhwc' in ops_of('ops.USE_FUSED_MAC off')
    assert table['SKIP_PADDING off']['plan'] is not None and 'embed_worklists' not in ops_of('SKIP_PADDING off')
    assert 'vgg_stem_fused' not in ops_of('USE_FUSED_STEM off, 8 channels, N = 5')
    assert table['default, N = 0']['calls'] == []
    assert 'conv3x3_halo_strips2' in ops_of(es.DEFAULT) and 'conv3x3_halo_strips2' not in ops_of("SKIP_FINE_PARTS ('halo2',)")
    assert 'conv3x3_halo_strips' not in ops_of('SKIP_STRIPS off') and 'mac_init' not in ops_of('SKIP_MAC off')
    assert table['vgg16_bn']['calls'] == table[es.DEFAULT]['calls']                                        # (BatchNorm is folded into the weights)
    # the second call leaves out only the constant crop's pass through the plain kernels (`mac_tables`)
    first, second = table[es.DEFAULT]['calls'], table['second call on the same engine']['calls']
    at = [c[0] for c in first].index('embed_worklists')
    assert at > 0 and second == first[at:]


def test_every_list_row_and_count_slot_is_used(table):
    """Over the default case: after every `embed_worklists` call, the launches up to the next one take every row of `lists` and every
    slot of `counts` that the packed layout gives the call's layers (main lists in rows j, strip lists k + j, thin lists 2 k + j; tiles at
    j, MFMA units k + j, strip entries 2 k + j, thin entries 3 k + j), and no other.  The units are read by the profile's records only,
    and a layer with strips files a difference, a new tensor: their slots show for the layers without strip lists."""
    calls, records = table[es.DEFAULT]['calls'], table[es.DEFAULT]['records']
    starts = [i for i, c in enumerate(calls) if c[0] == 'embed_worklists'] + [len(calls)]
    listed = {'vgg_stem_fused_list', 'conv3x3_halo_list', 'conv3x3_halo_strips', 'conv3x3_halo_strips2'}
    unit_slots = {v[1] for r in records for v in r[2:] if isinstance(v, list) and v[0] == [1]}
    seen_thin = seen_strips = 0
    for a, b in zip(starts, starts[1:]):
        _, (_, lists, counts, _), scalars = calls[a]
        flat = [s for s in scalars if isinstance(s, list)][0]
        modes, in_ops, k = flat[8::9], flat[7::9], len(flat) // 9
        stride = lists[0][1]
        assert lists[0][0] == (3 if 5 in modes else 2) * k and counts[0] == [(4 if 5 in modes else 3) * k]
        want_rows = {j for j in range(k)} | {k + j for j in range(k) if modes[j] in (3, 5)} | {2 * k + j for j in range(k) if modes[j] == 5}
        want_slots = {j for j in range(k)} | {2 * k + j for j in range(k) if modes[j] in (3, 5)} | {3 * k + j for j in range(k) if modes[j] == 5}
        rows, slots = set(), set()
        for name, tensors, _ in calls[a + 1:b]:
            if name in listed:
                (wshape, woff), (cshape, coff) = tensors[-2:]
                assert wshape == [stride] and woff % stride == 0 and cshape == [1]
                rows.add(woff // stride)
                slots.add(coff)
        assert rows == want_rows and slots == want_slots, (a, rows, want_rows, slots, want_slots)
        for j in range(k):
            if modes[j] not in (3, 5) and in_ops[j] != 0:           # (a conv layer without strips; the stem files its tile count)
                assert k + j in unit_slots, (a, j)
        seen_strips += any(m in (3, 5) for m in modes)
        seen_thin += 5 in modes
    assert seen_strips and seen_thin


def test_batchnorm_fold_is_the_arithmetic_it_was():
    """The eval-mode BatchNorm folded into the packed weights: scale = weight * (var + eps).rsqrt(), shift = bias - mean * scale, in
    that order -- the convs' and the stem's packed weights and biases, bit for bit."""
    import torch
    from torch import nn
    from cvpce_amd import ops
    from cvpce_amd.models import classification as C
    model = es._model('vgg16_bn')
    eng = C.MACVGGEngine(model, torch.device('cpu'))
    mods = list(model.block1) + list(model.block2)
    pairs = [(m, mods[i + 1]) for i, m in enumerate(mods) if isinstance(m, nn.Conv2d)]
    assert all(isinstance(bn, nn.BatchNorm2d) for _, bn in pairs) and len(pairs) == 13
    with torch.no_grad():
        folded = []
        for conv, bn in pairs[:2]:
            sc = (bn.weight * (bn.running_var + bn.eps).rsqrt()).float()
            folded += [conv.weight.float() * sc[:, None, None, None], conv.bias.float() * sc + (bn.bias.float() - bn.running_mean.float() * sc)]
        stem = ops.PackedStem(*folded, device='cpu')
        for name in ('w1', 'b1', 'w2', 'b2'):
            assert torch.equal(getattr(eng.stem, name), getattr(stem, name)), name
        convs = [pc for kind, pc in eng.plan if pc is not None]
        assert len(convs) == 11
        for (conv, bn), pc in zip(pairs[2:], convs):
            scale = bn.weight * (bn.running_var + bn.eps).rsqrt()
            want = ops.PackedConv(conv.weight, conv.bias, 1, 1, scale=scale, shift=bn.bias - bn.running_mean * scale, device='cpu')
            assert torch.equal(pc.weight, want.weight) and torch.equal(pc.bias, want.bias) and torch.equal(pc.weight_halo, want.weight_halo)
