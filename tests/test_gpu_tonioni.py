"""The Tonioni matcher on the GPU: the matchings equal the host `tonioni_mcs` pair by pair in growth order, every start's (M, F)
equals `tonioni_cases.model_tonioni`'s, the launches write only their workspace, pairs and counts, an image over the limit takes
the host path, and the comparator gives the host route's verdicts and reports on every device route at the waits of
matcher='large'."""
import re

import pytest
import torch

import footprint
import planogram_device_cases as cases
import tonioni_cases as tc
from cvpce_amd import planograms
from test_gpu_cli import _run, world  # noqa: F401  (the synthetic on-disk set of the command-line tests, as a fixture of this module too)

pytestmark = pytest.mark.gpu


def _device_graph(pd, tables, labels, cuda):
    return pd.Graph(labels, *(t.to(cuda) for t in tables))


@pytest.fixture(scope='module')
def fixture_pairs(cuda, golden_dir):
    """every fixture case: its host graphs, the same graphs in table form on the device, and the host's pairs in growth order"""
    from cvpce_amd import planograms_device as pd
    out = []
    for c in tc.golden(golden_dir):
        g1, g2 = planograms.build_graph(c['boxes1'], c['labels1']), planograms.build_graph(c['boxes2'], c['labels2'])
        t1, t2 = tc.tables_of_host(g1), tc.tables_of_host(g2)
        out.append(dict(c, t1=t1, t2=t2, d1=_device_graph(pd, t1, c['labels1'], cuda), d2=_device_graph(pd, t2, c['labels2'], cuda),
                        host=planograms.tonioni_pairs(g1, g2, min_score=c['min_score'])))
    return out


def _pairs_in_order(matching, p):
    """pair p's rows of a `DeviceMatching` as the kernel left them -> (list of pairs up to the count, the rows beyond it)"""
    count = int(matching.count[p])
    rows = matching.pairs[matching.rows[p]:matching.rows[p + 1]].cpu().tolist()
    return [tuple(r) for r in rows[:count]], rows[count:]


def test_matchings_equal_the_host_in_one_batch(cuda, fixture_pairs):
    from cvpce_amd import planograms_device as pd
    for min_score in (-0.2, -0.5):
        group = [c for c in fixture_pairs if c['min_score'] == min_score]
        sets = pd.common_subgraphs([c['d1'] for c in group], [c['d2'] for c in group], min_score=min_score, matcher='tonioni')
        matching = pd.match_on_device([c['d1'] for c in group], [c['d2'] for c in group], min_score=min_score, matcher='tonioni')
        assert len({(len(c['labels1']), len(c['labels2'])) for c in group}) > 1 or len(group) < 3       # mixed sizes in one batch
        for p, (c, found) in enumerate(zip(group, sets)):
            pairs, beyond = _pairs_in_order(matching, p)
            assert pairs == c['host'], c['name']
            assert all(r == [-1, -1] for r in beyond), c['name']
            assert sorted(found) == c['tonioni'] and list(found) == list(planograms.tonioni_mcs(pd.to_networkx(c['d1']), pd.to_networkx(c['d2']),
                                                                                               min_score=min_score)), c['name']
    # stop_at_fraction has no meaning for this search
    c = fixture_pairs[0]
    assert pd.common_subgraphs([c['d1']], [c['d2']], stop_at_fraction=0.0, matcher='tonioni')[0] == set(c['host'])
    with pytest.raises(ValueError):
        pd.common_subgraphs([c['d1']], [c['d2']], matcher='other')


@pytest.mark.parametrize('n', (7, 26, 65))
def test_matchings_on_graphs_built_on_the_device(cuda, n):
    """tie-free scenes: the device graph is the host graph, so the whole device route equals the whole host route"""
    from cvpce_amd import planograms_device as pd
    eb, el = cases.scene(n, cases.TIE_FREE_SEEDS[n])
    el = [cases.NAMES[i % 3] for i in range(n)]                                     # few labels, many equal-label pairs
    keep = [i for i in range(n) if i % 9 != 4]
    ab, al = (eb + torch.tensor([30.0, 12.0, 30.0, 12.0]))[keep].contiguous(), [el[(i + 1) % n] if i % 5 == 3 else el[i] for i in keep]
    assert cases.is_tie_free(ab)
    ge, ga = pd.build_graphs([(eb, el), (ab, al)], 0.5, device=cuda)
    he, ha = planograms.build_graph(eb, el, 0.5), planograms.build_graph(ab, al, 0.5)
    for min_score in (-0.2, 0.0):
        want = planograms.tonioni_pairs(he, ha, min_score=min_score)
        matching = pd.match_on_device([ge], [ga], min_score=min_score, matcher='tonioni')
        assert _pairs_in_order(matching, 0)[0] == want and int(matching.count[0]) == len(want), min_score
        # (the 7 scattered boxes have no pair of hypotheses that agree in two directions: an empty set at the default min_score)
        assert len(want) >= 2 or (n == 7 and min_score == -0.2 and not want)


def _per_start(cuda, t1, l1, t2, l2, min_score=-0.2):
    from cvpce_amd import planograms_device as pd
    matching = pd.match_on_device([_device_graph(pd, t1, l1, cuda)], [_device_graph(pd, t2, l2, cuda)], min_score=min_score, matcher='tonioni')
    return matching, matching.launch.per_start(0).cpu().tolist()


def _shelf_6x10():
    b1, l1 = tc.shelf(6, 10, 3)
    b2, l2 = tc.detections_of(b1, l1, 41, tc.NAMES[:3])
    return cases.model_graph(b1), l1, cases.model_graph(b2), l2


@pytest.mark.parametrize('which', ('below_64', 'between_256_and_1024', 'shelf_6x10'))
def test_per_start_values_equal_the_model(cuda, fixture_pairs, which):
    if which == 'shelf_6x10':
        t1, l1, t2, l2 = _shelf_6x10()
    else:
        lo, hi = (1, 63) if which == 'below_64' else (257, 1023)
        c = next(c for c in fixture_pairs if lo <= c['hypotheses'] <= hi and c['tonioni'])
        t1, l1, t2, l2 = c['t1'], c['labels1'], c['t2'], c['labels2']
    pairs, mf, start, _ = tc.model_tonioni(t1, l1, t2, l2)
    matching, got = _per_start(cuda, t1, l1, t2, l2)
    h = len(mf)
    print(f'{which}: H {h}, adopted start {start}, size {len(pairs)}, longest run {max(f for _, f in mf.values())}')
    if which == 'shelf_6x10':
        assert 1000 < h < 1500 and max(f for _, f in mf.values()) > 40
    assert len(got) == h and [tuple(r) for r in got] == [mf[i] for i in range(h)]
    assert _pairs_in_order(matching, 0)[0] == pairs
    hyp = matching.launch.workspace[:h].cpu().tolist()                              # the hypotheses themselves, in the match kernel's order
    agree, x1, x2 = tc.hypotheses_of(t1[0], l1, t2[0], l2)
    assert hyp == [(int(a) << 20) | (int(i) << 10) | int(j) for a, i, j in zip(agree, x1, x2)]
    assert int(matching.launch.workspace[3 * h]) == h


def test_near_the_limit(cuda):
    """two graphs of one label with n1 * n2 hypotheses = the limit: 32 sampled starts against the model, and the output"""
    from cvpce_amd import planograms_device as pd
    b1, l1 = tc.shelf(8, 16, 1)
    b2, l2 = tc.detections_of(b1, l1, 5, tc.NAMES[:1], drop=0.0, mislabel=0.0)
    assert len(l1) * len(l2) == pd.TONIONI_MAX_HYPOTHESES
    t1, t2 = cases.model_graph(b1), cases.model_graph(b2)
    h = pd.TONIONI_MAX_HYPOTHESES
    starts = sorted({0, h - 1} | set(range(500, h, (h - 500) // 29)))[:31] + [h - 1]
    assert len(set(starts)) == 32
    _, mf, _, _ = tc.model_tonioni(t1, l1, t2, l2, starts=set(starts))
    matching, got = _per_start(cuda, t1, l1, t2, l2)
    assert len(got) == h
    for i in set(starts):
        assert tuple(got[i]) == mf[i], i
    arg, size = tc.choose(got, h)
    rerun = tc.model_run(*(v[arg:] for v in tc.hypotheses_of(t1[0], l1, t2[0], l2)), t1[0].numpy().astype('int64'), t2[0].numpy().astype('int64'),
                         tc.score8_limit(-0.2))
    pairs, _ = _pairs_in_order(matching, 0)
    print(f'adopted start {arg}, size {size}')
    assert int(matching.count[0]) == len(rerun[0]) == size and pairs == rerun[0]
    # one more hypothesis is refused, by the Python surface and by the entry point
    b3, l3 = tc.shelf(8, 17, 1)
    big = pd.build_graphs([(b3, l3)], 0.5, device=cuda)[0]
    with pytest.raises(ValueError):
        pd.match_on_device([big], [_device_graph(pd, t2, l2, cuda)], matcher='tonioni')
    launch = matching.launch
    with pytest.raises(RuntimeError):
        launch.run._replace(max_hyp=h + 1).launch()
    with pytest.raises(RuntimeError):
        launch.select._replace(max_hyp=h + 1).launch()


def _plano(boxes, labels):
    return {'boxes': boxes, 'labels': labels}


def test_over_the_limit_takes_the_host_path(cuda, monkeypatch):
    from cvpce_amd import planograms_device as pd, production
    scenes = [tc.window_scene(i) for i in range(3)]
    host = production.PlanogramComparator(matcher='tonioni')
    want = [float(host.compare(_plano(b1, l1), _plano(b2, l2))) for b1, l1, b2, l2 in scenes]
    counts = [pd.hypothesis_count(l1, l2) for _, l1, _, l2 in scenes]
    limit = sorted(counts)[1]                                                       # the largest of the three is over it
    monkeypatch.setattr(pd, 'TONIONI_MAX_HYPOTHESES', limit)
    for switches in (dict(), dict(device_tail=True)):
        dev = production.PlanogramComparator(device_graphs=True, matcher='tonioni', **switches)
        got = dev.compare_batch([_plano(b1, l1) for b1, l1, _, _ in scenes], [_plano(b2, l2) for _, _, b2, l2 in scenes])
        assert dev.host_routed == sum(c > limit for c in counts) == 1
        assert float(got[counts.index(max(counts))]) == want[counts.index(max(counts))]
    large = production.PlanogramComparator(device_graphs=True)
    large.compare_batch([_plano(b1, l1) for b1, l1, _, _ in scenes], [_plano(b2, l2) for _, _, b2, l2 in scenes])
    assert large.host_routed == 0                                                   # the limit is the Tonioni matcher's alone


def test_footprint_of_both_launches(cuda, fixture_pairs):
    """two pairs of different sizes: only workspace, pairs and count are written, within their extents, under every fill"""
    from cvpce_amd import planograms_device as pd, torch_ops_tonioni
    picked = [c for c in fixture_pairs if c['name'] in ('grid3x8_k5_s0', 'grid2x6_k7_s2')]
    assert len(picked) == 2
    n1, n2 = [len(c['labels1']) for c in picked], [len(c['labels2']) for c in picked]
    ids = {}
    lab1 = torch.tensor([ids.setdefault(l, len(ids)) for c in picked for l in c['labels1']], dtype=torch.int32)
    lab2 = torch.tensor([ids.setdefault(l, len(ids)) for c in picked for l in c['labels2']], dtype=torch.int32)
    hyps = [c['hypotheses'] for c in picked]
    rows = [min(a, b) for a, b in zip(n1, n2)]
    i32 = lambda v: footprint.put(torch.tensor(v, dtype=torch.int32), cuda)
    nbr1, nbr2 = (footprint.put(torch.cat([c[k][0] for c in picked]).contiguous(), cuda) for k in ('t1', 't2'))
    l1, l2 = footprint.put(lab1, cuda), footprint.put(lab2, cuda)
    off1, off2, params = i32([0, n1[0], sum(n1)]), i32([0, n2[0], sum(n2)]), i32([pd.score8_limit(-0.2)] * 2)
    hyp_off, out_off = i32([0, hyps[0], sum(hyps)]), i32([0, rows[0], sum(rows)])
    words = torch_ops_tonioni.workspace_words(sum(hyps), 2)
    assert words == 3 * sum(hyps) + 2
    work = footprint.out((words,), torch.int32, cuda)
    run = lambda: torch.ops.cvpce_amd.tonioni_run(nbr1[0], l1[0], off1[0], nbr2[0], l2[0], off2[0], params[0], hyp_off[0], max(n1), max(n2),
                                                  max(hyps), sum(hyps), work[0])
    ins = [nbr1, l1, off1, nbr2, l2, off2, params, hyp_off]
    got_work, = footprint.check(run, ins, [work], written=[None])                   # every word: hypotheses, (M, F) of every start, counts
    assert got_work[3 * sum(hyps):].tolist() == hyps
    kept = footprint.put(got_work.cpu(), cuda)
    pairs, count = footprint.out((sum(rows), 2), torch.int32, cuda), footprint.out((2,), torch.int32, cuda)
    select = lambda: torch.ops.cvpce_amd.tonioni_select(nbr1[0], off1[0], nbr2[0], off2[0], params[0], hyp_off[0], out_off[0], max(n1), max(n2),
                                                        max(hyps), sum(hyps), kept[0], pairs[0], count[0])
    got_pairs, got_count = footprint.check(select, [nbr1, off1, nbr2, off2, params, hyp_off, out_off, kept], [pairs, count])
    got_pairs, at = got_pairs.cpu().tolist(), 0
    for c, r, k in zip(picked, rows, got_count.tolist()):
        assert [tuple(p) for p in got_pairs[at:at + k]] == c['host'] and all(p == [-1, -1] for p in got_pairs[at + k:at + r]), c['name']
        at += r
    # a launch sized by a bound: slices longer than the real counts -- the starts beyond a pair's count are not written
    bound = [h + 37 for h in hyps]
    hyp_off2 = i32([0, bound[0], sum(bound)])
    work2 = footprint.out((torch_ops_tonioni.workspace_words(sum(bound), 2),), torch.int32, cuda)
    run2 = lambda: torch.ops.cvpce_amd.tonioni_run(nbr1[0], l1[0], off1[0], nbr2[0], l2[0], off2[0], params[0], hyp_off2[0], max(n1), max(n2),
                                                   max(bound), sum(bound), work2[0])
    mask = torch.zeros(work2[0].numel(), dtype=torch.bool)
    for o, h in zip((0, bound[0]), hyps):
        mask[o:o + h] = True
        mask[sum(bound) + 2 * o:sum(bound) + 2 * (o + h)] = True
    mask[3 * sum(bound):] = True
    got2, = footprint.check(run2, ins[:7] + [hyp_off2], [work2], written=[mask])
    assert got2[3 * sum(bound):].tolist() == hyps


def _window(cuda):
    """the window of tests/test_gpu_reclass.py's pipeline twice over: 8 scenes of 6 labels, two ways of withholding detections"""
    from test_gpu_reclass import _pipeline, _planograms
    p = _pipeline(cuda)
    imgs, dets = p['imgs'] * 2, p['dets'] * 2
    planos = _planograms(dets)
    actuals = []
    for k, (b, l) in enumerate(dets):
        keep = [i for i in range(len(b)) if i % 3 != (1 if k < 4 else 2)]
        actuals.append({'boxes': b[keep], 'labels': [l[i] for i in keep]})
    return p, imgs, planos, actuals


def _report_fields(r):
    return (float(r.compliance), r.status, None if r.outcomes is None else r.outcomes.tolist(), None if r.occupant is None else r.occupant.tolist(),
            r.occupant_labels, r.seen_labels, None if r.stray is None else r.stray.tolist())


def test_whole_comparator_on_every_route(cuda):
    from cvpce_amd import planograms_device as pd, production
    from test_gpu_actuals import _window_counter
    from test_gpu_reclass import _device_actuals, _same
    p, imgs, planos, actuals = _window(cuda)
    clf = p['clf']
    host = production.PlanogramComparator(matcher='tonioni')
    want = host.compare_batch(planos, actuals, imgs, clf)
    want_reports = host.report_batch(planos, actuals, imgs, clf)
    sizes = [len(planograms.tonioni_mcs(planograms.build_graph(e['boxes'], e['labels']), planograms.build_graph(a['boxes'], a['labels'])))
             for e, a in zip(planos, actuals)]
    large = [len(planograms.large_common_subgraph(planograms.build_graph(e['boxes'], e['labels']), planograms.build_graph(a['boxes'], a['labels'])))
             for e, a in zip(planos, actuals)]
    print(f'verdicts {[float(v) for v in want]}, matchings tonioni {sizes}, large {large}, '
          f'hypotheses {[pd.hypothesis_count(e["labels"], a["labels"]) for e, a in zip(planos, actuals)]}')
    assert all(r.status == 'ok' for r in want_reports) and any(0.0 < float(v) < 1.0 for v in want)
    routes = {'graphs': (dict(device_graphs=True), False), 'tail': (dict(device_graphs=True, device_tail=True), False),
              'tail_reclass': (dict(device_graphs=True, device_tail=True, device_reclass=True), False),
              'actuals': (dict(device_graphs=True, device_tail=True), True),
              'actuals_reclass': (dict(device_graphs=True, device_tail=True, device_reclass=True), True)}
    for name, (switches, on_device) in routes.items():
        waits = {}
        for matcher in ('tonioni', 'large'):
            side = _device_actuals(cuda, clf, actuals) if on_device else actuals
            fresh = [dict(boxes=e['boxes'], labels=e['labels']) for e in planos]
            cmp = production.PlanogramComparator(matcher=matcher, **switches)
            verdicts, reports = cmp.compare_batch(fresh, side, imgs, clf), cmp.report_batch(fresh, side, imgs, clf)
            counter = _window_counter()
            with counter:
                cmp.compare_batch(fresh, side, imgs, clf)
                cmp.report_batch(fresh, side, imgs, clf)
            waits[matcher] = counter.waits
            assert cmp.host_routed == 0 and cmp.reclass_host_routed == 0
            if matcher == 'tonioni':
                print(f'{name}: verdicts {[float(v) for v in verdicts]}')
                assert [float(v) for v in verdicts] == [float(v) for v in want], name
                assert [_report_fields(r) for r in reports] == [_report_fields(r) for r in want_reports], name
                if name == 'graphs':                                                # (the host's own tail on the device's matching: every bit)
                    _same(verdicts, want)
                    for r, w in zip(reports, want_reports):
                        assert torch.equal(r.expected_positions, w.expected_positions) and torch.equal(r.seen_distance, w.seen_distance)
            if matcher == 'tonioni' and not on_device:
                # without a classifier nothing is re-classified: the verdict is what the matching and the tail leave
                bare, bare_want = cmp.compare_batch(fresh, side, imgs, None), host.compare_batch(planos, actuals, imgs, None)
                print(f'{name}, no classifier: {[float(v) for v in bare]}')
                assert [float(v) for v in bare] == [float(v) for v in bare_want], name
        print(f'{name}: waits per compare_batch + report_batch: tonioni {waits["tonioni"]}, large {waits["large"]}')
        assert waits['tonioni'] == waits['large'], name


def test_device_detections_through_the_pipeline(cuda):
    """`BatchedPipeline.run(actuals=True)`: the detections never leave the device, the launch is sized by the host's bound"""
    from cvpce_amd import production
    from test_gpu_reclass import _pipeline, _planograms, _same
    p = _pipeline(cuda)
    clf, pg, imgs = p['clf'], p['pg'], p['imgs']
    planos = _planograms(p['dets'])
    host = production.PlanogramEvaluator(pg, clf, production.PlanogramComparator(matcher='tonioni'))
    want = host.evaluate_batch(imgs, planos)
    for switches in (dict(), dict(device_reclass=True)):
        make = lambda: production.PlanogramComparator(device_graphs=True, device_tail=True, matcher='tonioni', **switches)
        off, on = production.PlanogramEvaluator(pg, clf, make()), production.PlanogramEvaluator(pg, clf, make(), device_detections=True)
        got_off, got_on = off.evaluate_batch(imgs, planos), on.evaluate_batch(imgs, planos)
        print(f'{switches}: host {[float(v) for v in want]}, device detections {[float(v) for v in got_on]}')
        _same(got_on, got_off)
        assert [float(v) for v in got_on] == [float(v) for v in want]
        assert on.planogram_comparator.host_routed == 0 and on.detections_host_routed == 0
        _same([r.compliance for r in on.report_batch(imgs, planos)], got_on)


def test_cli_matcher_switch(world):
    """`eval-planograms --matcher tonioni` with every device switch prints the host route's accuracy lines, on the synthetic set of
    tests/test_gpu_cli.py"""
    common = ['eval-planograms', '--img-dir', world / 'Training', '--test-imgs', world / 'Testing', '--test-annotations', world / 'ann',
              '--planograms', world / 'plano', '--verbose']
    tail = [world / 'gln.tar', world / 'dihe.tar']
    lines = lambda out: re.findall(r'Detected accuracy: [^\n]+', out) + re.findall(r'--> Mean accuracy [^\n]+', out)
    want = lines(_run(common + ['--matcher', 'tonioni'] + tail))
    got = lines(_run(common + ['--matcher=tonioni', '--device-graphs', '--device-tail', '--device-reclass', '--device-detections'] + tail))
    print(want)
    assert len(want) == 3 and got == want
