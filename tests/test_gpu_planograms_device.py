"""The device planogram comparator on the GPU: the graph kernel equals the plain restatement of the device rule bit for bit
(tests/planogram_device_cases.py, pinned against the stock host functions in test_planograms_device_cpu.py), the match kernel
equals the host `large_common_subgraph` run on the device graphs, and the comparator's verdict with the switch on equals the
host comparator's wherever the two graph builders are comparable."""
import pytest
import torch

import footprint
import planogram_device_cases as cases
from cvpce_amd import planograms

pytestmark = pytest.mark.gpu

TIE_FREE_SIZES = (1, 2, 3, 7, 26, 64, 65)
_MODEL = {}


def _model(key, boxes, thresh_size):
    """the rule model's tables, computed once per case"""
    if key not in _MODEL:
        _MODEL[key] = cases.model_graph(boxes, thresh_size)
    return _MODEL[key]


def _host_tables(g):
    return g.nbr.cpu(), g.weight.cpu(), g.stamp.cpu()


def _assert_tables_equal(got, want, what):
    for name, a, b in zip(('nbr', 'weight', 'stamp'), got, want):
        a, b = a.cpu(), b.cpu()
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name)
        bits = (lambda t: t.view(torch.int32)) if a.dtype == torch.float32 else (lambda t: t)
        assert torch.equal(bits(a.contiguous()), bits(b.contiguous())), f'{what}: {name} differs in {int((a != b).sum())} slots'


def _graph_cases():
    out = []
    for n in (1, 2, 7, 26, 63, 64, 65, 200):
        out.append((f'scene{n}', *cases.scene(n, 0), 0.5))
    out.append(('scene1024', *cases.scene(1024, 0), 0.05))
    out.append(('grid4x6', *cases.grid(4, 6, 1), 0.5))
    out.append(('grid8x25', *cases.grid(8, 25, 2), 0.5))
    shared = cases.scene(9, 4)
    shared[0][5] = shared[0][2]                                              # two boxes sharing a centre: d = 0
    out.append(('shared_centre', *shared, 0.5))
    line = torch.tensor([[10.0 + 37 * i, 50.0, 40.0 + 37 * i, 90.0] for i in range(70)])
    out.append(('one_line', line, [cases.NAMES[i % 5] for i in range(70)], 0.5))
    return out


GRAPH_CASES = _graph_cases()


@pytest.mark.parametrize('case', GRAPH_CASES, ids=lambda c: c[0])
def test_graph_equals_the_rule_model(cuda, case):
    from cvpce_amd import planograms_device as pd
    name, boxes, labels, thresh_size = case
    g = pd.build_graphs([(boxes, labels)], thresh_size, device=cuda)[0]
    want = _model(name, boxes, thresh_size)
    _assert_tables_equal((g.nbr, g.weight, g.stamp), want, name)
    if len(labels) > 2:
        assert int((want[0] >= 0).sum()) > 0, 'the case has no edge'


def test_graph_batch_of_mixed_sizes_equals_single_launches(cuda):
    from cvpce_amd import planograms_device as pd
    picked = [c for c in GRAPH_CASES if c[0] in ('scene1', 'scene65', 'grid4x6', 'scene200', 'shared_centre')]
    assert len(picked) == 5
    batch = pd.build_graphs([(c[1], c[2]) for c in picked], 0.5, device=cuda)
    for c, g in zip(picked, batch):
        alone = pd.build_graphs([(c[1], c[2])], 0.5, device=cuda)[0]
        _assert_tables_equal((g.nbr, g.weight, g.stamp), (alone.nbr, alone.weight, alone.stamp), c[0])
        _assert_tables_equal((g.nbr, g.weight, g.stamp), _model(c[0], c[1], 0.5), c[0])


@pytest.mark.parametrize('n', TIE_FREE_SIZES)
def test_graph_equals_stock_build_graph_on_tie_free_scenes(cuda, n):
    from cvpce_amd import planograms_device as pd
    boxes, labels = cases.scene(n, cases.TIE_FREE_SEEDS[n])
    assert cases.is_tie_free(boxes)
    g = pd.build_graphs([(boxes, labels)], 0.5, device=cuda)[0]
    host = planograms.build_graph(boxes, labels, 0.5)
    # (bitwise weights wherever this machine's torch.sqrt, which the host's distances go through, returns the correctly rounded root)
    cases.assert_same_as_stock(cases.adjacency_of_tables(*_host_tables(g)), cases.adjacency_of_host(host), boxes)
    assert cases.adjacency_of_host(pd.to_networkx(g)) == cases.adjacency_of_tables(*_host_tables(g))


# ---------------------------------------------------------------------------------------------------------------------
def _match_cases():
    out = []
    for n in (3, 26, 65, 200):
        eb, el = cases.scene(n, 0)
        out.append((f'scene{n}', eb, el, *cases.detections_of(eb, el, 7 + n)))
    eb, el = cases.grid(8, 25, 2)
    out.append(('grid8x25', eb, el, *cases.detections_of(eb, el, 11)))                    # returns at an early hypothesis
    eb, el = cases.repeated_blocks(5)
    out.append(('blocks', eb, el, *cases.detections_of(eb, el, 5, drop=0.2)))             # runs through several hypotheses
    out.append(('blocks_self', eb, el, eb, el))                                           # returns at the first hypothesis
    ab, al = cases.scene(40, 9)
    out.append(('no_equal_label', eb, el, ab, ['elsewhere'] * 40))                        # count 0
    eb, el = cases.grid(4, 6, 1)
    ab, al = cases.detections_of(*cases.grid(6, 9, 1), 3)
    out.append(('n1_lt_n2', eb, el, ab, al))
    out.append(('n1_gt_n2', ab, al, eb, el))
    return out


MATCH_CASES = _match_cases()


def _hypotheses_walked(ge, ga, el, al):
    """how many hypotheses the host rule grows before it returns (test of the cases, on the model tables)"""
    from cvpce_amd import planograms_device as pd
    n1, n2 = pd.to_networkx(ge), pd.to_networkx(ga)
    want = planograms.large_common_subgraph(n1, n2)
    hyp = planograms.build_hypotheses(n1, n2)
    first = planograms.large_common_subgraph(n1, n2, min_score=-9.0, stop_at_fraction=0.0)     # what the first hypothesis alone grows
    return want, hyp, first


@pytest.fixture(scope='module')
def device_pairs(cuda):
    """every match case's two device graphs, built by one launch"""
    from cvpce_amd import planograms_device as pd
    graphs = pd.build_graphs([(c[1], c[2]) for c in MATCH_CASES] + [(c[3], c[4]) for c in MATCH_CASES], 0.5, device=cuda)
    return graphs[:len(MATCH_CASES)], graphs[len(MATCH_CASES):]


@pytest.mark.parametrize('k', range(len(MATCH_CASES)), ids=[c[0] for c in MATCH_CASES])
def test_match_equals_host_on_the_device_graphs(cuda, device_pairs, k):
    from cvpce_amd import planograms_device as pd
    name = MATCH_CASES[k][0]
    ge, ga = device_pairs[0][k], device_pairs[1][k]
    got = pd.common_subgraphs([ge], [ga])[0]
    want, hyp, first = _hypotheses_walked(ge, ga, ge.labels, ga.labels)
    assert got == want and list(got) == list(want), name
    model = cases.model_match(_host_tables(ge), ge.labels, _host_tables(ga), ga.labels)
    assert set(model) == got
    if name == 'no_equal_label':
        assert got == set() and not hyp
    if name == 'blocks_self':
        assert got == first and len(got) > min(len(ge), len(ga)) / 2
    if name == 'blocks':
        assert got != first and len(hyp) > 1, 'the case was meant to run through several hypotheses'
    for kw in ({'min_score': -0.5, 'stop_at_fraction': 0.9}, {'min_score': 0.0, 'stop_at_fraction': 1.0}):
        assert pd.common_subgraphs([ge], [ga], **kw)[0] == planograms.large_common_subgraph(pd.to_networkx(ge), pd.to_networkx(ga), **kw), (name, kw)


def test_match_batch_of_mixed_pairs_equals_single_launches(cuda, device_pairs):
    from cvpce_amd import planograms_device as pd
    batch = pd.common_subgraphs(*device_pairs)
    assert len(batch) == len(MATCH_CASES)
    for k, got in enumerate(batch):
        alone = pd.common_subgraphs([device_pairs[0][k]], [device_pairs[1][k]])[0]
        assert got == alone and list(got) == list(alone), MATCH_CASES[k][0]
    # graphs that are not slices of one launch's tables (a cached planogram beside fresh detections) are packed by a copy
    picked = [4, 0, 7]
    mixed = pd.common_subgraphs([device_pairs[0][k] for k in picked], [device_pairs[1][k] for k in picked])
    assert mixed == [batch[k] for k in picked]


def test_match_on_the_golden_cases(cuda, golden_dir):
    """as a set, the device matching is the reference's wherever the device graphs have the host graphs' adjacency order"""
    from cvpce_amd import planograms_device as pd
    golden = cases.golden_cases(golden_dir)
    graphs = pd.build_graphs([(c['expected_boxes'], c['expected_labels']) for c in golden]
                             + [(c['actual_boxes'], c['actual_labels']) for c in golden], 0.5, device=cuda)
    ge, ga = graphs[:len(golden)], graphs[len(golden):]
    got = pd.common_subgraphs(ge, ga)
    comparable = 0
    structure = lambda adj: [[(nb, d) for nb, d, _ in row] for row in adj]
    for c, e, a, m in zip(golden, ge, ga, got):
        he = planograms.build_graph(c['expected_boxes'], c['expected_labels'], 0.5)
        ha = planograms.build_graph(c['actual_boxes'], c['actual_labels'], 0.5)
        assert m == planograms.large_common_subgraph(pd.to_networkx(e), pd.to_networkx(a))
        if (structure(cases.adjacency_of_tables(*_host_tables(e))) == structure(cases.adjacency_of_host(he))
                and structure(cases.adjacency_of_tables(*_host_tables(a))) == structure(cases.adjacency_of_host(ha))):
            comparable += 1
            assert sorted(m) == [tuple(p) for p in c['matching']]
    assert comparable >= 2


# ---------------------------------------------------------------------------------------------------------------------
def _plano(boxes, labels):
    return {'boxes': boxes, 'labels': labels}


def test_comparator_verdict_equals_the_host_comparator(cuda, golden_dir):
    from cvpce_amd import production
    host, dev = production.PlanogramComparator(), production.PlanogramComparator(device_graphs=True)
    c = cases.golden_cases(golden_dir)[1]
    pairs = [(_plano(c['expected_boxes'], c['expected_labels']), _plano(c['actual_boxes'], c['actual_labels']))]
    want1 = float(host.compare(*pairs[0]))
    assert want1 == pytest.approx(23 / 24) and float(dev.compare(*pairs[0])) == want1
    for n in (7, 26, 64, 65):
        eb, el = cases.scene(n, cases.TIE_FREE_SEEDS[n])
        ab, al = eb + torch.tensor([30.0, 12.0, 30.0, 12.0]), list(el)       # integer centres again: the host's distances stay exact and tie-free
        keep = [i for i in range(n) if i % 9 != 4]
        ab, al = ab[keep].contiguous(), [('swapped' if i % 11 == 3 else al[i]) for i in keep]
        assert cases.is_tie_free(ab)
        pairs.append((_plano(eb, el), _plano(ab, al)))
    want = [float(host.compare(e, a)) for e, a in pairs]
    assert [float(dev.compare(e, a)) for e, a in pairs] == want and any(0 < v < 1 for v in want)
    # compare_batch: the whole batch in two launches, equal to the per-pair calls; an image without detections never reaches the device
    pairs.insert(2, (pairs[0][0], _plano(torch.zeros(0, 4), [])))
    want.insert(2, 0.0)
    assert [float(v) for v in dev.compare_batch([e for e, _ in pairs], [a for _, a in pairs])] == want
    assert dev.host_routed == 0
    # a cached planogram graph is used as it is
    from cvpce_amd import planograms_device as pd
    cached = dict(pairs[1][0])
    g = pd.prepare(cached, 0.5)
    assert pd.prepare(cached, 0.5) is g and cached[pd.CACHE_KEY][1] is g
    assert float(dev.compare(cached, pairs[1][1])) == want[1]


def test_graphs_beyond_the_cap_take_the_host_path(cuda):
    from cvpce_amd import planograms_device as pd, production
    big = cases.scene(pd.MAX_NODES + 1, 0)
    with pytest.raises(ValueError):
        pd.build_graphs([big], 0.5, device=cuda)

    class Routed(production.PlanogramComparator):
        seen = 0

        def _compare_host(self, expected, actual, image, classifier):
            Routed.seen += 1
            return 0.25                                    # (the host path itself is tested elsewhere: not run on 1025 boxes here)

    cmp = Routed(device_graphs=True)
    small = _plano(*cases.scene(7, 0))
    assert cmp.compare_batch([_plano(*big), small, small], [small, _plano(*big), small])[:2] == [0.25, 0.25]
    assert cmp.host_routed == 2 and Routed.seen == 2


def test_evaluate_iter_with_the_switch_equals_without(cuda):
    """the small synthetic pipeline of tests/test_gpu_harness.py (a copy: detector, embedder, gallery, four shelf images of two sizes)"""
    from cvpce_amd import production, synthetic
    det = synthetic.synthetic_gln(seed=0, detections_per_img=40).to(cuda)
    enc = synthetic.synthetic_macvgg(seed=1).to(cuda)
    gal = synthetic.gallery_images(24, seed=17)
    clf = production.Classifier(enc, synthetic.TensorGallery(gal, [f'sku{i % 6}' for i in range(24)]), device=cuda, emb_device=cuda,
                                batch_size=8)
    pg = production.ProposalGenerator(det, device=cuda, confidence_threshold=0.5)
    off = production.PlanogramEvaluator(pg, clf, production.PlanogramComparator())
    on = production.PlanogramEvaluator(pg, clf, production.PlanogramComparator(device_graphs=True))
    imgs = [synthetic.shelf_image(60, 512, 640), synthetic.shelf_image(61, 512, 640), synthetic.shelf_image(62, 448, 512),
            synthetic.shelf_image(63, 512, 640)]
    planos = []
    for k, (b, l) in enumerate(off.detect_and_classify_batch(imgs)):
        keep = [i for i in range(len(b)) if i % 3 != k % 3]
        planos.append({'boxes': b[keep] * 0.5, 'labels': [('other' if i % 7 == 0 else l[i]) for i in keep]})
    want = [float(v) for v in off.evaluate_iter(zip(imgs, planos), lookahead=4)]
    assert any(0.0 < v < 1.0 for v in want)
    for la in (1, 4):
        assert [float(v) for v in on.evaluate_iter(zip(imgs, planos), lookahead=la)] == want, la
    assert [float(v) for v in on.evaluate_batch(imgs, planos)] == want
    assert on.planogram_comparator.host_routed == 0


# ---------------------------------------------------------------------------------------------------------------------
def test_footprint_of_both_entry_points(cuda):
    """output guard bands unchanged, inputs unchanged, every slot of every node written (-1 included), every row of the pairs written"""
    picked = [c for c in GRAPH_CASES if c[0] in ('scene7', 'grid4x6', 'scene65')]
    sizes = [len(c[2]) for c in picked]
    off = [0]
    for n in sizes:
        off.append(off[-1] + n)
    boxes = footprint.put(torch.cat([c[1] for c in picked]), cuda)
    offsets = footprint.put(torch.tensor(off, dtype=torch.int32), cuda)
    thresh = footprint.put(torch.stack([cases.threshold(c[1], 0.5) for c in picked]).float(), cuda)
    nbr, weight, stamp = (footprint.out((off[-1], 8), dt, cuda) for dt in (torch.int32, torch.float32, torch.int32))
    run = lambda: torch.ops.cvpce_amd.planogram_graphs(boxes[0], offsets[0], thresh[0], min(sizes), max(sizes), nbr[0], weight[0], stamp[0])
    got = footprint.check(run, [boxes, offsets, thresh], [nbr, weight, stamp])
    for c, o, n in zip(picked, off, sizes):
        _assert_tables_equal([t[o:o + n] for t in got], _model(c[0], c[1], 0.5), c[0])

    # match: graph 0 against graph 1, graph 2 against itself
    ids = {}
    lab = torch.tensor([ids.setdefault(l, len(ids)) for c in picked for l in c[2]], dtype=torch.int32)
    nbr1 = torch.cat((got[0][off[0]:off[1]], got[0][off[2]:off[3]]))
    st1 = torch.cat((got[2][off[0]:off[1]], got[2][off[2]:off[3]]))
    lab1 = torch.cat((lab[off[0]:off[1]], lab[off[2]:off[3]]))
    nbr2, st2, lab2 = got[0][off[1]:off[3]].contiguous(), got[2][off[1]:off[3]].contiguous(), lab[off[1]:off[3]].contiguous()
    n1, n2 = [sizes[0], sizes[2]], [sizes[1], sizes[2]]
    count_equal = lambda a, b: int((a[:, None] == b[None, :]).sum())
    hyps = [count_equal(lab1[:n1[0]], lab2[:n2[0]]), count_equal(lab1[n1[0]:], lab2[n2[0]:])]
    i32 = lambda v: footprint.put(torch.tensor(v, dtype=torch.int32), cuda)
    ins = [footprint.put(t.cpu().contiguous(), cuda) for t in (nbr1, st1, lab1)] + [i32([0, n1[0], sum(n1)])] + \
          [footprint.put(t.cpu().contiguous(), cuda) for t in (nbr2, st2, lab2)] + [i32([0, n2[0], sum(n2)])] + \
          [i32([[2, min(n1[0], n2[0]) // 2], [2, sizes[2] // 2]]), i32([0, hyps[0], sum(hyps)]), i32([0, min(n1[0], n2[0]), min(n1[0], n2[0]) + sizes[2]])]
    rows = min(n1[0], n2[0]) + sizes[2]
    work = footprint.out((sum(hyps),), torch.int32, cuda)
    pairs, count = footprint.out((rows, 2), torch.int32, cuda), footprint.out((2,), torch.int32, cuda)
    run = lambda: torch.ops.cvpce_amd.planogram_match(*[p[0] for p in ins], max(n1), max(n2), sum(hyps), work[0], pairs[0], count[0])
    _, got_pairs, got_count = footprint.check(run, ins, [work, pairs, count], written=[footprint.SCRATCH, None, None])
    got_pairs, got_count = got_pairs.cpu(), got_count.tolist()
    assert got_count[1] == sizes[2]
    assert sorted(got_pairs[min(n1[0], n2[0]):, 0].tolist()) == list(range(sizes[2]))          # a graph against itself: every node, with itself
    assert torch.equal(got_pairs[min(n1[0], n2[0]):, 0], got_pairs[min(n1[0], n2[0]):, 1])
    assert bool((got_pairs[got_count[0]:min(n1[0], n2[0])] == -1).all())                        # the rows beyond the count


def test_fifty_launches_are_bit_identical(cuda):
    from cvpce_amd import planograms_device as pd
    eb, el = cases.grid(8, 25, 2)
    ab, al = cases.detections_of(eb, el, 11)
    first = pd.build_graphs([(eb, el), (ab, al)], 0.5, device=cuda)
    first_match = pd.common_subgraphs([first[0]], [first[1]])[0]
    same = torch.ones((), dtype=torch.bool, device=cuda)
    for _ in range(49):
        again = pd.build_graphs([(eb, el), (ab, al)], 0.5, device=cuda)
        for a, b in zip(first, again):
            same &= (a.nbr == b.nbr).all() & (a.weight.view(torch.int32) == b.weight.view(torch.int32)).all() & (a.stamp == b.stamp).all()
        m = pd.common_subgraphs([again[0]], [again[1]])[0]
        assert m == first_match and list(m) == list(first_match)
    assert bool(same)
