"""The step pictures through the evaluator: `step_pictures_batch` gives `report_batch`'s reports and `pictures_batch`'s three pictures on
every route, the device routes agree on all nine, each graph picture is the model (tests/render_cases.py, tests/stroke_cases.py) painted
from `to_networkx` of the same graphs and the same matching, and the window costs two launches more than its report and no wait."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import render_cases as rc
import stroke_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_PIPE = {}
SCALE, SHIFT, WINDOW, GALLERY, SIDE = 1.2, (30.3, 12.3), 4, 24, 512
ON = dict(device_graphs=True, device_tail=True)
ALL = dict(ON, device_reclass=True)


def _bench():
    spec = importlib.util.spec_from_file_location('bench_planogram_compare', os.path.join(ROOT, 'tools', 'bench_planogram_compare.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _pipeline(cuda):
    """The planted window of test_gpu_render.py / test_gpu_report.py, four images wide, made once: images of 512^2 with 24 boxes each (a
    4 x 6 grid photographed at another scale), every 9th detection withheld, every 11th expected label one no gallery item has.  The
    detections are the planogram's boxes scaled and shifted with no jitter, the shift keeping every projected coordinate a tenth of a
    pixel from an integer, so the integer extents of the picture rule are the same on every route (see test_gpu_render.py)."""
    if 'clf' not in _PIPE:
        from cvpce_amd import production, rendering as rd, synthetic
        bench = _bench()
        det = synthetic.synthetic_gln(seed=0, detections_per_img=40).to(cuda)
        enc = synthetic.synthetic_macvgg(seed=1).to(cuda)
        gallery = synthetic.TensorGallery(synthetic.gallery_images(GALLERY, seed=17))
        clf = production.Classifier(enc, gallery, device=cuda, emb_device=cuda, batch_size=8)
        pg = production.ProposalGenerator(det, device=cuda, confidence_threshold=0.5)
        imgs = [synthetic.shelf_image(70 + k, SIDE, SIDE).to(cuda) for k in range(WINDOW)]
        grids = [synthetic.planogram_grid(4, 6, 100 + k, cell=(40, 60), gap=(6, 14)) for k in range(WINDOW)]
        full = [synthetic.perturbed_detections(eb, el, 200 + k, scale=SCALE, shift=SHIFT, jitter=0.0, drop=0.0, mislabel=0.0)[0] for k, (eb, el) in enumerate(grids)]
        assert all(float(b.max()) < SIDE for b in full)
        assert all(float(((b - b.round()).abs()).min()) > 0.05 for b in full)

        def planted(boxes):
            packed = torch.zeros((WINDOW, det.detections_per_img, 4))
            for k, b in enumerate(boxes):
                packed[k, :len(b)] = b
            return packed.to(cuda), torch.tensor([len(b) for b in boxes], dtype=torch.int32, device=cuda)

        def evaluator(cmp, boxes, **kw):
            ev = bench.PlantedDetectionsEvaluator(pg, clf, cmp, **kw)
            ev._pipeline().planted = planted(boxes)
            return ev
        all_dets = evaluator(production.PlanogramComparator(), full).detect_and_classify_batch(imgs)
        assert all(len(labels) == 24 for _, labels in all_dets)
        planos = [{'boxes': eb, 'labels': [('not_in_the_gallery' if i % 11 == 5 else l) for i, l in enumerate(labels)]}
                  for (eb, _), (_, labels) in zip(grids, all_dets)]
        withheld = [b[[i for i in range(24) if i % 9 != 4]].contiguous() for b in full]
        atlas = rd.ThumbnailAtlas(gallery, clf.annotations, cuda, max_side=64)
        _PIPE.update(clf=clf, imgs=imgs, planos=planos, withheld=withheld, evaluator=evaluator, atlas=atlas, bench=bench,
                     images=[atlas.image(r).cpu().numpy() for r in range(len(atlas))], table=rd.label_rows(clf.annotations))
    return _PIPE


def _host(pics):
    from cvpce_amd import rendering as rd
    return [getattr(pics, n).cpu() for n in rd.StepPictures.NAMES]


def _arrays(items):
    return items.box.numpy(), items.src.numpy(), items.colour.numpy(), items.thickness.numpy()


def _drawn(canvas, g, boxes, nodes=None):
    """the model's drawing of the networkx graph `g` (of its subgraph on `nodes`) over `canvas`: black edges, then the nodes' discs"""
    from cvpce_amd import rendering as rd
    b = boxes.to(torch.float32).numpy()
    cx, cy = (b[:, 0] + b[:, 2]) / np.float32(2), (b[:, 1] + b[:, 3]) / np.float32(2)
    g = g if nodes is None else g.subgraph(nodes)
    ends = [(cx[i], cy[i], cx[j], cy[j]) for i, j in g.edges()] + [(cx[i], cy[i], cx[i], cy[i]) for i in sorted(g.nodes())]
    colour = [rd.GRAPH_EDGE_COLOUR] * g.number_of_edges() + [rd.GRAPH_NODE_COLOUR] * g.number_of_nodes()
    radius = [rd.GRAPH_EDGE_RADIUS] * g.number_of_edges() + [rd.GRAPH_NODE_RADIUS] * g.number_of_nodes()
    return sc.paint(canvas.copy(), np.array(ends, dtype=np.float32).reshape(-1, 4), np.array(colour, dtype=np.int32), np.array(radius, dtype=np.int32))


def _model(p, img, plano, rep, boxes, labels, ge, ga, matching):
    """the nine pictures by the two models, from the networkx graphs and the set of matched pairs"""
    from cvpce_amd import rendering as rd
    hw = (SIDE, SIDE)
    ehw = rd.expected_canvas_hw(plano['boxes'], SIDE)
    base = rd.float_image_bytes(img.cpu()).numpy()
    paint = lambda items, size, b=None: rc.paint(size, *_arrays(items), p['images'], b, rd.WHITE)
    observed = paint(rd.observed_items(boxes, rd.rows_of_labels(labels, p['table'])), hw)
    expected = paint(rd.expected_items(plano['boxes'], rd.rows_of_labels(plano['labels'], p['table']), ehw), ehw)
    on_canvas = rd.expected_boxes_on_canvas(plano['boxes'], ehw)
    if matching is None:
        graphs = [expected, observed, expected, observed]
    else:
        graphs = [_drawn(expected, ge, on_canvas), _drawn(observed, ga, boxes), _drawn(expected, ge, on_canvas, sorted({a for a, _ in matching})),
                  _drawn(observed, ga, boxes, sorted({b for _, b in matching}))]
    return [paint(rd.ring_items(boxes, rd.DETECTION_COLOUR, rd.ANNOTATION_THICKNESS, hw), hw, base),
            paint(rd.ring_items(rep.expected_positions if rep.status == 'ok' else None, rd.POSITION_COLOUR, rd.ANNOTATION_THICKNESS, hw), hw, base),
            *graphs, paint(rd.annotation_items(rep, boxes, rd.ANNOTATION_THICKNESS, hw), hw, base), observed, expected]


def _assert_pictures(got, want, what):
    from cvpce_amd import rendering as rd
    for n, a, b in zip(rd.StepPictures.NAMES, got, want):
        a = a.numpy() if torch.is_tensor(a) else a
        assert a.shape == b.shape and np.array_equal(a, b), (what, n, a.shape, b.shape, int((a != b).any(axis=2).sum()) if a.shape == b.shape else None)


def test_step_pictures_give_the_reports_and_the_pictures_on_every_route(cuda):
    from cvpce_amd import planograms, planograms_device as pd, production, rendering as rd
    from test_gpu_report import SEEN_DISTANCE_BOUND, _same_reports
    p = _pipeline(cuda)
    imgs, planos = p['imgs'], p['planos']
    renderer = rd.SceneRenderer(p['atlas'])
    routes = (('host', dict(), dict()), ('device_graphs', dict(device_graphs=True), dict()), ('device_graphs + device_tail', ON, dict()),
              ('all switches', ALL, dict(device_detections=True)))
    device = None
    for name, switches, more in routes:
        cmp = production.PlanogramComparator(**switches)
        ev = p['evaluator'](cmp, p['withheld'], **more)
        want = ev.report_batch(imgs, planos)
        got = ev.step_pictures_batch(imgs, planos, renderer)
        assert len(got) == WINDOW and all(isinstance(pic, rd.StepPictures) for _, pic in got)
        _same_reports([rep for rep, _ in got], want, name, SEEN_DISTANCE_BOUND)
        assert all(r.status == 'ok' for r in want)
        pics = [_host(pic) for _, pic in got]
        # the last three are `pictures_batch`'s, byte for byte
        for k, (_, three) in enumerate(ev.pictures_batch(imgs, planos, renderer)):
            for n, a in zip(rd.CompliancePictures.NAMES, pics[k][-3:]):
                assert torch.equal(a, getattr(three, n).cpu()), (name, k, n)
        if name == 'all switches':
            assert ev.detections_host_routed == 0 and cmp.host_routed == 0
        # the device routes agree on all nine
        if switches.get('device_tail'):
            if device is None:
                device = pics
            else:
                for k in range(WINDOW):
                    _assert_pictures(pics[k], [b.numpy() for b in device[k]], (name, k))
        # the iterator yields the same, one window after another
        if name in ('host', 'all switches'):
            again = list(ev.step_pictures_iter(zip(imgs, planos), renderer, lookahead=WINDOW))
            _same_reports([rep for rep, _ in again], want, name + ' iter', SEEN_DISTANCE_BOUND)
            for k, (_, pic) in enumerate(again):
                _assert_pictures(_host(pic), [b.numpy() for b in pics[k]], (name + ' iter', k))
        # the model, from the networkx form of the route's own graphs and its own matching
        if name == 'all switches':
            continue                                  # (its detections never reach the host; its pictures are the route's above)
        dets = ev.detect_and_classify_batch(imgs)
        for k, (img, plano, rep, (boxes, labels)) in enumerate(zip(imgs, planos, want, dets)):
            if name == 'host':
                ge = planograms.build_graph(plano['boxes'], plano['labels'], cmp.graph_threshold)
                ga = planograms.build_graph(boxes, labels, cmp.graph_threshold)
                matching = planograms.large_common_subgraph(ge, ga)
            else:
                dge, dga = pd.build_graphs([(plano['boxes'], plano['labels']), (boxes, labels)], cmp.graph_threshold)
                ge, ga, matching = pd.to_networkx(dge), pd.to_networkx(dga), pd.common_subgraphs([dge], [dga])[0]
            assert 3 <= len(matching) and ge.number_of_edges() > 24 and ga.number_of_edges() > 20
            model = _model(p, img, plano, rep, boxes, labels, ge, ga, matching)
            _assert_pictures(pics[k], model, (name, k))
            # something was drawn, and less on the matched pictures than on the graphs'
            for full, part, plain in ((model[2], model[4], model[8]), (model[3], model[5], model[7])):
                assert 0 < int((part != plain).any(axis=2).sum()) <= int((full != plain).any(axis=2).sum())
            assert (model[0] != model[1]).any()


def test_the_tonioni_matcher_draws_its_own_matching(cuda):
    from cvpce_amd import planograms_device as pd, production, rendering as rd
    from test_gpu_report import SEEN_DISTANCE_BOUND, _same_reports
    p = _pipeline(cuda)
    imgs, planos = p['imgs'], p['planos']
    renderer = rd.SceneRenderer(p['atlas'])
    cmp = production.PlanogramComparator(matcher='tonioni', **ON)
    ev = p['evaluator'](cmp, p['withheld'])
    want = ev.report_batch(imgs, planos)
    got = ev.step_pictures_batch(imgs, planos, renderer)
    _same_reports([rep for rep, _ in got], want, 'tonioni', SEEN_DISTANCE_BOUND)
    dets = ev.detect_and_classify_batch(imgs)
    for k, (img, plano, rep, (boxes, labels)) in enumerate(zip(imgs, planos, want, dets)):
        dge, dga = pd.build_graphs([(plano['boxes'], plano['labels']), (boxes, labels)], cmp.graph_threshold)
        matching = pd.common_subgraphs([dge], [dga], matcher='tonioni')[0]
        assert len(matching) >= 3
        _assert_pictures(_host(got[k][1]), _model(p, img, plano, rep, boxes, labels, pd.to_networkx(dge), pd.to_networkx(dga), matching), ('tonioni', k))
    # with every switch on: the same pictures, the detections never on the host
    on = p['evaluator'](production.PlanogramComparator(matcher='tonioni', **ALL), p['withheld'], device_detections=True)
    for k, (_, pic) in enumerate(on.step_pictures_batch(imgs, planos, renderer)):
        _assert_pictures(_host(pic), [b.numpy() for b in _host(got[k][1])], ('tonioni, all switches', k))


def test_the_atlas_takes_unit_floats_of_any_size(cuda):
    """what `datautils.SimpleFolderSet(train=False)` yields: (3, h, w) in [0, 1] -> bytes by floor(clamp(x, 0, 1) * 255 + 0.5)"""
    from cvpce_amd import rendering as rd, synthetic
    g = torch.Generator().manual_seed(12)
    items = [torch.rand(3, h, w, generator=g) * 1.2 - 0.1 for h, w in ((7, 5), (1, 1), (40, 33))]
    gallery = synthetic.TensorGallery(items)
    atlas = rd.ThumbnailAtlas(gallery, gallery.annotations, cuda, max_side=None, float_items='unit')
    assert all(torch.equal(atlas.image(r).cpu(), rd.float_image_bytes(im)) for r, im in enumerate(items))
    tanh = rd.ThumbnailAtlas(gallery, gallery.annotations, cuda, max_side=None)
    assert not torch.equal(tanh.image(2).cpu(), atlas.image(2).cpu())                     # the default reads a float item as [-1, 1]
    with pytest.raises(ValueError):
        rd.ThumbnailAtlas(gallery, None, cuda, float_items='bytes')


def test_a_host_routed_image_is_drawn_beside_the_device_window(cuda):
    """every switch on, the detections on the device, and the first image of the window sent through the host by the comparator's own
    hypothesis limit (forced: `_over_limit` answers yes for it): its detections come back through `to_host`, its graphs are the host's
    networkx graphs as tables on the host, its boxes the device pack's -- and the images beside it stay on the device route"""
    from cvpce_amd import planograms, production, rendering as rd
    p = _pipeline(cuda)
    imgs, planos = p['imgs'], p['planos']
    renderer = rd.SceneRenderer(p['atlas'])
    plain = p['evaluator'](production.PlanogramComparator(matcher='tonioni', **ALL), p['withheld'], device_detections=True)
    want = [_host(pic) for _, pic in plain.step_pictures_batch(imgs, planos, renderer)]
    cmp = production.PlanogramComparator(matcher='tonioni', **ALL)
    asked = []
    cmp._over_limit = lambda hypotheses: (asked.append(hypotheses), len(asked) % WINDOW == 1)[1]          # the first image of every window
    ev = p['evaluator'](cmp, p['withheld'], device_detections=True)
    got = ev.step_pictures_batch(imgs, planos, renderer)
    assert cmp.host_routed == 1 and len(asked) == WINDOW and [rep.status for rep, _ in got] == ['ok'] * WINDOW
    for k in range(1, WINDOW):
        _assert_pictures(_host(got[k][1]), [b.numpy() for b in want[k]], ('beside a host-routed image', k))
    boxes, labels = p['evaluator'](production.PlanogramComparator(), p['withheld']).detect_and_classify_batch(imgs)[0]
    ge = planograms.build_graph(planos[0]['boxes'], planos[0]['labels'], cmp.graph_threshold)
    ga = planograms.build_graph(boxes, labels, cmp.graph_threshold)
    matching = planograms.tonioni_mcs(ge, ga)
    assert len(matching) >= 3
    _assert_pictures(_host(got[0][1]), _model(p, imgs[0], planos[0], got[0][0], boxes, labels, ge, ga, matching), 'host-routed')


def test_an_image_without_detections_or_without_a_matching_has_no_strokes(cuda):
    from cvpce_amd import production, rendering as rd
    p = _pipeline(cuda)
    imgs = p['imgs']
    renderer = rd.SceneRenderer(p['atlas'])
    # (a fresh dict: a planogram's dict caches its device graph and its label ids)
    planos = [p['planos'][0], {'boxes': p['planos'][1]['boxes'], 'labels': ['nothing_the_gallery_has'] * 24}, p['planos'][2], p['planos'][3]]
    planted = [p['withheld'][0][:0]] + p['withheld'][1:]
    for name, switches in (('host', dict()), ('device_graphs + device_tail + device_reclass', ALL)):
        ev = p['evaluator'](production.PlanogramComparator(**switches), planted)
        got = ev.step_pictures_batch(imgs, planos, renderer)
        assert [rep.status for rep, _ in got] == ['no_detections', 'no_matching', 'ok', 'ok'], name
        dets = ev.detect_and_classify_batch(imgs)
        for k in (0, 1):
            rep, pic = got[k]
            model = _model(p, imgs[k], planos[k], rep, dets[k][0], dets[k][1], None, None, None)
            _assert_pictures(_host(pic), model, (name, k))
            base = rd.float_image_bytes(imgs[k].cpu()).numpy()
            assert np.array_equal(model[1], base) and np.array_equal(model[6], base)            # no positions: the photo alone
            assert np.array_equal(model[0], base) == (k == 0)                                   # no detections: nothing ringed
        for k in (2, 3):                               # the images beside them are drawn as ever
            pics = _host(got[k][1])
            assert not torch.equal(pics[2], pics[8]) and not torch.equal(pics[3], pics[7]) and not torch.equal(pics[5], pics[7])


def test_step_pictures_cost_two_launches_more_than_the_report_and_no_wait(cuda):
    from cvpce_amd import production, rendering as rd
    p = _pipeline(cuda)
    imgs, planos = p['imgs'], p['planos']
    renderer = rd.SceneRenderer(p['atlas'])
    ev = p['evaluator'](production.PlanogramComparator(**ALL), p['withheld'], device_detections=True)
    ev.report_batch(imgs, planos), ev.step_pictures_batch(imgs, planos, renderer)          # (caches, allocator)
    counts = {}
    for key, call in (('report', lambda: ev.report_batch(imgs, planos)), ('pictures', lambda: ev.pictures_batch(imgs, planos, renderer)),
                      ('steps', lambda: ev.step_pictures_batch(imgs, planos, renderer))):
        with p['bench'].WindowCounter() as c:
            call()
        counts[key] = c
    print('; '.join(f'{key} {c.kernels} launches, {c.waits} waits, {c.torch_device_ops} other device operators' for key, c in counts.items()))
    assert counts['steps'].kernels == counts['report'].kernels + 2 and counts['steps'].waits == counts['report'].waits
    assert counts['pictures'].kernels == counts['report'].kernels + 1
