"""The comparator's compliance report on the GPU: the two kernels of csrc/report.hip equal the plain restatement of the rule
(tests/report_cases.py, pinned against the host path of `PlanogramComparator.report` in test_report_cpu.py) bit for bit, write only
what the header says, agree with `reclass_verdict`, and the report is the same on every device route at the waits `compare_batch`
pays."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import footprint
import report_cases as rp

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PREFILL = 0x5A5A5A5A
POS_IN = ('status', 'matched_expected', 'matched_actual', 'expected_positions', 'actual_boxes', 'off1', 'off2', 'image', 'actual_row')
POS_OUT = ('outcome', 'occupant', 'occupant_iou', 'occupant_row', 'stray')


# ---------------------------------------------------------------------------------------------------------------------
# the kernels against the model
# ---------------------------------------------------------------------------------------------------------------------
def _launch_positions(cuda, t, iou_threshold=0.5):
    """the first kernel on plain tensors prefilled with a pattern -> host outputs as int32 bits, in POS_OUT's order"""
    d = [None if t[name] is None else t[name].to(cuda) for name in POS_IN]
    sum1, sum2 = t['matched_expected'].numel(), t['matched_actual'].numel()
    outs = [torch.full((n,), PREFILL, dtype=torch.int32, device=cuda) for n in (sum1, sum1, sum1, sum1, sum2)]
    torch.ops.cvpce_amd.report_positions(*d, iou_threshold, outs[0], outs[1], outs[2].view(torch.float32), outs[3], outs[4])
    return [o.cpu() for o in outs]


def _assert_positions(got, want, what):
    for name, g in zip(POS_OUT, got):
        rows = torch.from_numpy(want['rows2' if name == 'stray' else 'rows1'])
        w = torch.from_numpy(want[name]).view(torch.int32)
        assert torch.equal(g[rows], w[rows]), (what, name, int((g[rows] != w[rows]).sum()))             # bit for bit
        assert bool((g[~rows] == PREFILL).all()), (what, name, 'a row of an image without a homography was written')


def test_positions_equal_the_model_bit_for_bit(cuda):
    from cvpce_amd import torch_ops_report  # noqa: F401
    images = rp.window_images()
    assert {len(im['matched']) for im in images} >= {1, 63, 64, 65, 257, 1024} and {len(im['claimed']) for im in images} >= {1, 63, 64, 65, 257, 1024}
    assert {im['status'] for im in images} == {rp.OK, rp.NONE, rp.INVALID} and any(not im['enabled'] for im in images)
    t = rp.report_tables(images)
    want = rp.run_model_positions(t)
    got = _launch_positions(cuda, t)
    _assert_positions(got, want, 'window')
    # without the detections' gallery rows: every occupant_row is -1, nothing else changes
    bare = _launch_positions(cuda, dict(t, actual_row=None))
    rows = torch.from_numpy(want['rows1'])
    assert bool((bare[3][rows] == -1).all()) and all(torch.equal(a, b) for k, (a, b) in enumerate(zip(bare, got)) if k != 3)
    # another threshold, one no float32 holds exactly
    _assert_positions(_launch_positions(cuda, t, 0.3), rp.run_model_positions(t, 0.3), 'threshold 0.3')
    # a threshold of 0: an IoU of 0 passes, so every undetected position has an occupant where a detection is unclaimed -- ties all over
    zero = rp.run_model_positions(t, 0.0)
    assert int((zero['occupant'][zero['rows1']] >= 0).sum()) > 2 * int((want['occupant'][want['rows1']] >= 0).sum())
    _assert_positions(_launch_positions(cuda, t, 0.0), zero, 'threshold 0')
    # an image launched alone gives the rows it gives inside the window
    o1, o2 = t['off1'].tolist(), t['off2'].tolist()
    for p, im in enumerate(images):
        t1 = rp.report_tables([im])
        t1['actual_row'] = t['actual_row'][o2[p]:o2[p + 1]].contiguous()
        alone = _launch_positions(cuda, t1)
        _assert_positions(alone, rp.run_model_positions(t1), p)
        for name, a, g in zip(POS_OUT, alone, got):
            o = o2 if name == 'stray' else o1
            assert torch.equal(a, g[o[p]:o[p + 1]]), (p, name)


def _launch_reclass(cuda, host):
    d = [host[name].to(cuda) for name in rp.RECLASS_ORDER]
    sum1 = host['outcome'].numel()
    outcome = host['outcome'].to(cuda)
    seen_row = torch.full((sum1,), PREFILL, dtype=torch.int32, device=cuda)
    seen_distance = torch.full((sum1,), PREFILL, dtype=torch.int32, device=cuda)
    torch.ops.cvpce_amd.report_reclass(*d, outcome, seen_row, seen_distance.view(torch.float32))
    return outcome.cpu(), seen_row.cpu(), seen_distance.cpu()


def _reclass_window(k):
    images = rp.window_images()
    first = rp.run_model_positions(rp.report_tables(images))
    outcome = np.where(first['rows1'], first['outcome'], PREFILL).astype(np.int32)              # rows no kernel wrote hold the pattern
    return rp.reclass_case(images, outcome, k)


@pytest.mark.parametrize('k', (1, 3))
def test_reclass_equals_the_model_and_agrees_with_the_verdict(cuda, k):
    from cvpce_amd import torch_ops_reclass, torch_ops_report  # noqa: F401
    host, cap = _reclass_window(k)
    assert cap == 1024
    want_outcome, want_row, want_distance, written = rp.run_model_reclass(host, cap)
    outcome, seen_row, seen_distance = _launch_reclass(cuda, host)
    m = torch.from_numpy(written)
    assert torch.equal(outcome[m], torch.from_numpy(want_outcome)[m]) and torch.equal(outcome[~m], host['outcome'][~m])
    assert torch.equal(seen_row[m], torch.from_numpy(want_row)[m]) and bool((seen_row[~m] == PREFILL).all())
    assert torch.equal(seen_distance[m], torch.from_numpy(want_distance).view(torch.int32)[m]) and bool((seen_distance[~m] == PREFILL).all())
    codes = outcome[m].tolist()
    assert rp.PENDING not in codes and codes.count(rp.RECOVERED) > 50 and codes.count(rp.MISSING) > 50
    # found of reclass_verdict is outcome in {DETECTED, RECOVERED}, row by row
    t, _ = rp.rc.plan_tables(rp.window_images())
    d = {name: host[name].to(cuda) for name in rp.RECLASS_ORDER}
    found = torch.full((outcome.numel(),), PREFILL, dtype=torch.int32, device=cuda)
    found_count = torch.empty(host['status'].numel(), dtype=torch.int32, device=cuda)
    torch.ops.cvpce_amd.reclass_verdict(d['expected_index'], d['count'], d['slot_row'], d['indices'], d['gallery_label_id'], d['expected_label_id'],
                                        t['matched_expected'].to(cuda), d['off1'], d['status'], found, found_count)
    found = found.cpu()
    assert torch.equal(found[m] != 0, outcome[m] <= rp.RECOVERED) and bool((found[~m] == PREFILL).all())
    off = host['off1'].tolist()
    for p, c in enumerate(found_count.cpu().tolist()):
        if c >= 0:
            assert c == int((outcome[off[p]:off[p + 1]] <= rp.RECOVERED).sum()), p
    # column 0 alone is read; an image launched alone gives the rows it gives inside the window
    if k > 1:
        other = dict(host, indices=host['indices'].clone(), distances=host['distances'].clone())
        other['indices'][:, 1:], other['distances'][:, 1:] = 0, 9.0
        assert all(torch.equal(a, b) for a, b in zip(_launch_reclass(cuda, other), (outcome, seen_row, seen_distance)))
    for p in (1, 4, 10):
        one = dict(host, expected_index=host['expected_index'][p:p + 1].contiguous(), count=host['count'][p:p + 1].contiguous(),
                   slot_row=host['slot_row'][p:p + 1].contiguous(), expected_label_id=host['expected_label_id'][off[p]:off[p + 1]].contiguous(),
                   off1=torch.tensor([0, off[p + 1] - off[p]], dtype=torch.int32), status=host['status'][p:p + 1].contiguous(),
                   outcome=host['outcome'][off[p]:off[p + 1]].contiguous())
        alone = _launch_reclass(cuda, one)
        assert all(torch.equal(a, b[off[p]:off[p + 1]]) for a, b in zip(alone, (outcome, seen_row, seen_distance))), p


def test_footprint_of_both_entry_points(cuda):
    """inputs and guard bands unchanged; the rows of an image without a homography stay unwritten"""
    from cvpce_amd import torch_ops_report  # noqa: F401
    images = rp.small_images()
    t = rp.report_tables(images)
    want = rp.run_model_positions(t)
    assert not want['rows1'].all() and not want['rows2'].all()
    ins = {name: footprint.put(v, cuda) for name, v in t.items()}
    sum1, sum2 = t['matched_expected'].numel(), t['matched_actual'].numel()
    outs = [footprint.out((n,), dt, cuda) for n, dt in ((sum1, torch.int32), (sum1, torch.int32), (sum1, torch.float32), (sum1, torch.int32), (sum2, torch.int32))]
    run = lambda: torch.ops.cvpce_amd.report_positions(*[ins[name][0] for name in POS_IN], 0.5, *[o[0] for o in outs])
    rows1, rows2 = torch.from_numpy(want['rows1']), torch.from_numpy(want['rows2'])
    # (NaN detections and positions are part of the window: an IoU that is a NaN is never an occupant's, so occupant_iou stays finite)
    res = footprint.check(run, list(ins.values()), outs, written=[rows1, rows1, rows1, rows1, rows2])
    for name, r in zip(POS_OUT, res):
        rows = rows2 if name == 'stray' else rows1
        assert torch.equal(r.cpu().view(torch.int32)[rows], torch.from_numpy(want[name]).view(torch.int32)[rows]), name

    host, cap = rp.reclass_case(images, np.where(want['rows1'], want['outcome'], PREFILL).astype(np.int32), 3)
    want_outcome, want_row, want_distance, written = rp.run_model_reclass(host, cap)
    vin = {name: footprint.put(host[name], cuda) for name in rp.RECLASS_ORDER}
    outcome = host['outcome'].to(cuda)                                                     # (in / out: checked by value below)
    vouts = [footprint.out((sum1,), torch.int32, cuda), footprint.out((sum1,), torch.float32, cuda)]

    def reclass():
        outcome.copy_(host['outcome'])
        torch.ops.cvpce_amd.report_reclass(*[vin[name][0] for name in rp.RECLASS_ORDER], outcome, *[o[0] for o in vouts])
    m = torch.from_numpy(written)
    res = footprint.check(reclass, list(vin.values()), vouts, written=[m, m])
    assert torch.equal(res[0].cpu()[m], torch.from_numpy(want_row)[m])
    assert torch.equal(res[1].cpu().view(torch.int32)[m], torch.from_numpy(want_distance).view(torch.int32)[m])
    assert torch.equal(outcome.cpu()[m], torch.from_numpy(want_outcome)[m]) and torch.equal(outcome.cpu()[~m], host['outcome'][~m])


def test_ten_launches_are_bit_identical(cuda):
    from cvpce_amd import torch_ops_report  # noqa: F401
    t = rp.report_tables(rp.window_images())
    first = _launch_positions(cuda, t)
    host, _ = _reclass_window(3)
    vfirst = _launch_reclass(cuda, host)
    for _ in range(9):
        assert all(torch.equal(a, b) for a, b in zip(first, _launch_positions(cuda, t)))
        assert all(torch.equal(a, b) for a, b in zip(vfirst, _launch_reclass(cuda, host)))


def test_ops_refuse_bad_calls_before_any_launch(cuda):
    from cvpce_amd import torch_ops_report  # noqa: F401
    t = rp.report_tables(rp.small_images()[:2])
    d = {name: v.to(cuda) for name, v in t.items()}
    sum1, sum2 = t['matched_expected'].numel(), t['matched_actual'].numel()
    o = {'outcome': torch.empty(sum1, dtype=torch.int32, device=cuda), 'occupant': torch.empty(sum1, dtype=torch.int32, device=cuda),
         'occupant_iou': torch.empty(sum1, device=cuda), 'occupant_row': torch.empty(sum1, dtype=torch.int32, device=cuda),
         'stray': torch.empty(sum2, dtype=torch.int32, device=cuda)}
    call = lambda **kw: torch.ops.cvpce_amd.report_positions(*[kw.get(n, d[n]) for n in POS_IN], 0.5, *[kw.get(n, o[n]) for n in POS_OUT])
    call()
    for bad in (dict(status=d['status'].to(torch.int64)), dict(actual_boxes=d['actual_boxes'].double()), dict(off2=d['off2'][:-1]), dict(stray=o['stray'][:-1]),
                dict(occupant_iou=o['outcome']), dict(image=d['image'][:, :2].contiguous()), dict(actual_row=d['actual_row'][:-1]),
                dict(expected_positions=d['expected_positions'].t().contiguous().t())):
        with pytest.raises(RuntimeError, match='cvpce_report_positions'):
            call(**bad)
    host, cap = rp.reclass_case(rp.small_images()[:2], rp.run_model_positions(t)['outcome'], 2)
    dv = {name: host[name].to(cuda) for name in rp.RECLASS_ORDER}
    ov = {'outcome': host['outcome'].to(cuda), 'seen_row': torch.empty(sum1, dtype=torch.int32, device=cuda), 'seen_distance': torch.empty(sum1, device=cuda)}
    reclass = lambda **kw: torch.ops.cvpce_amd.report_reclass(*[kw.get(n, dv[n]) for n in rp.RECLASS_ORDER], *[kw.get(n, ov[n]) for n in ov])
    reclass()
    for bad in (dict(indices=dv['indices'].to(torch.int32)), dict(distances=dv['distances'][:, :1].contiguous()), dict(slot_row=dv['slot_row'][:, :-1].contiguous()),
                dict(seen_row=ov['seen_row'][:-1]), dict(expected_label_id=dv['expected_label_id'][:-1]), dict(seen_distance=ov['seen_row'])):
        with pytest.raises(RuntimeError, match='cvpce_report_reclass'):
            reclass(**bad)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# through the comparator and the evaluator
# ---------------------------------------------------------------------------------------------------------------------
_PIPE = {}
SCALE = 1.2
WINDOW = 4


def _bench():
    if 'bench' not in _PIPE:
        spec = importlib.util.spec_from_file_location('bench_planogram_compare', os.path.join(ROOT, 'tools', 'bench_planogram_compare.py'))
        _PIPE['bench'] = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(_PIPE['bench'])
    return _PIPE['bench']


def _pipeline(cuda):
    """A small synthetic pipeline and a planted window, made once: 24 boxes per image (a 4 x 6 grid photographed at another scale), a
    window of 4, every 9th detection withheld; the planograms carry the labels the pipeline itself gives ALL 24 boxes, every 11th
    replaced by a label no gallery item has (as the reclass leg of tools/bench_planogram_compare.py plants them)."""
    if 'clf' not in _PIPE:
        from cvpce_amd import production, synthetic
        bench = _bench()
        det = synthetic.synthetic_gln(seed=0, detections_per_img=40).to(cuda)
        enc = synthetic.synthetic_macvgg(seed=1).to(cuda)
        names = synthetic.PLANOGRAM_LABELS
        clf = production.Classifier(enc, synthetic.TensorGallery(synthetic.gallery_images(24, seed=17), [names[i % 6] for i in range(24)]), device=cuda,
                                    emb_device=cuda, batch_size=8)
        pg = production.ProposalGenerator(det, device=cuda, confidence_threshold=0.5)
        imgs = [synthetic.shelf_image(70 + k, 640, 640).to(cuda) for k in range(WINDOW)]
        grids = [synthetic.planogram_grid(4, 6, 100 + k) for k in range(WINDOW)]
        full = [synthetic.perturbed_detections(eb, el, 200 + k, scale=SCALE, drop=0.0, mislabel=0.0)[0] for k, (eb, el) in enumerate(grids)]

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
        dets = evaluator(production.PlanogramComparator(), withheld).detect_and_classify_batch(imgs)
        actuals = [{'boxes': b, 'labels': labels} for b, labels in dets]
        _PIPE.update(clf=clf, pg=pg, imgs=imgs, planos=planos, withheld=withheld, actuals=actuals, evaluator=evaluator)
    return _PIPE


def _window_counter():
    return _bench().WindowCounter()


def _same_verdicts(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert type(g) is type(w) and float(g) == float(w), (g, w)
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.shape == w.shape and g.device == w.device, (g, w)


def _same_reports(got, want, what, distance_bound=None):
    """field by field; `seen_distance` bit for bit unless a bound is given -> the largest difference of seen_distance"""
    assert len(got) == len(want)
    worst = 0.0
    for k, (g, w) in enumerate(zip(got, want)):
        assert g.status == w.status, (what, k)
        _same_verdicts([g.compliance], [w.compliance])
        if w.status != 'ok':
            assert all(getattr(g, name) is None for name in g.FIELDS)
            continue
        assert g.outcomes.dtype == torch.int8 and torch.equal(g.outcomes, w.outcomes), (what, k, g.outcomes, w.outcomes)
        assert torch.equal(g.expected_positions.view(torch.int32), w.expected_positions.view(torch.int32)), (what, k)
        assert g.seen_labels == w.seen_labels and g.occupant_labels == w.occupant_labels, (what, k)
        assert torch.equal(g.occupant, w.occupant) and torch.equal(g.occupant_iou.view(torch.int32), w.occupant_iou.view(torch.int32)), (what, k)
        assert g.stray.dtype == torch.int64 and torch.equal(g.stray, w.stray), (what, k)
        assert torch.equal(g.seen_distance < 0, w.seen_distance < 0), (what, k)
        diff = float((g.seen_distance - w.seen_distance).abs().max()) if len(w.seen_distance) else 0.0
        worst = max(worst, diff)
        if distance_bound is None:
            assert torch.equal(g.seen_distance.view(torch.int32), w.seen_distance.view(torch.int32)), (what, k, diff)
        else:
            assert diff <= distance_bound, (what, k, diff)
    return worst


# `seen_distance` across the routes.  The per-image route (`device_tail` alone) matches each image's positions in a launch of their
# own, the window routes match the window's positions in one launch.  Measured on the MI355X (profiles/r28_compliance_report.md): the
# bits are identical, so equality is asserted (None = bit for bit).
SEEN_DISTANCE_BOUND = None


def test_the_report_is_the_same_on_every_device_route(cuda):
    from cvpce_amd import production
    p = _pipeline(cuda)
    clf, imgs, planos, actuals = p['clf'], p['imgs'], p['planos'], p['actuals']
    tail = production.PlanogramComparator(device_graphs=True, device_tail=True)
    both = production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True)
    want = tail.report_batch(planos, actuals, imgs, clf)
    _same_verdicts([r.compliance for r in want], tail.compare_batch(planos, actuals, imgs, clf))
    # the preconditions: every image has a homography, and the window holds every outcome but UNCHECKED, occupants and substitutions
    assert all(r.status == 'ok' and len(r.outcomes) == 24 for r in want)
    codes = sorted({c for r in want for c in r.outcomes.tolist()})
    print(f'outcomes {[r.outcomes.tolist() for r in want]}, occupants {[r.occupant.tolist() for r in want]}, strays {[r.stray.tolist() for r in want]}')
    assert {rp.DETECTED, rp.RECOVERED, rp.MISSING} <= set(codes) and rp.PENDING not in codes
    assert sum(len(r.substituted()) for r in want) >= 1 and all(float((r.outcomes <= 1).sum() / 24) == float(r.compliance) for r in want)
    for r in want:
        seen = torch.tensor([l is not None for l in r.seen_labels])
        assert torch.equal(seen, (r.outcomes == rp.RECOVERED) | (r.outcomes == rp.MISSING)) and torch.equal(seen, r.seen_distance >= 0)
    for k, r in enumerate(want):
        for i, c in enumerate(r.outcomes.tolist()):
            if c in (rp.RECOVERED, rp.MISSING):
                assert (r.seen_labels[i] == planos[k]['labels'][i]) == (c == rp.RECOVERED), (k, i)
    # device_tail + device_reclass
    got = both.report_batch(planos, actuals, imgs, clf)
    worst = _same_reports(got, want, 'device_reclass', SEEN_DISTANCE_BOUND if SEEN_DISTANCE_BOUND is not None else float('inf'))
    print(f'seen_distance, device_reclass against the per-image route: largest difference {worst!r}')
    _same_reports(got, want, 'device_reclass', SEEN_DISTANCE_BOUND)
    _same_verdicts([r.compliance for r in got], both.compare_batch(planos, actuals, imgs, clf))
    _same_reports([both.report(pl, a, img, clf) for pl, a, img in zip(planos, actuals, imgs)], got, 'report per image', SEEN_DISTANCE_BOUND)
    assert both.host_routed == 0 and both.reclass_host_routed == 0
    # device_detections: the detections never leave the device, the occupants' labels come from their gallery rows
    for cmp, name in ((tail, 'device_detections'), (both, 'device_detections + device_reclass')):
        on = p['evaluator'](cmp, p['withheld'], device_detections=True)
        got = on.report_batch(imgs, planos)
        worst = _same_reports(got, want, name, SEEN_DISTANCE_BOUND if SEEN_DISTANCE_BOUND is not None else float('inf'))
        print(f'seen_distance, {name} against the per-image route: largest difference {worst!r}')
        _same_reports(got, want, name, SEEN_DISTANCE_BOUND)
        _same_verdicts([r.compliance for r in got], on.evaluate_batch(imgs, planos))
        assert on.detections_host_routed == 0 and cmp.host_routed == 0
    # no classifier, no image: nothing is checked, on the device as on the host
    for kw in (dict(images=imgs, classifier=None), dict(images=None, classifier=clf)):
        a, b = both.report_batch(planos, actuals, **kw), tail.report_batch(planos, actuals, **kw)
        _same_reports(a, b, kw)
        _same_verdicts([r.compliance for r in a], both.compare_batch(planos, actuals, **kw))
        assert all(set(r.outcomes.tolist()) <= {rp.DETECTED, rp.UNCHECKED} and rp.UNCHECKED in r.outcomes.tolist() for r in a)
    # the other statuses beside an 'ok' image
    none = {'boxes': torch.zeros(0, 4), 'labels': []}
    other = dict(actuals[1], labels=['nothing_the_planogram_has'] * len(actuals[1]['labels']))
    mixed = both.report_batch(planos[:3], [none, other, actuals[2]], imgs[:3], clf)
    assert [r.status for r in mixed] == ['no_detections', 'no_matching', 'ok']
    _same_verdicts([r.compliance for r in mixed], both.compare_batch(planos[:3], [none, other, actuals[2]], imgs[:3], clf))
    _same_reports(mixed[2:], want[2:3], 'beside other statuses', SEEN_DISTANCE_BOUND)


def test_report_iter_yields_what_report_returns(cuda):
    from cvpce_amd import production
    p = _pipeline(cuda)
    imgs, planos = p['imgs'], p['planos']
    for switches, more in ((dict(device_graphs=True, device_tail=True, device_reclass=True), dict()),
                           (dict(device_graphs=True, device_tail=True, device_reclass=True), dict(device_detections=True)), (dict(), dict())):
        ev = p['evaluator'](production.PlanogramComparator(**switches), p['withheld'], **more)
        # (the planted pipeline takes whole windows: `report` of one image is `report_batch`'s row)
        want = ev.report_batch(imgs, planos)
        got = list(ev.report_iter(zip(imgs, planos), lookahead=WINDOW))
        _same_reports(got, want, (switches, more), SEEN_DISTANCE_BOUND)
        _same_verdicts([r.compliance for r in got], list(ev.evaluate_iter(zip(imgs, planos), lookahead=WINDOW)))
    # an evaluator of the plain kind, image by image: report_iter is report, pair by pair
    plain = production.PlanogramEvaluator(p['pg'], p['clf'], production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True))
    half = [{'boxes': b * 0.5, 'labels': list(l)} for b, l in plain.detect_and_classify_batch(imgs[:2])]
    want = [plain.report(img, pl) for img, pl in zip(imgs[:2], half)]
    for la in (1, 4):
        _same_reports(list(plain.report_iter(zip(imgs[:2], half), lookahead=la)), want, la, SEEN_DISTANCE_BOUND)
    _same_verdicts([r.compliance for r in want], [plain.evaluate(img, pl) for img, pl in zip(imgs[:2], half)])


def test_the_report_costs_no_wait(cuda):
    """a `device_reclass` window costs with the report what `compare_batch` costs without it: two waits with positions to classify,
    one without; and two launches more, one"""
    from cvpce_amd import production
    p = _pipeline(cuda)
    clf, imgs, planos, actuals = p['clf'], p['imgs'], p['planos'], p['actuals']
    both = production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True)
    full = [{'boxes': a['boxes'], 'labels': list(a['labels'])} for a in actuals]
    exact = [{'boxes': (a['boxes'] / SCALE).contiguous(), 'labels': list(a['labels'])} for a in actuals]     # every expected box has its detection
    for name, (es, acts), waits, launches in (('positions', (planos, actuals), 2, 2), ('none', (exact, full), 1, 1)):
        both.report_batch(es, acts, imgs, clf), both.compare_batch(es, acts, imgs, clf)                       # (caches, allocator)
        counts = {}
        for key, call in (('compare', both.compare_batch), ('report', both.report_batch)):
            with _window_counter() as c:
                res = call(es, acts, imgs, clf)
            counts[key] = c
        print(f'{name}: compare {counts["compare"].kernels} launches, {counts["compare"].waits} waits; report {counts["report"].kernels} launches, '
              f'{counts["report"].waits} waits')
        assert counts['compare'].waits == waits and counts['report'].waits == waits, name
        assert counts['report'].kernels - counts['compare'].kernels == launches, name
        if name == 'none':
            assert all(r.status == 'ok' and set(r.outcomes.tolist()) == {rp.DETECTED} and len(r.stray) == 0 for r in res)
    # `device_tail` alone re-classifies per image: one launch more for the window, and per image the one wait `compare_batch` pays there
    tail = production.PlanogramComparator(device_graphs=True, device_tail=True)
    tail.report_batch(planos, actuals, imgs, clf), tail.compare_batch(planos, actuals, imgs, clf)
    counts = {}
    for key, call in (('compare', tail.compare_batch), ('report', tail.report_batch)):
        with _window_counter() as c:
            call(planos, actuals, imgs, clf)
        counts[key] = c
    print(f'device_tail: compare {counts["compare"].kernels} launches, {counts["compare"].waits} waits; report {counts["report"].kernels} launches, '
          f'{counts["report"].waits} waits')
    assert counts['report'].waits == counts['compare'].waits and counts['report'].kernels - counts['compare'].kernels == 1
