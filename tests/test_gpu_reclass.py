"""The comparator's re-classification on the GPU: the two kernels of csrc/reclass.hip equal the plain restatement of the rule
(tests/reclass_cases.py, pinned against `PlanogramComparator._finish`'s lines in test_reclass_cpu.py) bit for bit, write only what
the header says, and the comparator with `device_reclass` on gives the verdicts of the `device_tail`-only path exactly."""
import hashlib

import numpy as np
import pytest
import torch

import footprint
import reclass_cases as rc
from test_gpu_homography_device import _host_margins

pytestmark = pytest.mark.gpu

PREFILL = 0x5A5A5A5A
# the wave (64) and workgroup (256) boundaries of the ordered compaction, and the largest graph
PLAN_BATCH = ((1, 'all_missing', 480, 640), (63, 'mixed', 333, 517), (64, 'all_missing', 480, 640), (65, 'edges', 333, 517),
              (257, 'mixed', 480, 640), (1024, 'all_missing', 2161, 3847), (64, 'none_missing', 333, 517), (1024, 'mixed', 480, 640),
              (19, 'edges', 480, 640))
_PLAN = {}


def _plan_images():
    if 'images' not in _PLAN:
        images = [rc.plan_image(n1, kind, h, w, 100 + k) for k, (n1, kind, h, w) in enumerate(PLAN_BATCH)]
        images.insert(2, rc.plan_image(40, 'all_missing', 480, 640, 7, status=rc.NONE))
        images.insert(5, rc.plan_image(40, 'all_missing', 480, 640, 8, enabled=0))
        images.append(rc.plan_image(40, 'all_missing', 480, 640, 9, status=rc.INVALID))
        _PLAN['images'] = images
    return _PLAN['images']


def _model_plan(images):
    t, cap = rc.plan_tables(images)
    return t, cap, rc.model_plan(t['status'].numpy(), t['matched_expected'].numpy(), t['expected_positions'].numpy(), t['off1'].tolist(),
                                 t['image'].tolist(), cap)


def _launch_plan(cuda, t, cap):
    """the plan kernel on plain tensors prefilled with a pattern -> host (boxes as int32 bits, expected_index, count)"""
    b = t['status'].numel()
    d = {name: v.to(cuda) for name, v in t.items()}
    boxes = torch.full((b, cap, 4), PREFILL, dtype=torch.int32, device=cuda).view(torch.float32)
    index = torch.full((b, cap), PREFILL, dtype=torch.int32, device=cuda)
    count = torch.full((b,), PREFILL, dtype=torch.int32, device=cuda)
    torch.ops.cvpce_amd.reclass_plan(d['status'], d['matched_expected'], d['expected_positions'], d['off1'], d['image'], boxes, index, count)
    return boxes.view(torch.int32).cpu(), index.cpu(), count.cpu()


def _assert_plan(got, want, what):
    boxes, index, count = got
    wboxes, windex, wcount, written = want
    assert count.tolist() == wcount.tolist(), what
    m = torch.from_numpy(written)
    assert torch.equal(index[m], torch.from_numpy(windex)[m]), what
    assert torch.equal(boxes[m], torch.from_numpy(wboxes).view(torch.int32)[m]), what           # bit for bit, -0 included
    assert bool((index[~m] == PREFILL).all()) and bool((boxes[~m] == PREFILL).all()), (what, 'a slot beyond the count was written')


def test_plan_equals_the_model_bit_for_bit(cuda):
    from cvpce_amd import torch_ops_reclass  # noqa: F401
    images = _plan_images()
    t, cap, want = _model_plan(images)
    assert cap == 1024 and {len(im['matched']) for im in images} >= {1, 63, 64, 65, 257, 1024}
    counts = want[2].tolist()
    assert counts[2] == counts[5] == counts[-1] == 0 and counts[8] == 0                  # status none, disabled, invalid, none missing
    assert counts[7] > 768 and counts[0] + counts[1] > 0                                    # every chunk of the largest image holds positions
    _assert_plan(_launch_plan(cuda, t, cap), want, 'batch')
    # the same images launched alone give the same rows
    got = _launch_plan(cuda, t, cap)
    for p, im in enumerate(images):
        t1, cap1, want1 = _model_plan([im])
        alone = _launch_plan(cuda, t1, cap1)
        _assert_plan(alone, want1, p)
        c = int(alone[2][0])
        assert c == int(got[2][p]) and torch.equal(alone[0][0, :c], got[0][p, :c]) and torch.equal(alone[1][0, :c], got[1][p, :c]), p


def _verdict_case(k, seed=0):
    """a window of five images for the verdict kernel, from the model's own plan: host tensors in the op's order, and cap"""
    g = torch.Generator().manual_seed(seed)
    images = [rc.plan_image(n1, kind, 480, 640, 300 + i) for i, (n1, kind) in enumerate(((65, 'mixed'), (257, 'all_missing'), (30, 'mixed'), (1, 'all_missing')))]
    images.insert(2, rc.plan_image(40, 'mixed', 480, 640, 310, status=rc.NONE))
    t, cap, (_, index, count, written) = _model_plan(images)
    total, gsize = int(count.sum()), 24
    m = total - 3                                                                          # the last three rows lie beyond the match result
    slot_row = np.full(index.shape, -1, dtype=np.int32)
    slot_row[written] = np.arange(total)
    slot_row[0, 1] = -7                                                                    # a negative row
    indices = torch.randint(0, gsize, (m, k), generator=g, dtype=torch.int64)
    indices[3, 0], indices[5, 0], indices[8, 0] = gsize, -1, 2 ** 40                        # indices outside the gallery
    gallery_id = torch.tensor([i % 6 for i in range(gsize)], dtype=torch.int32)
    sum1 = int(t['off1'][-1])
    expected_id = torch.randint(0, 6, (sum1,), generator=g).to(torch.int32)
    expected_id[::7] = -1                                                                  # labels no gallery item has
    index = index.copy()
    index[1, 0], index[1, 2] = 257, -1                                                     # indices outside the image
    index[~written] = 0x5A5A5A5A
    host = {'expected_index': torch.from_numpy(index), 'count': torch.from_numpy(count), 'slot_row': torch.from_numpy(slot_row), 'indices': indices,
            'gallery_label_id': gallery_id, 'expected_label_id': expected_id, 'matched_expected': t['matched_expected'], 'off1': t['off1'],
            'status': t['status']}
    return host, cap


VERDICT_ORDER = ('expected_index', 'count', 'slot_row', 'indices', 'gallery_label_id', 'expected_label_id', 'matched_expected', 'off1', 'status')


def _model_verdict(host, cap):
    return rc.model_verdict(host['expected_index'].numpy(), host['count'].numpy(), host['slot_row'].numpy(), host['indices'].numpy(),
                            host['gallery_label_id'].tolist(), host['expected_label_id'].tolist(), host['matched_expected'].numpy(),
                            host['off1'].tolist(), host['status'].tolist(), cap)


def _launch_verdict(cuda, host):
    d = [host[name].to(cuda) for name in VERDICT_ORDER]
    found = torch.full((host['matched_expected'].numel(),), PREFILL, dtype=torch.int32, device=cuda)
    found_count = torch.full((host['status'].numel(),), PREFILL, dtype=torch.int32, device=cuda)
    torch.ops.cvpce_amd.reclass_verdict(*d, found, found_count)
    return found.cpu(), found_count.cpu()


@pytest.mark.parametrize('k', (1, 3))
def test_verdict_equals_the_model(cuda, k):
    from cvpce_amd import torch_ops_reclass  # noqa: F401
    host, cap = _verdict_case(k)
    want_found, want_count, written = _model_verdict(host, cap)
    found, found_count = _launch_verdict(cuda, host)
    assert found_count.tolist() == want_count.tolist() and want_count[2] == -1
    m = torch.from_numpy(written)
    assert torch.equal(found[m], torch.from_numpy(want_found)[m]) and bool((found[~m] == PREFILL).all()) and int((~m).sum()) == 40
    matched = host['matched_expected'] != 0
    assert int(found[m].sum()) > int(matched[m].sum())                                    # the re-classification found some
    assert int((found[m] == 0).sum()) > 0                                                  # and not all
    # column 0 alone is read: other columns change nothing
    if k > 1:
        other = dict(host, indices=host['indices'].clone())
        other['indices'][:, 1:] = 0
        again, again_count = _launch_verdict(cuda, other)
        assert torch.equal(again, found) and torch.equal(again_count, found_count)
    # an empty match result: every row is beyond it, found = matched
    none = dict(host, indices=torch.zeros((0, k), dtype=torch.int64))
    f0, c0 = _launch_verdict(cuda, none)
    assert torch.equal(f0[m] != 0, matched[m]) and c0.tolist() == _model_verdict(none, cap)[1].tolist()


def test_footprint_of_both_entry_points(cuda):
    """inputs and guard bands unchanged; slots beyond an image's count and the rows of an image without a homography stay unwritten"""
    from cvpce_amd import torch_ops_reclass  # noqa: F401
    images = [im for im in _plan_images() if len(im['matched']) <= 257]
    t, cap, (wboxes, windex, wcount, written) = _model_plan(images)
    assert cap == 257 and 0 in wcount.tolist() and (t['status'] != rc.OK).any()
    ins = {name: footprint.put(v, cuda) for name, v in t.items()}
    b = len(images)
    outs = [footprint.out((b, cap, 4), torch.float32, cuda), footprint.out((b, cap), torch.int32, cuda), footprint.out((b,), torch.int32, cuda)]
    v = lambda name: ins[name][0]
    run = lambda: torch.ops.cvpce_amd.reclass_plan(v('status'), v('matched_expected'), v('expected_positions'), v('off1'), v('image'), *[o[0] for o in outs])
    mask = torch.from_numpy(written)
    # (float boxes: the footprint's finiteness test holds because a NaN position is never valid, an infinite one is clamped)
    res = footprint.check(run, list(ins.values()), outs, written=[mask[:, :, None], mask, None])
    assert res[2].cpu().tolist() == wcount.tolist()
    assert torch.equal(res[0].cpu().view(torch.int32)[mask], torch.from_numpy(wboxes).view(torch.int32)[mask])

    host, cap = _verdict_case(3)
    want_found, want_count, rows = _model_verdict(host, cap)
    vin = {name: footprint.put(x, cuda) for name, x in host.items()}
    vouts = [footprint.out((host['matched_expected'].numel(),), torch.int32, cuda), footprint.out((host['status'].numel(),), torch.int32, cuda)]
    verdict = lambda: torch.ops.cvpce_amd.reclass_verdict(*[vin[name][0] for name in VERDICT_ORDER], *[o[0] for o in vouts])
    res = footprint.check(verdict, list(vin.values()), vouts, written=[torch.from_numpy(rows), None])
    assert res[1].cpu().tolist() == want_count.tolist()
    assert torch.equal(res[0].cpu()[torch.from_numpy(rows)], torch.from_numpy(want_found)[torch.from_numpy(rows)])


def test_thirty_launches_are_bit_identical(cuda):
    from cvpce_amd import torch_ops_reclass  # noqa: F401
    t, cap, _ = _model_plan(_plan_images())
    first = _launch_plan(cuda, t, cap)
    host, vcap = _verdict_case(3)
    vfirst = _launch_verdict(cuda, host)
    for _ in range(29):
        assert all(torch.equal(a, b) for a, b in zip(first, _launch_plan(cuda, t, cap)))
        assert all(torch.equal(a, b) for a, b in zip(vfirst, _launch_verdict(cuda, host)))


def test_ops_refuse_bad_calls_before_any_launch(cuda):
    from cvpce_amd import torch_ops_reclass  # noqa: F401
    t, cap, _ = _model_plan(_plan_images()[:2])
    d = {name: v.to(cuda) for name, v in t.items()}
    b = 2
    boxes, index, count = torch.empty((b, cap, 4), device=cuda), torch.empty((b, cap), dtype=torch.int32, device=cuda), torch.empty(b, dtype=torch.int32, device=cuda)
    plan = lambda **kw: torch.ops.cvpce_amd.reclass_plan(*[kw.get(n, d[n]) for n in ('status', 'matched_expected', 'expected_positions', 'off1', 'image')],
                                                         kw.get('boxes', boxes), kw.get('expected_index', index), kw.get('count', count))
    plan()
    for bad in (dict(status=d['status'].to(torch.int64)), dict(expected_positions=d['expected_positions'].double()), dict(off1=d['off1'][:-1]),
                dict(boxes=torch.empty((b, cap + 1, 4), device=cuda)), dict(expected_index=index.t().contiguous().t()), dict(image=d['image'][:, :2].contiguous()),
                dict(expected_index=torch.empty((b, 1025), dtype=torch.int32, device=cuda), boxes=torch.empty((b, 1025, 4), device=cuda))):
        with pytest.raises(RuntimeError, match='cvpce_reclass_plan'):
            plan(**bad)
    host, vcap = _verdict_case(1)
    dv = {name: host[name].to(cuda) for name in VERDICT_ORDER}
    found, fc = torch.empty(host['matched_expected'].numel(), dtype=torch.int32, device=cuda), torch.empty(5, dtype=torch.int32, device=cuda)
    verdict = lambda **kw: torch.ops.cvpce_amd.reclass_verdict(*[kw.get(n, dv[n]) for n in VERDICT_ORDER], kw.get('found', found), kw.get('found_count', fc))
    verdict()
    for bad in (dict(indices=dv['indices'].to(torch.int32)), dict(slot_row=dv['slot_row'][:, :-1].contiguous()), dict(found=found[:-1]),
                dict(expected_label_id=dv['expected_label_id'][:-1]), dict(indices=dv['indices'][:, 0]), dict(found_count=fc[:-1])):
        with pytest.raises(RuntimeError, match='cvpce_reclass_verdict'):
            verdict(**bad)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# through planograms_device and the comparator
# ---------------------------------------------------------------------------------------------------------------------
_PIPE = {}


def _pipeline(cuda):
    """the small synthetic pipeline of tests/test_gpu_homography_device.py (detector, embedder, a gallery of 24 under 6 labels, four shelf
    images of two sizes) and its detections, made once"""
    if not _PIPE:
        from cvpce_amd import production, synthetic
        det = synthetic.synthetic_gln(seed=0, detections_per_img=40).to(cuda)
        enc = synthetic.synthetic_macvgg(seed=1).to(cuda)
        gal = synthetic.gallery_images(24, seed=17)
        clf = production.Classifier(enc, synthetic.TensorGallery(gal, [f'sku{i % 6}' for i in range(24)]), device=cuda, emb_device=cuda, batch_size=8)
        pg = production.ProposalGenerator(det, device=cuda, confidence_threshold=0.5)
        imgs = [synthetic.shelf_image(60, 512, 640), synthetic.shelf_image(61, 512, 640), synthetic.shelf_image(62, 448, 512),
                synthetic.shelf_image(63, 512, 640)]
        dets = production.PlanogramEvaluator(pg, clf, production.PlanogramComparator()).detect_and_classify_batch(imgs)
        _PIPE.update(det=det, enc=enc, clf=clf, pg=pg, imgs=imgs, dets=dets)
    return _PIPE


def _withheld(b, labels):
    """the detections minus every third"""
    keep = [i for i in range(len(b)) if i % 3 != 1]
    return b[keep], [labels[i] for i in keep]


def _planograms(dets):
    """ALL detections with their labels at half scale, every seventh label replaced by one outside the gallery"""
    return [{'boxes': b * 0.5, 'labels': [('other' if i % 7 == 0 else l[i]) for i in range(len(b))]} for b, l in dets]


class _Spy:
    """stands in for `Classifier.classify` on one classifier object and counts what went through it"""

    def __init__(self, clf):
        self.clf, self.calls, self.crops = clf, 0, 0

    def __enter__(self):
        inner = self.clf.classify

        def classify(images, *a, **kw):
            self.calls += 1
            self.crops += len(images)
            return inner(images, *a, **kw)
        self.clf.classify = classify
        return self

    def __exit__(self, *exc):
        del self.clf.classify


def _same(got, want):
    """equal as floats, and of equal type (and dtype and shape where they are tensors)"""
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert type(g) is type(w) and float(g) == float(w), (g, w)
        if torch.is_tensor(w):
            assert g.dtype == w.dtype and g.shape == w.shape and g.device == w.device, (g, w)


def test_all_three_switches_equal_the_tail_switch_exactly(cuda):
    from cvpce_amd import datautils, planograms, production
    p = _pipeline(cuda)
    clf, pg, imgs, dets = p['clf'], p['pg'], p['imgs'], p['dets']
    planos = _planograms(dets)
    actuals = [dict(zip(('boxes', 'labels'), _withheld(b, l))) for b, l in dets]
    # the host tail stays clear of both thresholds on these planograms: a differing verdict cannot hide behind a borderline input
    for img, plano, a in zip(imgs, planos, actuals):
        m = planograms.large_common_subgraph(planograms.build_graph(plano['boxes'], plano['labels'], 0.5), planograms.build_graph(a['boxes'], a['labels'], 0.5))
        assert len(m) >= 2
        margins = _host_margins(m, plano, a, min(datautils.image_hw(img)) * 0.01)
        assert margins is not None and margins[0] >= 1e-6 and margins[1] >= 1e-4, margins
    tail = production.PlanogramComparator(device_graphs=True, device_tail=True)
    # the precondition, on the switch-off path: the re-classification recovers at least one position and fails on at least one
    with _Spy(clf) as spy:
        want = tail.compare_batch(planos, actuals, imgs, clf)
    without = tail.compare_batch(planos, actuals, imgs, None)
    recovered = sum(round((float(w) - float(o)) * len(pl['labels'])) for w, o, pl in zip(want, without, planos))
    print(f'classify calls {spy.calls}, positions {spy.crops}, recovered {recovered}, verdicts {[float(v) for v in want]}')
    assert spy.calls >= 2 and recovered >= 1 and spy.crops - recovered >= 1
    assert any(0.0 < float(v) < 1.0 for v in want)

    class Withholding(production.PlanogramEvaluator):
        def detect_and_classify_batch(self, images):
            return [_withheld(b, l) for b, l in super().detect_and_classify_batch(images)]

    on_cmp = production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True)
    off, on = Withholding(pg, clf, tail), Withholding(pg, clf, on_cmp)
    want_batch = off.evaluate_batch(imgs, planos)
    want_iter = {la: list(off.evaluate_iter(zip(imgs, planos), lookahead=la)) for la in (1, 4)}
    _same(want_batch, want)
    with _Spy(clf) as spy:
        _same(on_cmp.compare_batch(planos, actuals, imgs, clf), want)
        _same(on.evaluate_batch(imgs, planos), want_batch)
        for la in (1, 4):
            _same(list(on.evaluate_iter(zip(imgs, planos), lookahead=la)), want_iter[la])
        _same([on_cmp.compare(pl, a, img, clf) for pl, a, img in zip(planos, actuals, imgs)], want)
    assert spy.calls == 0, 'classify ran with the switch on'
    assert on_cmp.host_routed == 0 and on_cmp.reclass_host_routed == 0
    assert all(pl[production.PlanogramComparator.LABEL_IDS_KEY][0] == clf.index_generation for pl in planos)


def test_the_other_branches_return_what_the_switch_off_path_returns(cuda, monkeypatch):
    from cvpce_amd import planograms_device as pd, production
    import planogram_device_cases as cases
    p = _pipeline(cuda)
    clf, imgs, dets = p['clf'], p['imgs'], p['dets']
    planos = _planograms(dets)
    actuals = [dict(zip(('boxes', 'labels'), _withheld(b, l))) for b, l in dets]
    tail = production.PlanogramComparator(device_graphs=True, device_tail=True)
    on = production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True)
    passes = []
    inner = pd.reclassify_batch
    monkeypatch.setattr(pd, 'reclassify_batch', lambda *a, **kw: passes.append(1) or inner(*a, **kw))
    # an image of None beside images that are there; no detections; an empty planogram
    some = [imgs[0], None, imgs[2], None]
    _same(on.compare_batch(planos, actuals, some, clf), tail.compare_batch(planos, actuals, some, clf))
    assert len(passes) == 1
    empty = [actuals[0], {'boxes': torch.zeros(0, 4), 'labels': []}, actuals[2], actuals[3]]
    _same(on.compare_batch(planos, empty, imgs, clf), tail.compare_batch(planos, empty, imgs, clf))
    assert len(passes) == 2
    # no image at all, and no classifier: nothing is classified
    _same(on.compare_batch(planos, actuals, None, clf), tail.compare_batch(planos, actuals, None, clf))
    _same(on.compare_batch(planos, actuals, imgs, None), tail.compare_batch(planos, actuals, imgs, None))
    assert len(passes) == 2
    # a window whose counts are all 0: every expected box has its detection
    full = [{'boxes': b, 'labels': list(l)} for b, l in dets]
    exact = [{'boxes': b * 0.5, 'labels': list(l)} for b, l in dets]
    with _Spy(clf) as spy:
        want = tail.compare_batch(exact, full, imgs, clf)
        _same(on.compare_batch(exact, full, imgs, clf), want)
    assert len(passes) == 2 and spy.calls == 0
    # a matching without a homography beside one with: a single shared label leaves one pair
    lone_e, lone_a = cases.scene(30, 3), cases.scene(30, 4)
    lone = ({'boxes': lone_e[0], 'labels': list(lone_e[1])}, {'boxes': lone_a[0], 'labels': ['nothing'] * 29 + [lone_e[1][0]]})
    mixed_e, mixed_a, mixed_i = [planos[0], lone[0]], [actuals[0], lone[1]], [imgs[0], imgs[0]]
    _same(on.compare_batch(mixed_e, mixed_a, mixed_i, clf), tail.compare_batch(mixed_e, mixed_a, mixed_i, clf))
    assert len(passes) == 3
    # an image beyond the cap takes the host path, with the switch on as with it off
    big = dict(zip(('boxes', 'labels'), cases.scene(pd.MAX_NODES + 1, 0)))

    class Routed(production.PlanogramComparator):
        def _compare_host(self, expected, actual, image, classifier):
            return 0.25

    r_on, r_off = Routed(device_graphs=True, device_tail=True, device_reclass=True), Routed(device_graphs=True, device_tail=True)
    _same(r_on.compare_batch([big, planos[0]], [actuals[0], actuals[0]], [imgs[0], imgs[0]], clf),
          r_off.compare_batch([big, planos[0]], [actuals[0], actuals[0]], [imgs[0], imgs[0]], clf))
    assert r_on.host_routed == 1 and len(passes) == 4
    # annotations that cannot be hashed leave no id space: the window takes the per-image re-classification and is counted
    odd = production.Classifier.from_embedding(p['enc'], clf.embedding, [[a] for a in clf.annotations], device=cuda, emb_device=cuda, batch_size=8)
    with _Spy(odd) as spy:
        got = on.compare_batch(planos[:1], actuals[:1], imgs[:1], odd)
    assert on.reclass_host_routed == 1 and spy.calls == 1 and len(passes) == 4
    _same(got, tail.compare_batch(planos[:1], actuals[:1], imgs[:1], odd))


# digest of `BatchedPipeline.run` on two images with planted proposals, computed on the commit before `production.roi_crops` was factored out of `_crops`
CROP_HELPER_DIGEST = 'b5350ddb1e48faae8719ab7b17985673a01a08b0a3b04607cf8440b7d83a4dc8'


def _run_digest(out):
    """sha256 over what a run returns for the confident boxes of every image (slots beyond an image's count hold no result)"""
    h = hashlib.sha256()
    parts = [('count', out['count']), ('embeddings', out['embeddings'])]
    for j, c in enumerate(out['counts_host']):
        parts += [(f'{key}{j}', out[key][j, :c]) for key in ('boxes', 'scores', 'labels', 'indices')]
    for name, t in parts:
        t = t.detach().cpu().contiguous()
        h.update(name.encode() + str(tuple(t.shape)).encode() + str(t.dtype).encode())
        h.update(t.view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def test_the_refactored_crop_helper_leaves_the_batched_pipeline_unchanged(cuda):
    from cvpce_amd import production
    p = _pipeline(cuda)
    pipe = production.BatchedPipeline(p['det'], p['clf'], 0.5)
    imgs = [p['imgs'][0].to(cuda), p['imgs'][1].to(cuda)]
    out = pipe.run(imgs, proposals=_planted_proposals(cuda))
    torch.cuda.synchronize()
    assert out['counts_host'] == [17, 33]                        # (fewer than the 40 slots: the compaction of `_select` is on the path)
    assert _run_digest(out) == CROP_HELPER_DIGEST
    again = pipe.run(imgs, proposals=_planted_proposals(cuda))
    assert all(torch.equal(out[key], again[key]) for key in ('indices', 'embeddings'))


# The comparator's device window before its routes were folded into one (planograms_device's named launches and blob layouts,
# `PlanogramComparator._device_window`): measured on commit f40041d on an MI355X, per route sha256 of compare_batch's verdicts and of
# every field of report_batch's reports, and what the two calls cost together under `WindowCounter` (kernels, torch_device_ops, waits).
WINDOW_ROUTES = {
    'tail': (dict(), False),
    'tail_reclass': (dict(device_reclass=True), False),
    'actuals': (dict(), True),
    'actuals_reclass': (dict(device_reclass=True), True),
}
WINDOW_DIGEST = 'e9eff137e882e015e012b760ef6550964bff73b6c1ad9ab66ab1cc0e9d11e1e1'                   # (the parent's on all four routes)
WINDOW_PARENT = {
    'tail': (WINDOW_DIGEST, 329, 829, 10),
    'tail_reclass': (WINDOW_DIGEST, 104, 401, 4),
    'actuals': (WINDOW_DIGEST, 331, 831, 10),
    'actuals_reclass': (WINDOW_DIGEST, 106, 403, 4),
}


def _device_actuals(cuda, clf, actuals):
    """host detections as the pack `actuals_pack` would leave of them: a label's gallery row is the first that carries it"""
    from cvpce_amd import planograms_device as pd, staging
    n2 = [len(a['labels']) for a in actuals]
    rows = [clf.annotations.index(l) for a in actuals for l in a['labels']]
    i32 = lambda values: torch.tensor(values, dtype=torch.int32, device=cuda)
    boxes = torch.cat([a['boxes'] for a in actuals]).to(torch.float32).contiguous().to(cuda)
    thresh = torch.stack([pd.graph_threshold(a['boxes'].to(torch.float32), 0.5) for a in actuals]).to(torch.float32).to(cuda)
    return pd.DeviceActuals(boxes, i32(rows), i32([clf.label_ids[clf.annotations[r]] for r in rows]), thresh, i32([0] * len(n2)),
                            i32(staging.offsets(n2)), n2, 0.5)


def _window_digest(verdicts, reports):
    """sha256 over the verdicts of a window and over every field of its reports (tensors by shape, dtype and bytes)"""
    h = hashlib.sha256()

    def add(name, v):
        if torch.is_tensor(v):
            v = v.detach().cpu().contiguous()
            h.update(name.encode() + str(tuple(v.shape)).encode() + str(v.dtype).encode())
            h.update(v.reshape(-1).view(torch.uint8).numpy().tobytes())
        else:
            h.update(name.encode() + type(v).__name__.encode() + repr(v).encode())
    for i, v in enumerate(verdicts):
        add(f'verdict{i}', v)
    for i, r in enumerate(reports):
        add(f'compliance{i}', r.compliance)
        add(f'reason{i}', r.status)
        for field in r.FIELDS:
            add(f'{field}{i}', getattr(r, field))
    return h.hexdigest()


def _window_route(cuda, name):
    """one route of WINDOW_ROUTES over the window of `_pipeline` -> (digest, kernels, torch_device_ops, waits, verdicts, reports)"""
    from cvpce_amd import production
    from test_gpu_actuals import _window_counter
    p = _pipeline(cuda)
    clf, imgs, dets = p['clf'], p['imgs'], p['dets']
    switches, on_device = WINDOW_ROUTES[name]
    planos = _planograms(dets)                                    # (fresh dicts: every route fills its own caches in its first call)
    actuals = [dict(zip(('boxes', 'labels'), _withheld(b, l))) for b, l in dets]
    side = _device_actuals(cuda, clf, actuals) if on_device else actuals
    cmp = production.PlanogramComparator(device_graphs=True, device_tail=True, **switches)
    verdicts, reports = cmp.compare_batch(planos, side, imgs, clf), cmp.report_batch(planos, side, imgs, clf)
    counter = _window_counter()
    with counter:
        cmp.compare_batch(planos, side, imgs, clf)
        cmp.report_batch(planos, side, imgs, clf)
    assert cmp.host_routed == 0 and cmp.reclass_host_routed == 0
    return _window_digest(verdicts, reports), counter.kernels, counter.torch_device_ops, counter.waits, verdicts, reports


def test_the_single_device_window_leaves_every_route_unchanged(cuda):
    """the window of `test_all_three_switches_equal_the_tail_switch_exactly` (positions recovered and missing, verdicts strictly
    between 0 and 1) on each device route: the outputs and the launches and waits are the parent's, the torch operators no more"""
    got = {route: _window_route(cuda, route) for route in WINDOW_ROUTES}
    for route, (digest, kernels, torch_ops, waits, verdicts, _) in got.items():
        print(f'{route}: digest {digest}, kernels {kernels}, torch_device_ops {torch_ops}, waits {waits}, verdicts {[float(v) for v in verdicts]}')
    for route, (digest, kernels, torch_ops, waits, verdicts, reports) in got.items():
        assert any(0.0 < float(v) < 1.0 for v in verdicts) and all(r.status == 'ok' for r in reports), route
        outcomes = torch.cat([r.outcomes for r in reports]).tolist()
        assert 1 in outcomes and 2 in outcomes, route                                     # recovered and missing, both
        want = WINDOW_PARENT[route]
        assert digest == want[0], route
        assert (kernels, waits) == (want[1], want[3]) and torch_ops <= want[2], route


def _planted_proposals(cuda):
    """planted boxes for two 512 x 640 images of 40 slots, 17 and 33 of them counted: some small, some large, some at the image's edge"""
    g = torch.Generator().manual_seed(5)
    wh = torch.rand(2, 40, 2, generator=g) * torch.tensor([200.0, 160.0]) + 6
    xy = torch.rand(2, 40, 2, generator=g) * (torch.tensor([640.0, 512.0]) - wh)
    xy[:, ::9] = 0.0
    boxes = torch.cat((xy, xy + wh), dim=2).to(torch.float32).contiguous()
    return boxes.to(cuda), torch.tensor([17, 33], dtype=torch.int32, device=cuda)
