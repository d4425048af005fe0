"""The device detections path on the GPU: the two kernels of csrc/actuals.hip equal the plain restatement of the rule
(tests/actuals_cases.py, pinned against `production._nondegenerate` and `planograms_device.graph_threshold` in test_actuals_cpu.py) bit
for bit and write only what the header says; `BatchedPipeline.run(actuals=True)` packs what `detect_and_classify_batch` derives from
the same result; and the evaluator with `device_detections` on gives the verdicts of the switch-off path exactly, with two waits
less per size group."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import actuals_cases as ac
import footprint
from test_gpu_reclass import CROP_HELPER_DIGEST, _Spy, _pipeline, _planograms, _planted_proposals, _run_digest, _same

pytestmark = pytest.mark.gpu

PREFILL = 0x5A5A5A5A
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the share of the confident detections the evaluator's higher threshold keeps (end-to-end test).  One generator has one threshold, so
# the share is taken over the window: 107 of its 160 detections -- 29, 29, 33 and 16 of the four images' 40
KEEP = 2 / 3


def _inputs(cuda, k, indices=None):
    _, gallery_ids = ac.label_ids()
    indices = ac.make_indices(k) if indices is None else indices
    return (torch.from_numpy(ac.BOXES).to(cuda), torch.from_numpy(ac.COUNT).to(cuda), torch.from_numpy(indices).to(cuda),
            torch.from_numpy(gallery_ids).to(cuda)), indices, gallery_ids


def _launch_count(cuda):
    from cvpce_amd import torch_ops_actuals  # noqa: F401
    kept = torch.full((ac.B,), PREFILL, dtype=torch.int32, device=cuda)
    torch.ops.cvpce_amd.actuals_count(torch.from_numpy(ac.BOXES).to(cuda), torch.from_numpy(ac.COUNT).to(cuda), kept)
    return kept.cpu()


def _launch_pack(cuda, k, thresh_size, off2=None, indices=None):
    """the pack kernel on plain tensors prefilled with a pattern -> host (boxes as int32 bits, row, label, thresh as bits, status)"""
    from cvpce_amd import torch_ops_actuals  # noqa: F401
    (boxes, count, idx, gallery), _, _ = _inputs(cuda, k, indices)
    off2 = ac.OFF2 if off2 is None else off2
    sum2 = int(off2[-1])
    outs = [torch.full(shape, PREFILL, dtype=torch.int32, device=cuda) for shape in ((sum2, 4), (sum2,), (sum2,), (ac.B,), (ac.B,))]
    torch.ops.cvpce_amd.actuals_pack(boxes, count, idx, gallery, torch.from_numpy(off2).to(cuda), thresh_size, outs[0].view(torch.float32), outs[1],
                                     outs[2], outs[3].view(torch.float32), outs[4])
    return [o.cpu() for o in outs]


def _assert_pack(got, want, what):
    boxes, row, label, thresh, status = got
    wboxes, wrow, wlabel, wthresh, wstatus, rows, tw = want
    rows, tw = torch.from_numpy(rows), torch.from_numpy(tw)
    assert status.tolist() == wstatus.tolist(), what
    assert torch.equal(boxes[rows], torch.from_numpy(wboxes).view(torch.int32)[rows]), what                # bit for bit
    assert torch.equal(row[rows], torch.from_numpy(wrow)[rows]) and torch.equal(label[rows], torch.from_numpy(wlabel)[rows]), what
    assert torch.equal(thresh[tw], torch.from_numpy(wthresh).view(torch.int32)[tw]), (what, thresh.view(torch.float32), wthresh)
    assert bool((boxes[~rows] == PREFILL).all()) and bool((row[~rows] == PREFILL).all()) and bool((label[~rows] == PREFILL).all()), (what, 'a row beyond the kept boxes was written')
    assert bool((thresh[~tw] == PREFILL).all()), (what, 'the threshold of an image that keeps nothing was written')


@pytest.mark.parametrize('k', ac.KS)
def test_both_kernels_equal_the_model_bit_for_bit(cuda, k):
    assert _launch_count(cuda).tolist() == ac.KEPT.tolist()
    for thresh_size in ac.THRESH_SIZES:
        (_, _, _, _), indices, gallery_ids = _inputs(cuda, k)
        want = ac.model_pack(ac.BOXES, ac.COUNT, indices, gallery_ids, ac.OFF2, thresh_size)
        assert want[5].all() and want[6].tolist() == [bool(n) for n in ac.KEPT] and not want[4].any()
        _assert_pack(_launch_pack(cuda, k, thresh_size), want, (k, thresh_size))
    if k > 1:                                      # column 0 alone is read: other columns change nothing
        other = ac.make_indices(k)
        other[:, :, 1:] = 0
        assert all(torch.equal(a, b) for a, b in zip(_launch_pack(cuda, k, 0.5), _launch_pack(cuda, k, 0.5, indices=other)))


def test_footprint_of_both_entry_points(cuda):
    """inputs and guard bands unchanged (the NaN boxes and -1 indices beyond the counts never reach a result); every output row is
    written, nothing beyond `sum2`; the thresholds of the two images that keep nothing stay unwritten"""
    from cvpce_amd import torch_ops_actuals  # noqa: F401
    _, gallery_ids = ac.label_ids()
    indices = ac.make_indices(3)
    want = ac.model_pack(ac.BOXES, ac.COUNT, indices, gallery_ids, ac.OFF2, 0.3)
    ins = [footprint.put(torch.from_numpy(x), cuda) for x in (ac.BOXES, ac.COUNT)]
    kept = footprint.out((ac.B,), torch.int32, cuda)
    res = footprint.check(lambda: torch.ops.cvpce_amd.actuals_count(ins[0][0], ins[1][0], kept[0]), ins, [kept])
    assert res[0].cpu().tolist() == ac.KEPT.tolist()

    pins = ins + [footprint.put(torch.from_numpy(x), cuda) for x in (indices, gallery_ids, ac.OFF2)]
    sum2 = int(ac.OFF2[-1])
    outs = [footprint.out((sum2, 4), torch.float32, cuda), footprint.out((sum2,), torch.int32, cuda), footprint.out((sum2,), torch.int32, cuda),
            footprint.out((ac.B,), torch.float32, cuda), footprint.out((ac.B,), torch.int32, cuda)]
    run = lambda: torch.ops.cvpce_amd.actuals_pack(pins[0][0], pins[1][0], pins[2][0], pins[3][0], pins[4][0], 0.3, *[o[0] for o in outs])
    tw = torch.from_numpy(want[6])
    assert int((~tw).sum()) == 2
    res = footprint.check(run, pins, outs, written=[None, None, None, tw, None])
    assert torch.equal(res[0].cpu().view(torch.int32), torch.from_numpy(want[0]).view(torch.int32))
    assert res[1].cpu().tolist() == want[1].tolist() and res[2].cpu().tolist() == want[2].tolist() and res[4].cpu().tolist() == [0] * ac.B
    assert torch.equal(res[3].cpu().view(torch.int32)[tw], torch.from_numpy(want[3]).view(torch.int32)[tw])


def test_thirty_launches_are_bit_identical(cuda):
    first, cfirst = _launch_pack(cuda, 3, 0.3), _launch_count(cuda)
    for _ in range(29):
        assert torch.equal(cfirst, _launch_count(cuda))
        assert all(torch.equal(a, b) for a, b in zip(first, _launch_pack(cuda, 3, 0.3)))


def test_stale_offsets_and_rows_outside_the_gallery_are_reported(cuda):
    """both inputs are in bounds by construction: the offsets stay inside the output, the row is checked before it is used"""
    _, gallery_ids = ac.label_ids()
    stale = ac.OFF2.copy()
    stale[4:] -= 3                                                             # image 3 is given three rows too few
    want = ac.model_pack(ac.BOXES, ac.COUNT, ac.make_indices(1), gallery_ids, stale, 0.5)
    assert want[4].tolist() == [0, 0, 0, 1, 0, 0, 0, 0]
    _assert_pack(_launch_pack(cuda, 1, 0.5, off2=stale), want, 'stale off2')
    indices = ac.make_indices(3)
    first = int(np.nonzero(ac.kept_mask(ac.BOXES[5, :256]))[0][0])
    indices[5, first, 0] = ac.G                                                # the first row beyond the gallery
    indices[7, int(np.nonzero(ac.kept_mask(ac.BOXES[7, :300]))[0][-1]), 0] = -1
    want = ac.model_pack(ac.BOXES, ac.COUNT, indices, gallery_ids, ac.OFF2, 0.5)
    assert want[4].tolist() == [0, 0, 0, 0, 0, 2, 0, 2] and want[1][ac.OFF2[5]] == -1 and want[2][ac.OFF2[5]] == 0
    _assert_pack(_launch_pack(cuda, 3, 0.5, indices=indices), want, 'row outside the gallery')


def test_ops_refuse_bad_calls_before_any_launch(cuda):
    from cvpce_amd import torch_ops_actuals  # noqa: F401
    (boxes, count, idx, gallery), _, _ = _inputs(cuda, 3)
    off2, sum2 = torch.from_numpy(ac.OFF2).to(cuda), int(ac.OFF2[-1])
    i32 = lambda *s: torch.empty(s, dtype=torch.int32, device=cuda)
    kept = i32(ac.B)
    d = dict(boxes=boxes, count=count, kept=kept)
    call = lambda **kw: torch.ops.cvpce_amd.actuals_count(*[kw.get(n, d[n]) for n in ('boxes', 'count', 'kept')])
    call()
    for bad in (dict(boxes=boxes.double()), dict(count=count.long()), dict(kept=kept[:-1]), dict(boxes=boxes[:, :, :3].contiguous()),
                dict(boxes=boxes.transpose(0, 1)), dict(count=count[:-1]), dict(boxes=boxes[:, :0])):
        with pytest.raises(RuntimeError, match='cvpce_actuals_count'):
            call(**bad)
    names = ('boxes', 'count', 'indices', 'gallery_label_id', 'off2', 'thresh_size', 'out_boxes', 'out_row', 'out_label', 'thresh', 'status')
    p = dict(boxes=boxes, count=count, indices=idx, gallery_label_id=gallery, off2=off2, thresh_size=0.5, out_boxes=torch.empty((sum2, 4), device=cuda),
             out_row=i32(sum2), out_label=i32(sum2), thresh=torch.empty(ac.B, device=cuda), status=i32(ac.B))
    pack = lambda **kw: torch.ops.cvpce_amd.actuals_pack(*[kw.get(n, p[n]) for n in names])
    pack()
    for bad in (dict(indices=idx.to(torch.int32)), dict(indices=idx[:, :, 0]), dict(indices=idx[:, :-1].contiguous()), dict(indices=idx.transpose(1, 2)),
                dict(gallery_label_id=gallery.long()), dict(off2=off2[:-1]), dict(out_boxes=torch.empty((sum2, 3), device=cuda)),
                dict(out_row=i32(sum2 - 1)), dict(out_label=i32(sum2 + 1)), dict(thresh=i32(ac.B)), dict(thresh=torch.empty(ac.B - 1, device=cuda)),
                dict(status=i32(ac.B + 1)), dict(out_boxes=torch.empty((sum2, 4), dtype=torch.float64, device=cuda))):
        with pytest.raises(RuntimeError, match='cvpce_actuals_pack'):
            pack(**bad)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------
# through BatchedPipeline
# ---------------------------------------------------------------------------------------------------------------------
def _degenerate_proposals(cuda):
    """`_planted_proposals` (two 512 x 640 images, 17 and 33 of 40 slots counted) with degenerate boxes planted inside the counts, at
    irregular slots, and beyond them"""
    boxes, counts = _planted_proposals(cuda)
    boxes = boxes.cpu().clone()
    fraction, zero, flat, negative = (10.2, 5.0, 10.9, 9.0), (-0.5, 5.0, 0.4, 9.0), (3.0, 7.2, 30.0, 7.9), (50.0, 5.0, 20.0, 9.0)
    for img, slot, box in ((0, 0, fraction), (0, 5, zero), (0, 16, flat), (0, 30, negative), (1, 3, negative), (1, 4, flat), (1, 11, zero), (1, 32, fraction),
                           (1, 36, flat)):
        boxes[img, slot] = torch.tensor(box)
    boxes[0, 9] = torch.tensor((10.9, 5.0, 11.1, 9.0))                        # a width of exactly 1 after truncation: kept
    return boxes.to(cuda), counts


def test_run_with_actuals_packs_what_the_host_derives_from_the_same_result(cuda):
    from cvpce_amd import planograms_device as pd, production
    p = _pipeline(cuda)
    clf = p['clf']
    pipe = production.BatchedPipeline(p['det'], clf, 0.5)
    pipe.actuals_thresh_size = 0.3
    imgs = [p['imgs'][0].to(cuda), p['imgs'][1].to(cuda)]
    out = pipe.run(imgs, proposals=_degenerate_proposals(cuda), actuals=True)
    pack = out['actuals']
    assert isinstance(pack, pd.DeviceActuals) and out['counts_host'] == [17, 33] and pack.n2 == [14, 29] and pack.thresh_size == 0.3
    assert pack.status.tolist() == [0, 0] and pack.off2.tolist() == [0, 14, 43]
    # today's `detect_and_classify_batch` arithmetic on the same result dict
    boxes, indices = out['boxes'].cpu(), out['indices'][:, :, 0].cpu()
    for j, c in enumerate(out['counts_host']):
        b, ix = boxes[j, :c], indices[j, :c]
        ok = production._nondegenerate(b)
        b, ix = b[ok], ix[ok]
        labels = [clf.annotations[r] for r in ix.tolist()]
        got_boxes, got_labels = pack.to_host(j, clf.annotations)
        assert not got_boxes.is_cuda and torch.equal(got_boxes.view(torch.int32), b.view(torch.int32)) and got_labels == labels
        o = pack.off2.tolist()
        assert pack.label[o[j]:o[j + 1]].tolist() == [clf.label_ids[l] for l in labels]
        want = pd.graph_threshold(b, 0.3)
        assert pack.thresh[j:j + 1].cpu().view(torch.int32).item() == want.reshape(1).view(torch.int32).item()
    # the packs of two groups joined, and a part of a pack, are the same rows
    both = pd.DeviceActuals.concat([pack, pack])
    assert both.n2 == [14, 29, 14, 29] and both.off2.tolist() == [0, 14, 43, 57, 86] and torch.equal(both.boxes[43:], pack.boxes)
    one = pack.select([1])
    assert one.n2 == [29] and one.off2.tolist() == [0, 29] and torch.equal(one.boxes, pack.boxes[14:]) and torch.equal(one.thresh, pack.thresh[1:])
    assert pack.select([0, 1]) is pack
    # the flag changes nothing else: the same keys and bits with it, and without it the run of before
    plain = pipe.run(imgs, proposals=_degenerate_proposals(cuda))
    assert set(plain) == set(out) - {'actuals'} == {'boxes', 'scores', 'labels', 'count', 'det_count', 'indices', 'gaussians', 'embeddings', 'counts_host'}
    assert _run_digest(plain) == _run_digest(out)
    before = pipe.run(imgs, proposals=_planted_proposals(cuda))
    torch.cuda.synchronize()
    assert _run_digest(before) == CROP_HELPER_DIGEST
    odd = production.Classifier.from_embedding(p['enc'], clf.embedding, [[a] for a in clf.annotations], device=cuda, emb_device=cuda, batch_size=8)
    with pytest.raises(ValueError, match='id space'):
        production.BatchedPipeline(p['det'], odd, 0.5).run(imgs, actuals=True)


def test_compare_batch_on_device_actuals_takes_the_other_branches(cuda):
    """an image whose planogram has no device form comes back through `to_host`; an image without detections needs no launch; the
    comparator refuses a pack it cannot read"""
    from cvpce_amd import planograms_device as pd, production
    import planogram_device_cases as cases
    p = _pipeline(cuda)
    clf = p['clf']
    pipe = production.BatchedPipeline(p['det'], clf, 0.5)
    imgs = [p['imgs'][0].to(cuda), p['imgs'][1].to(cuda)]
    boxes, counts = _degenerate_proposals(cuda)
    pack = pipe.run(imgs, proposals=(boxes, counts), actuals=True)['actuals']
    host = [dict(zip(('boxes', 'labels'), pack.to_host(j, clf.annotations))) for j in range(2)]
    plano = {'boxes': host[0]['boxes'] * 0.5, 'labels': ['other' if i % 7 == 0 else l for i, l in enumerate(host[0]['labels'])]}
    big = dict(zip(('boxes', 'labels'), cases.scene(pd.MAX_NODES + 1, 0)))

    class Routed(production.PlanogramComparator):
        seen = None

        def _compare_host(self, expected, actual, image, classifier):
            self.seen = actual
            return 0.25

    on, off = Routed(device_graphs=True, device_tail=True), Routed(device_graphs=True, device_tail=True)
    got = on.compare_batch([plano, big], pack, imgs, clf)
    _same(got, off.compare_batch([plano, big], host, imgs, clf))
    assert got[1] == 0.25 and on.host_routed == off.host_routed == 1 and 0 < float(got[0]) <= 1
    assert torch.equal(on.seen['boxes'], host[1]['boxes']) and on.seen['labels'] == host[1]['labels'] == off.seen['labels']
    # a label that cannot be hashed: no ids, the window goes back to the host
    odd = {'boxes': plano['boxes'], 'labels': [[l] for l in plano['labels']]}
    assert on.compare_batch([odd, plano], pack, imgs, clf) == [0.25, 0.25] and on.host_routed == 3
    # no detections in the first image
    none = pipe.run(imgs, proposals=(boxes, torch.tensor([0, 33], dtype=torch.int32, device=cuda)), actuals=True)['actuals']
    assert none.n2 == [0, 29]
    plano1 = {'boxes': host[1]['boxes'] * 0.5, 'labels': list(host[1]['labels'])}
    empty = {'boxes': torch.zeros(0, 4), 'labels': []}
    cmp = production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True)
    for first in (plano, empty):
        got = cmp.compare_batch([first, plano1], none, imgs, clf)
        _same(got, cmp.compare_batch([first, plano1], [empty, host[1]], imgs, clf))
        assert got[0] == (0 if first is plano else 1) and float(got[1]) > 0
    assert cmp.host_routed == 0
    for bad in (production.PlanogramComparator(device_graphs=True), production.PlanogramComparator(0.3, device_graphs=True, device_tail=True)):
        with pytest.raises(ValueError, match='device_graphs and device_tail|graph_threshold'):
            bad.compare_batch([plano, plano1], pack, imgs, clf)


# ---------------------------------------------------------------------------------------------------------------------
# through the evaluator
# ---------------------------------------------------------------------------------------------------------------------
def _window_counter():
    """`WindowCounter` of tools/bench_planogram_compare.py, and beside it what every blocking copy or scalar read was"""
    spec = importlib.util.spec_from_file_location('bench_planogram_compare', os.path.join(ROOT, 'tools', 'bench_planogram_compare.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)

    class Counter(mod.WindowCounter):
        def __init__(self):
            super().__init__()
            self.blocking = []

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            before = self.waits
            out = super().__torch_dispatch__(func, types, args, kwargs)
            if self.waits > before:
                self.blocking.append((str(func), [tuple(t.shape) for t in args if torch.is_tensor(t)]))
            return out
    return Counter()


def _higher_threshold(cuda, p, keep):
    """a confidence threshold above the planograms' 0.5 that keeps about `keep` of each image's confident detections: the score at
    that rank of the pooled confident scores, from the detector's own result"""
    from cvpce_amd import production
    pipe = production.BatchedPipeline(p['det'], p['clf'], 0.5)
    scores = []
    for idxs in ([0, 1, 3], [2]):
        out = pipe.run([p['imgs'][i].to(cuda) for i in idxs])
        scores += [out['scores'][j, :c].cpu() for j, c in enumerate(out['counts_host'])]
    pooled = torch.cat(scores).sort(descending=True).values
    at = int(round(len(pooled) * keep))
    t = float((pooled[at - 1] + pooled[at]) / 2)
    assert pooled[at - 1] > t > pooled[at] > 0.5, 'no threshold between two scores at this rank'
    return t, [int((s > t).sum()) for s in scores], [len(s) for s in scores]


def test_device_detections_equal_the_switch_off_path_exactly(cuda):
    from cvpce_amd import datautils, planograms_device as pd, production
    p = _pipeline(cuda)
    clf, det, imgs, dets = p['clf'], p['det'], p['imgs'], p['dets']
    planos = _planograms(dets)
    threshold, kept, confident = _higher_threshold(cuda, p, KEEP)
    print(f'threshold {threshold}: {kept} of {confident} detections kept')
    pg = production.ProposalGenerator(det, device=cuda, confidence_threshold=threshold)
    assert len({datautils.image_hw(i) for i in imgs}) == 2                                   # a window of two size groups
    # the preconditions, on the switch-off path
    tail = production.PlanogramComparator(device_graphs=True, device_tail=True)
    off_tail = production.PlanogramEvaluator(pg, clf, tail)
    actuals = [{'boxes': b, 'labels': l} for b, l in off_tail.detect_and_classify_batch(imgs)]
    ge = pd.build_graphs([(pl['boxes'], pl['labels']) for pl in planos])
    ga = pd.build_graphs([(a['boxes'], a['labels']) for a in actuals])
    records = pd.finalize_batch(ge, ga, pd.match_on_device(ge, ga), [pl['boxes'] for pl in planos], [a['boxes'] for a in actuals],
                                [min(datautils.image_hw(i)) * 0.01 for i in imgs])
    with _Spy(clf) as spy:
        want = tail.compare_batch(planos, actuals, imgs, clf)
    without = tail.compare_batch(planos, actuals, imgs, None)
    recovered = sum(round((float(w) - float(o)) * len(pl['labels'])) for w, o, pl in zip(want, without, planos))
    print(f"matchings {[r['matching'] for r in records]}, status {[r['status'] for r in records]}, classify calls {spy.calls}, positions {spy.crops}, "
          f'recovered {recovered}, verdicts {[float(v) for v in want]}')
    assert all(r['matching'] >= 2 and r['status'] == 'ok' for r in records)
    assert recovered >= 1 and spy.crops - recovered >= 1
    assert any(0.0 < float(v) < 1.0 for v in want)

    counter = None
    for switches in (dict(), dict(device_reclass=True)):
        off = production.PlanogramEvaluator(pg, clf, production.PlanogramComparator(device_graphs=True, device_tail=True, **switches))
        on = production.PlanogramEvaluator(pg, clf, production.PlanogramComparator(device_graphs=True, device_tail=True, **switches), device_detections=True)
        want_batch = off.evaluate_batch(imgs, planos)
        if not switches:
            _same(want_batch, want)
        _same(on.evaluate_batch(imgs, planos), want_batch)
        for la in (1, 4):
            _same(list(on.evaluate_iter(zip(imgs, planos), lookahead=la)), list(off.evaluate_iter(zip(imgs, planos), lookahead=la)))
        _same([on.evaluate(img, pl) for img, pl in zip(imgs, planos)], [off.evaluate(img, pl) for img, pl in zip(imgs, planos)])
        assert on.planogram_comparator.host_routed == 0 and on.detections_host_routed == 0
        assert all(pl[pd.IDS_KEY][0] == clf.index_generation and pl[pd.BOXES_KEY][1].is_cuda for pl in planos)
        # one window of g = 2 size groups: two blocking copies (boxes, indices) per group less, and no blocking copy left
        counts = {}
        for name, ev in (('off', off), ('on', on)):
            counter = _window_counter()
            with counter:
                ev.evaluate_batch(imgs, planos)
            counts[name] = counter
        print(f'{switches}: waits off {counts["off"].waits}, on {counts["on"].waits}; blocking off {counts["off"].blocking}, on {counts["on"].blocking}')
        assert counts['off'].waits - counts['on'].waits == 2 * 2
        dpi = det.detections_per_img
        copied = [shapes[0] for _, shapes in counts['on'].blocking if shapes]
        assert not any(s[-2:] == (dpi, 4) or s[-1:] == (dpi,) or s[-2:-1] == (dpi,) for s in copied), counts['on'].blocking
        assert sum(shapes[:1] in ([(3, dpi, 4)], [(1, dpi, 4)]) for _, shapes in counts['off'].blocking) == 2
    # an annotation that cannot be hashed leaves no id space: the window takes today's route and is counted.  (The extra gallery row
    # is never the nearest: MAC embeddings are non-negative, its cosine with every query is negative.)
    far = -clf.embedding.mean(dim=0, keepdim=True)
    odd = production.Classifier.from_embedding(p['enc'], torch.cat((clf.embedding, far / far.norm())), list(clf.annotations) + [['unhashable']],
                                               device=cuda, emb_device=cuda, batch_size=8)
    assert odd.label_ids is None and bool((clf.embedding >= 0).all())
    routed = production.PlanogramEvaluator(pg, odd, production.PlanogramComparator(device_graphs=True, device_tail=True), device_detections=True)
    _same(routed.evaluate_batch(imgs, planos), production.PlanogramEvaluator(pg, odd, tail).evaluate_batch(imgs, planos))
    assert routed.detections_host_routed == 1
    _same(routed.evaluate_batch(imgs, planos), want)
