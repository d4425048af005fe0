"""Detection matching on the device (csrc/evalmatch.hip, cvpce_amd.device_metrics) against the unchanged CPU routines of
cvpce_amd/metrics.py on the same inputs: flags, recall_300 and the whole result dictionary must be identical (torch.equal)."""
import re

import pytest
import torch

import device_metrics_cases as cases          # tests/device_metrics_cases.py
from test_gpu_cli import world, _run           # noqa: F401  (the tiny on-disk data sets and the CLI runner of tests/test_gpu_cli.py)

pytestmark = pytest.mark.gpu

COCO = tuple(torch.linspace(.5, .95, 10))
# seeds of synthetic.dense_detection_scene whose 1 000 `torch.rand` confidences are pairwise distinct (float32 rand has 2^24
# values: about 3 % of the seeds draw one twice -- 1015 and 1027 do, and are left out; the tests assert it for the rest)
DENSE_SEEDS = [s for s in range(1000, 1034) if s not in (1015, 1027)]


def _cpu_image(target, prediction, confidence, thresholds):
    """metrics._process_one -> (flags (K,P) float, recall_300 list, sorted confidences)."""
    from cvpce_amd import metrics
    m, conf, _ = metrics._process_one(target, prediction, confidence, thresholds)
    return (torch.stack([m[t]['true_positives'] for t in thresholds]) if len(thresholds) else None,
            [m[t]['recall_300'] for t in thresholds], conf)


def _check_against_cpu(cuda, targets, predictions, confidences, thresholds, name=''):
    """Flags of match_detections, and recall_300 / the result dictionary of DetectionMetrics, against metrics.py."""
    from cvpce_amd import metrics
    from cvpce_amd.device_metrics import DetectionMetrics, match_detections
    dev = lambda lst: [t.to(cuda) for t in lst]
    flags, first = match_detections(dev(targets), dev(predictions), dev(confidences), thresholds)
    for i, (t, p, c) in enumerate(zip(targets, predictions, confidences)):
        want, _, _ = _cpu_image(t, p, c, thresholds)
        assert flags[i].dtype == torch.uint8 and flags[i].shape == want.shape
        assert torch.equal(flags[i].cpu().float(), want), (name, i)
        assert torch.equal(first[i].cpu().long(), cases.closed_form(t, p, c, thresholds)[1]), (name, i)
    acc = DetectionMetrics(thresholds)
    acc.update(dev(targets), dev(predictions), dev(confidences))
    got = acc.compute()
    want = metrics.calculate_metrics(targets, predictions, confidences, thresholds)
    cases.assert_results_equal(got, want, thresholds)           # every field, 'raw' and ar_300 (the mean of recall_300) included
    # recall_300 per image: the host half's own unit list against _process_one
    rec = acc._fetch()
    for r, t, p, c in zip(rec, targets, predictions, confidences):
        _, want300, want_conf = _cpu_image(t, p, c, thresholds)
        assert torch.equal(r['conf'], want_conf)
        tp = r['tp'].float()
        _, recall = metrics.precision_and_recall(tp.t(), (1 - tp).t(), len(t))
        for k in range(len(thresholds)):
            got300 = recall[:300][-1][k] if len(recall) else 0
            assert torch.equal(torch.as_tensor(got300), torch.as_tensor(want300[k])), (name, k)
    return got


# ---- 1. known answers and golden data ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('thresholds', cases.THRESHOLD_SETS, ids=('t50', 'coco', 't70_95'))
def test_known_answers_and_golden_data(cuda, golden_dir, thresholds):
    for name, targets, predictions, confidences in cases.known_answer_cases(golden_dir) + cases.golden_cases(golden_dir):
        _check_against_cpu(cuda, targets, predictions, confidences, thresholds, name)
    # two updates accumulate to what one call over all images gives
    from cvpce_amd import metrics
    from cvpce_amd.device_metrics import DetectionMetrics
    acc = DetectionMetrics(thresholds)
    for i in range(3):
        acc.update([cases.TARGETS[i].to(cuda)], [cases.PREDICTIONS[i].to(cuda)], [cases.CONFIDENCES[i].to(cuda)])
    cases.assert_results_equal(acc.compute(), metrics.calculate_metrics(cases.TARGETS, cases.PREDICTIONS, cases.CONFIDENCES, thresholds), thresholds)
    # inputs on the host are accepted as well
    acc = DetectionMetrics(thresholds)
    acc.update(cases.TARGETS, cases.PREDICTIONS, cases.CONFIDENCES)
    cases.assert_results_equal(acc.compute(), metrics.calculate_metrics(cases.TARGETS, cases.PREDICTIONS, cases.CONFIDENCES, thresholds), thresholds)
    # nothing accumulated: what the host routine does with no image at all (it cannot merge an empty list)
    with pytest.raises(ValueError):
        metrics.calculate_metrics([], [], [], thresholds)
    with pytest.raises(ValueError):
        DetectionMetrics(thresholds).compute()


# ---- 2. boundaries -------------------------------------------------------------------------------------------------------------
def test_boundaries(cuda):
    from cvpce_amd import metrics, synthetic
    from cvpce_amd.device_metrics import match_detections
    f = lambda *rows: torch.tensor(rows, dtype=torch.float32).reshape(-1, 4)
    one = torch.tensor([0.9])
    # IoU exactly 0.5 at threshold 0.5: a match
    t, p = f([0, 0, 1, 1]), f([0, 0, 2, 1])
    assert float(metrics.box_iou(p, t)) == 0.5
    flags, first = match_detections([t.to(cuda)], [p.to(cuda)], [one.to(cuda)], (0.5,))
    assert flags[0].tolist() == [[1]] and first[0].tolist() == [[0]]
    _check_against_cpu(cuda, [t], [p], [one], (0.5,), 'iou==0.5')
    # fp32 IoU == float32(0.7), which is below 0.7 as a double: torch compares in float32, so it is a match at the Python threshold 0.7
    t, p = f([0, 0, 10, 10]), f([0, 0, 10, 7])
    iou = metrics.box_iou(p, t).reshape(1)
    assert iou.view(torch.int32).item() == torch.tensor([0.7], dtype=torch.float32).view(torch.int32).item() == 0x3F333333
    assert float(iou) < 0.7 and bool(iou >= 0.7)
    flags, _ = match_detections([t.to(cuda)], [p.to(cuda)], [one.to(cuda)], (0.7,))
    assert flags[0].tolist() == [[1]]
    _check_against_cpu(cuda, [t], [p], [one], (0.7,), 'iou==f32(0.7)')
    _check_against_cpu(cuda, [t], [p], [one], (0.7, 0.95), 'iou==f32(0.7)')
    # one ulp above float32(0.7) as the threshold: no match
    above = torch.tensor([0.7], dtype=torch.float32).view(torch.int32).add(1).view(torch.float32).item()
    flags, _ = match_detections([t.to(cuda)], [p.to(cuda)], [one.to(cuda)], (above,))
    assert flags[0].tolist() == [[0]]
    # zero-area boxes: 0/0 = NaN never matches (identical point boxes; a point prediction inside a target has IoU 0)
    t, p = f([3, 3, 3, 3], [0, 0, 4, 4]), f([3, 3, 3, 3], [1, 1, 1, 1])
    assert torch.isnan(metrics.box_iou(p, t)[0, 0])
    for thr in ((0.5,), (0.0, 0.5)):
        _check_against_cpu(cuda, [t], [p], [torch.tensor([0.9, 0.8])], thr, 'zero area')
    flags, first = match_detections([t.to(cuda)], [p.to(cuda)], [torch.tensor([0.9, 0.8]).to(cuda)], (0.5,))
    assert flags[0].tolist() == [[0, 0]] and first[0].tolist() == [[-1, -1]]
    # no predictions, no targets, neither -- alone and between ordinary images of one batch
    e4, e1 = torch.zeros(0, 4), torch.zeros(0)
    T, P, C = cases.TARGETS, cases.PREDICTIONS, cases.CONFIDENCES
    for thr in ((0.5,), COCO):
        _check_against_cpu(cuda, [T[0]], [e4], [e1], thr, 'no predictions')
        _check_against_cpu(cuda, [e4], [P[0]], [C[0]], thr, 'no targets')
        _check_against_cpu(cuda, [e4], [e4], [e1], thr, 'neither')
        _check_against_cpu(cuda, [T[0], e4, T[1], e4, T[2], T[0]], [P[0], P[1], e4, e4, P[2], e4], [C[0], C[1], e1, e1, C[2], e1], thr, 'mixed')
    # 700 targets in one image (11 tiles of 64), next to a small one; P = 1; P = 20 480 (the detector's cap)
    t700, p700, c700 = synthetic.dense_detection_scene(7, n_pred=1000, n_tgt=700)
    t700 = torch.cat([t700, t700[:700 - len(t700)] + 3.0]) if len(t700) < 700 else t700[:700]
    assert len(t700) == 700 and len(c700.unique()) == len(c700)
    _check_against_cpu(cuda, [T[0], t700, T[1]], [P[0], p700, P[1]], [C[0], c700, C[1]], COCO, '700 targets')
    _check_against_cpu(cuda, [t700], [t700[123:124] + 0.5], [one], (0.5, 0.75, 0.9), 'P=1')
    tb, pb, cb = synthetic.dense_detection_scene(11, n_pred=20480, n_tgt=150)
    cb = torch.randperm(20480, generator=torch.Generator().manual_seed(1)).float() / 20480         # pairwise distinct by construction
    _check_against_cpu(cuda, [tb, T[0]], [pb, P[0]], [cb, C[0]], (0.5, 0.75), 'P=20480')
    # every instantiation of the kernel (1, 2, 4, 8, 16 running minima per lane)
    ts, ps, cs = synthetic.dense_detection_scene(DENSE_SEEDS[0])
    for k in (3, 4, 5, 8, 9, 16):
        _check_against_cpu(cuda, [ts], [ps], [cs], tuple(torch.linspace(.3, .9, k).tolist()), f'K={k}')
    with pytest.raises(ValueError):
        match_detections([ts.to(cuda)], [ps.to(cuda)], [cs.to(cuda)], tuple(torch.linspace(.3, .9, 17).tolist()))


# ---- 3. dense random scenes ----------------------------------------------------------------------------------------------------
def test_dense_random_scenes(cuda):
    from cvpce_amd import metrics, synthetic
    from cvpce_amd.device_metrics import DetectionMetrics, match_detections
    scenes = [synthetic.dense_detection_scene(s) for s in DENSE_SEEDS]
    assert len(scenes) == 32
    targets, predictions, confidences = (list(x) for x in zip(*scenes))
    for p, c in zip(predictions, confidences):
        assert len(p) == 1000 and len(c.unique()) == 1000          # pairwise distinct: the CPU order is then well defined
    assert 120 <= sum(len(t) for t in targets) / 32 <= 180
    dev = lambda lst: [t.to(cuda) for t in lst]
    flags, _ = match_detections(dev(targets), dev(predictions), dev(confidences), COCO)
    covered_twice = 0
    for i, (t, p, c) in enumerate(zip(targets, predictions, confidences)):
        conf, order = torch.sort(c, descending=True)
        ious, idx = metrics.iou_matrices(t, p[order])
        covered_twice += int(((metrics.box_iou(p, t) >= 0.5).sum(0) > 1).sum())
        for k, thr in enumerate(COCO):
            tp, _ = metrics.check_matches(ious, idx, thr)
            assert torch.equal(flags[i][k].cpu().float(), tp), (i, float(thr))
    assert covered_twice > 32 * 50                                  # the scenes are dense: many predictions cover the same target
    acc = DetectionMetrics(COCO)
    for b in range(0, 32, 8):                                       # four batches of eight images
        acc.update(dev(targets[b:b + 8]), dev(predictions[b:b + 8]), dev(confidences[b:b + 8]))
    cases.assert_results_equal(acc.compute(), metrics.calculate_metrics(targets, predictions, confidences, COCO), COCO)


# ---- 4. tied confidences -------------------------------------------------------------------------------------------------------
def test_tied_confidences_follow_the_stable_order(cuda):
    """The device rule: equal confidences keep input order (stable descending sort).  The CPU routines are fed predictions
    pre-ordered that way (metrics._process_one would re-sort them with an unstable sort, so iou_matrices / check_matches /
    precision_and_recall / _do_calculate are called on the pre-ordered input directly)."""
    from cvpce_amd import metrics, synthetic
    from cvpce_amd.device_metrics import DetectionMetrics
    thresholds = (0.5, 0.75)
    scenes = [synthetic.dense_detection_scene(s, n_pred=400, n_tgt=60) for s in (1, 2, 3)]
    targets, predictions, confidences = (list(x) for x in zip(*scenes))
    confidences = [(c * 20).floor() / 20 for c in confidences]      # 20 levels for 400 predictions: about 20 predictions per level
    confidences[2] = torch.full_like(confidences[2], 0.5)           # and one image whose confidences are all equal
    per_thr = {t: {'true_positives': [], 'false_positives': [], 'recall_300': []} for t in thresholds}
    confs = []
    for t, p, c in zip(targets, predictions, confidences):
        assert len(c.unique()) <= 21
        conf, order = torch.sort(c, stable=True, descending=True)
        ious, idx = metrics.iou_matrices(t, p[order])
        for thr in thresholds:
            tp, fp = metrics.check_matches(ious, idx, thr)
            _, rec = metrics.precision_and_recall(tp, fp, len(t))
            per_thr[thr]['true_positives'].append(tp); per_thr[thr]['false_positives'].append(fp)
            per_thr[thr]['recall_300'].append(rec[:300][-1])
        confs.append(conf)
    want = metrics._do_calculate(thresholds, per_thr, confs, sum(len(t) for t in targets))
    acc = DetectionMetrics(thresholds)
    acc.update([t.to(cuda) for t in targets], [p.to(cuda) for p in predictions], [c.to(cuda) for c in confidences])
    cases.assert_results_equal(acc.compute(), want, thresholds)
    for r, thr_tp in zip(acc._fetch(), zip(*[per_thr[t]['true_positives'] for t in thresholds])):
        assert torch.equal(r['tp'].float(), torch.stack(thr_tp))


# ---- 5. class-aware ------------------------------------------------------------------------------------------------------------
def test_class_aware_matching_and_per_class_grouping(cuda):
    """compute_per_class against the grouping of detection_eval.evaluate_detections (its lines restated on host tensors and fed to
    metrics.calculate_metrics): (image, class) units for every class on either side, class -1 pooled only."""
    from cvpce_amd import metrics, synthetic
    from cvpce_amd.device_metrics import DetectionMetrics
    n_cls, thresholds = 6, (0.5, 0.75, 0.9)
    g = torch.Generator().manual_seed(17)
    acc = DetectionMetrics(thresholds)
    all_t, all_p, all_c = [], [], []
    per = {c: ([], [], []) for c in range(n_cls)}
    batch = []
    for i, seed in enumerate((41, 42, 43, 44, 45)):
        t, p, s = synthetic.dense_detection_scene(seed, n_pred=300, n_tgt=50)
        assert len(s.unique()) == len(s)
        tl = torch.randint(-1, n_cls, (len(t),), generator=g)
        # a prediction mostly carries the class of the target it overlaps best, otherwise a random one (-1 included)
        best = metrics.box_iou(p, t).argmax(dim=1)
        pl = torch.where(torch.rand(len(p), generator=g) < 0.6, tl[best], torch.randint(-1, n_cls, (len(p),), generator=g))
        if i == 0:
            pl[pl == 2] = 3                       # class 2 only among the targets of this image
            tl[tl == 4] = 5                       # class 4 only among its predictions
        if i == 3:
            t, tl = t[:0], tl[:0]                 # an image without targets
        if i == 4:
            p, s, pl = p[:0], s[:0], pl[:0]       # an image without predictions
        batch.append((t, p, s, tl, pl))
        for c in {int(x) for x in pl} | {int(x) for x in tl}:
            b, sc, tb = p[pl == c], s[pl == c], t[tl == c]
            all_p.append(b); all_c.append(sc); all_t.append(tb)
            if c != -1:
                per[c][1].append(b); per[c][2].append(sc); per[c][0].append(tb)
        if len(batch) == 2 or i == 4:
            acc.update(*[[x[j].to(cuda) for x in batch] for j in (0, 1, 2)], [x[3].to(cuda) for x in batch], [x[4] for x in batch])
            batch = []
    strip = lambda res: {thr: {k: v for k, v in itm.items() if k != 'raw'} for thr, itm in res.items()}
    want_per = {c: strip(metrics.calculate_metrics(*per[c], thresholds)) for c in range(n_cls) if per[c][0] or per[c][1]}
    want_all = strip(metrics.calculate_metrics(all_t, all_p, all_c, thresholds))
    got_per, got_all = acc.compute_per_class(n_cls)
    assert sorted(got_per) == sorted(want_per) == list(range(n_cls))
    for c in want_per:
        cases.assert_results_equal(got_per[c], want_per[c], thresholds)
    cases.assert_results_equal(got_all, want_all, thresholds)
    assert float(want_all[0.5]['ap']) > 0.05       # (not a degenerate comparison of zeros)


# ---- 6. harnesses --------------------------------------------------------------------------------------------------------------
def _all_distinct(score_lists):
    return all(len(s.unique()) == len(s) for s in score_lists)


def test_evaluate_gln_with_device_metrics_equals_the_default(cuda):
    from cvpce_amd import proposals_eval, synthetic
    model = synthetic.synthetic_gln(seed=0, detections_per_img=60).to(cuda)
    imgs = [synthetic.shelf_image(s, 512, 512) for s in (21, 22, 23)]
    dets = model([i.to(cuda) for i in imgs[:2]]) + model([imgs[2].to(cuda)])      # (batched as the harness will batch them)
    # the comparison is exact only where the CPU's (unstable) confidence order is well defined
    assert _all_distinct([d['scores'].cpu() for d in dets]), 'tied detector confidences: choose other image seeds'
    # ground truth: every other detection, moved by a few per cent of its size (IoU near 0.9: the thresholds below cut through them)
    shifted = lambda b: b + (b[:, 2:] - b[:, :2]).repeat(1, 2) * torch.tensor([0.05, -0.03, 0.04, 0.02])
    data = [(i, {'boxes': shifted(d['boxes'][::2].cpu())}) for i, d in zip(imgs, dets)]
    thresholds = [0.5, 0.75, 0.9]
    want = proposals_eval.evaluate_gln_sync(model, data, thresholds, batch_size=2)
    got = proposals_eval.evaluate_gln_sync(model, data, thresholds, batch_size=2, device_metrics=True)
    cases.assert_results_equal(got, want, thresholds)
    assert float(want[0.5]['ap']) > 0.05            # (not a comparison of zeros)
    got = proposals_eval.evaluate_gln_async(model, data, thresholds, batch_size=2, num_metric_processes=2, device_metrics=True)
    cases.assert_results_equal(got, want, thresholds)


def test_evaluate_detections_with_device_metrics_equals_the_default(cuda):
    from cvpce_amd import detection_eval, synthetic
    from test_gpu_harness import _GP180Like
    det = synthetic.synthetic_gln(seed=0, detections_per_img=60).to(cuda)
    enc = synthetic.synthetic_macvgg(seed=1).to(cuda)
    gal = synthetic.gallery_images(6, seed=9)
    gallery_anns = ['a', 'b', 'c', 'zz_unknown', 'a', 'b']              # 'zz_unknown' is not a test-set class: class -1
    # the host path's order at equal confidences is unspecified, so the comparison is exact only on images whose confidences are
    # pairwise distinct.  This random-weight detector saturates (many scores near 0.998 share a float32 value): seeds 31-33 and
    # others produce ties on the MI355X, so the first three tie-free images among the candidates are taken, and that is asserted.
    items, n = [], 12
    for seed in range(21, 61):
        img = synthetic.shelf_image(seed, 512, 512)
        pred = det([img.to(cuda)])[0]
        if len(pred['scores']) >= n and _all_distinct([pred['scores'].cpu()]):
            b = pred['boxes'][:n].cpu()
            items.append((img, {'boxes': b + (b[:, 2:] - b[:, :2]).repeat(1, 2) * torch.tensor([0.04, 0.02, -0.03, 0.05]), 'labels': torch.arange(n) % 3}))
        if len(items) == 3:
            break
    assert len(items) == 3, 'fewer than three candidate images with pairwise distinct confidences'
    tset = _GP180Like(items, ['a', 'b', 'c'])
    gallery = synthetic.TensorGallery(gal, gallery_anns)
    thresholds = (0.5, 0.75)
    # (one image per detector pass, as the confidences above were collected)
    want_per, want_all = detection_eval.evaluate_detections(det, enc, tset, gallery, thresholds, proposal_batch_size=1, classification_batch_size=8)
    got_per, got_all = detection_eval.evaluate_detections(det, enc, tset, gallery, thresholds, proposal_batch_size=1, classification_batch_size=8,
                                                          device_metrics=True)
    assert sorted(got_per) == sorted(want_per) and len(want_per) >= 1
    for c in want_per:
        cases.assert_results_equal(got_per[c], want_per[c], thresholds)
    cases.assert_results_equal(got_all, want_all, thresholds)


# ---- 7. command line -----------------------------------------------------------------------------------------------------------
CLI_HEAD = (2.0, -2.0)          # logit gain and bias of the classification head (synthetic.calibrate_head) for the CLI test's checkpoint
def test_cli_device_metrics_prints_the_same_figures(world, tmp_path):
    """`gln eval ... --device-metrics` against the same command without it, on an on-disk SKU-110K-like set read as the command
    reads it.  The comparison is exact only where every image's confidences are pairwise distinct (the host order at ties is
    unspecified).  The command keeps 200 detections per image, and the checkpoint of tests/test_gpu_cli.py has a saturated head
    (logit gain 8, bias 1: dozens of scores near 0.998 share a float32 value), so on the MI355X none of 40 candidate images was
    tie-free with it.  This test therefore writes a checkpoint of the same detector with an unsaturated head (CLI_HEAD) and takes
    the first two candidate images whose detections -- through the 8-bit reader the command uses -- are tie-free; that is
    asserted, not assumed."""
    from PIL import Image
    from cvpce_amd import datautils, proposals_eval, synthetic
    det = synthetic.calibrate_head(synthetic.synthetic_gln(seed=0, calibrate=False), *CLI_HEAD)
    gln_tar = tmp_path / 'gln.tar'
    torch.save({'model_state_dict': det.state_dict()}, gln_tar)
    model = proposals_eval.load_gln(str(gln_tar), False)                           # (as the command loads it)
    rows, kept = [], 0
    for seed in range(21, 61):
        pixels = (synthetic.shelf_image(seed, 512, 512).clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
        det = model([pixels.cuda()])[0]
        if len(det['scores']) < 8 or not _all_distinct([det['scores'].cpu()]):
            continue
        Image.fromarray(pixels.numpy()).save(tmp_path / f'test_{kept}.png')
        for x1, y1, x2, y2 in det['boxes'][::2].cpu().round().int().tolist():      # ground truth: every other detection, on the pixel grid
            if x2 > x1 and y2 > y1:
                rows.append(f'test_{kept}.png,{x1},{y1},{x2},{y2},object,512,512')
        kept += 1
        if kept == 2:
            break
    assert kept == 2, 'fewer than two candidate images with pairwise distinct confidences'
    (tmp_path / 'annotations.csv').write_text('\n'.join(rows) + '\n')
    data = datautils.SKU110KDataset(str(tmp_path), str(tmp_path / 'annotations.csv'), image_format='uint8')
    assert _all_distinct([model([img.cuda()])[0]['scores'].cpu() for img, _ in data])          # (what the command will see)
    args = ['gln', 'eval', '--dataset', 'sku110k', '--imgs', tmp_path, '--annotations', tmp_path / 'annotations.csv',
            '-t', '0.5', '-t', '0.75', '--no-plots', '--metric-workers', '0']
    plain = _run(args + [gln_tar])
    device = _run(args + ['--device-metrics', gln_tar])
    figures = lambda out: [l for l in out.splitlines() if re.match(r'^(0\.5|0\.75):\t|^--> (AP|AR300) ', l)]
    assert len(figures(plain)) == 4 and figures(device) == figures(plain)
    assert float(re.search(r'--> AP ([0-9.e-]+)', plain).group(1)) > 0.05           # (not a comparison of zeros)
    coco = _run(args + ['--coco', '--device-metrics', '--metric-workers', '3', gln_tar])      # workers are ignored
    summary = lambda out: [l for l in out.splitlines() if l.startswith('--> ')]
    assert len(summary(coco)) == 2 and summary(coco) == summary(_run(args + ['--coco', gln_tar]))
    from click.testing import CliRunner
    from cvpce_amd.cli import cli
    for cmd in (['gln', 'eval', '--help'], ['eval-product-detection', '--help']):
        text = ''.join(CliRunner().invoke(cli, cmd).output.split())               # (click wraps the help text: compare without white space)
        assert '--device-metrics/--no-device-metrics' in text and '--metric-workersisignored' in text
    # the class-aware command runs with the switch and prints its summary (its exact agreement with the host path is checked on
    # tie-free detections in test_evaluate_detections_with_device_metrics_equals_the_default: this set's 200 detections per image tie)
    if not (world / 'out' / 'classifier_index.pkl').exists():
        _run(['dihe', 'prebuild-index', '--img-dir', world / 'Training', '--out-dir', world / 'out', world / 'dihe.tar'])
    out = _run(['eval-product-detection', '--img-dir', world / 'Training', '--test-imgs', world / 'Testing', '--annotations', world / 'ann',
                '--load-classifier-index', world / 'out' / 'classifier_index.pkl', '--device-metrics', world / 'gln.tar', world / 'dihe.tar'])
    assert re.search(r'--> mAP [0-9.e-]+', out) and re.search(r'--> mAR300 [0-9.e-]+', out)


# ---- 8. no host synchronisation in update() ------------------------------------------------------------------------------------
def test_update_does_not_synchronise_the_host(cuda):
    """torch.cuda.set_sync_debug_mode('error') makes every synchronising torch call raise (blocking copies, .item(), nonzero,
    boolean-mask indexing ...): `update` on device-resident inputs must run through under it.  The mode is shown to be armed on
    this stack by a deliberate `.item()` first."""
    from cvpce_amd import synthetic
    from cvpce_amd.device_metrics import DetectionMetrics
    scenes = [synthetic.dense_detection_scene(s, n_pred=300, n_tgt=70) for s in (5, 6)]
    targets, predictions, confidences = ([x.to(cuda) for x in col] for col in zip(*scenes))
    labels_t = [torch.zeros(len(t), dtype=torch.int32, device=cuda) for t in targets]
    labels_p = [torch.zeros(len(p), dtype=torch.int32, device=cuda) for p in predictions]
    warm = DetectionMetrics(COCO)
    warm.update(targets, predictions, confidences)                 # (first use: library loading, allocator growth)
    warm.compute()
    acc, acc_cls = DetectionMetrics(COCO), DetectionMetrics((0.5,))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=cuda).sum().item()                # the mode is armed
        for _ in range(3):
            acc.update(targets, predictions, confidences)
            acc_cls.update(targets, predictions, confidences, labels_t, labels_p)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    from cvpce_amd import metrics
    host = lambda col: [x.cpu() for x in col] * 3
    cases.assert_results_equal(acc.compute(), metrics.calculate_metrics(host(targets), host(predictions), host(confidences), COCO), COCO)
