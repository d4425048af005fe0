"""Time the planogram comparator per image: the host path stage by stage, the two device launches, the host tail, and the drop-in
evaluation loop with the comparator's `device_graphs` switch off and on.

Scenes: gridded planograms of 24 (4 x 6) and 200 (8 x 25) boxes (synthetic.planogram_grid) against detections made from them
(synthetic.perturbed_detections: scaled 1.7x, shifted, jittered by 3 px, 5 % dropped, 5 % mislabelled), in batches of 8.
  host_*          planograms.build_graph (expected + actual), large_common_subgraph, finalize_via_ransac: wall clock per image
  device_graphs   the one launch that builds the 16 graphs of a batch, HIP events, median of --launches
  device_match    the one launch that matches the 8 pairs, HIP events
  device_e2e      PlanogramComparator(device_graphs=True).compare_batch without its host tail: uploads, both launches, the copy back
  host_tail       finalize_via_ransac on the device matching (what stays on the host without `device_tail`)
  device_tail_launches   the two launches of planograms_device.finalize_batch (RANSAC scoring, then winner / refit / projection / claim)
                  on the 8 matchings as they lie on the device, HIP events
  device_e2e_tail PlanogramComparator(device_graphs=True, device_tail=True).compare_batch: uploads, the four launches, the one copy
                  back and the verdict, wall clock.  Its yardstick in the same run is host_tail + device_e2e
  evaluate_iter   images/s of PlanogramEvaluator.evaluate_iter with the real comparator, switch off and on, in this one call: the
                  detector / embedder / matcher run on synthetic shelf images as in bench.py and the comparator is handed the scene's
                  detections (the synthetic detector's own boxes are noise); `tail`: both switches on
  reclass leg     (--reclass-markdown) the re-classification stage with a stated miss rate: every 9th planted detection is withheld from
                  the comparator and every 11th expected label is replaced by one no gallery item has, the gallery carries the planograms'
                  own labels and the shelf images are large enough to hold the projected positions.  compare_batch ms per image and
                  evaluate_iter images/s with `device_tail` alone and with `device_reclass` as well, in this one process, and what a
                  window costs in launches and waits on either path

  detections leg  (--detections-markdown) `PlanogramEvaluator.evaluate_iter` with `device_detections` off and on over the comparator with
                  all three switches on: the detector's confident boxes are replaced by the scene's detections inside the pipeline
                  (`run(proposals=...)`), the planograms are the pipeline's own detections shrunk; images/s and what a window costs in
                  launches and waits on either path

    python tools/bench_planogram_compare.py [--batch 8] [--launches 30] [--markdown profiles/r23_planogram_tail.md]
                                            [--reclass-markdown profiles/r25_reclass.md]
                                            [--detections-only] [--detections-markdown profiles/r27_device_detections.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
from torch.utils._python_dispatch import TorchDispatchMode

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvpce_amd import planograms, planograms_device as pd, production, staging, synthetic     # noqa: E402


def scenes(rows, cols, batch):
    out = []
    for k in range(batch):
        eb, el = synthetic.planogram_grid(rows, cols, 100 + k)
        ab, al = synthetic.perturbed_detections(eb, el, 200 + k)
        out.append(({'boxes': eb, 'labels': el}, {'boxes': ab, 'labels': al}))
    return out


def time_host(pairs):
    t = {'host_build_graph_x2': 0.0, 'host_common_subgraph': 0.0, 'host_ransac_tail': 0.0}
    verdict_inputs = []
    for e, a in pairs:
        t0 = time.perf_counter()
        ge = planograms.build_graph(e['boxes'], e['labels'], 0.5)
        ga = planograms.build_graph(a['boxes'], a['labels'], 0.5)
        t1 = time.perf_counter()
        m = planograms.large_common_subgraph(ge, ga)
        t2 = time.perf_counter()
        if m:
            planograms.finalize_via_ransac(m, e['boxes'], a['boxes'], e['labels'], a['labels'], reproj_threshold=10)
        t3 = time.perf_counter()
        t['host_build_graph_x2'] += t1 - t0
        t['host_common_subgraph'] += t2 - t1
        t['host_ransac_tail'] += t3 - t2
        verdict_inputs.append(m)
    return {k: 1e3 * v / len(pairs) for k, v in t.items()}, verdict_inputs


def events(launch, launches):
    for _ in range(3):
        launch()
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def time_device(pairs, launches):
    items = [(e['boxes'], e['labels']) for e, _ in pairs] + [(a['boxes'], a['labels']) for _, a in pairs]
    n = len(pairs)
    graphs = pd.build_graphs(items, 0.5)
    nbr, weight, stamp, _ = graphs[0]._parent
    sizes = [len(l) for _, l in items]
    dev = nbr.device
    boxes = torch.cat([b for b, _ in items]).to(dev)
    offsets = torch.tensor(staging.offsets(sizes), dtype=torch.int32, device=dev)
    thresh = torch.stack([pd.graph_threshold(b, 0.5) for b, _ in items]).float().to(dev)
    out = [torch.empty_like(t) for t in (nbr, weight, stamp)]
    g_ms = events(lambda: torch.ops.cvpce_amd.planogram_graphs(boxes, offsets, thresh, min(sizes), max(sizes), *out), launches)
    assert all(torch.equal(a, b) for a, b in zip(out, (nbr, weight, stamp)))
    match, _, _ = pd._prepare_match(graphs[:n], graphs[n:], -0.2, 0.5)
    m_ms = events(match.launch, launches)
    e2e = []
    for r in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        built = pd.build_graphs(items, 0.5)
        matchings = pd.common_subgraphs(built[:n], built[n:])
        if r:
            e2e.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    for (e, a), m in zip(pairs, matchings):
        if m:
            planograms.finalize_via_ransac(m, e['boxes'], a['boxes'], e['labels'], a['labels'], reproj_threshold=10)
    tail = time.perf_counter() - t0
    on_device = pd.match_on_device(graphs[:n], graphs[n:])
    ransac, finish, *_ = pd._prepare_tail(on_device, [e['boxes'] for e, _ in pairs], [a['boxes'] for _, a in pairs], [10] * n, 0.5, 0,
                                          pd.RANSAC_HYPOTHESES)
    t_ms = events(lambda: (ransac.launch(), finish.launch()), launches)
    cmp = production.PlanogramComparator(device_graphs=True, device_tail=True)
    e2e_tail, verdicts = [], None
    for r in range(6):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        verdicts = cmp.compare_batch([e for e, _ in pairs], [a for _, a in pairs])
        if r:
            e2e_tail.append(time.perf_counter() - t0)
    host_verdicts = production.PlanogramComparator(device_graphs=True).compare_batch([e for e, _ in pairs], [a for _, a in pairs])
    return {'device_graphs_launch': g_ms / n, 'device_match_launch': m_ms / n, 'device_e2e': 1e3 * statistics.median(e2e) / n,
            'host_tail': 1e3 * tail / n, 'device_tail_launches': t_ms / n, 'device_e2e_tail': 1e3 * statistics.median(e2e_tail) / n,
            'same_verdict_tail': sum(float(a) == float(b) for a, b in zip(verdicts, host_verdicts))}, matchings


class PlantedEvaluator(production.PlanogramEvaluator):
    """The GPU half runs as always; the comparator gets the scene's detections instead of the synthetic detector's."""
    planted = ()

    def detect_and_classify_batch(self, images):
        super().detect_and_classify_batch(images)
        at = self.__dict__.setdefault('_at', 0)
        self._at = at + len(images)
        return [self.planted[(at + i) % len(self.planted)] for i in range(len(images))]


def time_evaluate_iter(pairs, images, evaluators):
    res = {}
    for name, ev in evaluators.items():
        ev.planted = [(a['boxes'], a['labels']) for _, a in pairs]
        vals = None
        for r in range(2):                                  # (round 0 is the warm-up)
            ev._at = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vals = [float(v) for v in ev.evaluate_iter(((img, e) for img, (e, _) in zip(images, pairs)), lookahead=len(pairs))]
            dt = time.perf_counter() - t0
        res[name] = (len(pairs) / dt, vals)
    return res


def miss_scenes(rows, cols, batch):
    """`scenes` with a stated miss rate: every 9th planted detection is withheld from the comparator, every 11th expected label is
    replaced by a label no gallery item has -> pairs, and (h, w) of a shelf image that holds every detection."""
    out, far = [], torch.zeros(2)
    for e, a in scenes(rows, cols, batch):
        keep = [i for i in range(len(a['labels'])) if i % 9 != 4]
        labels = [('not_in_the_gallery' if i % 11 == 5 else l) for i, l in enumerate(e['labels'])]
        far = torch.maximum(far, a['boxes'][:, 2:].amax(dim=0))
        out.append(({'boxes': e['boxes'], 'labels': labels}, {'boxes': a['boxes'][keep].contiguous(), 'labels': [a['labels'][i] for i in keep]}))
    w, h = (max(1024, -(-int(v + 8) // 64) * 64) for v in far.tolist())
    return out, (h, w)


class WindowCounter(TorchDispatchMode):
    """What one window costs: `kernels` = calls of the project's own ops (one launch each), `torch_device_ops` = every other operator
    that touches a device tensor (copies, gathers, fills: at most a launch each), `waits` = the points at which the host waits for the
    device (stream / event synchronize, a blocking device-to-host copy, a scalar read off a device tensor)."""

    def __init__(self):
        super().__init__()
        self.kernels = self.torch_device_ops = self.waits = 0

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        kwargs = kwargs or {}
        tensors = [t for t in list(args) + list(kwargs.values()) if torch.is_tensor(t)]
        for a in args:
            if isinstance(a, (list, tuple)):
                tensors += [t for t in a if torch.is_tensor(t)]
        on_device = any(t.is_cuda for t in tensors)
        name = func.name() if hasattr(func, 'name') else str(func)
        if name.startswith('cvpce_amd::'):
            self.kernels += 1
        elif on_device:
            self.torch_device_ops += 1
        out = func(*args, **kwargs)
        if on_device and name.startswith('aten::_local_scalar_dense'):
            self.waits += 1
        elif on_device and torch.is_tensor(out) and not out.is_cuda and not kwargs.get('non_blocking', False) \
                and name.startswith(('aten::_to_copy', 'aten::copy_')) and not (name.startswith('aten::copy_') and len(args) > 2 and args[2]):
            self.waits += 1
        return out

    def __enter__(self):
        self._saved = (torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize, torch.cuda.synchronize)
        counter = self

        def wrap(fn):
            def counted(*a, **kw):
                counter.waits += 1
                return fn(*a, **kw)
            return counted
        torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize, torch.cuda.synchronize = (wrap(f) for f in self._saved)
        return super().__enter__()

    def __exit__(self, *exc):
        torch.cuda.Stream.synchronize, torch.cuda.Event.synchronize, torch.cuda.synchronize = self._saved
        return super().__exit__(*exc)


def time_reclass(name, rows, cols, batch, det, enc, dev):
    """The leg with a stated miss rate -> one row: `device_tail` alone against `device_reclass` as well, same process, same inputs."""
    pairs, (h, w) = miss_scenes(rows, cols, batch)
    gallery = synthetic.TensorGallery(synthetic.gallery_images(64, seed=100), [synthetic.PLANOGRAM_LABELS[i % len(synthetic.PLANOGRAM_LABELS)] for i in range(64)])
    clf = production.Classifier(enc, gallery, device=dev, emb_device=dev, batch_size=32, match_dtype=torch.bfloat16)
    pg = production.ProposalGenerator(det, device=dev, confidence_threshold=0.5)
    images = [synthetic.shelf_image(400 + k, h, w).to(dev) for k in range(batch)]
    es, acts = [e for e, _ in pairs], [a for _, a in pairs]
    cmps = {'tail': production.PlanogramComparator(device_graphs=True, device_tail=True),
            'reclass': production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True)}
    row = {'scene': name, 'batch': batch, 'image': f'{h} x {w}', 'expected_boxes': sum(len(e['labels']) for e in es) / batch}
    # what the stage has to do on this input: positions classified, recovered, not recovered (from the `device_tail` path itself)
    crops = []
    inner = clf.classify
    clf.classify = lambda imgs, *a, **kw: (crops.append(len(imgs)), inner(imgs, *a, **kw))[1]
    with_clf = cmps['tail'].compare_batch(es, acts, images, clf)
    del clf.classify
    without = cmps['tail'].compare_batch(es, acts, images, None)
    recovered = sum(round((float(a) - float(b)) * len(e['labels'])) for a, b, e in zip(with_clf, without, es))
    row.update(images_with_positions=len(crops), positions=sum(crops) / batch, recovered=recovered / batch, not_recovered=(sum(crops) - recovered) / batch,
               unmatched=sum(round((1 - float(b)) * len(e['labels'])) for b, e in zip(without, es)) / batch)
    verdicts, times = {}, {key: [] for key in cmps}
    for r in range(REPEATS + 2):                            # (the two paths alternate window by window; the first two rounds warm up)
        for key, cmp in cmps.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            verdicts[key] = cmp.compare_batch(es, acts, images, clf)
            torch.cuda.synchronize()
            if r > 1:
                times[key].append(time.perf_counter() - t0)
    for key, cmp in cmps.items():
        row[f'compare_batch_{key}'] = 1e3 * statistics.median(times[key]) / batch
        row[f'compare_batch_{key}_min_max'] = [1e3 * min(times[key]) / batch, 1e3 * max(times[key]) / batch]
        with WindowCounter() as c:
            cmp.compare_batch(es, acts, images, clf)
        row.update({f'kernels_{key}': c.kernels, f'torch_ops_{key}': c.torch_device_ops, f'waits_{key}': c.waits})
    row['same_verdict'] = sum(float(a) == float(b) and type(a) is type(b) for a, b in zip(verdicts['tail'], verdicts['reclass']))
    evaluators = {key: PlantedEvaluator(pg, clf, cmp) for key, cmp in cmps.items()}
    rates, vals = {key: [] for key in cmps}, {}
    for r in range(REPEATS + 1):                            # (alternating again; round 0 warms up)
        for key, ev in evaluators.items():
            ev.planted, ev._at = [(a['boxes'], a['labels']) for a in acts], 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vals[key] = [float(v) for v in ev.evaluate_iter(zip(images, es), lookahead=batch)]
            dt = time.perf_counter() - t0
            if r:
                rates[key].append(batch / dt)
    for key in cmps:
        row[f'evaluate_iter_{key}'] = statistics.median(rates[key])
        row[f'evaluate_iter_{key}_min_max'] = [min(rates[key]), max(rates[key])]
    row['same_verdict_iter'] = sum(a == b for a, b in zip(vals['tail'], vals['reclass']))
    return row


REPEATS = 15                # timed windows per path and figure of the re-classification leg
RECLASS_COLS = ('image', 'expected_boxes', 'unmatched', 'positions', 'recovered', 'not_recovered', 'compare_batch_tail', 'compare_batch_reclass',
                'evaluate_iter_tail', 'evaluate_iter_reclass', 'kernels_tail', 'kernels_reclass', 'torch_ops_tail', 'torch_ops_reclass',
                'waits_tail', 'waits_reclass')


def write_reclass(path, rows, args):
    def fmt(row, c):
        v = row[c]
        if isinstance(v, str):
            return v
        lo_hi = row.get(c + '_min_max')
        return f'{v:.4g}' + (f' ({lo_hi[0]:.4g} - {lo_hi[1]:.4g})' if lo_hi else '')
    with open(path, 'w') as f:
        f.write('# Planogram comparator: the re-classification in one device pass against the per-image pass\n\n'
                f'`python tools/bench_planogram_compare.py --batch {args.batch} --launches {args.launches} --reclass-markdown ...`, one process, MI355X.  '
                'Every 9th planted detection is withheld from the comparator and every 11th expected label is replaced by a label no gallery item '
                'has; the gallery of 64 carries the planograms\' 12 labels; the shelf images hold every projected position.  `unmatched`: expected '
                'boxes per image the per-label claim leaves; `positions`: how many of them are valid and classified again; `recovered` / '
                '`not_recovered`: what the re-classification makes of them (synthetic noise images: a position is recovered when the nearest '
                'gallery item happens to carry its label).  `compare_batch_*`: ms per image, wall clock around a window that ends in a synchronise; '
                '`evaluate_iter_*`: images/s of `PlanogramEvaluator.evaluate_iter` with the window as lookahead (detector, crops, embedder and '
                f'matcher included); both as median (min - max) of {REPEATS} windows per path, the two paths alternating window by window.  `tail`: `device_graphs` + `device_tail` (the '
                'yardstick: the re-classification per image through the host); `reclass`: `device_reclass` as well.  Per window of '
                f'{args.batch} images: `kernels` = launches of the project\'s own kernels, `torch_ops` = other torch operators on device tensors '
                '(copies, gathers), `waits` = points at which the host waits for the device.\n\n')
        f.write('| scene | ' + ' | '.join(RECLASS_COLS) + ' | same verdict (compare_batch / evaluate_iter) |\n|---|' + '---|' * (len(RECLASS_COLS) + 1) + '\n')
        for row in rows:
            f.write(f"| {row['scene']} | " + ' | '.join(fmt(row, c) for c in RECLASS_COLS) +
                    f" | {row['same_verdict']}/{row['batch']} / {row['same_verdict_iter']}/{row['batch']} |\n")


class PlantedPipeline(production.BatchedPipeline):
    """The detector runs as always; its confident boxes are replaced by the scene's detections (`run(proposals=...)`), so that both
    paths of the detections leg -- which take their detections from the pipeline, not from the host -- see the scene."""
    planted = None

    def run(self, images, **kw):
        assert len(images) == self.planted[0].shape[0]
        return super().run(images, proposals=self.planted, **kw)


class PlantedDetectionsEvaluator(production.PlanogramEvaluator):
    def _pipeline(self):
        pipe = self.__dict__.get('_planted_pipe')
        if pipe is None:
            pipe = self._planted_pipe = PlantedPipeline(self.proposal_generator.detector, self.classifier, self.proposal_generator.condfidence_threshold)
        return pipe


def time_detections(name, rows, cols, batch, det, enc, dev):
    """The detections leg -> one row: `PlanogramEvaluator(device_detections=False)` against `True` over one comparator setting (all
    three comparator switches on), same process, same inputs, the two paths alternating window by window."""
    pairs, (h, w) = miss_scenes(rows, cols, batch)
    gallery = synthetic.TensorGallery(synthetic.gallery_images(64, seed=100), [synthetic.PLANOGRAM_LABELS[i % len(synthetic.PLANOGRAM_LABELS)] for i in range(64)])
    clf = production.Classifier(enc, gallery, device=dev, emb_device=dev, batch_size=32, match_dtype=torch.bfloat16)
    pg = production.ProposalGenerator(det, device=dev, confidence_threshold=0.5)
    images = [synthetic.shelf_image(400 + k, h, w).to(dev) for k in range(batch)]
    dpi = det.detections_per_img
    boxes, counts = torch.zeros((batch, dpi, 4)), []
    for k, (_, a) in enumerate(pairs):
        n = min(len(a['labels']), dpi)
        boxes[k, :n] = a['boxes'][:n]
        counts.append(n)
    planted = (boxes.to(dev), torch.tensor(counts, dtype=torch.int32, device=dev))
    switches = dict(device_graphs=True, device_tail=True, device_reclass=True)
    evaluators = {'off': PlantedDetectionsEvaluator(pg, clf, production.PlanogramComparator(**switches)),
                  'on': PlantedDetectionsEvaluator(pg, clf, production.PlanogramComparator(**switches), device_detections=True)}
    for ev in evaluators.values():
        ev._pipeline().planted = planted
    # the planograms: what the pipeline itself makes of the planted boxes (the labels of noise crops are whatever is nearest), shrunk,
    # every 11th label replaced by one no gallery item has -- so the comparator has matchings, homographies and positions to classify
    dets = evaluators['off'].detect_and_classify_batch(images)
    planos = [{'boxes': (b / 1.7).contiguous(), 'labels': [('not_in_the_gallery' if i % 11 == 5 else l) for i, l in enumerate(labels)]} for b, labels in dets]
    row = {'scene': name, 'batch': batch, 'image': f'{h} x {w}', 'boxes': sum(counts) / batch}
    rates, vals = {key: [] for key in evaluators}, {}
    for r in range(REPEATS + 1):                            # (alternating; round 0 warms up)
        for key, ev in evaluators.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            vals[key] = list(ev.evaluate_iter(zip(images, planos), lookahead=batch))
            dt = time.perf_counter() - t0
            if r:
                rates[key].append(batch / dt)
    for key, ev in evaluators.items():
        row[f'evaluate_iter_{key}'] = statistics.median(rates[key])
        row[f'evaluate_iter_{key}_min_max'] = [min(rates[key]), max(rates[key])]
        with WindowCounter() as c:
            list(ev.evaluate_iter(zip(images, planos), lookahead=batch))
        row.update({f'kernels_{key}': c.kernels, f'torch_ops_{key}': c.torch_device_ops, f'waits_{key}': c.waits})
    row['same_verdict'] = sum(float(a) == float(b) and type(a) is type(b) for a, b in zip(vals['off'], vals['on']))
    row['mean_verdict'] = sum(float(v) for v in vals['off']) / batch
    row['host_routed'] = evaluators['on'].planogram_comparator.host_routed + evaluators['on'].detections_host_routed
    return row


DETECTIONS_COLS = ('image', 'boxes', 'mean_verdict', 'evaluate_iter_off', 'evaluate_iter_on', 'kernels_off', 'kernels_on', 'torch_ops_off', 'torch_ops_on',
                   'waits_off', 'waits_on', 'host_routed')


def write_detections(path, rows, args):
    def fmt(row, c):
        v = row[c]
        if isinstance(v, str):
            return v
        lo_hi = row.get(c + '_min_max')
        return f'{v:.4g}' + (f' ({lo_hi[0]:.4g} - {lo_hi[1]:.4g})' if lo_hi else '')
    with open(path, 'w') as f:
        f.write('# Planogram evaluator: detections kept on the device from the matcher to the comparator\n\n'
                f'`python tools/bench_planogram_compare.py --batch {args.batch} --detections-only --detections-markdown ...`, one process, MI355X.  '
                'The detector, the crops, the embedder and the matcher run on synthetic shelf images; the detector\'s confident boxes are replaced '
                'by the scene\'s detections (`run(proposals=...)`), and the planograms are the pipeline\'s own detections shrunk by 1.7, every '
                '11th label replaced by one no gallery item has.  `off` / `on`: `PlanogramEvaluator(device_detections=...)` over '
                '`PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True)`.  `evaluate_iter_*`: images/s of '
                f'`evaluate_iter` with the window of {args.batch} images as lookahead, median (min - max) of {REPEATS} windows per path, the two '
                'paths alternating window by window.  Per window: `kernels` = launches of the project\'s own kernels, `torch_ops` = other torch '
                'operators on device tensors (copies, gathers), `waits` = points at which the host waits for the device.\n\n')
        f.write('| scene | ' + ' | '.join(DETECTIONS_COLS) + ' | same verdict |\n|---|' + '---|' * (len(DETECTIONS_COLS) + 1) + '\n')
        for row in rows:
            f.write(f"| {row['scene']} | " + ' | '.join(fmt(row, c) for c in DETECTIONS_COLS) + f" | {row['same_verdict']}/{row['batch']} |\n")


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--markdown', help='also write the table to this file')
    ap.add_argument('--reclass-markdown', help='run the re-classification leg and write its table to this file')
    ap.add_argument('--reclass-only', action='store_true', help='skip everything but the re-classification leg')
    ap.add_argument('--detections-markdown', help='run the detections leg and write its table to this file')
    ap.add_argument('--detections-only', action='store_true', help='skip everything but the detections leg')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    det = synthetic.synthetic_gln(seed=0, detections_per_img=200).to(dev)
    enc = synthetic.synthetic_macvgg(seed=1).to(dev)
    clf = production.Classifier(enc, synthetic.TensorGallery(synthetic.gallery_images(64, seed=100)), device=dev, emb_device=dev, batch_size=32,
                                match_dtype=torch.bfloat16)
    pg = production.ProposalGenerator(det, device=dev, confidence_threshold=0.5)
    evaluators = {'off': PlantedEvaluator(pg, clf, production.PlanogramComparator()),
                  'on': PlantedEvaluator(pg, clf, production.PlanogramComparator(device_graphs=True)),
                  'tail': PlantedEvaluator(pg, clf, production.PlanogramComparator(device_graphs=True, device_tail=True))}
    images = [synthetic.shelf_image(300 + k, 1024, 1024).to(dev) for k in range(args.batch)]
    rows = []
    grids = (('24 boxes (4 x 6)', (4, 6)), ('200 boxes (8 x 25)', (8, 25)))
    if args.detections_markdown or args.detections_only:
        detections_rows = []
        for name, (r, c) in grids:
            detections_rows.append(time_detections(name, r, c, args.batch, det, enc, dev))
            print(json.dumps(detections_rows[-1]), flush=True)
        if args.detections_markdown:
            write_detections(args.detections_markdown, detections_rows, args)
        if args.detections_only:
            return 0
    if args.reclass_markdown:
        reclass_rows = []
        for name, (r, c) in grids:
            reclass_rows.append(time_reclass(name, r, c, args.batch, det, enc, dev))
            print(json.dumps(reclass_rows[-1]), flush=True)
        write_reclass(args.reclass_markdown, reclass_rows, args)
    for name, (r, c) in (() if args.reclass_only else grids):
        pairs = scenes(r, c, args.batch)
        host, host_m = time_host(pairs)
        device, dev_m = time_device(pairs, args.launches)
        it = time_evaluate_iter(pairs, images, evaluators)
        row = {'scene': name, 'batch': args.batch, **host, **device,
               'host_graph_stages': host['host_build_graph_x2'] + host['host_common_subgraph'],
               'evaluate_iter_off_img_s': it['off'][0], 'evaluate_iter_on_img_s': it['on'][0], 'evaluate_iter_tail_img_s': it['tail'][0],
               'same_verdict_iter_tail': sum(a == b for a, b in zip(it['on'][1], it['tail'][1])),
               'same_matching_size': sum(len(a) == len(b) for a, b in zip(host_m, dev_m)),
               'same_verdict': sum(a == b for a, b in zip(it['off'][1], it['on'][1]))}
        row['speedup_graph_stages'] = row['host_graph_stages'] / row['device_e2e']
        row['tail_yardstick'] = row['host_tail'] + row['device_e2e']
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.markdown:
        cols = ['host_build_graph_x2', 'host_common_subgraph', 'host_ransac_tail', 'device_graphs_launch', 'device_match_launch', 'device_e2e',
                'host_tail', 'device_tail_launches', 'device_e2e_tail', 'evaluate_iter_off_img_s', 'evaluate_iter_on_img_s', 'evaluate_iter_tail_img_s']
        with open(args.markdown, 'w') as f:
            f.write('# Planogram comparator: graph stages and tail on the device against the host path\n\n'
                    f'`python tools/bench_planogram_compare.py --batch {args.batch} --launches {args.launches}`, one process, MI355X; ms per image '
                    'unless the column says images/s.  Host columns: the path with every switch off.  Grids are full of exact ties, '
                    'so the device graphs follow the device rule (DESIGN.md 4b) there: `same verdict` counts the images of the batch whose '
                    'verdict is the host\'s all the same.  `device_e2e_tail` (graphs, matching and tail on the device, one copy back) is to be '
                    'read against `host_tail + device_e2e` of the same run; `tail verdicts` counts the images whose verdict with the device '
                    'tail equals the verdict with the device graphs and the host tail (compare_batch / evaluate_iter).\n\n')
            f.write('| scene | ' + ' | '.join(cols) + ' | graph stages host / device | same verdict | host_tail + device_e2e | tail verdicts |\n|---|'
                    + '---|' * (len(cols) + 4) + '\n')
            for row in rows:
                f.write(f"| {row['scene']} | " + ' | '.join(f'{row[c]:.4g}' for c in cols) +
                        f" | {row['speedup_graph_stages']:.1f}x | {row['same_verdict']}/{row['batch']} | {row['tail_yardstick']:.4g} | "
                        f"{row['same_verdict_tail']}/{row['batch']} / {row['same_verdict_iter_tail']}/{row['batch']} |\n")
    return 0


if __name__ == '__main__':
    sys.exit(main())
