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

    python tools/bench_planogram_compare.py [--batch 8] [--launches 30] [--markdown profiles/r23_planogram_tail.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvpce_amd import planograms, planograms_device as pd, production, synthetic     # noqa: E402


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
    offsets = torch.tensor(pd._offsets(sizes), dtype=torch.int32, device=dev)
    thresh = torch.stack([pd.graph_threshold(b, 0.5) for b, _ in items]).float().to(dev)
    out = [torch.empty_like(t) for t in (nbr, weight, stamp)]
    g_ms = events(lambda: torch.ops.cvpce_amd.planogram_graphs(boxes, offsets, thresh, min(sizes), max(sizes), *out), launches)
    assert all(torch.equal(a, b) for a, b in zip(out, (nbr, weight, stamp)))
    args, _, _ = pd._prepare_match(graphs[:n], graphs[n:], -0.2, 0.5)
    m_ms = events(lambda: torch.ops.cvpce_amd.planogram_match(*args), launches)
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
    ransac, finish, _, _ = pd._prepare_tail(on_device, [e['boxes'] for e, _ in pairs], [a['boxes'] for _, a in pairs], [10] * n, 0.5, 0,
                                            pd.RANSAC_HYPOTHESES)
    t_ms = events(lambda: (torch.ops.cvpce_amd.homography_ransac(*ransac), torch.ops.cvpce_amd.homography_finish(*finish)), launches)
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--markdown', help='also write the table to this file')
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
    for name, (r, c) in (('24 boxes (4 x 6)', (4, 6)), ('200 boxes (8 x 25)', (8, 25))):
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
