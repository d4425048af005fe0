"""Time the comparator's two graph matchers per pair: Tonioni's search on the host and on the device, and the first-found common
subgraph on the device, on shelves with ever fewer labels.

Scenes: gridded planograms of 24 (4 x 6) and 200 (10 x 20) boxes whose labels are assigned in row blocks -- every position its own
label, 6 labels, 3 labels -- against detections made from them (synthetic.perturbed_detections: scaled 1.7x, shifted, jittered by
3 px, 10 % dropped, 10 % given the next label), in windows of --batch pairs.  All figures of a row come from this one process.
  hypotheses        equal-label node pairs per pair (mean and largest of the window)
  host_tonioni      planograms.tonioni_mcs on the graphs read back from the device, wall clock per pair, over the first --host-pairs
                    pairs of the window (the 200-box shelves with few labels take tens of seconds a pair)
  device_tonioni    the three launches of the Tonioni matcher for the whole window (hypotheses, runs, choice), HIP events, median of
                    --launches, divided by the pairs of the window
  device_large      the one launch of `planogram_match` for the same window, the same way
  sizes             the mean matching size of either matcher over the window, and the pairs whose host Tonioni matching equals the
                    device's as a set (of the pairs the host was run on)
  verdicts          compare_batch without a classifier (the matched fraction after the tail) with all device switches on: the mean
                    verdict of either matcher
  evaluate_iter     images/s of PlanogramEvaluator.evaluate_iter with device_graphs, device_tail and device_reclass on, per matcher:
                    the detector / embedder / matcher run on synthetic shelf images and the comparator is handed the scene's
                    detections (bench_planogram_compare.PlantedEvaluator)

    python tools/bench_tonioni.py [--batch 8] [--launches 30] [--host-pairs 2] [--markdown profiles/r32_tonioni_matcher.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from cvpce_amd import planograms, planograms_device as pd, production, synthetic     # noqa: E402
from bench_planogram_compare import PlantedEvaluator, events, time_evaluate_iter      # noqa: E402


def scenes(rows, cols, labels, batch):
    """`batch` (planogram, detections) pairs: labels names in row blocks (0: every position its own)"""
    n = rows * cols
    names = [f'product_{i:03d}' for i in range(labels or n)]
    out = []
    for k in range(batch):
        eb, _ = synthetic.planogram_grid(rows, cols, 100 + k)
        el = [names[i * len(names) // n] for i in range(n)]
        ab, al = synthetic.perturbed_detections(eb, el, 200 + k, drop=0.10, mislabel=0.10, names=names)
        out.append(({'boxes': eb, 'labels': el}, {'boxes': ab, 'labels': al}))
    return out


def measure(name, pairs, launches, host_pairs, images, evaluators):
    n = len(pairs)
    graphs = pd.build_graphs([(e['boxes'], e['labels']) for e, _ in pairs] + [(a['boxes'], a['labels']) for _, a in pairs], 0.5)
    ge, ga = graphs[:n], graphs[n:]
    hyps = [pd.hypothesis_count(e['labels'], a['labels']) for e, a in pairs]
    row = {'scene': name, 'batch': n, 'hypotheses_mean': statistics.mean(hyps), 'hypotheses_max': max(hyps)}
    tonioni, _, _ = pd._prepare_match(ge, ga, -0.2, 0.5, matcher='tonioni')
    large, _, _ = pd._prepare_match(ge, ga, -0.2, 0.5)
    row['device_tonioni'] = events(tonioni.launch, launches) / n
    row['device_large'] = events(large.launch, launches) / n
    dev_t, dev_l = pd.common_subgraphs(ge, ga, matcher='tonioni'), pd.common_subgraphs(ge, ga)
    row['size_tonioni'], row['size_large'] = statistics.mean(len(m) for m in dev_t), statistics.mean(len(m) for m in dev_l)
    host_ms, same = [], 0
    for p in range(min(host_pairs, n)):
        h1, h2 = pd.to_networkx(ge[p]), pd.to_networkx(ga[p])
        t0 = time.perf_counter()
        found = planograms.tonioni_mcs(h1, h2)
        host_ms.append(1e3 * (time.perf_counter() - t0))
        same += found == dev_t[p]
    row['host_tonioni'], row['host_pairs'], row['same_as_host'] = statistics.mean(host_ms), len(host_ms), same
    for matcher in ('tonioni', 'large'):
        cmp = production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True, matcher=matcher)
        verdicts = cmp.compare_batch([e for e, _ in pairs], [a for _, a in pairs])
        row[f'verdict_{matcher}'] = statistics.mean(float(v) for v in verdicts)
        assert cmp.host_routed == 0
    it = time_evaluate_iter(pairs, images, evaluators)
    row['evaluate_iter_tonioni_img_s'], row['evaluate_iter_large_img_s'] = it['tonioni'][0], it['large'][0]
    row['speedup_host_over_device'] = row['host_tonioni'] / row['device_tonioni']
    return row


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--host-pairs', type=int, default=2, help='pairs of a 200-box window the host matcher is timed on (24 boxes: all)')
    ap.add_argument('--markdown', help='also write the table to this file')
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    det = synthetic.synthetic_gln(seed=0, detections_per_img=200).to(dev)
    enc = synthetic.synthetic_macvgg(seed=1).to(dev)
    clf = production.Classifier(enc, synthetic.TensorGallery(synthetic.gallery_images(64, seed=100)), device=dev, emb_device=dev, batch_size=32,
                                match_dtype=torch.bfloat16)
    pg = production.ProposalGenerator(det, device=dev, confidence_threshold=0.5)
    evaluators = {m: PlantedEvaluator(pg, clf, production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True, matcher=m))
                  for m in ('large', 'tonioni')}
    images = [synthetic.shelf_image(300 + k, 1024, 1024).to(dev) for k in range(args.batch)]
    rows = []
    for boxes, (r, c) in (('24 boxes (4 x 6)', (4, 6)), ('200 boxes (10 x 20)', (10, 20))):
        for labels in (0, 6, 3):
            name = f"{boxes}, {'every position its own label' if not labels else f'{labels} labels'}"
            rows.append(measure(name, scenes(r, c, labels, args.batch), args.launches, args.batch if r * c < 100 else args.host_pairs,
                                images, evaluators))
            print(json.dumps(rows[-1]), flush=True)
    if args.markdown:
        with open(args.markdown, 'w') as f:
            f.write('# Tonioni matcher: the host search against the device kernels, beside the first-found matcher\n\n'
                    f'`python tools/bench_tonioni.py --batch {args.batch} --launches {args.launches} --host-pairs {args.host_pairs}`, one process, '
                    'MI355X.  ms per pair unless the column says otherwise; `host tonioni_mcs` is this repository\'s host matcher on the graphs '
                    'read back from the device, timed on the first pairs of the window (their number in brackets); the device columns are HIP '
                    'events around the window\'s launches (Tonioni: hypotheses, runs, choice; large: `planogram_match`), median of '
                    f'{args.launches}, divided by the {args.batch} pairs.  `sizes` and `verdicts` are means over the window, Tonioni / large; the '
                    'verdicts are compare_batch without a classifier with device_graphs, device_tail and device_reclass on.  `same` counts the '
                    'pairs whose host Tonioni matching is the device\'s.  evaluate_iter: images/s with the three switches on, Tonioni / large.\n\n')
            f.write('| scene | hypotheses mean / max | host tonioni_mcs | device tonioni | host / device | device large | sizes | same | verdicts | '
                    'evaluate_iter img/s |\n|---|---|---|---|---|---|---|---|---|---|\n')
            for row in rows:
                f.write(f"| {row['scene']} | {row['hypotheses_mean']:.0f} / {row['hypotheses_max']} | {row['host_tonioni']:.4g} ({row['host_pairs']}) | "
                        f"{row['device_tonioni']:.4g} | {row['speedup_host_over_device']:.1f}x | {row['device_large']:.4g} | "
                        f"{row['size_tonioni']:.1f} / {row['size_large']:.1f} | {row['same_as_host']}/{row['host_pairs']} | "
                        f"{row['verdict_tonioni']:.3f} / {row['verdict_large']:.3f} | "
                        f"{row['evaluate_iter_tonioni_img_s']:.3g} / {row['evaluate_iter_large_img_s']:.3g} |\n")
    return 0


if __name__ == '__main__':
    sys.exit(main())
