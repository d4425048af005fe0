"""What the compliance report costs: `PlanogramEvaluator.report_iter` against `evaluate_iter`, the two report kernels alone, and the
launches and waits of a window.

Scenes: those of the re-classification leg of tools/bench_planogram_compare.py (`miss_scenes`: gridded planograms of 24 and 200 boxes,
every 9th planted detection withheld, every 11th expected label one no gallery item has), windows of 8.
  evaluate_iter / report_iter   images/s with the window as lookahead (detector, crops, embedder and matcher included; the comparator is
                                handed the scene's detections), wall clock around a window that ends in a synchronise: three timed
                                windows per path after a warm-up window, the paths alternating window by window
  kernels                       `report_positions` and `report_reclass` alone at n1 = n2 = 200 and 1024, 8 images: HIP events around
                                --launches back-to-back launches, per launch, three timed groups after a warm-up group
  launches / waits              per window, counted by `WindowCounter` of tools/bench_planogram_compare.py

The yardstick is `evaluate_iter` of the commit BEFORE the report: run the tool there with `--root <that checkout> --json parent.json`
(a tree without `report_iter` measures `evaluate_iter` alone), then here with `--baseline parent.json --markdown ...`.

    python tools/bench_compliance_report.py [--root DIR] [--batch 8] [--launches 200] [--json out.json] [--baseline parent.json]
                                            [--markdown profiles/r28_compliance_report.md]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import time

import torch

WINDOWS = 3                 # timed windows (and timed groups of launches) per figure
SWITCHES = {'tail': dict(device_graphs=True, device_tail=True), 'reclass': dict(device_graphs=True, device_tail=True, device_reclass=True)}
GRIDS = (('grid_4x6', 4, 6), ('grid_8x25', 8, 25))


def load(root):
    """cvpce_amd and the comparator bench's helpers of the checkout at `root`"""
    sys.path.insert(0, root)
    spec = importlib.util.spec_from_file_location('bench_planogram_compare', os.path.join(root, 'tools', 'bench_planogram_compare.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from cvpce_amd import production, synthetic
    return bench, production, synthetic


def spread(values):
    return {'median': statistics.median(values), 'min': min(values), 'max': max(values)}


def time_iter(name, rows, cols, batch, bench, production, synthetic, det, enc, dev):
    """One scene -> {switches: {path: images/s}, and per path the launches and waits of a window}"""
    pairs, (h, w) = bench.miss_scenes(rows, cols, batch)
    names = synthetic.PLANOGRAM_LABELS
    gallery = synthetic.TensorGallery(synthetic.gallery_images(64, seed=100), [names[i % len(names)] for i in range(64)])
    clf = production.Classifier(enc, gallery, device=dev, emb_device=dev, batch_size=32, match_dtype=torch.bfloat16)
    pg = production.ProposalGenerator(det, device=dev, confidence_threshold=0.5)
    images = [synthetic.shelf_image(400 + k, h, w).to(dev) for k in range(batch)]
    es, acts = [e for e, _ in pairs], [a for _, a in pairs]
    row = {'scene': name, 'batch': batch, 'image': f'{h} x {w}', 'expected_boxes': sum(len(e['labels']) for e in es) / batch}
    for key, switches in SWITCHES.items():
        ev = bench.PlantedEvaluator(pg, clf, production.PlanogramComparator(**switches))
        ev.planted = [(a['boxes'], a['labels']) for a in acts]
        paths = {'evaluate_iter': ev.evaluate_iter}
        if hasattr(ev, 'report_iter'):
            paths['report_iter'] = ev.report_iter
        rates, last = {p: [] for p in paths}, {}
        for r in range(WINDOWS + 1):                        # (alternating; window 0 warms up)
            for p, run in paths.items():
                ev._at = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                last[p] = list(run(zip(images, es), lookahead=batch))
                torch.cuda.synchronize()
                if r:
                    rates[p].append(batch / (time.perf_counter() - t0))
        for p in paths:
            row[f'{p}_{key}'] = spread(rates[p])
        if 'report_iter' in paths:
            reports = last['report_iter']
            row[f'same_verdict_{key}'] = sum(float(a) == float(b.compliance) for a, b in zip(last['evaluate_iter'], reports))
            ok = [r for r in reports if r.status == 'ok']
            row[f'outcomes_{key}'] = [sum(int((r.outcomes == c).sum()) for r in ok) / batch for c in range(5)]
            row[f'occupants_{key}'] = sum(int((r.occupant >= 0).sum()) for r in ok) / batch
            row[f'strays_{key}'] = sum(len(r.stray) for r in ok) / batch
        cmp = ev.planogram_comparator
        calls = {'compare_batch': cmp.compare_batch}
        if hasattr(cmp, 'report_batch'):
            calls['report_batch'] = cmp.report_batch
        for p, call in calls.items():
            call(es, acts, images, clf)
            with bench.WindowCounter() as c:
                call(es, acts, images, clf)
            row[f'{p}_{key}'] = {'kernels': c.kernels, 'torch_ops': c.torch_device_ops, 'waits': c.waits}
    return row


def events(launch, launches):
    """ms per launch: HIP events around `launches` back-to-back launches, WINDOWS timed groups after a warm-up group"""
    times = []
    for r in range(WINDOWS + 1):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            launch()
        b.record()
        b.synchronize()
        if r:
            times.append(a.elapsed_time(b) / launches)
    return spread(times)


def time_kernels(n, batch, launches, dev):
    """The two kernels alone on `batch` images of n positions and n detections: a grid of positions, the detections their jittered
    copies, half of either side claimed, every position that is not detected classifiable and in the plan."""
    from cvpce_amd import torch_ops_report as ops_report            # noqa: F401  (registers torch.ops.cvpce_amd.report_*)
    g = torch.Generator().manual_seed(n)
    cols = 32
    one = torch.tensor([[20 + (i % cols) * 72, 30 + (i // cols) * 120, 84 + (i % cols) * 72, 126 + (i // cols) * 120] for i in range(n)], dtype=torch.float32)
    h, w = int(one[:, 3].max()) + 40, int(one[:, 2].max()) + 40
    pos = one.repeat(batch, 1)
    boxes = pos + (torch.rand(batch * n, 4, generator=g) - 0.5) * 10
    me = (torch.rand(batch * n, generator=g) < 0.5).to(torch.int32)
    ma = (torch.rand(batch * n, generator=g) < 0.5).to(torch.int32)
    off = torch.arange(batch + 1, dtype=torch.int32) * n
    i32 = lambda *shape: torch.empty(shape, dtype=torch.int32, device=dev)
    d = lambda t: t.to(dev)
    status, image = torch.zeros(batch, dtype=torch.int32), torch.tensor([[h, w, 1]] * batch, dtype=torch.int32)
    rows = torch.randint(0, 64, (batch * n,), generator=g).to(torch.int32)
    ins = [d(t) for t in (status, me, ma, pos, boxes, off, off, image, rows)]
    outcome, occupant, occupant_row, stray, occupant_iou = i32(batch * n), i32(batch * n), i32(batch * n), i32(batch * n), torch.empty(batch * n, device=dev)
    positions = lambda: torch.ops.cvpce_amd.report_positions(*ins, 0.5, outcome, occupant, occupant_iou, occupant_row, stray)
    res = {'n': n, 'batch': batch, 'report_positions_ms': events(positions, launches)}
    torch.cuda.synchronize()
    first = outcome.clone()
    pending = (first.view(batch, n) == ops_report.PENDING).cpu()
    counts = pending.sum(dim=1).to(torch.int32)
    index, slot_row, at = torch.zeros((batch, n), dtype=torch.int32), torch.full((batch, n), -1, dtype=torch.int32), 0
    for p in range(batch):
        c = int(counts[p])
        index[p, :c] = torch.where(pending[p])[0].to(torch.int32)
        slot_row[p, :c] = torch.arange(at, at + c, dtype=torch.int32)
        at += c
    indices = torch.randint(0, 64, (max(at, 1), 1), generator=g)
    distances = torch.rand(max(at, 1), 1, generator=g)
    gallery_id = (torch.arange(64) % 12).to(torch.int32)
    expected_id = torch.randint(0, 12, (batch * n,), generator=g).to(torch.int32)
    rin = [d(t) for t in (index, counts, slot_row, indices, distances, gallery_id, expected_id, off, status)]
    seen_row, seen_distance = i32(batch * n), torch.empty(batch * n, device=dev)
    work = first.clone()

    def reclass():
        work.copy_(first)                                   # (the kernel decides the pending rows in place: every launch starts from them)
        torch.ops.cvpce_amd.report_reclass(*rin, work, seen_row, seen_distance)
    copy_alone = events(lambda: work.copy_(first), launches)
    both = events(reclass, launches)
    res.update(pending_per_image=at / batch, occupants_per_image=int((occupant >= 0).sum()) / batch,
               report_reclass_with_copy_ms=both, copy_alone_ms=copy_alone)
    return res


def fmt(s, digits=4):
    return f"{s['median']:.{digits}g} ({s['min']:.{digits}g} - {s['max']:.{digits}g})"


def write_markdown(path, result, baseline, args):
    with open(path, 'w') as f:
        f.write('# Compliance report: what it costs beside the verdict\n\n'
                f'`python tools/bench_compliance_report.py --batch {args.batch} --launches {args.launches} --baseline ... --markdown ...`, one process per '
                'checkout, MI355X.  Scenes of the re-classification leg (every 9th planted detection withheld, every 11th expected label one no gallery '
                f'item has), windows of {args.batch}.  Rates are images/s of `PlanogramEvaluator.evaluate_iter` / `report_iter` with the window as '
                f'lookahead, wall clock around a window that ends in a synchronise, median (min - max) of {WINDOWS} timed windows after a warm-up window, '
                'the two paths alternating window by window.  `parent`: `evaluate_iter` of the commit before the report, same tool, same scenes and '
                'switches, a process of its own on the same machine.  `tail`: `device_graphs` + `device_tail`; `reclass`: `device_reclass` as well.\n\n')
        f.write('| scene | switches | evaluate_iter, parent | evaluate_iter | report_iter | report_iter / parent | same verdict |\n|---|---|---|---|---|---|---|\n')
        for row in result['scenes']:
            base = next((b for b in (baseline or {}).get('scenes', []) if b['scene'] == row['scene']), None)
            for key in SWITCHES:
                parent = base[f'evaluate_iter_{key}'] if base else None
                ratio = f"{row[f'report_iter_{key}']['median'] / parent['median']:.3f}" if parent else 'not measured'
                f.write(f"| {row['scene']} ({row['expected_boxes']:.0f} boxes, {row['image']}) | {key} | {fmt(parent) if parent else 'not measured'} | "
                        f"{fmt(row[f'evaluate_iter_{key}'])} | {fmt(row[f'report_iter_{key}'])} | {ratio} | {row[f'same_verdict_{key}']}/{row['batch']} |\n")
        f.write('\nPer window, counted by `WindowCounter`: `kernels` = launches of the project\'s own kernels, `torch_ops` = other torch operators on '
                'device tensors (copies, gathers, fills), `waits` = points at which the host waits for the device.  What was expected: two launches '
                'and no wait more with `device_reclass`.\n\n')
        f.write('| scene | switches | compare_batch kernels / torch_ops / waits | report_batch kernels / torch_ops / waits |\n|---|---|---|---|\n')
        for row in result['scenes']:
            for key in SWITCHES:
                a, b = row[f'compare_batch_{key}'], row[f'report_batch_{key}']
                f.write(f"| {row['scene']} | {key} | {a['kernels']} / {a['torch_ops']} / {a['waits']} | {b['kernels']} / {b['torch_ops']} / {b['waits']} |\n")
        f.write('\nWhat the reports say, per image (`reclass`): outcomes detected / recovered / missing / out of view / unchecked, positions with an '
                'occupant, stray detections.\n\n| scene | outcomes | occupants | strays |\n|---|---|---|---|\n')
        for row in result['scenes']:
            f.write(f"| {row['scene']} | {' / '.join(f'{v:.3g}' for v in row['outcomes_reclass'])} | {row['occupants_reclass']:.3g} | {row['strays_reclass']:.3g} |\n")
        f.write(f'\nThe kernels alone, {args.batch} images a launch, ms per launch: HIP events around {args.launches} back-to-back launches, median (min - max) of '
                f'{WINDOWS} timed groups after a warm-up group.  `report_reclass` decides the pending rows in place, so every timed launch is preceded by '
                'the device copy that restores them; the copy alone is timed beside it.\n\n')
        f.write('| n1 = n2 | pending / image | occupants / image | report_positions | report_reclass + copy | copy alone |\n|---|---|---|---|---|---|\n')
        for k in result['kernels']:
            f.write(f"| {k['n']} | {k['pending_per_image']:.4g} | {k['occupants_per_image']:.4g} | {fmt(k['report_positions_ms'])} | "
                    f"{fmt(k['report_reclass_with_copy_ms'])} | {fmt(k['copy_alone_ms'])} |\n")
        if result.get('notes'):
            f.write('\n' + '\n'.join(result['notes']) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='the checkout to measure')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--launches', type=int, default=200)
    ap.add_argument('--json', help='write the result here')
    ap.add_argument('--baseline', help='the --json of a run on the commit before the report')
    ap.add_argument('--markdown', help='write the tables here')
    ap.add_argument('--note', action='append', default=[], help='a line for the end of the markdown')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_compliance_report: no GPU -- nothing here is measured without one')
    bench, production, synthetic = load(os.path.abspath(args.root))
    dev = torch.device('cuda:0')
    det = synthetic.synthetic_gln(seed=0, detections_per_img=200).to(dev)
    enc = synthetic.synthetic_macvgg(seed=1).to(dev)
    result = {'root': os.path.abspath(args.root), 'scenes': [], 'kernels': [], 'notes': args.note}
    for name, r, c in GRIDS:
        result['scenes'].append(time_iter(name, r, c, args.batch, bench, production, synthetic, det, enc, dev))
        print(json.dumps(result['scenes'][-1]), flush=True)
    if hasattr(production.PlanogramComparator, 'report_batch'):
        for n in (200, 1024):
            result['kernels'].append(time_kernels(n, args.batch, args.launches, dev))
            print(json.dumps(result['kernels'][-1]), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(result, f)
    if args.markdown:
        baseline = json.load(open(args.baseline)) if args.baseline else None
        write_markdown(args.markdown, result, baseline, args)


if __name__ == '__main__':
    main()
