"""What the compliance pictures cost: the compositor alone against a device copy of the same bytes, `PlanogramEvaluator.pictures_iter`
against `report_iter`, and the thumbnail atlas.

  kernel    8 canvases of 2048^2, each with a base image of its size and 200 (then 1 024) product items over it: `render_canvases` alone,
            HIP events around --launches back-to-back launches, three timed groups after a warm-up group -- and `out.copy_(base)` of
            the same bytes in the same process, the floor no compositor can beat
  window    `pictures_iter` against `report_iter` on the scenes of tools/bench_compliance_report.py (gridded planograms of 24 and 200
            boxes, every 9th planted detection withheld, every 11th expected label one no gallery item has), windows of 8, images/s,
            wall clock around a window that ends in a synchronise: three timed windows per path after a warm-up window, the paths
            alternating.  `pictures_iter` twice: the pictures left on the device, and every picture saved as PNG on --save-threads host
            threads (what writing files costs: a host copy and a host encode per picture, not the kernel's cost)
  atlas     build time and resident bytes of a `ThumbnailAtlas` over 3 200 synthetic 256 x 256 gallery byte images, max_side 128 and None

The yardstick of the window is `report_iter` of the commit BEFORE the pictures: run the tool there with `--root <that checkout> --json
parent.json` (a tree without `pictures_iter` measures `report_iter` alone), then here with `--baseline parent.json --markdown ...`.

    python tools/bench_scene_render.py [--root DIR] [--batch 8] [--launches 20] [--json out.json] [--baseline parent.json]
                                       [--markdown profiles/r29_scene_render.md]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import torch

WINDOWS = 3
SWITCHES = dict(device_graphs=True, device_tail=True, device_reclass=True)
GRIDS = (('grid_4x6', 4, 6), ('grid_8x25', 8, 25))
SIDE = 2048
GALLERY = 3200


def load(root):
    sys.path.insert(0, root)
    spec = importlib.util.spec_from_file_location('bench_planogram_compare', os.path.join(root, 'tools', 'bench_planogram_compare.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    from cvpce_amd import production, synthetic
    return bench, production, synthetic


def spread(values):
    return {'median': statistics.median(values), 'min': min(values), 'max': max(values)}


def events(launch, launches):
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


class ByteGallery:
    """`n` gallery byte images of side x side, a seeded pool of 64 cycled: nothing but the pool is held on the host"""

    def __init__(self, n, side=256, seed=7):
        g = torch.Generator().manual_seed(seed)
        self.pool = [torch.randint(0, 256, (side, side, 3), dtype=torch.uint8, generator=g) for _ in range(64)]
        self.n = n

    def __len__(self):
        return self.n

    def __getitem__(self, i):
        return self.pool[i % len(self.pool)], f'sku_{i:05d}'


def time_kernel(items, batch, launches, atlas, dev, with_base=True):
    """`batch` canvases of SIDE^2: the base over the whole canvas (with_base), then `items` products of 60 .. 260 pixels a side at random
    places.  items = 0 without a base is the background alone: what the tiles, the table search and the stores cost."""
    from cvpce_amd import rendering
    g = torch.Generator().manual_seed(items)
    base = torch.randint(0, 256, (batch, SIDE, SIDE, 3), dtype=torch.uint8, generator=g).to(dev)
    lists = []
    for _ in range(batch):
        xy = torch.rand(items, 2, generator=g) * (SIDE - 100)
        wh = 60 + torch.rand(items, 2, generator=g) * 200
        boxes = torch.cat([torch.tensor([[0.0, 0.0, SIDE, SIDE]] if with_base else []).reshape(-1, 4), torch.cat([xy, xy + wh], dim=1)])
        rows = torch.cat([torch.tensor([rendering.R.SRC_BASE] if with_base else [], dtype=torch.int64),
                          torch.randint(0, len(atlas), (items,), generator=g)]).to(torch.int32)
        lists.append(rendering.Items(boxes.to(dev), rows.to(dev), torch.zeros(len(rows), dtype=torch.int32, device=dev),
                                     torch.zeros(len(rows), dtype=torch.int32, device=dev)))
    renderer = rendering.SceneRenderer(atlas)
    sizes, bases = [(SIDE, SIDE)] * batch, list(base) if with_base else None
    out = torch.empty_like(base)
    res = {'items': items, 'base': with_base, 'batch': batch, 'bytes': base.numel(), 'render_ms': events(lambda: renderer.render(lists, sizes, bases), launches)}
    launch, flat = renderer.last_launch, out.view(-1)        # the op's inputs of the last call: the launch alone, into a buffer of ours
    res['kernel_ms'] = events(lambda: torch.ops.cvpce_amd.render_canvases(*launch, flat), launches)
    res['copy_ms'] = events(lambda: out.copy_(base), launches)
    res['ratio'] = res['kernel_ms']['median'] / res['copy_ms']['median']
    return res


def time_window(name, rows, cols, batch, bench, production, synthetic, det, enc, dev, save_threads):
    pairs, (h, w) = bench.miss_scenes(rows, cols, batch)
    names = synthetic.PLANOGRAM_LABELS
    gallery = synthetic.TensorGallery(synthetic.gallery_images(64, seed=100), [names[i % len(names)] for i in range(64)])
    clf = production.Classifier(enc, gallery, device=dev, emb_device=dev, batch_size=32, match_dtype=torch.bfloat16)
    pg = production.ProposalGenerator(det, device=dev, confidence_threshold=0.5)
    images = [synthetic.shelf_image(400 + k, h, w).to(dev) for k in range(batch)]
    es, acts = [e for e, _ in pairs], [a for _, a in pairs]
    ev = bench.PlantedEvaluator(pg, clf, production.PlanogramComparator(**SWITCHES))
    ev.planted = [(a['boxes'], a['labels']) for a in acts]
    row = {'scene': name, 'batch': batch, 'image': f'{h} x {w}', 'expected_boxes': sum(len(e['labels']) for e in es) / batch}
    paths = {'report_iter': lambda: list(ev.report_iter(zip(images, es), lookahead=batch))}
    if hasattr(ev, 'pictures_iter'):
        from cvpce_amd import rendering
        renderer = rendering.SceneRenderer(rendering.ThumbnailAtlas(gallery, clf.annotations, dev))
        tmp = tempfile.mkdtemp(prefix='scene_render_')

        def saved():
            with ThreadPoolExecutor(save_threads) as pool:
                jobs = [pool.submit(pic.save, os.path.join(tmp, str(i))) for i, (_, pic) in enumerate(ev.pictures_iter(zip(images, es), renderer, lookahead=batch))]
                return [j.result() for j in jobs]
        paths['pictures_iter'] = lambda: list(ev.pictures_iter(zip(images, es), renderer, lookahead=batch))
        paths['pictures_iter_saved'] = saved
    rates = {p: [] for p in paths}
    for r in range(WINDOWS + 1):
        for p, run in paths.items():
            ev._at = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if r:
                rates[p].append(batch / (time.perf_counter() - t0))
    for p in paths:
        row[p] = spread(rates[p])
    return row


def time_atlas(max_side, dev, workers):
    from cvpce_amd import rendering
    gallery = ByteGallery(GALLERY)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    atlas = rendering.ThumbnailAtlas(gallery, None, dev, num_workers=workers, max_side=max_side)
    torch.cuda.synchronize()
    return {'max_side': max_side, 'images': len(atlas), 'build_s': time.perf_counter() - t0, 'bytes': atlas.nbytes}


def fmt(s, digits=4):
    return f"{s['median']:.{digits}g} ({s['min']:.{digits}g} - {s['max']:.{digits}g})"


def write_markdown(path, result, baseline, args):
    with open(path, 'w') as f:
        f.write('# Compliance pictures: what the compositor, the window and the atlas cost\n\n'
                f'`python tools/bench_scene_render.py --batch {args.batch} --launches {args.launches} --baseline ... --markdown ...`, one process per checkout, '
                f'MI355X.  Median (min - max) of {WINDOWS} timed groups or windows after a warm-up one.\n\n'
                f'## The kernel alone\n\n{args.batch} canvases of {SIDE} x {SIDE}, each a base image of its size with product items of 60 .. 260 pixels a side over it, one '
                f'launch of `render_canvases`, ms per launch from HIP events around {args.launches} back-to-back launches; `render`: the whole '
                '`SceneRenderer.render` call (table upload, item concatenation, output allocation and the launch); `copy`: `out.copy_(base)` of the same '
                'bytes in the same process.\n\n'
                '| items per canvas over | bytes | kernel, ms | render, ms | copy, ms | kernel / copy |\n|---|---|---|---|---|---|\n')
        for k in result['kernel']:
            f.write(f"| {k['items']} over {'the base' if k['base'] else 'the background'} | {k['bytes']} | {fmt(k['kernel_ms'])} | {fmt(k['render_ms'])} | {fmt(k['copy_ms'])} | {k['ratio']:.2f} |\n")
        f.write(f'\n## The window\n\nImages/s, windows of {args.batch}, all comparator switches on, the comparator handed the scene\'s detections.  `parent`: '
                '`report_iter` of the commit before the pictures, same tool, a process of its own on the same machine.  `saved`: every picture also '
                f'written as PNG on {args.save_threads} host threads -- a device-to-host copy and a host encode per picture, the cost of writing files, not the kernel\'s.\n\n'
                '| scene | report_iter, parent | report_iter | pictures_iter | pictures_iter / report_iter | pictures_iter, saved |\n|---|---|---|---|---|---|\n')
        for row in result['window']:
            base = next((b for b in (baseline or {}).get('window', []) if b['scene'] == row['scene']), None)
            ratio = row['pictures_iter']['median'] / row['report_iter']['median']
            f.write(f"| {row['scene']} ({row['expected_boxes']:.0f} boxes, {row['image']}) | {fmt(base['report_iter']) if base else 'not measured'} | "
                    f"{fmt(row['report_iter'])} | {fmt(row['pictures_iter'])} | {ratio:.3f} | {fmt(row['pictures_iter_saved'])} |\n")
        f.write(f'\n## The atlas\n\n{GALLERY} synthetic gallery byte images of 256 x 256, read by {args.workers} threads.\n\n'
                '| max_side | build, s | resident bytes |\n|---|---|---|\n')
        for a in result['atlas']:
            f.write(f"| {a['max_side']} | {a['build_s']:.3g} | {a['bytes']} |\n")
        if result.get('notes'):
            f.write('\n' + '\n'.join(result['notes']) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='the checkout to measure')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--workers', type=int, default=8, help='reader threads of the atlas build')
    ap.add_argument('--save-threads', type=int, default=8)
    ap.add_argument('--json')
    ap.add_argument('--baseline')
    ap.add_argument('--markdown')
    ap.add_argument('--note', action='append', default=[])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_scene_render: no GPU -- nothing here is measured without one')
    bench, production, synthetic = load(os.path.abspath(args.root))
    dev = torch.device('cuda:0')
    det = synthetic.synthetic_gln(seed=0, detections_per_img=200).to(dev)
    enc = synthetic.synthetic_macvgg(seed=1).to(dev)
    result = {'root': os.path.abspath(args.root), 'window': [], 'kernel': [], 'atlas': [], 'notes': args.note}
    for name, r, c in GRIDS:
        result['window'].append(time_window(name, r, c, args.batch, bench, production, synthetic, det, enc, dev, args.save_threads))
        print(json.dumps(result['window'][-1]), flush=True)
    if hasattr(production.PlanogramEvaluator, 'pictures_iter'):
        from cvpce_amd import rendering
        for max_side in (128, None):
            result['atlas'].append(time_atlas(max_side, dev, args.workers))
            print(json.dumps(result['atlas'][-1]), flush=True)
        atlas = rendering.ThumbnailAtlas(ByteGallery(256), None, dev)
        for items, with_base in ((0, False), (0, True), (200, True), (1024, True)):
            result['kernel'].append(time_kernel(items, args.batch, args.launches, atlas, dev, with_base))
            print(json.dumps(result['kernel'][-1]), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(result, f)
    if args.markdown:
        baseline = json.load(open(args.baseline)) if args.baseline else None
        write_markdown(args.markdown, result, baseline, args)


if __name__ == '__main__':
    main()
