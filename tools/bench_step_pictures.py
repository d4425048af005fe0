"""What the step pictures cost: the stroke launch alone beside the compositor and a device copy of the same bytes,
`PlanogramEvaluator.step_pictures_iter` against `pictures_iter` and `report_iter`, and the launches and waits of a window.

  kernel    8 canvases of 2048^2 with the graph of 200 (then 1 024) boxes on a grid drawn over each -- 9 strokes a node: its 8 direction
            slots and its disc -- `strokes_draw` alone, HIP events around --launches back-to-back launches, three timed groups after a
            warm-up group; beside it `render_canvases` of the same canvases (a base image and the boxes' product items) and
            `out.copy_(base)` of the same bytes, all in the same process
  window    `step_pictures_iter` against `pictures_iter` and `report_iter` on the scenes of tools/bench_scene_render.py (gridded planograms
            of 24 and 200 boxes, every 9th planted detection withheld, every 11th expected label one no gallery item has), windows of 8,
            images/s, wall clock around a window that ends in a synchronise: three timed windows per path after a warm-up window, the
            paths alternating; the pictures are left on the device (the PNG encode is not measured here)
  counts    launches, waits and other device operators of one window per path (`WindowCounter`), the window's switches

The yardstick of the window is `pictures_iter` and `report_iter` of the commit BEFORE the step pictures: run the tool there with
`--root <that checkout> --json parent.json` (a tree without `step_pictures_iter` measures the two alone), then here with
`--baseline parent.json --markdown ...`.

    python tools/bench_step_pictures.py [--root DIR] [--batch 8] [--launches 20] [--json out.json] [--baseline parent.json]
                                        [--markdown profiles/r33_step_pictures.md]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import torch

SWITCHES = dict(device_graphs=True, device_tail=True, device_reclass=True)
GRIDS = (('grid_4x6', 4, 6), ('grid_8x25', 8, 25))
NODE_GRIDS = ((200, 10, 20), (1024, 32, 32))
SIDE = 2048


def load(root, name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, 'tools', name + '.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def grid_graph(rows, cols, dev):
    """rows x cols boxes spread over a SIDE^2 canvas and the full 8-neighbour grid graph over them: every inner node fills all 8 slots
    -> (boxes (n, 4), nbr (n, 8) int32), on the device"""
    from cvpce_amd.planograms import CARDINALS
    step = {'E': (0, 1), 'NE': (-1, 1), 'N': (-1, 0), 'NW': (-1, -1), 'W': (0, -1), 'SW': (1, -1), 'S': (1, 0), 'SE': (1, 1)}
    cw, ch = SIDE / cols, SIDE / rows
    boxes = torch.tensor([[c * cw + 0.1 * cw, r * ch + 0.1 * ch, (c + 1) * cw - 0.1 * cw, (r + 1) * ch - 0.1 * ch] for r in range(rows) for c in range(cols)])
    nbr = torch.full((rows * cols, 8), -1, dtype=torch.int32)
    for r in range(rows):
        for c in range(cols):
            for s, d in enumerate(CARDINALS):
                rr, cc = r + step[d][0], c + step[d][1]
                if 0 <= rr < rows and 0 <= cc < cols:
                    nbr[r * cols + c, s] = rr * cols + cc
    return boxes.to(dev), nbr.to(dev)


def time_kernel(nodes, rows, cols, batch, launches, atlas, dev, scene):
    from cvpce_amd import rendering
    g = torch.Generator().manual_seed(nodes)
    base = torch.randint(0, 256, (batch, SIDE, SIDE, 3), dtype=torch.uint8, generator=g).to(dev)
    boxes, nbr = grid_graph(rows, cols, dev)
    whole = rendering._items(torch.tensor([[0.0, 0.0, SIDE, SIDE]], device=dev), rendering.R.SRC_BASE, 0, 0)
    products = rendering.observed_items(boxes, torch.randint(0, len(atlas), (len(boxes),), generator=g).to(dev))
    lists = [rendering.Items.cat([whole, products])] * batch
    strokes = [rendering.graph_strokes(nbr, boxes)] * batch
    renderer = rendering.SceneRenderer(atlas)
    sizes = [(SIDE, SIDE)] * batch
    renderer.render(lists, sizes, list(base), strokes=strokes)
    draw, paint = renderer.last_strokes, renderer.last_launch
    out = torch.empty_like(base)
    flat = out.view(-1)
    res = {'nodes': nodes, 'strokes': len(strokes[0]), 'edges': int((nbr >= 0).sum()), 'batch': batch, 'bytes': base.numel(),
           'strokes_ms': scene.events(lambda: torch.ops.cvpce_amd.strokes_draw(*draw, flat), launches),
           'render_ms': scene.events(lambda: torch.ops.cvpce_amd.render_canvases(*paint, flat), launches),
           'copy_ms': scene.events(lambda: out.copy_(base), launches)}
    res['strokes_over_render'] = res['strokes_ms']['median'] / res['render_ms']['median']
    return res


def time_window(name, rows, cols, batch, bench, scene, production, synthetic, det, enc, dev):
    pairs, (h, w) = bench.miss_scenes(rows, cols, batch)
    names = synthetic.PLANOGRAM_LABELS
    gallery = synthetic.TensorGallery(synthetic.gallery_images(64, seed=100), [names[i % len(names)] for i in range(64)])
    clf = production.Classifier(enc, gallery, device=dev, emb_device=dev, batch_size=32, match_dtype=torch.bfloat16)
    pg = production.ProposalGenerator(det, device=dev, confidence_threshold=0.5)
    images = [synthetic.shelf_image(400 + k, h, w).to(dev) for k in range(batch)]
    es, acts = [e for e, _ in pairs], [a for _, a in pairs]
    ev = bench.PlantedEvaluator(pg, clf, production.PlanogramComparator(**SWITCHES))
    ev.planted = [(a['boxes'], a['labels']) for a in acts]
    from cvpce_amd import rendering
    renderer = rendering.SceneRenderer(rendering.ThumbnailAtlas(gallery, clf.annotations, dev))
    row = {'scene': name, 'batch': batch, 'image': f'{h} x {w}', 'expected_boxes': sum(len(e['labels']) for e in es) / batch}
    paths = {'report_iter': lambda: list(ev.report_iter(zip(images, es), lookahead=batch)),
             'pictures_iter': lambda: list(ev.pictures_iter(zip(images, es), renderer, lookahead=batch))}
    if hasattr(ev, 'step_pictures_iter'):
        paths['step_pictures_iter'] = lambda: list(ev.step_pictures_iter(zip(images, es), renderer, lookahead=batch))
    rates = {p: [] for p in paths}
    for r in range(scene.WINDOWS + 1):
        for p, run in paths.items():
            ev._at = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            run()
            torch.cuda.synchronize()
            if r:
                rates[p].append(batch / (time.perf_counter() - t0))
    for p in paths:
        row[p] = scene.spread(rates[p])
    counts = {}
    for p, run in paths.items():
        ev._at = 0
        with bench.WindowCounter() as c:
            run()
        counts[p] = {'launches': c.kernels, 'waits': c.waits, 'other_device_operators': c.torch_device_ops}
    row['counts'] = counts
    return row


def write_markdown(path, result, baseline, args, scene):
    fmt = scene.fmt
    with open(path, 'w') as f:
        f.write('# Step pictures: what the stroke launch and the window cost\n\n'
                f'`python tools/bench_step_pictures.py --batch {args.batch} --launches {args.launches} --baseline ... --markdown ...`, one process per checkout, '
                f'MI355X.  Median (min - max) of {scene.WINDOWS} timed groups or windows after a warm-up one.\n\n'
                f'## The stroke launch alone\n\n{args.batch} canvases of {SIDE} x {SIDE}, the full 8-neighbour graph of a grid of boxes drawn over each (9 stroke slots a '
                'node, radius 2 edges and radius 10 discs), one launch of `strokes_draw`, ms per launch from HIP events around '
                f'{args.launches} back-to-back launches; `render_canvases`: the compositor on the same canvases (a base image and one product item a box); `copy`: '
                '`out.copy_(base)` of the same bytes.  All three in the same process.\n\n'
                '| nodes per graph | strokes (filled edges) per canvas | bytes | strokes_draw, ms | render_canvases, ms | copy, ms | strokes / render |\n|---|---|---|---|---|---|---|\n')
        for k in result['kernel']:
            f.write(f"| {k['nodes']} | {k['strokes']} ({k['edges']}) | {k['bytes']} | {fmt(k['strokes_ms'])} | {fmt(k['render_ms'])} | {fmt(k['copy_ms'])} | {k['strokes_over_render']:.2f} |\n")
        f.write(f'\n## The window\n\nImages/s, windows of {args.batch}, all comparator switches on, the comparator handed the scene\'s detections, the pictures left on '
                'the device.  `parent`: the commit before the step pictures, same tool, a process of its own on the same machine.\n\n'
                '| scene | report_iter, parent | report_iter | pictures_iter, parent | pictures_iter | step_pictures_iter | step_pictures_iter / pictures_iter |\n|---|---|---|---|---|---|---|\n')
        for row in result['window']:
            base = next((b for b in (baseline or {}).get('window', []) if b['scene'] == row['scene']), None)
            of = lambda r, p: fmt(r[p]) if r and p in r else 'not measured'
            ratio = row['step_pictures_iter']['median'] / row['pictures_iter']['median'] if 'step_pictures_iter' in row else float('nan')
            f.write(f"| {row['scene']} ({row['expected_boxes']:.0f} boxes, {row['image']}) | {of(base, 'report_iter')} | {of(row, 'report_iter')} | "
                    f"{of(base, 'pictures_iter')} | {of(row, 'pictures_iter')} | {of(row, 'step_pictures_iter')} | {ratio:.3f} |\n")
        f.write('\n## Launches and waits per window\n\n| scene | path | launches | waits | other device operators |\n|---|---|---|---|---|\n')
        for row in result['window']:
            for p, c in row['counts'].items():
                f.write(f"| {row['scene']} | {p} | {c['launches']} | {c['waits']} | {c['other_device_operators']} |\n")
        if result.get('notes'):
            f.write('\n' + '\n'.join(result['notes']) + '\n')


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--root', default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help='the checkout to measure')
    ap.add_argument('--batch', type=int, default=8)
    ap.add_argument('--launches', type=int, default=20)
    ap.add_argument('--json')
    ap.add_argument('--baseline')
    ap.add_argument('--markdown')
    ap.add_argument('--note', action='append', default=[])
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('bench_step_pictures: no GPU -- nothing here is measured without one')
    root = os.path.abspath(args.root)
    sys.path.insert(0, root)
    bench, scene = load(root, 'bench_planogram_compare'), load(root, 'bench_scene_render')
    from cvpce_amd import production, rendering, synthetic
    dev = torch.device('cuda:0')
    det = synthetic.synthetic_gln(seed=0, detections_per_img=200).to(dev)
    enc = synthetic.synthetic_macvgg(seed=1).to(dev)
    result = {'root': root, 'window': [], 'kernel': [], 'notes': args.note}
    for name, r, c in GRIDS:
        result['window'].append(time_window(name, r, c, args.batch, bench, scene, production, synthetic, det, enc, dev))
        print(json.dumps(result['window'][-1]), flush=True)
    if hasattr(rendering, 'graph_strokes'):
        atlas = rendering.ThumbnailAtlas(scene.ByteGallery(256), None, dev)
        for nodes, r, c in NODE_GRIDS:
            result['kernel'].append(time_kernel(nodes, r, c, args.batch, args.launches, atlas, dev, scene))
            print(json.dumps(result['kernel'][-1]), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(result, f)
    if args.markdown:
        baseline = json.load(open(args.baseline)) if args.baseline else None
        write_markdown(args.markdown, result, baseline, args, scene)


if __name__ == '__main__':
    main()
