#!/usr/bin/env python
"""`dihe eval` a window at a time on the device against the per-image loop (profiles/r26_dihe_eval.md).

    python tools/bench_dihe_eval.py                                         # -> tables + one JSON line
    python tools/bench_dihe_eval.py --markdown profiles/r26_dihe_eval.md    # ... also written as a document

One section per --boxes value (boxes per shelf image), each in a child process of its own under `timeout -k 10`, one after the
other; the first that fails ends the run (this process never opens the GPU).

A section builds a synthetic in-memory test set -- seeded 8-bit shelf images with gallery products pasted into a grid of boxes, every
11th target replaced by a label no gallery item has -- and a gallery of --gallery products under a seeded MAC-VGG16, builds the index
ONCE, and runs `classification_eval.eval_dihe` over the set with `device_eval` off (the host path) and on (windows of --window), the
two alternating pass by pass in the same process: images/s and boxes/s by the host clock around a pass that ends in the harness's own
last wait plus a device synchronise, median [min .. max] of --passes passes after a warm-up pass of each.  The two accuracy dicts
are compared first.  One further pass of each path runs under `bench_planogram_compare.WindowCounter`: the project's own kernel
launches, the other torch operators on device tensors, and the points at which the host waits for the device, per image (that pass
reads the set in the calling thread, so that no reader thread's waits for its staging ring are mixed in).
"""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

STEP_TIMEOUT = 420          # seconds per child
# boxes per image -> (grid rows, grid columns, image height, image width): the scenes of tools/bench_planogram_compare.py
SCENES = {24: (4, 6, 1024, 1024), 200: (8, 25, 1728, 3136)}
OUTSIDE = 'label-outside-the-gallery'


def _median(v):
    return {'median': round(statistics.median(v), 3), 'min': round(min(v), 3), 'max': round(max(v), 3)}


def _library():
    from cvpce_amd import _lib
    return hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()


def shelf_set(products, annotations, boxes_per_image, images, seed=26):
    """`images` 8-bit shelf images (H,W,3) with rows x cols products pasted at seeded sizes inside their grid cells
    -> list of (image, targets, boxes (T,4) int64 xyxy), as `GroceryProductsTestSet(image_format='uint8')` yields them"""
    import torch
    import torch.nn.functional as F
    rows, cols, h, w = SCENES[boxes_per_image]
    g = torch.Generator().manual_seed(seed + boxes_per_image)
    cell_h, cell_w = h // rows, w // cols
    out = []
    for _ in range(images):
        img = torch.full((3, h, w), 0.32) + 0.04 * torch.rand(3, h, w, generator=g)
        boxes, targets = [], []
        for r in range(rows):
            for c in range(cols):
                bh = int(cell_h * (0.6 + 0.35 * float(torch.rand(1, generator=g))))
                bw = int(cell_w * (0.6 + 0.35 * float(torch.rand(1, generator=g))))
                y, x = r * cell_h + (cell_h - bh) // 2, c * cell_w + (cell_w - bw) // 2
                pid = int(torch.randint(0, len(products), (1,), generator=g))
                img[:, y:y + bh, x:x + bw] = F.interpolate(products[pid][None], size=(bh, bw), mode='bilinear', align_corners=False)[0]
                boxes.append([x, y, x + bw, y + bh])
                targets.append(OUTSIDE if len(boxes) % 11 == 0 else annotations[pid])
        u8 = (img.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
        out.append((u8, targets, torch.tensor(boxes, dtype=torch.int64)))
    return out


def section(args):
    import torch
    from bench_planogram_compare import WindowCounter
    from cvpce_amd import classification_eval, production, synthetic
    if not torch.cuda.is_available():
        raise SystemExit('bench_dihe_eval needs a GPU: there is nothing to fall back to')
    dev = torch.device('cuda:0')
    n_boxes = args.child
    enc = synthetic.synthetic_macvgg(seed=1).to(dev)
    products = synthetic.product_images(args.gallery, seed=200)
    annotations = [f'sku_{i // 2:05d}' if i % 10 < 2 else f'item_{i:05d}' for i in range(args.gallery)]        # (a fifth of the rows share a label pairwise)
    testset = shelf_set(products, annotations, n_boxes, args.images)
    knn = tuple(args.knn)
    clf = production.Classifier(enc, synthetic.TensorGallery(products * 2 - 1, annotations), device=dev, emb_device=dev, batch_size=64,
                                num_workers=0, k=max(knn))
    print(f'[{n_boxes} boxes] test set and index built', file=sys.stderr, flush=True)
    real = production.Classifier
    production.Classifier = lambda *a, **kw: clf          # the index is built once: both paths time the loop over the test set alone
    try:
        def one(device_eval, workers=args.workers):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            acc = classification_eval.eval_dihe(enc, None, testset, 8, workers, k=knn, device_eval=device_eval, window=args.window)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, acc
        legs = {'host': False, 'device': True}
        accs = {name: one(flag)[1] for name, flag in legs.items()}                  # warm-up pass of each
        assert accs['host'] == accs['device'], f'the two paths disagree: {accs}'
        times = {name: [] for name in legs}
        for p in range(args.passes):
            for name, flag in legs.items():
                times[name].append(one(flag)[0])
            print(f'[{n_boxes} boxes] pass {p + 1} of {args.passes}', file=sys.stderr, flush=True)
        counts = {}
        for name, flag in legs.items():
            with WindowCounter() as c:
                one(flag, workers=0)                                                # (read in this thread: no reader thread's ring waits are mixed in)
            counts[name] = {'kernels': round(c.kernels / args.images, 2), 'torch_ops': round(c.torch_device_ops / args.images, 2),
                            'waits': round((c.waits - 2) / args.images, 3)}         # (minus the two synchronises of the timing itself)
    finally:
        production.Classifier = real
    rows, cols, h, w = SCENES[n_boxes]
    total_boxes = sum(len(t) for _, t, _ in testset)
    out = {'library_sha256': _library(), 'boxes_per_image': n_boxes, 'image': f'{h} x {w}', 'images': args.images, 'gallery': args.gallery,
           'window': args.window, 'workers': args.workers, 'passes': args.passes, 'knn': list(knn), 'accuracy': {str(k): v for k, v in accs['device'].items()},
           'per_image': counts}
    for name in legs:
        out[f'images_per_s_{name}'] = _median([args.images / t for t in times[name]])
        out[f'boxes_per_s_{name}'] = _median([total_boxes / t for t in times[name]])
    out['device_over_host'] = round(out['images_per_s_device']['median'] / out['images_per_s_host']['median'], 3)
    return out


def document(result, args):
    out = ['# r26: `dihe eval` a window at a time on the device against the per-image loop', '',
           'Written by `tools/bench_dihe_eval.py --markdown`; every figure below was measured on an MI355X in the run that wrote this file (one child',
           'process per section, each under its own time limit).  A section that was not run says so.', '',
           f'Synthetic in-memory test set: seeded 8-bit shelf images, gallery products pasted into a grid of boxes at seeded sizes, every 11th target a label no',
           f'gallery item has; gallery of {args.gallery} seeded products (a fifth of the rows share a label pairwise), MAC-VGG16 with seeded weights, fp32 matcher, knn',
           f'{tuple(args.knn)}; the index is built once per section and both paths time `eval_dihe`\'s loop over the test set alone, read through `feeding.feed` with',
           f'{args.workers} reader threads.  `host`: `device_eval=False`, the per-image loop; `device`: `device_eval=True`, windows of {args.window}.  The two alternate pass by pass',
           f'in one process; images/s and boxes/s by the host clock around a pass that ends in a device synchronise, median [min .. max] of {args.passes} passes after a',
           'warm-up pass of each.  Both paths return the same accuracy dict (asserted).  Per image: `kernels` = launches of the project\'s own kernels,',
           '`torch_ops` = other torch operators on device tensors (copies, gathers, fills), `waits` = points at which the host waits for the device; counted in',
           'one further pass of each path that reads the set in the calling thread.', '']
    cols = ('boxes per image', 'image', 'images', 'images/s host', 'images/s device', 'boxes/s host', 'boxes/s device', 'device / host', 'kernels host', 'kernels device',
            'torch_ops host', 'torch_ops device', 'waits host', 'waits device')
    out += ['| ' + ' | '.join(cols) + ' |', '|' + '---|' * len(cols)]
    fmt = lambda v: f'{v["median"]:.1f} [{v["min"]:.1f} .. {v["max"]:.1f}]'
    for n in args.boxes:
        s = result.get(str(n))
        if s is None:
            out.append(f'| {n} | ' + ' | '.join(['not measured'] * (len(cols) - 1)) + ' |')
            continue
        p = s['per_image']
        out.append(f'| {n} | {s["image"]} | {s["images"]} | {fmt(s["images_per_s_host"])} | {fmt(s["images_per_s_device"])} | {fmt(s["boxes_per_s_host"])} | '
                   f'{fmt(s["boxes_per_s_device"])} | {s["device_over_host"]:.3f} | {p["host"]["kernels"]} | {p["device"]["kernels"]} | {p["host"]["torch_ops"]} | '
                   f'{p["device"]["torch_ops"]} | {p["host"]["waits"]} | {p["device"]["waits"]} |')
    out.append('')
    rec = result.get('24')
    out += ['## The figure of record', '']
    if rec is None:
        out += ['not measured (the section at 24 boxes per image was not run)', '']
    else:
        ratio = rec['device_over_host']
        verdict = 'faster' if ratio > 1 else 'NOT faster'
        out += [f'At 24 boxes per image the device path runs at **{ratio:.3f}** times the host path\'s images/s in the same run: it is {verdict} there.  '
                'The switch is opt-in either way.', '']
    out += ['## Not measured', '',
            '- A real GP-180 test set: its box sizes, aspect ratios and the cost of decoding its files.',
            '- A MACResNet encoder (plain schedule, no work lists): it takes the same path through `roi_crops`; covered by no timing here.',
            '- The gallery build at the head of `dihe eval`: it is the same on both paths (`tools/bench_gallery_build.py`).', '']
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--boxes', type=int, nargs='+', default=[24, 200], choices=sorted(SCENES), help='sections: boxes per shelf image')
    ap.add_argument('--images', type=int, default=192, help='shelf images of the test set')
    ap.add_argument('--gallery', type=int, default=1000, help='gallery products')
    ap.add_argument('--window', type=int, default=8, help='images per window of the device path')
    ap.add_argument('--workers', type=int, default=4, help='reader threads of feeding.feed (0 = read in the calling thread)')
    ap.add_argument('--knn', type=int, nargs='+', default=[1, 5])
    ap.add_argument('--passes', type=int, default=5, help='timed passes per path (at least 5)')
    ap.add_argument('--json', help='write the JSON result to this file')
    ap.add_argument('--markdown', help='write the document to this file')
    ap.add_argument('--child', type=int, choices=sorted(SCENES), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.passes < 5:
        ap.error('--passes: at least 5 (medians of at least 5 runs)')
    if args.child:
        print('RESULT ' + json.dumps(section(args)), flush=True)
        return
    result, failed = {}, None
    for n in args.boxes:                                    # chained: the first section that fails ends the run
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), '--child', str(n), '--knn', *map(str, args.knn)]
        for k in ('images', 'gallery', 'window', 'workers', 'passes'):
            cmd += ['--' + k, str(getattr(args, k))]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = next((l for l in proc.stdout.splitlines() if l.startswith('RESULT ')), None)
        if proc.returncode != 0 or line is None:
            sys.stdout.write(proc.stdout)
            failed = f'section {n} ended with exit status {proc.returncode}: nothing further was started'
            break
        result[str(n)] = json.loads(line[len('RESULT '):])
        print(f'section {n} done', flush=True)
    print(json.dumps(result), flush=True)
    if args.json:
        with open(args.json, 'w') as f:
            json.dump(result, f, indent=1)
    doc = document(result, args)
    print('\n' + doc)
    if args.markdown:
        with open(args.markdown, 'w') as f:
            f.write(doc)
    if failed:                                              # (what was measured before it is written; the rest says "not measured")
        raise SystemExit(failed)


if __name__ == '__main__':
    main()
