#!/usr/bin/env python
"""Byte-reading input kernels against the conversion path, in one process and one call (profiles/r12_u8_kernels.md).

    python tools/bench_u8_kernels.py                  # -> a table + one JSON line
    python tools/bench_u8_kernels.py --json out.json  # ... also written to a file

Workload: the input-path benchmark's scenes (tools/bench_input_path.py: 2048 x 2048 JPEG files of 8 distinct seeded shelves), 200
planted boxes per image (bench.py's distribution: sides 60-250 px, seed 7).  The 8 distinct images are on the device as the
decoder's (H,W,3) bytes; per repetition, alternating, HIP events on the launch stream around

    (a) today's path:  ops.uint8_to_float of the 8 images, the detector's transform of the 8 float images (one launch), 8 crop
                       launches from the float images (mode 2, content only: the product path's form);
    (b) byte kernels:  the transform of the 8 byte images (one launch), 8 crop launches from the bytes.

and, each on its own, around the conversions, the transform and the crop launches (content only, and whole crops) in both forms.
Medians of --reps repetitions (at least 20) after --warmup; everything per image.  The outputs of (a) and (b) are compared bit
for bit before anything is timed.  Then, end to end: `PlanogramEvaluator.evaluate_iter` over the JPEG files behind
`ImageFeeder(workers=4)` with ops.U8_KERNELS off and on, alternating passes, images/s per pass (host clock around a pass that ends
in a device synchronise), so that the spread of one setting stands beside the difference between the two.

The measurement runs in ONE child process under `timeout -k 10`; this process never opens the GPU.
"""
import argparse
import hashlib
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tools')):
    if p not in sys.path:
        sys.path.insert(0, p)

STEP_TIMEOUT = 540          # seconds for the child
DISTINCT = 8
BOXES = 200


def planted_boxes(n_images, dpi, image_size, seed=7):
    """bench.py's planted proposals: sides uniform in 60-250 px, uniformly placed."""
    import torch
    g = torch.Generator().manual_seed(seed)
    wh = 60 + 190 * torch.rand(n_images * dpi, 2, generator=g)
    xy = torch.rand(n_images * dpi, 2, generator=g) * (float(image_size) - wh)
    return torch.cat((xy, xy + wh), dim=1).view(n_images, dpi, 4)


def measure(args):
    import torch
    from bench_input_path import Scenes, CountingComparator
    from cvpce_amd import _lib, datautils, feeding, ops, production, synthetic
    from cvpce_amd.models.classification import TANH_MEAN, TANH_STD
    if not torch.cuda.is_available():
        raise SystemExit('bench_u8_kernels needs a GPU: there is nothing to fall back to')
    dev = torch.device('cuda:0')
    paths = sorted(os.path.join(args.dir, f) for f in os.listdir(args.dir) if f.endswith('.jpg'))[:args.images]
    data = Scenes(paths, datautils.pil_to_uint8)
    det = synthetic.synthetic_gln(seed=0, detections_per_img=BOXES).to(dev)
    eng = det.engine()
    us = [data[i][0].to(dev) for i in range(min(DISTINCT, len(paths)))]
    n = len(us)
    h, w = datautils.image_hw(us[0])
    boxes = planted_boxes(n, BOXES, min(h, w)).to(dev)
    count = torch.full((n,), BOXES, dtype=torch.int32, device=dev)
    size = datautils.CLASSIFICATION_IMAGE_SIZE
    ext = ops.crop_extents(boxes.reshape(n * BOXES, 4), count, h, w, size, per_image=BOXES)
    crops = {k: torch.empty((n * BOXES, size, size, 4), dtype=torch.bfloat16, device=dev) for k in 'ab'}

    def convert():
        return [ops.uint8_to_float(u) for u in us]

    def transform(images):
        return eng.transform(images)[0]

    def crop(images, out, content=True):
        for i, img in enumerate(images):
            sl = slice(i * BOXES, (i + 1) * BOXES)
            ops.crop_resize(img, boxes[i], size, mode=2, mean=TANH_MEAN, std=TANH_STD, count=count[i:i + 1], out=out[sl],
                            content_ext=ext[sl] if content else None)

    ops.U8_KERNELS = True          # (ops.gln_transform_batch / ops.crop_resize handed bytes launch the byte kernels)
    fs = convert()

    # the two paths compute the same bits
    for k in 'ab':
        crops[k].zero_()
    ta, tb = transform(fs), transform(us)
    crop(fs, crops['a']); crop(us, crops['b'])
    torch.cuda.synchronize()
    assert torch.equal(ta.view(torch.int16), tb.view(torch.int16)), 'transform: the byte kernel differs from the float kernel'
    assert torch.equal(crops['a'].view(torch.int16), crops['b'].view(torch.int16)), 'crops: the byte kernel differs from the float kernel'
    crop(fs, crops['a'], False); crop(us, crops['b'], False)
    torch.cuda.synchronize()
    assert torch.equal(crops['a'].view(torch.int16), crops['b'].view(torch.int16)), 'whole crops: the byte kernel differs from the float kernel'
    del ta, tb

    def total_a():
        f = convert()
        transform(f)
        crop(f, crops['a'])

    def total_b():
        transform(us)
        crop(us, crops['b'])

    legs = {
        'total_a': total_a, 'total_b': total_b,
        'convert_a': convert,
        'transform_a': lambda: transform(fs), 'transform_b': lambda: transform(us),
        'crop_content_a': lambda: crop(fs, crops['a']), 'crop_content_b': lambda: crop(us, crops['b']),
        'crop_whole_a': lambda: crop(fs, crops['a'], False), 'crop_whole_b': lambda: crop(us, crops['b'], False),
    }
    times = {k: [] for k in legs}
    for rep in range(args.warmup + args.reps):          # every repetition runs every leg once: the two forms alternate
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if rep >= args.warmup:
                times[k].append(e0.elapsed_time(e1) / n)
    device = {k: {'median_ms': round(statistics.median(v), 4), 'min_ms': round(min(v), 4), 'max_ms': round(max(v), 4)} for k, v in times.items()}

    # bytes resident: what the kernels read, and the peak while it is made
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    f0 = ops.uint8_to_float(us[0])
    torch.cuda.synchronize()
    resident = {'a_image_bytes': f0.numel() * 4, 'a_peak_bytes_beside_the_upload': torch.cuda.max_memory_allocated() - base,
                'b_image_bytes': us[0].numel(), 'uploaded_bytes': us[0].numel()}
    del f0, fs

    # end to end: files -> evaluate_iter behind the feeder, the switch off and on, alternating
    enc = synthetic.synthetic_macvgg(seed=1).to(dev)
    clf = production.Classifier(enc, synthetic.TensorGallery(synthetic.gallery_images(256, seed=100)), device=dev, emb_device=dev,
                                batch_size=64)
    ev = production.PlanogramEvaluator(production.ProposalGenerator(det, device=dev), clf, CountingComparator())
    rates, detections = {False: [], True: []}, None
    for p in range(args.passes + 1):                    # pass 0 of each setting warms up
        for on in (False, True):
            ops.U8_KERNELS = on
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            got = [int(v) for v in ev.evaluate_iter(feeding.ImageFeeder(data, workers=args.workers, device=dev), lookahead=4)]
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            assert len(got) == len(paths) and (detections is None or got == detections), 'the settings must agree on the detections'
            detections = got
            if p:
                rates[on].append(round(len(paths) / dt, 2))
    return {'library_sha256': hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest(), 'images': n, 'height': h, 'width': w,
            'boxes_per_image': BOXES, 'reps': args.reps, 'warmup': args.warmup, 'device_ms_per_image': device, 'resident': resident,
            'end_to_end': {'files': len(paths), 'workers': args.workers, 'passes': args.passes,
                           'images_per_s_off': rates[False], 'images_per_s_on': rates[True],
                           'median_off': statistics.median(rates[False]), 'median_on': statistics.median(rates[True])},
            'detections_checksum': sum(detections)}


def table(r):
    d, e, m = r['device_ms_per_image'], r['end_to_end'], r['resident']
    rows = [('conversion (a only)', 'convert_a', None), ('transform', 'transform_a', 'transform_b'),
            ('crops, content only', 'crop_content_a', 'crop_content_b'), ('crops, whole', 'crop_whole_a', 'crop_whole_b'),
            ('TOTAL conversion + transform + crops', 'total_a', 'total_b')]
    out = [f'library sha256 {r["library_sha256"]}',
           f'{r["images"]} images {r["height"]} x {r["width"]}, {r["boxes_per_image"]} boxes each; ms per image, median [min .. max] of {r["reps"]} repetitions', '',
           f'| {"per image":<38} | {"(a) conversion + float kernels":<32} | {"(b) byte kernels":<32} | b / a |', '|' + '-' * 40 + '|' + '-' * 34 + '|' + '-' * 34 + '|-------|']
    cell = lambda k: f'{d[k]["median_ms"]:.4f} [{d[k]["min_ms"]:.4f} .. {d[k]["max_ms"]:.4f}]' if k else '-'
    for name, a, b in rows:
        ratio = f'{d[b]["median_ms"] / d[a]["median_ms"]:.3f}' if b else '-'
        out.append(f'| {name:<38} | {cell(a):<32} | {cell(b):<32} | {ratio:>5} |')
    out += ['', f'image bytes the kernels read: (a) {m["a_image_bytes"] / 1e6:.1f} MB (peak {m["a_peak_bytes_beside_the_upload"] / 1e6:.1f} MB allocated beside the '
                f'{m["uploaded_bytes"] / 1e6:.1f} MB upload while it is made), (b) {m["b_image_bytes"] / 1e6:.1f} MB (the upload itself)', '',
            f'end to end, evaluate_iter over {e["files"]} JPEG files behind ImageFeeder(workers={e["workers"]}), images/s per pass:',
            f'  CVPCE_U8_KERNELS=0  {e["images_per_s_off"]}  median {e["median_off"]:.2f}',
            f'  CVPCE_U8_KERNELS=1  {e["images_per_s_on"]}  median {e["median_on"]:.2f}']
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--images', type=int, default=32, help='JPEG files per end-to-end pass (the first 8 are the device-side workload)')
    ap.add_argument('--height', type=int, default=2048)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--reps', type=int, default=25, help='timed repetitions of every device-side leg (at least 20)')
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--passes', type=int, default=5, help='timed end-to-end passes per setting after the warm-up pass')
    ap.add_argument('--workers', type=int, default=4)
    ap.add_argument('--dir', help='directory of the JPEG files (kept); default: a temporary directory, removed afterwards')
    ap.add_argument('--json', help='write the JSON result to this file')
    ap.add_argument('--child', action='store_true', help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 20:
        ap.error('--reps: at least 20')
    if args.child:
        print('RESULT ' + json.dumps(measure(args)), flush=True)
        return
    from bench_input_path import write_scenes
    directory = args.dir or tempfile.mkdtemp(prefix='cvpce_u8_kernels_')
    os.makedirs(directory, exist_ok=True)
    try:
        write_scenes(directory, args.images, args.height, args.width)
        cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), '--child', '--dir', directory]
        for k in ('images', 'reps', 'warmup', 'passes', 'workers'):
            cmd += [f'--{k}', str(getattr(args, k))]
        proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        line = next((l for l in proc.stdout.splitlines() if l.startswith('RESULT ')), None)
        if proc.returncode != 0 or line is None:
            sys.stdout.write(proc.stdout)
            raise SystemExit(f'the measurement ended with exit status {proc.returncode}')
        result = json.loads(line[len('RESULT '):])
        print(json.dumps(result), flush=True)
        print('\n' + table(result))
        if args.json:
            with open(args.json, 'w') as f:
                json.dump(result, f, indent=1)
    finally:
        if not args.dir:
            shutil.rmtree(directory, ignore_errors=True)


if __name__ == '__main__':
    main()
