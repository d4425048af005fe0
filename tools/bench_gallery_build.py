#!/usr/bin/env python
"""Gallery build from 8-bit product images against the float gallery path (profiles/r24_gallery_u8.md).

    python tools/bench_gallery_build.py                                        # -> tables + one JSON line
    python tools/bench_gallery_build.py --markdown profiles/r24_gallery_u8.md  # ... also written as a document

Four measurements, each in a child process of its own under `timeout -k 10`, one after the other; the first that fails ends the run
(this process never opens the GPU):

  (a) kernel   the byte kernel (csrc/gallery.hip: C = 8 whole, C = 4 whole, C = 4 content only) against the launch it replaces,
               `pack_embed_input` over the float images of the same n; device time per image: HIP events around --launches launches
               back to back, the legs alternating, medians of --reps repetitions.  The outputs are compared bit for bit first.
  (b) memory   `Classifier.build_index` over an in-memory sample set (no decode): float items against uint8 items, the work-list
               schedule (classification.SKIP_PADDING) on and off, at every --memory-batch (images per pass); images/s by the host
               clock around a pass that ends in a device synchronise, the settings alternating, medians of --passes passes after a
               warm-up pass.
  (d) flops    in the same child: executed over algorithmic conv FLOPs of one uint8 pass with the work lists on (ops.PROFILE).
  (c) files    `build_index` over a PNG tree this tool writes into a temporary directory: the float reader against the uint8 reader
               (GroceryProductsDataset image_format), num_workers 0 and 8; images/s as in (b).

The images' aspect ratios are the fixed mix ASPECT_MIX below, cycled, tall and wide alternating.  It is NOT derived from a real product
set: how much padding a real gallery has, and with it the gain of the work lists, is not known here.
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
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STEP_TIMEOUT = 420          # seconds per child
S = 256
# shorter side over longer side of the product photos, cycled; even positions are tall (h > w), odd ones wide
ASPECT_MIX = (1.0, 0.8, 0.66, 0.5, 0.75, 0.4, 0.9, 0.3, 0.6, 0.25)


def shape_of(i, longer=S):
    short = max(1, round(longer * ASPECT_MIX[i % len(ASPECT_MIX)]))
    return (longer, short) if i % 2 == 0 else (short, longer)


def byte_images(n, seed=24):
    import torch
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, shape_of(i) + (3,), dtype=torch.uint8, generator=g) for i in range(n)]


class Items:
    """in-memory gallery sample set: (image, image, categories, annotation)"""

    def __init__(self, images):
        self.images = images

    def __len__(self):
        return len(self.images)

    def __getitem__(self, i):
        return self.images[i], self.images[i], ['Food'], f'Food/{i:05d}'


def _median(v):
    return {'median': round(statistics.median(v), 4), 'min': round(min(v), 4), 'max': round(max(v), 4)}


def _library():
    from cvpce_amd import _lib
    return hashlib.sha256(open(_lib.LIB_PATH, 'rb').read()).hexdigest()


def _need_gpu():
    import torch
    if not torch.cuda.is_available():
        raise SystemExit('bench_gallery_build needs a GPU: there is nothing to fall back to')
    return torch.device('cuda:0')


def step_kernel(args):
    import torch
    from cvpce_amd import datautils, ops, production
    from cvpce_amd.models.classification import TANH_MEAN, TANH_STD
    dev = _need_gpu()
    T = torch.ops.cvpce_amd
    mean, std = [float(v) for v in TANH_MEAN], [float(v) for v in TANH_STD]
    out = {}
    for n in args.kernel_n:
        images = byte_images(n)
        buf = torch.empty(n * S * S * 3, dtype=torch.uint8)
        geom = torch.empty((n, 3), dtype=torch.int32)
        used = production.pack_gallery_bytes(images, buf, geom, S)
        data, geom_dev = buf[:used].to(dev), geom.to(dev)
        floats = torch.stack([datautils.gallery_float(u, S) for u in images]).to(dev)
        table = ops.gallery_table(dev, mean, std)
        o8f, o8, o4 = (torch.empty((n, S, S, c), dtype=torch.bfloat16, device=dev) for c in (8, 8, 4))
        ext = torch.empty((n, 2), dtype=torch.int32, device=dev)
        legs = {
            'pack_embed_input (float, C=8)': lambda: T.pack_embed_input(floats, o8f, 0, mean, std),
            'gallery_pack_u8 C=8 whole': lambda: T.gallery_pack_u8(data, geom_dev, table, o8, 0, ext),
            'gallery_pack_u8 C=4 whole': lambda: T.gallery_pack_u8(data, geom_dev, table, o4, 0, ext),
            'gallery_pack_u8 C=4 content only': lambda: T.gallery_pack_u8(data, geom_dev, table, o4, 1, ext),
        }
        for fn in legs.values():
            fn()
        torch.cuda.synchronize()
        assert torch.equal(o8.view(torch.int16)[..., :3], o8f.view(torch.int16)[..., :3]) and not bool(o8.view(torch.int16)[..., 3:].any()), 'C=8 differs from the float path'
        assert torch.equal(o4.view(torch.int16)[..., :3], o8f.view(torch.int16)[..., :3]), 'C=4 differs from the float path'
        area = sum(u.shape[0] * u.shape[1] for u in images)
        nbytes = {'pack_embed_input (float, C=8)': n * S * S * (12 + 16), 'gallery_pack_u8 C=8 whole': area * 3 + n * S * S * 16,
                  'gallery_pack_u8 C=4 whole': area * 3 + n * S * S * 8, 'gallery_pack_u8 C=4 content only': area * 3 + area * 8}
        times = {k: [] for k in legs}
        for rep in range(args.warmup + args.reps):
            for k, fn in legs.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.launches):
                    fn()
                e1.record()
                e1.synchronize()
                if rep >= args.warmup:
                    times[k].append(e0.elapsed_time(e1) * 1000.0 / args.launches / n)        # us per image
        out[str(n)] = {k: dict(_median(v), algorithmic_bytes_per_image=round(nbytes[k] / n), gb_per_s=round(nbytes[k] / n / statistics.median(v) / 1e3, 1))
                       for k, v in times.items()}
        out[str(n)]['content_share_of_pixels'] = round(area / (n * S * S), 4)
    return {'library_sha256': _library(), 'us_per_image': out, 'launches_per_window': args.launches, 'reps': args.reps}


def _timed_build(production, torch, enc, dev, sample_set, workers, batch_size=64):
    clf = production.Classifier.__new__(production.Classifier)
    clf.batch_size, clf.num_workers, clf.device, clf.emb_device, clf.encoder = batch_size, workers, dev, dev, enc
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    emb, ann = clf.build_index(sample_set)
    torch.cuda.synchronize()
    return len(ann) / (time.perf_counter() - t0), emb


def step_memory(args):
    import torch
    from cvpce_amd import datautils, ops, production, synthetic
    from cvpce_amd.models import classification as C
    dev = _need_gpu()
    enc = synthetic.synthetic_macvgg(seed=1).to(dev)
    images = byte_images(args.memory_n)
    sets = {'uint8': Items(images), 'float': Items([datautils.gallery_float(u, S) for u in images])}
    settings = [(bs, form, skip) for bs in args.memory_batch for skip in (True, False) for form in ('float', 'uint8')]
    rates, ref = {s: [] for s in settings}, None
    for p in range(args.passes + 1):                        # pass 0 of every setting warms up
        for bs, form, skip in settings:
            C.SKIP_PADDING = skip
            rate, emb = _timed_build(production, torch, enc, dev, sets[form], 0, bs)
            assert ref is None or torch.equal(emb, ref), 'the settings must agree on the embeddings, bit for bit'
            ref = emb
            if p:
                rates[(bs, form, skip)].append(rate)
    C.SKIP_PADDING = True
    prof = ops.PROFILE = ops.ConvProfile()                  # (d): one uint8 pass with the work lists on
    try:
        _timed_build(production, torch, enc, dev, sets['uint8'], 0)
        summ = prof.summary()
    finally:
        ops.PROFILE = None
    done, alg = sum(v['flops_executed'] for v in summ.values()), sum(v['flops'] for v in summ.values())
    return {'library_sha256': _library(), 'images': args.memory_n, 'passes': args.passes,
            'images_per_s': {f'batch_size {bs}: {form} items, work lists {"on" if skip else "off"}': _median(v) for (bs, form, skip), v in rates.items()},
            'flops': {'executed': done, 'algorithmic': alg, 'executed_over_algorithmic': round(done / alg, 4)}}


def write_tree(directory, n, longer, seed=24):
    """n PNG files of smooth seeded content (8 x 8 random blocks, upsampled), the aspect mix at `longer` px, in a GP-shaped tree."""
    import numpy as np
    from PIL import Image
    rng = np.random.RandomState(seed)
    for i in range(n):
        h, w = shape_of(i, longer)
        small = rng.randint(0, 256, (max(1, h // 8), max(1, w // 8), 3), dtype=np.uint8)
        img = Image.fromarray(small).resize((w, h), Image.BILINEAR)
        d = os.path.join(directory, 'Training', 'Food', f'Cat{i % 7}')
        os.makedirs(d, exist_ok=True)
        img.save(os.path.join(d, f'{i:05d}.png'), compress_level=1)


def step_files(args):
    import torch
    from cvpce_amd import datautils, production, synthetic
    dev = _need_gpu()
    enc = synthetic.synthetic_macvgg(seed=1).to(dev)
    root = os.path.join(args.dir, 'Training')
    sets = {form: datautils.GroceryProductsDataset([root], include_annotations=True, image_format=form) for form in ('float', 'uint8')}
    assert len(sets['float']) == args.files_n
    settings = [(form, w) for w in (0, 8) for form in ('float', 'uint8')]
    rates, ref = {s: [] for s in settings}, None
    for p in range(args.passes + 1):
        for form, w in settings:
            rate, emb = _timed_build(production, torch, enc, dev, sets[form], w)
            assert ref is None or torch.equal(emb, ref), 'the readers must agree on the embeddings, bit for bit'
            ref = emb
            if p:
                rates[(form, w)].append(rate)
    return {'library_sha256': _library(), 'files': args.files_n, 'longer_side': args.files_longer, 'passes': args.passes,
            'images_per_s': {f'{form} reader, num_workers {w}': _median(v) for (form, w), v in rates.items()}}


STEPS = {'kernel': step_kernel, 'memory': step_memory, 'files': step_files}


def document(r, args):
    mix = ', '.join(f'{a:g}' for a in ASPECT_MIX)
    out = ['# r24: gallery build from 8-bit product images', '',
           'Written by `tools/bench_gallery_build.py --markdown`; every figure below was measured on an MI355X in the run that wrote this file',
           '(one child process per section, each under its own time limit).  A section that was not run says so.', '',
           f'Aspect-ratio mix (shorter over longer side, cycled, tall and wide alternating): {mix}.  It is **not derived from a real product set**:',
           'the share of padding in a real gallery, and with it what the work lists save, is not known here.', '']
    k = r.get('kernel')
    out += ['## (a) the byte kernel against the launch it replaces', '']
    if k is None:
        out += ['not measured', '']
    else:
        out += [f'library sha256 {k["library_sha256"]}; device time per image in microseconds, HIP events around {k["launches_per_window"]} launches back to back,',
                f'legs alternating, median [min .. max] of {k["reps"]} repetitions; algorithmic bytes = bytes read + pixels written.', '']
        for n, legs in k['us_per_image'].items():
            share = legs.pop('content_share_of_pixels')
            base = legs['pack_embed_input (float, C=8)']['median']
            out += [f'n = {n} images per launch (content = {share * 100:.1f} % of the pixels):', '',
                    '| launch | us per image | bytes per image | GB/s | over the float launch |', '|---|---|---|---|---|']
            for name, v in legs.items():
                out.append(f'| {name} | {v["median"]:.3f} [{v["min"]:.3f} .. {v["max"]:.3f}] | {v["algorithmic_bytes_per_image"]} | {v["gb_per_s"]} | {v["median"] / base:.3f} |')
            out.append('')
    m = r.get('memory')
    out += ['## (b) build_index over an in-memory sample set (no decode)', '']
    if m is None:
        out += ['not measured', '', '## (d) executed over algorithmic conv FLOPs of the gallery pass', '', 'not measured', '']
    else:
        out += [f'{m["images"]} items, num_workers 0, MAC-VGG16 with seeded weights; batch_size = images per pass of `build_index` (64 is the smallest it takes, and what the',
                f'eval commands get); images/s by the host clock around a pass that ends in a device synchronise, the settings alternating, median [min .. max] of {m["passes"]} passes after a warm-up pass.  All settings give the same embeddings, bit for bit.', '',
                '| setting | images/s |', '|---|---|']
        for name, v in m['images_per_s'].items():
            out.append(f'| {name} | {v["median"]:.1f} [{v["min"]:.1f} .. {v["max"]:.1f}] |')
        f = m['flops']
        out += ['', '## (d) executed over algorithmic conv FLOPs of the gallery pass', '',
                f'One uint8 pass with the work lists on, per-launch records (ops.PROFILE): {f["executed"] / 1e12:.3f} TFLOP executed of {f["algorithmic"] / 1e12:.3f} TFLOP',
                f'algorithmic = **{f["executed_over_algorithmic"]:.3f}** for the mix above.  The float path executes 1.000 (nothing tells it the extents).', '']
    c = r.get('files')
    out += ['## (c) build_index over a PNG tree', '']
    if c is None:
        out += ['not measured', '']
    else:
        out += [f'{c["files"]} PNG files (smooth seeded content, longer side {c["longer_side"]} px, the mix above) written into a temporary directory; GroceryProductsDataset with',
                f'image_format float / uint8; images/s as in (b), median [min .. max] of {c["passes"]} passes after a warm-up pass.  Both readers give the same embeddings, bit for bit.', '',
                '| setting | images/s |', '|---|---|']
        for name, v in c['images_per_s'].items():
            out.append(f'| {name} | {v["median"]:.1f} [{v["min"]:.1f} .. {v["max"]:.1f}] |')
        out.append('')
    out += ['## Not measured', '',
            '- A real product set (Grocery Products, the internal renders): neither its aspect ratios nor its file sizes and formats.',
            '- A MACResNet encoder (plain schedule, C = 8): covered by the tests for bits, not timed.',
            '- `dihe eval` / `eval-*` end to end: their gallery build is the `build_index` measured in (c).', '']
    return '\n'.join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--steps', default='kernel,memory,files', help='comma-separated subset of kernel,memory,files, run in this order')
    ap.add_argument('--kernel-n', type=int, nargs='+', default=[64, 512], help='(a) images per launch')
    ap.add_argument('--launches', type=int, default=50, help='(a) launches per timed window')
    ap.add_argument('--reps', type=int, default=15, help='(a) timed windows per leg (at least 5)')
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--memory-n', type=int, default=1024, help='(b) items of the in-memory sample set')
    ap.add_argument('--memory-batch', type=int, nargs='+', default=[64, 512], help='(b) batch_size values (images per pass)')
    ap.add_argument('--files-n', type=int, default=384, help='(c) PNG files')
    ap.add_argument('--files-longer', type=int, default=480, help='(c) longer side of the PNG files')
    ap.add_argument('--passes', type=int, default=5, help='(b), (c) timed passes per setting (at least 5)')
    ap.add_argument('--dir', help=argparse.SUPPRESS)
    ap.add_argument('--json', help='write the JSON result to this file')
    ap.add_argument('--markdown', help='write the document to this file')
    ap.add_argument('--child', choices=sorted(STEPS), help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.reps < 5 or args.passes < 5:
        ap.error('--reps / --passes: at least 5 (medians of at least 5 runs)')
    if args.child:
        print('RESULT ' + json.dumps(STEPS[args.child](args)), flush=True)
        return
    steps = [s for s in args.steps.split(',') if s]
    for s in steps:
        if s not in STEPS:
            ap.error(f'--steps: unknown step {s!r}')
    directory = tempfile.mkdtemp(prefix='cvpce_gallery_build_')
    result, failed = {'aspect_mix': list(ASPECT_MIX)}, None
    try:
        if 'files' in steps:
            write_tree(directory, args.files_n, args.files_longer)
        for s in steps:                                     # chained: the first step that fails ends the run
            cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), '--child', s, '--dir', directory,
                   '--kernel-n', *map(str, args.kernel_n), '--memory-batch', *map(str, args.memory_batch)]
            for k in ('launches', 'reps', 'warmup', 'memory_n', 'files_n', 'files_longer', 'passes'):
                cmd += ['--' + k.replace('_', '-'), str(getattr(args, k))]
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            line = next((l for l in proc.stdout.splitlines() if l.startswith('RESULT ')), None)
            if proc.returncode != 0 or line is None:
                sys.stdout.write(proc.stdout)
                failed = f'step {s} ended with exit status {proc.returncode}: nothing further was started'
                break
            result[s] = json.loads(line[len('RESULT '):])
            print(f'step {s} done', flush=True)
        print(json.dumps(result), flush=True)
        if args.json:
            with open(args.json, 'w') as f:
                json.dump(result, f, indent=1)
        doc = document(json.loads(json.dumps(result)), args)
        print('\n' + doc)
        if args.markdown:
            with open(args.markdown, 'w') as f:
                f.write(doc)
        if failed:                                          # (what was measured before it is written; the rest says "not measured")
            raise SystemExit(failed)
    finally:
        shutil.rmtree(directory, ignore_errors=True)


if __name__ == '__main__':
    main()
