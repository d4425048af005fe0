#!/usr/bin/env python
"""What the input path costs: shelf photographs as JPEG FILES through `PlanogramEvaluator.evaluate_iter` (bench.py measures the
kernels on device-resident float images; this measures what a user with files gets).

    python tools/bench_input_path.py                   # every configuration -> a table + one JSON line per configuration
    python tools/bench_input_path.py --baseline        # configuration (a) only, with calls that exist before the 8-bit form:
                                                       # copy this file into an older checkout to measure that one

N synthetic shelf scenes (cvpce_amd/synthetic.py) are written as JPEG files into a temporary directory (or --dir, which is kept and
reused), then read back through `evaluate_iter(..., lookahead=4)` with a trivial comparator:

    float_serial     (a) float readers (`pil_to_tensor`), read one after the other in the calling thread
    uint8_serial     (b) 8-bit readers (`pil_to_uint8`), read the same way
    uint8_feeder_W   (c) 8-bit readers behind `ImageFeeder(workers=W)`, W = 1 / 4 / 8 / 16
    device_resident      the float images already on the device: what the kernels alone do (the ceiling of every row above)

Per configuration: images/s (host clock around a pass that ends in a device synchronise; median of --passes passes after a warm-up
pass), bytes uploaded per image, the time of the 8-bit -> float conversion on the device (events around it), and the host's
reading time per image measured on its own (decode + tensor conversion, no GPU work).  Every configuration runs in a child process
of its own under `timeout -k 10`; the first one that fails ends the run.
"""
import argparse
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

FEEDER_WORKERS = (1, 4, 8, 16)
STEP_TIMEOUT = 300          # seconds, per configuration


def write_scenes(directory, n, h, w, distinct=8):
    """n JPEG files of `distinct` seeded scenes (products on shelf rows); nothing is written when they are all there."""
    import torch
    from PIL import Image
    from cvpce_amd import synthetic
    paths = [os.path.join(directory, f'shelf_{i:04d}.jpg') for i in range(n)]
    if all(os.path.exists(p) for p in paths):
        return paths
    products = synthetic.product_images(32, seed=200)
    for s in range(min(distinct, n)):
        img, _, _ = synthetic.structured_shelf(1000 + s, h, w, products)
        pil = Image.fromarray((img * 255).round().to(torch.uint8).permute(1, 2, 0).numpy())
        for p in paths[s::distinct]:
            pil.save(p, quality=90)
    return paths


class Scenes:
    """(image, planogram) pairs read from the files; `read` is datautils.pil_to_tensor or pil_to_uint8."""

    def __init__(self, paths, read):
        self.paths, self.read = paths, read

    def __len__(self):
        return len(self.paths)

    def __getitem__(self, i):
        from PIL import Image
        return self.read(Image.open(self.paths[i]).convert('RGB')), {'boxes': (), 'labels': ()}


class CountingComparator:
    """The trivial comparator: the verdict is the number of detections."""

    def compare(self, expected, actual, image=None, classifier=None):
        return len(actual['boxes'])


def run_configuration(args):
    """One configuration in this process -> a dict (printed as one JSON line by the caller)."""
    import torch
    from cvpce_amd import datautils, production, synthetic
    if not torch.cuda.is_available():
        raise SystemExit('bench_input_path needs a GPU: there is nothing to fall back to')
    dev = torch.device('cuda:0')
    name = args.config
    paths = sorted(os.path.join(args.dir, f) for f in os.listdir(args.dir) if f.endswith('.jpg'))[:args.images]
    det = synthetic.synthetic_gln(seed=0, detections_per_img=200).to(dev)
    enc = synthetic.synthetic_macvgg(seed=1).to(dev)
    clf = production.Classifier(enc, synthetic.TensorGallery(synthetic.gallery_images(256, seed=100)), device=dev, emb_device=dev,
                                batch_size=64)
    ev = production.PlanogramEvaluator(production.ProposalGenerator(det, device=dev), clf, CountingComparator())
    convert_events, feeders = [], []
    if name == 'float_serial':                    # (only calls that exist without the 8-bit form)
        data = Scenes(paths, datautils.pil_to_tensor)
        source = lambda: (data[i] for i in range(len(data)))
    elif name == 'device_resident':
        data = Scenes(paths, datautils.pil_to_tensor)
        resident = [(img.to(dev), p) for img, p in (data[i] for i in range(len(data)))]
        source = lambda: iter(resident)
    else:
        from cvpce_amd import feeding, ops
        data = Scenes(paths, datautils.pil_to_uint8)
        inner = ops.uint8_to_float

        def timed(u):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = inner(u)
            e1.record()
            convert_events.append((e0, e1))
            return out
        ops.uint8_to_float = timed
        if name == 'uint8_serial':
            source = lambda: (data[i] for i in range(len(data)))
        else:
            workers = int(name.rsplit('_', 1)[1])

            def source():
                feeders.append(feeding.ImageFeeder(data, workers=workers, device=dev))
                return feeders[-1]

    # the host's reading time on its own (no GPU work in flight)
    t0 = time.perf_counter()
    first = [data[i] for i in range(min(8, len(data)))]
    read_ms = (time.perf_counter() - t0) * 1000 / len(first)
    h, w = first[0][0].shape[-2:] if first[0][0].dtype.is_floating_point else first[0][0].shape[:2]
    per_image = first[0][0].numel() * first[0][0].element_size()
    del first

    rates, convert_ms, detections = [], [], None
    for p in range(args.passes + 1):              # pass 0 warms up: code objects, the detector's captured schedule, the pinned ring
        convert_events.clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        got = [int(v) for v in ev.evaluate_iter(source(), lookahead=4)]
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert len(got) == len(paths)
        assert detections is None or got == detections, 'the passes of one configuration must agree'
        detections = got
        if p:
            rates.append(len(paths) / dt)
            if convert_events:
                convert_ms.append(sum(a.elapsed_time(b) for a, b in convert_events) / len(convert_events))
    uploaded = feeders[-1].bytes_uploaded // len(paths) if feeders else (0 if name == 'device_resident' else per_image)
    return {'config': name, 'images': len(paths), 'height': int(h), 'width': int(w), 'passes': args.passes,
            'images_per_s': round(statistics.median(rates), 2), 'images_per_s_passes': [round(r, 2) for r in rates],
            'uploaded_bytes_per_image': int(uploaded), 'host_read_ms_per_image': round(read_ms, 2),
            'convert_ms_per_image': round(statistics.median(convert_ms), 4) if convert_ms else None,
            'detections_checksum': sum(detections), 'detections_min': min(detections)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument('--images', type=int, default=32, help='files per pass')
    ap.add_argument('--height', type=int, default=2048)
    ap.add_argument('--width', type=int, default=2048)
    ap.add_argument('--passes', type=int, default=3, help='timed passes after the warm-up pass (the median is reported)')
    ap.add_argument('--baseline', action='store_true', help='configuration (a) only: float readers, serial')
    ap.add_argument('--dir', help='directory of the JPEG files (kept); default: a temporary directory, removed afterwards')
    ap.add_argument('--json', help='append the JSON lines to this file')
    ap.add_argument('--config', help=argparse.SUPPRESS)          # (a child process: run this one configuration)
    args = ap.parse_args()
    if args.config:
        print('RESULT ' + json.dumps(run_configuration(args)), flush=True)
        return
    directory = args.dir or tempfile.mkdtemp(prefix='cvpce_input_path_')
    os.makedirs(directory, exist_ok=True)
    try:
        write_scenes(directory, args.images, args.height, args.width)
        configs = ['float_serial'] if args.baseline else (['float_serial', 'uint8_serial'] + [f'uint8_feeder_{w}' for w in FEEDER_WORKERS]
                                                          + ['device_resident'])
        results = []
        for config in configs:
            cmd = ['timeout', '-k', '10', str(STEP_TIMEOUT), sys.executable, os.path.abspath(__file__), '--config', config, '--dir', directory,
                   '--images', str(args.images), '--passes', str(args.passes)]
            proc = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
            line = next((l for l in proc.stdout.splitlines() if l.startswith('RESULT ')), None)
            if proc.returncode != 0 or line is None:          # nothing more is started on the GPU after a failure
                sys.stdout.write(proc.stdout)
                raise SystemExit(f'{config}: exit status {proc.returncode}; stopping')
            results.append(json.loads(line[len('RESULT '):]))
            print(json.dumps(results[-1]), flush=True)
            if args.json:
                with open(args.json, 'a') as f:
                    f.write(json.dumps(results[-1]) + '\n')
        base = results[0]['images_per_s']
        print(f'\n{"configuration":<18}{"images/s":>10}{"x (a)":>8}{"upload MB/img":>15}{"host read ms":>14}{"convert ms":>12}')
        for r in results:
            conv = f'{r["convert_ms_per_image"]:.3f}' if r['convert_ms_per_image'] is not None else '-'
            print(f'{r["config"]:<18}{r["images_per_s"]:>10.1f}{r["images_per_s"] / base:>8.2f}{r["uploaded_bytes_per_image"] / 1e6:>15.1f}'
                  f'{r["host_read_ms_per_image"]:>14.1f}{conv:>12}')
        if len({(r['detections_checksum'], r['detections_min']) for r in results}) != 1:
            raise SystemExit('the configurations disagree on the detections: the inputs are not the same bits')
    finally:
        if not args.dir:
            shutil.rmtree(directory, ignore_errors=True)


if __name__ == '__main__':
    main()
