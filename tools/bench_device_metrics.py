"""Time the detection matching per image: host routine, host worker processes, device path, kernel alone.

64 synthetic dense scenes (synthetic.dense_detection_scene: 1 000 predictions, about 150 targets each), at one IoU threshold and
at the ten COCO thresholds:
  cpu_1thread     metrics.calculate_metrics, torch limited to one thread
  async_4workers  metrics.calculate_metrics_async with 4 worker processes, from the first `put` to the result; the steady-state
                  figure is the difference between a 128- and a 64-image run (it leaves out starting the processes)
  device_e2e      DetectionMetrics: update() in batches of 8 device-resident images, then compute() (its device-to-host copy and
                  the host merge included), wall clock after a warm-up run
  device_update   the same without compute(): what the evaluation loop pays per image while the detector runs
  kernel          the one launch that matches all 64 images, HIP events, median of --launches after warm-up
The condition to hold: device_e2e is not slower than cpu_1thread at either threshold count (exit status 1 otherwise).

    python tools/bench_device_metrics.py [--images 64] [--launches 30] [--markdown profiles/r10_device_metrics.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cvpce_amd import metrics                                 # noqa: E402  (host-only: the worker processes re-import this file)


def time_cpu(scenes, thresholds):
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        t0 = time.perf_counter()
        metrics.calculate_metrics(*scenes, thresholds)
        return time.perf_counter() - t0
    finally:
        torch.set_num_threads(threads)


def time_async(scenes, thresholds, repeat, workers=4):
    queue, mqueue, pipe = metrics.calculate_metrics_async(processes=workers, iou_thresholds=thresholds)
    t0 = time.perf_counter()
    for _ in range(repeat):
        for t, p, c in zip(*scenes):
            queue.put((t, p, c))
    queue.join()
    for _ in range(workers):
        queue.put(None)
    queue.join()
    mqueue.join()
    mqueue.put(None)
    pipe.recv()
    mqueue.join()
    return time.perf_counter() - t0


def time_device(scenes, thresholds, device, batch=8, rounds=5):
    from cvpce_amd import device_metrics
    dev = [[x.to(device) for x in col] for col in scenes]
    n = len(dev[0])
    e2e, upd = [], []
    for r in range(rounds + 1):                                 # (round 0 is the warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        acc = device_metrics.DetectionMetrics(thresholds)
        for b in range(0, n, batch):
            acc.update(dev[0][b:b + batch], dev[1][b:b + batch], dev[2][b:b + batch])
        t1 = time.perf_counter()
        acc.compute()
        t2 = time.perf_counter()
        if r:
            e2e.append(t2 - t0)
            upd.append(t1 - t0)
    return statistics.median(e2e), statistics.median(upd)


def time_kernel(scenes, thresholds, device, launches):
    from cvpce_amd import device_metrics, staging
    thr = torch.tensor([float(t) for t in thresholds], dtype=torch.float32, device=device)
    dev = [[x.to(device) for x in col] for col in scenes]
    m = device_metrics._match_packed(dev[0], dev[1], dev[2], thr)
    pred, tgt = torch.cat(dev[1]), torch.cat(dev[0])
    poff = torch.tensor(staging.offsets(m['n_pred']), dtype=torch.int32, device=device)
    toff = torch.tensor(staging.offsets(m['n_tgt']), dtype=torch.int32, device=device)
    first, tp = torch.empty_like(m['first']), torch.zeros_like(m['tp'])
    launch = lambda: torch.ops.cvpce_amd.eval_match_detections(pred, poff, m['rank'], None, tgt, toff, None, thr, max(m['n_tgt']), first, tp)
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    assert torch.equal(tp, m['tp']) and torch.equal(first, m['first'])
    times = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        launch()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b) * 1e-3)
    return statistics.median(times)


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--markdown', help='also write the table to this file')
    args = ap.parse_args()
    assert args.launches >= 20
    from cvpce_amd import synthetic
    device = torch.device('cuda:0')
    seeds, s = [], 1000
    while len(seeds) < args.images:                             # scenes with pairwise distinct confidences only
        if len(synthetic.dense_detection_scene(s)[2].unique()) == 1000:
            seeds.append(s)
        s += 1
    scenes = [list(col) for col in zip(*[synthetic.dense_detection_scene(s) for s in seeds])]
    n = args.images
    rows, ok = [], True
    for name, thresholds in (('1 threshold', (0.5,)), ('10 thresholds', tuple(f.item() for f in torch.linspace(.5, .95, 10)))):
        cpu = time_cpu(scenes, thresholds)
        a1, a2 = time_async(scenes, thresholds, 1), time_async(scenes, thresholds, 2)
        e2e, upd = time_device(scenes, thresholds, device)
        kern = time_kernel(scenes, thresholds, device, args.launches)
        row = {'thresholds': name, 'images': n, 'cpu_1thread_ms': 1e3 * cpu / n, 'async_4workers_ms': 1e3 * a1 / n,
               'async_4workers_steady_ms': 1e3 * (a2 - a1) / n, 'device_e2e_ms': 1e3 * e2e / n, 'device_update_ms': 1e3 * upd / n,
               'kernel_ms': 1e3 * kern / n, 'kernel_launch_ms': 1e3 * kern}
        row['device_not_slower_than_cpu'] = row['device_e2e_ms'] <= row['cpu_1thread_ms']
        ok = ok and row['device_not_slower_than_cpu']
        rows.append(row)
        print(json.dumps(row), flush=True)
    if args.markdown:
        cols = ['cpu_1thread_ms', 'async_4workers_ms', 'async_4workers_steady_ms', 'device_e2e_ms', 'device_update_ms', 'kernel_ms']
        with open(args.markdown, 'w') as f:
            f.write(f'| per image, ms ({n} images) | ' + ' | '.join(c[:-3] for c in cols) + ' |\n|---|' + '---|' * len(cols) + '\n')
            for row in rows:
                f.write(f"| {row['thresholds']} | " + ' | '.join(f'{row[c]:.4g}' for c in cols) + ' |\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
