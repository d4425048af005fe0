"""Measure the Gaussian-map scoring in one process: 8 images of 2048 x 2048 originals, at 150 and at 700 boxes each.

  targets_ms        device time (HIP events, median of --launches) of the one launch that renders and resizes the batch's targets
  loss_ms           device time of the loss's stream operations (a memset and six launches), per-image scope
  torch_targets_ms  the same targets with torch device ops: the reference's per-box loop moved onto the device (one full-resolution
                    map per image), then F.interpolate -- host clock around a synchronise, median of 3
  torch_loss_ms     the reference's loss with torch device ops (masks, argsort), per image
  images/s          evaluate_gln_sync over 16 such images in batches of 8, with and without a GaussianScore, alternating, median of 3
  launches, waits   stream operations and host waits one GaussianScore.update adds (torch.profiler, a run of its own), and the host
                    time of update() behind a device queue that is kept busy: an update that waited for the device would take as long
                    as the backlog
Conditions (exit status 1 otherwise): a scored batch adds no host wait, and the same number of stream operations at 150 and 700 boxes.
T_ref, the host model's distance from the reference over the golden vectors, is measured on the host and written alongside.

    python tools/bench_gaussian_scoring.py [--launches 30] [--markdown profiles/r30_gaussian_scoring.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
import torch.nn.functional as nnf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

N, SIDE = 8, 2048


def boxes_for(seed, count):
    rng = np.random.RandomState(seed)
    x1, y1 = rng.randint(-20, SIDE - 40, count), rng.randint(-20, SIDE - 40, count)
    w, h = rng.randint(30, 160, count), rng.randint(40, 220, count)
    return torch.from_numpy(np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.int64))


def t_ref():
    import gaussian_cases as gc
    golden = torch.load(os.path.join(ROOT, 'tests', 'golden', 'gaussian_targets.pt'), weights_only=False)
    worst = 0.0
    for c in golden['targets'].values():
        got, _ = gc.render(c['w'], c['h'], c['boxes'], c['size_reduction'], c['method'], None, c['join'], c['tanh'])
        want = c['expected'].numpy()
        d = np.abs(got - want)
        worst = max(worst, float((d / np.maximum(1, np.abs(want)) if c['join'] == 'addition' else d).max()))
    return worst


def event_ms(fn, launches):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(launches):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return statistics.median(times)


def wall_ms(fn, repeats=3):
    times = []
    for _ in range(repeats + 1):                                 # (the first run is the warm-up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times[1:])


def torch_targets(boxes, out_hw, device):
    """The reference's generate_gaussians (multivariate_normal in its closed form, join_via_max) with torch ops on the device."""
    maps = []
    for bs in boxes:
        img = torch.zeros((SIDE, SIDE), device=device)
        for x1, y1, x2, y2 in bs.tolist():
            cx, cy, vw, vh = (x1 + x2) / 2, (y1 + y2) / 2, ((x2 - x1) / 2) ** 2, ((y2 - y1) / 2) ** 2
            xs = torch.arange(max(x1, 0), min(x2, SIDE), dtype=torch.float32, device=device)
            ys = torch.arange(max(y1, 0), min(y2, SIDE), dtype=torch.float32, device=device)
            ex, ey = (xs - cx) ** 2 / vw, (ys - cy) ** 2 / vh
            probs = torch.exp(-0.5 * ((ey - ey.min())[:, None] + (ex - ex.min())[None, :]))
            region = img[max(y1, 0):min(y2, SIDE), max(x1, 0):min(x2, SIDE)]
            region.copy_(torch.max(region, probs))
        maps.append(nnf.interpolate(img[None, None], size=out_hw, mode='bilinear', align_corners=False)[0])
    return torch.stack(maps)


def torch_loss(pred, target):
    """proposals.py:141-160 per image with torch ops on the device"""
    out = []
    for p, t in zip(pred, target):
        se = (p - t) ** 2
        pos, neg = se[t >= 0.1], se[t <= 0.0]
        top = neg[neg.argsort(descending=True)[:max(1000, 3 * len(pos))]]
        out.append((pos.sum() + top.sum()) / (len(pos) + len(top)))
    return torch.stack(out)


def profile_update(score, results, boxes, sizes):
    """-> (stream operations, host waits) of one update, by name, or None where the profiler gives no device events"""
    from torch.profiler import ProfilerActivity, profile, record_function
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with record_function('gaussian_score_update'):
            score.update(results, boxes, sizes)
        torch.cuda.synchronize()                                 # (closes the window; like the profiler's own, outside the marker)
    events = list(prof.events())
    marker = next(e for e in events if e.name == 'gaussian_score_update' and not str(e.device_type).endswith('CUDA'))
    device_ops, waits = [], []
    for e in events:
        name = e.name
        if str(e.device_type).endswith('CUDA'):
            if name != 'gaussian_score_update':
                device_ops.append(name)
        elif ('Synchronize' in name or 'hipMemcpyDtoH' in name or name in ('aten::item', 'aten::_local_scalar_dense')) \
                and marker.time_range.start <= e.time_range.start <= marker.time_range.end:
            waits.append(name)                                   # a host wait inside update()
    return (device_ops, waits) if device_ops else None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--markdown', help='also write the tables to this file')
    args = ap.parse_args()
    from cvpce_amd import device_gaussians as dg, proposals_eval, synthetic
    device = torch.device('cuda:0')
    model = synthetic.synthetic_gln(seed=0, detections_per_img=300).to(device)
    images = [synthetic.shelf_image(60 + k, SIDE, SIDE) for k in range(2 * N)]
    sizes = [(SIDE, SIDE)] * N
    results = model([i.to(device) for i in images[:N]])
    pred = torch.stack([r['gaussians'] for r in results])
    hb, wb = pred.shape[2:]
    (rh, rw), (ph, pw) = model.image_geometry(sizes[:1])[0]
    rows, ok, counts = [], True, {}
    for count in (150, 700):
        boxes = [boxes_for(100 * count + k, count) for k in range(2 * N)]
        geom = [(SIDE, SIDE, 1, rh // 2, rw // 2)] * N
        packed = torch.cat(boxes[:N]).to(torch.int32).to(device)
        offsets = torch.tensor([count * i for i in range(N + 1)], dtype=torch.int32, device=device)
        g = torch.tensor(geom, dtype=torch.int32, device=device)
        target = torch.empty((N, 1, hb, wb), device=device)
        launch = lambda: torch.ops.cvpce_amd.gauss_targets(packed, offsets, None, g, None, 0, 0, 1.0, 0.5, 0.0, 0, 1, target)
        row = {'boxes_per_image': count, 'images': N, 'target_shape': [N, 1, hb, wb], 'targets_ms': event_ms(launch, args.launches)}
        assert torch.equal(target, dg.render_boxes(boxes[:N], geom, hb, wb, device=device))
        ext = torch.tensor([[ph // 2, pw // 2]] * N, dtype=torch.int32, device=device)
        row['loss_ms'] = event_ms(lambda: dg.loss(pred, target, ext), args.launches)
        mine = dg.loss(pred, target, ext)[0][:, 0]
        row['torch_targets_ms'] = wall_ms(lambda: torch_targets(boxes[:N], (rh // 2, rw // 2), device))
        theirs_t = torch_targets(boxes[:N], (rh // 2, rw // 2), device)
        row['torch_loss_ms'] = wall_ms(lambda: torch_loss(pred[:, :, :rh // 2, :rw // 2], theirs_t))
        theirs = torch_loss(pred[:, :, :ph // 2, :pw // 2], nnf.pad(theirs_t, (0, pw // 2 - rw // 2, 0, ph // 2 - rh // 2)))
        row['max_target_difference_from_torch'] = float((target[:, :, :rh // 2, :rw // 2] - theirs_t).abs().max())
        row['max_relative_loss_difference_from_torch'] = float(((mine - theirs).abs() / theirs.abs()).max())
        # the harness, with and without a score
        data = [(img, {'boxes': b}) for img, b in zip(images, boxes)]
        plain = lambda: proposals_eval.evaluate_gln_sync(model, data, batch_size=N, device_metrics=True)
        scored = lambda: proposals_eval.evaluate_gln_sync(model, data, batch_size=N, device_metrics=True, gaussian_score=dg.GaussianScore(model))
        plain(), scored()
        tp, ts = [], []
        for _ in range(3):
            tp.append(wall_ms(plain, 1))
            ts.append(wall_ms(scored, 1))
        row['eval_images_per_s'] = 1e3 * len(data) / statistics.median(tp)
        row['eval_scored_images_per_s'] = 1e3 * len(data) / statistics.median(ts)
        # host time of update() behind a busy queue
        busy = torch.randn(8192, 8192, device=device)
        score = dg.GaussianScore(model)
        score.update(results, boxes[:N], sizes)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(40):
            busy @ busy
        b.record()
        t0 = time.perf_counter()
        score.update(results, boxes[:N], sizes)
        row['update_host_ms_behind_backlog'] = 1e3 * (time.perf_counter() - t0)
        b.synchronize()
        row['backlog_ms'] = a.elapsed_time(b)
        row['update_waits_for_the_device'] = row['update_host_ms_behind_backlog'] > 0.5 * row['backlog_ms']
        ok = ok and not row['update_waits_for_the_device']
        try:
            prof = profile_update(dg.GaussianScore(model), results, boxes[:N], sizes)
        except Exception as e:                                    # the counts are then the code's own, stated below
            prof = None
            row['profiler_error'] = repr(e)[:200]
        if prof is not None:
            row['stream_operations'], row['host_waits'] = len(prof[0]), len(prof[1])
            row['stream_operation_names'] = sorted(set(prof[0]))
            row['host_wait_names'] = sorted(set(prof[1]))
            counts[count] = (len(prof[0]), len(prof[1]))
            ok = ok and len(prof[1]) == 0
        rows.append(row)
        print(json.dumps(row), flush=True)
    if len(counts) == 2:
        ok = ok and counts[150][0] == counts[700][0]
    tref = t_ref()
    print(json.dumps({'T_ref': tref, 'launches_per_batch_by_construction': dg.LAUNCHES_PER_BATCH, 'host_waits_per_batch': dg.HOST_WAITS_PER_BATCH,
                      'conditions_hold': ok}))
    if args.markdown:
        with open(args.markdown, 'w') as f:
            f.write('# Gaussian-map scoring: targets and loss on the GPU\n\n')
            f.write(f'`python tools/bench_gaussian_scoring.py --launches {args.launches} --markdown ...`, one process on one MI355X; {N} images of '
                    f'{SIDE} x {SIDE} originals, target tensor {[N, 1, hb, wb]}.\n\n')
            f.write(f'T_ref (host model against the reference over tests/golden/gaussian_targets.pt, measured on the host; the kernel does not '
                    f'enter it): **{tref:.3e}**\n\n')
            cols = ['targets_ms', 'loss_ms', 'torch_targets_ms', 'torch_loss_ms', 'eval_images_per_s', 'eval_scored_images_per_s']
            f.write('| boxes per image | ' + ' | '.join(cols) + ' |\n|---|' + '---|' * len(cols) + '\n')
            for r in rows:
                f.write(f"| {r['boxes_per_image']} | " + ' | '.join(f'{r[c]:.4g}' for c in cols) + ' |\n')
            f.write('\ntargets_ms, loss_ms: HIP events, median.  torch_*: the same computation with torch device ops (per-box loop, '
                    'F.interpolate, masks, argsort), host clock around a synchronise.  images/s: evaluate_gln_sync(device_metrics=True), '
                    '16 images in batches of 8, without and with a GaussianScore.\n\n')
            f.write('| boxes per image | stream operations added per batch | host waits added per batch | update() host ms behind a backlog of (ms) | '
                    'largest target difference from torch | largest relative loss difference from torch |\n|---|---|---|---|---|---|\n')
            for r in rows:
                f.write(f"| {r['boxes_per_image']} | {r.get('stream_operations', 'not measured')} | {r.get('host_waits', 'not measured')} | "
                        f"{r['update_host_ms_behind_backlog']:.3g} ({r['backlog_ms']:.4g}) | {r['max_target_difference_from_torch']:.3g} | "
                        f"{r['max_relative_loss_difference_from_torch']:.3g} |\n")
            f.write(f'\nBy construction a scored batch queues {dg.LAUNCHES_PER_BATCH} launches (stack of the predictions, the targets launch, '
                    f'a memset and six loss launches) and {dg.UPLOADS_PER_BATCH} pinned asynchronous uploads (boxes, offsets, geometry, extents), '
                    f'whatever the number of boxes or pixels, and {dg.HOST_WAITS_PER_BATCH} host waits; the profiler counts launches and copies '
                    f'together (a pinned upload appears there as a host-to-device or a device-to-device copy).  Conditions hold: {ok}.\n')
            if rows and 'stream_operation_names' in rows[-1]:
                f.write('\nDevice operations seen by the profiler: ' + ', '.join(f'`{n}`' for n in rows[-1]['stream_operation_names']) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
