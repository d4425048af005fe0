"""Measure the head-loss scoring in one process: 8 images of 960 x 1600 originals -- the detector's default geometry, a
padded batch of 800 x 1344 and about 200 000 anchors per image -- at 150 and at 700 boxes each.

  headloss_ms       device time of the op's stream operations (a memset and the three launches), timed with ops' launch timer
                    (`ops._start` into a ConvProfile: HIP events around every call), mean of --launches after a warm-up
  torch_ms          the same computation with torch device ops, image by image: the (boxes x anchors) IoU matrix, its maxima, the
                    equality of the low-quality rule, masked focal and L1 sums -- host clock around a synchronise, median of 3
  images/s          evaluate_gln_sync over --eval-images such images (default 512: 16 distinct ones in rotation, a window of more
                    than half a second) in batches of 8, with and without a HeadScore, alternating, --eval-repeats times each after a
                    warm-up of both: median, and the smallest and largest as the spread
  launches, waits   stream operations and host waits one HeadScore.update adds (torch.profiler, a run of its own), and the host time
                    of update() behind a device queue that is kept busy: an update that waited for the device would take as long as
                    the backlog
Conditions (exit status 1 otherwise): a scored batch adds no host wait, and the same number of stream operations at 150 and 700 boxes.

    python tools/bench_head_losses.py [--launches 30] [--markdown profiles/r31_head_losses.md]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, H0, W0 = 8, 960, 1600


def targets_for(seed, count):
    rng = np.random.RandomState(seed)
    x1, y1 = rng.randint(0, W0 - 130, count), rng.randint(0, H0 - 170, count)
    w, h = rng.randint(40, 130, count), rng.randint(50, 170, count)
    boxes = torch.from_numpy(np.stack([x1, y1, x1 + w, y1 + h], 1).astype(np.int64))
    return {'boxes': boxes, 'labels': torch.zeros(count, dtype=torch.long)}


def wall_ms(fn, repeats=3):
    """median host time of `repeats` runs after one warm-up run; repeats = 0: ONE run, no warm-up (the caller has warmed up)"""
    times = []
    for _ in range(repeats + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(times[1:]) if repeats else times[0]


def timed_ms(launch, launches, nbytes):
    """mean device time of `launch` by ops' launch timer"""
    from cvpce_amd import ops
    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    ops.PROFILE = prof = ops.ConvProfile()
    try:
        for _ in range(launches):
            t = ops._start()
            launch()
            t.stop()
            t.file('headloss', nbytes=nbytes, hbm=True)
        rec = prof.summary_bytes()['headloss']
    finally:
        ops.PROFILE = None
    return rec['ms'] / rec['launches']


def grid_anchors(base_anchors, grids, strides):
    """(A_total,4) on the device: shift + base, the order of the head outputs"""
    out = []
    for base, (gh, gw), (sh, sw) in zip(base_anchors, grids, strides):
        sx = torch.arange(gw, dtype=torch.float32, device=base.device) * sw
        sy = torch.arange(gh, dtype=torch.float32, device=base.device) * sh
        yy, xx = torch.meshgrid(sy, sx, indexing='ij')
        shifts = torch.stack((xx, yy, xx, yy), dim=2).reshape(-1, 1, 4)
        out.append((shifts + base[None]).reshape(-1, 4))
    return torch.cat(out)


def torch_head_losses(anchors, logits, regs, boxes, labels):
    """torchvision 0.9's RetinaNet losses of one image with torch device ops -> (classification, bbox_regression, matched)"""
    area_a = (anchors[:, 2] - anchors[:, 0]) * (anchors[:, 3] - anchors[:, 1])
    area_b = (boxes[:, 2] - boxes[:, 0]) * (boxes[:, 3] - boxes[:, 1])
    lt, rb = torch.max(boxes[:, None, :2], anchors[:, :2]), torch.min(boxes[:, None, 2:], anchors[:, 2:])
    inter = (rb - lt).clamp(min=0).prod(dim=2)
    iou = inter / (area_b[:, None] + area_a - inter)                                 # (T, A): the matrix
    val, arg = iou.max(dim=0)
    m = torch.where(val >= 0.5, arg, torch.where(val >= 0.4, torch.full_like(arg, -2), torch.full_like(arg, -1)))
    low = (iou == iou.max(dim=1).values[:, None]).any(dim=0)
    m = torch.where(low, arg, m)
    fg = m >= 0
    nfg = fg.sum().clamp(min=1)
    t = torch.zeros_like(logits)
    t[fg, labels[m[fg]]] = 1
    p = torch.sigmoid(logits)
    ce = torch.nn.functional.binary_cross_entropy_with_logits(logits, t, reduction='none')
    p_t = p * t + (1 - p) * (1 - t)
    loss = (0.25 * t + 0.75 * (1 - t)) * ce * (1 - p_t) ** 2
    cls = loss[m != -2].sum() / nfg
    a, g = anchors[fg], boxes[m[fg]]
    w, h, gw, gh = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
    enc = torch.stack([(g[:, 0] + 0.5 * gw - (a[:, 0] + 0.5 * w)) / w, (g[:, 1] + 0.5 * gh - (a[:, 1] + 0.5 * h)) / h,
                       torch.log(gw / w), torch.log(gh / h)], dim=1)
    return cls, (regs[fg] - enc).abs().sum() / nfg, m


def profile_update(score, heads, targets, sizes):
    """-> (stream operations, host waits) of one update, by name, or None where the profiler gives no device events"""
    from torch.profiler import ProfilerActivity, profile, record_function
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        with record_function('head_score_update'):
            score.update(heads, targets, sizes)
        torch.cuda.synchronize()                                 # (closes the window; like the profiler's own, outside the marker)
    events = list(prof.events())
    marker = next(e for e in events if e.name == 'head_score_update' and not str(e.device_type).endswith('CUDA'))
    device_ops, waits = [], []
    for e in events:
        name = e.name
        if str(e.device_type).endswith('CUDA'):
            if name != 'head_score_update':
                device_ops.append(name)
        elif ('Synchronize' in name or 'hipMemcpyDtoH' in name or name in ('aten::item', 'aten::_local_scalar_dense')) \
                and marker.time_range.start <= e.time_range.start <= marker.time_range.end:
            waits.append(name)                                   # a host wait inside update()
    return (device_ops, waits) if device_ops else None


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--launches', type=int, default=30)
    ap.add_argument('--eval-images', type=int, default=512, help='images per timed evaluate_gln_sync window')
    ap.add_argument('--eval-repeats', type=int, default=5)
    ap.add_argument('--markdown', help='also write the tables to this file')
    args = ap.parse_args()
    from cvpce_amd import device_headloss as dh, proposals_eval, synthetic, torch_ops_headloss as H
    device = torch.device('cuda:0')
    model = synthetic.synthetic_gln(seed=0, detections_per_img=300).to(device)
    images = [synthetic.shelf_image(60 + k, H0, W0) for k in range(2 * N)]
    sizes = [(H0, W0)] * N
    model.keep_head_outputs(True)
    model([i.to(device) for i in images[:N]])
    heads = model.head_outputs()
    model.keep_head_outputs(False)
    eng = model.engine()
    cls, reg, padded = heads['cls'], heads['reg'], heads['padded']
    grids = [(c.shape[1], c.shape[2]) for c in cls]
    strides = [(padded[0] // g[0], padded[1] // g[1]) for g in grids]
    k, a = model.num_classes, eng.num_anchors
    total = a * sum(gh * gw for gh, gw in grids)
    scales = dh.scale_factors(heads['sizes'], sizes)
    anchors = grid_anchors(eng.base_anchors, grids, strides)
    logits = torch.cat([c.reshape(N, -1, k) for c in cls], dim=1)
    regs = torch.cat([r.reshape(N, -1, 4) for r in reg], dim=1)
    rows, ok, counts = [], True, {}
    for count in (150, 700):
        targets = [targets_for(100 * count + i, count) for i in range(2 * N)]
        packed = torch.cat([t['boxes'] for t in targets[:N]]).to(torch.float32).to(device)
        labels = torch.cat([t['labels'] for t in targets[:N]]).to(torch.int32).to(device)
        offsets = torch.tensor([count * i for i in range(N + 1)], dtype=torch.int32, device=device)
        sc = scales.to(device)
        workspace = torch.empty(H.workspace_bytes([g[0] for g in grids], [g[1] for g in grids], a, N, N * count), dtype=torch.uint8, device=device)
        matched = torch.empty((N, total), dtype=torch.int32, device=device)
        out_f, out_i = torch.empty((N, 2), device=device), torch.empty((N, 3), dtype=torch.int32, device=device)
        launch = lambda: torch.ops.cvpce_amd.headloss(cls, reg, [g[0] for g in grids], [g[1] for g in grids], [s[0] for s in strides],
                                                      [s[1] for s in strides], eng.base_anchors, packed, labels, offsets, sc, a, k,
                                                      workspace, matched, out_f, out_i)
        # bytes the algorithm needs: the head outputs and the matching read once, `matched` written once, the boxes once per image
        nbytes = logits.numel() * 4 + regs.numel() * 4 + matched.numel() * 4 + packed.numel() * 4
        row = {'boxes_per_image': count, 'images': N, 'padded': list(padded), 'anchors_per_image': total,
               'headloss_ms': timed_ms(launch, args.launches, nbytes)}
        row['anchor_box_pairs_per_s'] = 2 * N * total * count / (row['headloss_ms'] * 1e-3)      # (both walks)
        row['counts_first_image'] = out_i[0].tolist()
        scaled = [packed[count * i:count * (i + 1)] * torch.stack([sc[i, 1], sc[i, 0], sc[i, 1], sc[i, 0]]) for i in range(N)]
        per_image = lambda: [torch_head_losses(anchors, logits[i], regs[i], scaled[i], labels[count * i:count * (i + 1)].long()) for i in range(N)]
        row['torch_ms'] = wall_ms(per_image)
        theirs = per_image()
        tf = torch.stack([torch.stack(t[:2]) for t in theirs])
        row['max_relative_loss_difference_from_torch'] = float(((out_f - tf).abs() / tf.abs()).max())
        row['anchors_matched_otherwise_than_torch'] = int(sum((t[2] != matched[i]).sum() for i, t in enumerate(theirs)))
        del theirs, tf
        # the harness, with and without a score
        pairs = list(zip(images, targets))
        data = [pairs[i % len(pairs)] for i in range(args.eval_images)]
        plain = lambda: proposals_eval.evaluate_gln_sync(model, data, batch_size=N, device_metrics=True)
        scored = lambda: proposals_eval.evaluate_gln_sync(model, data, batch_size=N, device_metrics=True, head_score=dh.HeadScore(model))
        plain(), scored()                                         # warm-up: both graphs are captured
        tp, ts = [], []
        for _ in range(args.eval_repeats):
            tp.append(wall_ms(plain, 0))
            ts.append(wall_ms(scored, 0))
        rate = lambda ms: 1e3 * len(data) / ms
        row['eval_window_ms'] = statistics.median(tp)
        row['eval_images_per_s'], row['eval_images_per_s_range'] = rate(statistics.median(tp)), [rate(max(tp)), rate(min(tp))]
        row['eval_scored_images_per_s'], row['eval_scored_images_per_s_range'] = rate(statistics.median(ts)), [rate(max(ts)), rate(min(ts))]
        row['eval_scored_share'] = statistics.median(tp) / statistics.median(ts)
        # host time of update() behind a busy queue
        busy = torch.randn(8192, 8192, device=device)
        score = dh.HeadScore(model)
        score.update(heads, targets[:N], sizes)
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(40):
            busy @ busy
        e1.record()
        t0 = time.perf_counter()
        score.update(heads, targets[:N], sizes)
        row['update_host_ms_behind_backlog'] = 1e3 * (time.perf_counter() - t0)
        e1.synchronize()
        row['backlog_ms'] = e0.elapsed_time(e1)
        row['update_waits_for_the_device'] = row['update_host_ms_behind_backlog'] > 0.5 * row['backlog_ms']
        ok = ok and not row['update_waits_for_the_device']
        try:
            prof = profile_update(dh.HeadScore(model), heads, targets[:N], sizes)
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
    print(json.dumps({'launches_per_batch_by_construction': dh.LAUNCHES_PER_BATCH, 'uploads_per_batch': dh.UPLOADS_PER_BATCH,
                      'host_waits_per_batch': dh.HOST_WAITS_PER_BATCH, 'conditions_hold': ok}))
    if args.markdown:
        with open(args.markdown, 'w') as f:
            f.write('# Head-loss scoring: anchor matching, focal and L1 losses on the GPU\n\n')
            f.write(f'`python tools/bench_head_losses.py --launches {args.launches} --markdown ...`, one process on one MI355X; {N} images of '
                    f'{H0} x {W0} originals, padded batch {list(padded)}, {total} anchors per image, {k} class.\n\n')
            cols = ['headloss_ms', 'torch_ms', 'anchor_box_pairs_per_s']
            f.write('| boxes per image | ' + ' | '.join(cols) + ' | eval_images_per_s (smallest .. largest) | eval_scored_images_per_s '
                    '(smallest .. largest) | share kept |\n|---|' + '---|' * (len(cols) + 3) + '\n')
            span = lambda r, c: f"{r[c]:.4g} ({r[c + '_range'][0]:.4g} .. {r[c + '_range'][1]:.4g})"
            for r in rows:
                f.write(f"| {r['boxes_per_image']} | " + ' | '.join(f'{r[c]:.4g}' for c in cols) + f" | {span(r, 'eval_images_per_s')} | "
                        f"{span(r, 'eval_scored_images_per_s')} | {100 * r['eval_scored_share']:.1f} % |\n")
            f.write('\nheadloss_ms: the memset and the three launches of the whole batch, HIP events around each call (ops\' launch timer), '
                    'mean.  torch_ms: the same computation with torch device ops, image by image (IoU matrix, maxima, equality, masked '
                    'sums), host clock around a synchronise.  anchor_box_pairs_per_s: IoU evaluations, both walks counted, over headloss_ms.  '
                    f'images/s: evaluate_gln_sync(device_metrics=True) over {args.eval_images} images (16 distinct ones in rotation) in batches '
                    f'of 8, a window of about {rows[0]["eval_window_ms"]:.0f} ms, without and with a HeadScore, alternating, median of '
                    f'{args.eval_repeats} with the smallest and largest.\n\n')
            f.write('| boxes per image | stream operations added per batch | host waits added per batch | update() host ms behind a backlog of (ms) | '
                    'largest relative loss difference from torch | anchors matched otherwise than torch | foreground, between, restored (image 0) |\n'
                    '|---|---|---|---|---|---|---|\n')
            for r in rows:
                f.write(f"| {r['boxes_per_image']} | {r.get('stream_operations', 'not measured')} | {r.get('host_waits', 'not measured')} | "
                        f"{r['update_host_ms_behind_backlog']:.3g} ({r['backlog_ms']:.4g}) | {r['max_relative_loss_difference_from_torch']:.3g} | "
                        f"{r['anchors_matched_otherwise_than_torch']} | {r['counts_first_image']} |\n")
            f.write(f'\nBy construction a scored batch queues {dh.LAUNCHES_PER_BATCH} launches (a memset, headloss_match, headloss_terms, '
                    f'headloss_finish, the cat of the result row) and {dh.UPLOADS_PER_BATCH} pinned asynchronous uploads (boxes, labels, offsets, '
                    f'scale factors), whatever the number of boxes or anchors, and {dh.HOST_WAITS_PER_BATCH} host waits; the profiler counts '
                    f'launches and copies together.  Conditions hold: {ok}.\n')
            if rows and 'stream_operation_names' in rows[-1]:
                f.write('\nDevice operations seen by the profiler: ' + ', '.join(f'`{n}`' for n in rows[-1]['stream_operation_names']) + '\n')
    return 0 if ok else 1


if __name__ == '__main__':
    sys.exit(main())
