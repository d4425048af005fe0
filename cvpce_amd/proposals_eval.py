"""Detector-only evaluation harness -- counterpart of /root/reference/cvpce/proposals_eval.py:9-91
(`load_gln`, `evaluate_gln_sync`, `evaluate_gln_async`, `evaluate_gln`; the multiprocess variant only changes where the
CPU metric code runs).  The per-image triple handed to the metric routine is the reference's: (target boxes, predicted boxes,
scores).  By default the matching runs on the host as in the reference, in-process or in worker processes; with
`device_metrics=True` it runs on the device instead (device_metrics.DetectionMetrics: one kernel launch per batch queued behind
the detector, no per-image copy to the host, no worker processes, one device-to-host copy when the data set is exhausted) and
gives the same result wherever an image's confidences are pairwise distinct (equal confidences: see device_metrics).  `dataset` is any of the readers in datautils.py, or any iterable of `(image (3,H,W) f32 in [0,1] or (H,W,3) uint8,
target dict with 'boxes' (T,4))`.  num_workers > 0 reads it through `feeding.ImageFeeder` with that many threads (the reference's
DataLoader workers); 0, the default, reads it in the calling thread.

`gaussian_score` (a `device_gaussians.GaussianScore`, default None = exactly the code without it) also scores every batch's Gaussian
maps against targets rendered from the ground-truth boxes, on the device behind the detector with no host wait; its `compute()` is
returned under the extra key 'gaussians' of the result dict.

`head_score` (a `device_headloss.HeadScore`, default None = exactly the code without it) does the same for the other two losses of the
reference's compute_loss: the model keeps every pass's head outputs (`keep_head_outputs`), each batch's anchors are matched to its
ground-truth boxes and the focal and L1 losses summed on the device, and `compute()` is returned under 'head_losses'."""
import torch

from . import feeding, metrics, utils
from .datautils import image_hw
from .models import proposals


def load_gln(save_file, trim_module_prefix, **kwargs):
    """proposals_eval.py:9-17 (checkpoint dict key `model_state_dict`, optional DDP `module.` prefix)."""
    state_dict = torch.load(save_file, map_location='cpu')['model_state_dict']
    if trim_module_prefix:
        state_dict = utils.trim_module_prefix(state_dict)
    model = proposals.gln(pretrained_backbone=False, **kwargs)
    model.load_state_dict(state_dict)
    return model.cuda().eval()


def _score_gaussians(gaussian_score, result, batch):
    gaussian_score.update(result, [t['boxes'] for _, t in batch], [image_hw(img) for img, _ in batch])


def _with_gaussians(res, gaussian_score, head_score=None):
    if gaussian_score is not None:
        res['gaussians'] = gaussian_score.compute()
    if head_score is not None:
        res['head_losses'] = head_score.compute()
    return res


def _score_heads(head_score, model, batch):
    head_score.update(model.head_outputs(), [t for _, t in batch], [image_hw(img) for img, _ in batch])


class _kept_heads:
    """The model keeps its head outputs while a `head_score` is attached; None: nothing changes."""

    def __init__(self, model, head_score):
        self.model, self.on = model, head_score is not None

    def __enter__(self):
        if self.on:
            self.before = self.model._keep_head_outputs
            self.model.keep_head_outputs(True)

    def __exit__(self, *exc):
        if self.on:
            self.model.keep_head_outputs(self.before)


def _batches(dataset, batch_size):
    batch = []
    for item in dataset:
        batch.append(item)
        if len(batch) == batch_size:
            yield batch
            batch = []
    if batch:
        yield batch


@torch.no_grad()
def evaluate_gln_sync(model, dataset, thresholds=(.5,), batch_size=1, num_workers=0, plots=False, silent=True,
                      plot_res_reduction=1, device_metrics=False, gaussian_score=None, head_score=None):
    if device_metrics:
        return _evaluate_gln_device(model, dataset, thresholds, batch_size, num_workers, silent, gaussian_score, head_score)
    predictions, targets, confidences = [], [], []
    with _kept_heads(model, head_score):
        for i, batch in enumerate(_batches(feeding.feed(dataset, num_workers), batch_size)):
            if not silent and i % 100 == 0:
                print(f'{i}...')
            result = model([img.cuda(non_blocking=True) for img, _ in batch])
            if gaussian_score is not None:
                _score_gaussians(gaussian_score, result, batch)
            if head_score is not None:
                _score_heads(head_score, model, batch)
            for r, (_, t) in zip(result, batch):
                predictions.append(r['boxes'].detach().cpu())
                targets.append(t['boxes'].detach().cpu())
                confidences.append(r['scores'].detach().cpu())
    res = metrics.calculate_metrics(targets, predictions, confidences, thresholds)
    return _with_gaussians({thr: {k: v for k, v in itm.items() if k != 'raw'} for thr, itm in res.items()}, gaussian_score, head_score)


def _evaluate_gln_device(model, dataset, thresholds, batch_size, num_workers, silent, gaussian_score=None, head_score=None):
    from . import device_metrics
    accumulator = device_metrics.DetectionMetrics(thresholds)
    with _kept_heads(model, head_score):
        for i, batch in enumerate(_batches(feeding.feed(dataset, num_workers), batch_size)):
            if not silent and i % 100 == 0:
                print(f'{i}...')
            result = model([img.cuda(non_blocking=True) for img, _ in batch])
            accumulator.update([t['boxes'] for _, t in batch], [r['boxes'] for r in result], [r['scores'] for r in result])
            if gaussian_score is not None:
                _score_gaussians(gaussian_score, result, batch)
            if head_score is not None:
                _score_heads(head_score, model, batch)
    res = accumulator.compute()
    return _with_gaussians({thr: {k: v for k, v in itm.items() if k != 'raw'} for thr, itm in res.items()}, gaussian_score, head_score)


@torch.no_grad()
def evaluate_gln_async(model, dataset, thresholds=(.5,), batch_size=1, num_workers=0, num_metric_processes=4, plots=False,
                       plot_res_reduction=1, silent=True, device_metrics=False, gaussian_score=None, head_score=None):
    """proposals_eval.py:50-87: detections are handed to `num_metric_processes` matching workers as they are produced.
    device_metrics=True: no workers are started, the matching is queued on the device behind each batch."""
    if device_metrics:
        return _evaluate_gln_device(model, dataset, thresholds, batch_size, num_workers, silent, gaussian_score, head_score)
    # (the metric processes are started BEFORE the feeder's reader threads exist: a process forked beside running threads can deadlock)
    queue, mqueue, pipe = metrics.calculate_metrics_async(processes=num_metric_processes, iou_thresholds=thresholds)
    with _kept_heads(model, head_score):
        for i, batch in enumerate(_batches(feeding.feed(dataset, num_workers), batch_size)):
            if not silent and i % 100 == 0:
                print(f'GPU: {i}...')
            result = model([img.cuda(non_blocking=True) for img, _ in batch])
            if gaussian_score is not None:
                _score_gaussians(gaussian_score, result, batch)
            if head_score is not None:
                _score_heads(head_score, model, batch)
            for r, (_, t) in zip(result, batch):
                queue.put((t['boxes'], r['boxes'], r['scores']))
    queue.join()
    for _ in range(num_metric_processes):
        queue.put(None)
    queue.join()
    mqueue.join()
    mqueue.put(None)
    res = pipe.recv()
    mqueue.join()
    if res is None:                               # empty dataset: what the synchronous routine returns
        res = metrics.calculate_metrics([], [], [], thresholds)
    return _with_gaussians({thr: {k: v for k, v in itm.items() if k != 'raw'} for thr, itm in res.items()}, gaussian_score, head_score)


def evaluate_gln(save_file, dataset, thresholds=(.5,), batch_size=1, num_workers=0, num_metric_processes=4, plots=False,
                 trim_module_prefix=True, resolution_reduction=1, device_metrics=False, gaussian_score=None, head_score=None):
    """proposals_eval.py:89-91.  num_metric_processes = 0 runs the matching in-process (evaluate_gln_sync); device_metrics=True
    runs it on the device and ignores num_metric_processes.  gaussian_score: a `device_gaussians.GaussianScore`, or a callable
    that makes one from the loaded model (the model does not exist before this call); head_score: a `device_headloss.HeadScore`, or
    such a callable."""
    model = load_gln(save_file, trim_module_prefix)
    if gaussian_score is not None and not hasattr(gaussian_score, 'update'):
        gaussian_score = gaussian_score(model)
    if head_score is not None and not hasattr(head_score, 'update'):
        head_score = head_score(model)
    if device_metrics:
        return evaluate_gln_sync(model, dataset, thresholds, batch_size, num_workers, device_metrics=True, gaussian_score=gaussian_score,
                                 head_score=head_score)
    if num_metric_processes and num_metric_processes > 0:
        return evaluate_gln_async(model, dataset, thresholds, batch_size, num_workers, num_metric_processes, gaussian_score=gaussian_score,
                                  head_score=head_score)
    return evaluate_gln_sync(model, dataset, thresholds, batch_size, num_workers, gaussian_score=gaussian_score, head_score=head_score)
