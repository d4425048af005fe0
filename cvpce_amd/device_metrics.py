"""Detection metrics with the per-image matching on the device -- the opt-in counterpart of `metrics.calculate_metrics`
(which stays host-only: the metric worker processes import it without the HIP library).

`metrics.check_matches` visits predictions in descending confidence and, having no `break`, lets a matched prediction use up
every free target at or above the threshold.  So a prediction is a true positive iff it is the FIRST prediction, in confidence
order, that covers some target -- per target a min over the covering predictions' ranks, which the kernel of
csrc/evalmatch.hip takes for a whole batch of images at all thresholds in one launch, with the IoU bits of `metrics.box_iou`.

Order at equal confidences.  The rank of a prediction is its position in a STABLE descending sort of its image's confidences:
equal confidences keep their input order.  (`metrics._process_one` sorts with torch's default, unstable sort: its order at ties
is unspecified, so the two paths are only comparable there after pre-ordering the CPU's input the same way.)

`DetectionMetrics.update` queues device work only; `compute` brings everything accumulated to the host in one copy and runs
the existing host routines (`metrics.precision_and_recall`, `metrics._do_calculate`) on the flags, so the merge, AP and
F-score are the host path's by construction.
"""
import torch

from . import metrics, torch_ops_eval  # noqa: F401  (registers torch.ops.cvpce_amd.eval_match_detections)
from . import staging

MAX_THRESHOLDS = 16


def _device_of(*lists):
    for lst in lists:
        for t in lst or ():
            if t.is_cuda:
                return t.device
    return torch.device('cuda', torch.cuda.current_device())


def _threshold_values(iou_thresholds):
    vals = [float(t) for t in iou_thresholds]
    if not 1 <= len(vals) <= MAX_THRESHOLDS:
        raise ValueError(f'between 1 and {MAX_THRESHOLDS} IoU thresholds, got {len(vals)}')
    return vals


def _match_packed(targets, predictions, confidences, thr, target_labels=None, prediction_labels=None):
    """-> dict of packed device tensors for one batch (`thr`: the thresholds as a float32 device tensor) plus the host-known
    per-image lengths.  Device work only."""
    if not len(targets) == len(predictions) == len(confidences):
        raise ValueError('targets, predictions and confidences must have one entry per image')
    if (target_labels is None) != (prediction_labels is None):
        raise ValueError('class-aware matching needs both target_labels and prediction_labels')
    device = thr.device
    n_pred = [int(c.numel()) for c in confidences]
    n_tgt = [int(t.numel()) // 4 for t in targets]
    for p, n in zip(predictions, n_pred):
        if p.numel() != 4 * n:
            raise ValueError('one confidence per predicted box')
    pred = staging.pack(predictions, torch.float32, device, (4,))
    conf = staging.pack(confidences, torch.float32, device)
    tgt = staging.pack(targets, torch.float32, device, (4,))
    pcls = tcls = None
    if target_labels is not None:
        if [int(l.numel()) for l in target_labels] != n_tgt or [int(l.numel()) for l in prediction_labels] != n_pred:
            raise ValueError('one class id per box')
        pcls = staging.pack(prediction_labels, torch.int32, device)
        tcls = staging.pack(target_labels, torch.int32, device)
    sum_p, sum_t, k = sum(n_pred), sum(n_tgt), thr.numel()
    poff = staging.upload_values(staging.offsets(n_pred), torch.int32, device)
    toff = staging.upload_values(staging.offsets(n_tgt), torch.int32, device)
    # rank = position in the image's stable descending confidence order: a stable sort by confidence over the whole batch, then
    # a stable sort of that by image number (already ascending in the packed layout) -- a segmented sort without a host loop
    pos = torch.arange(sum_p, dtype=torch.int32, device=device)
    image = torch.searchsorted(poff[1:], pos, right=True)
    by_conf = torch.argsort(conf, descending=True, stable=True)
    order = by_conf[torch.argsort(image[by_conf], stable=True)]
    rank = torch.empty(sum_p, dtype=torch.int32, device=device)
    rank[order] = pos - poff[image]
    first = torch.empty((k, sum_t), dtype=torch.int32, device=device)
    tp = torch.zeros((k, sum_p), dtype=torch.uint8, device=device)
    torch.ops.cvpce_amd.eval_match_detections(pred, poff, rank, pcls, tgt, toff, tcls, thr, max(n_tgt, default=0), first, tp)
    return {'tp': tp, 'first': first, 'conf': conf[order], 'rank': rank, 'pcls': pcls, 'tcls': tcls, 'n_pred': n_pred, 'n_tgt': n_tgt}


def match_detections(targets, predictions, confidences, iou_thresholds, target_labels=None, prediction_labels=None):
    """Match each image's predictions to its targets at every threshold on the device.

    targets / predictions: lists of (T,4) / (P,4) xyxy boxes, confidences: list of (P,), on the device or the host; the labels
    (both or neither) make the matching class-aware.  -> (flags, first), two lists with one entry per image:
    flags[i] (K,P) uint8 in RANK order (row k, column r: is the r-th most confident prediction a true positive at threshold k),
    first[i] (K,T) int32, the rank of the first prediction that covers each target, -1 if none."""
    device = _device_of(predictions, confidences, targets)
    thr = torch.tensor(_threshold_values(iou_thresholds), dtype=torch.float32).to(device)
    m = _match_packed(targets, predictions, confidences, thr, target_labels, prediction_labels)
    poff, toff = staging.offsets(m['n_pred']), staging.offsets(m['n_tgt'])
    return ([m['tp'][:, poff[i]:poff[i + 1]] for i in range(len(targets))],
            [m['first'][:, toff[i]:toff[i + 1]] for i in range(len(targets))])


def _strip(res):
    return {thr: {k: v for k, v in itm.items() if k != 'raw'} for thr, itm in res.items()}


class DetectionMetrics:
    """Device-resident accumulator: `update` per batch, `compute` (or `compute_per_class`) once at the end."""

    def __init__(self, iou_thresholds=(0.5,), device=None):
        self.iou_thresholds = list(iou_thresholds)
        self._values = _threshold_values(self.iou_thresholds)
        self._device = torch.device(device) if device is not None else None
        self._thr = None
        self._batches = []
        self._labelled = None

    def update(self, targets, predictions, confidences, target_labels=None, prediction_labels=None):
        """Queue the matching of one batch of images.  With device-resident inputs the host never waits here: the per-image
        lengths are known from the shapes, everything else stays on the device until `compute`."""
        labelled = target_labels is not None
        if self._labelled is not None and labelled != self._labelled:
            raise ValueError('class ids must be given to every update or to none')
        if self._thr is None:
            if self._device is None:
                self._device = _device_of(predictions, confidences, targets)
            self._thr = staging.upload_values(self._values, torch.float32, self._device)
        m = _match_packed(targets, predictions, confidences, self._thr, target_labels, prediction_labels)
        self._labelled = labelled
        del m['first']
        self._batches.append(m)

    # ---- host half -----------------------------------------------------------------------------------------------------------
    def _fetch(self):
        """One device-to-host copy of everything accumulated -> per-image host records
        (flags (K,P) uint8 in rank order, sorted confidences (P,), target count, class ids of the predictions in rank order and
        in input order, class ids of the targets)."""
        b = self._batches
        words = [torch.cat([m[key] for m in b]) for key in (('conf', 'rank', 'pcls', 'tcls') if self._labelled else ('conf', 'rank'))]
        sizes = [w.numel() for w in words]
        buf = torch.cat([w.view(torch.uint8) for w in words] + [m['tp'].reshape(-1) for m in b]).cpu()
        host, at = [], 0
        for w, n in zip(words, sizes):
            host.append(buf[at:at + 4 * n].view(w.dtype))
            at += 4 * n
        conf, rank = host[0], host[1].long()
        pcls, tcls = (host[2], host[3]) if self._labelled else (None, None)
        records, p_at, t_at = [], 0, 0
        k = len(self._values)
        for m in b:
            sum_p = sum(m['n_pred'])
            tp = buf[at:at + k * sum_p].view(k, sum_p)
            at += k * sum_p
            off = 0
            for n_p, n_t in zip(m['n_pred'], m['n_tgt']):
                rec = {'tp': tp[:, off:off + n_p], 'conf': conf[p_at:p_at + n_p], 'n_tgt': n_t}
                if self._labelled:
                    given = pcls[p_at:p_at + n_p]
                    ranked = torch.empty_like(given)
                    ranked[rank[p_at:p_at + n_p]] = given
                    rec.update(pcls=ranked, pcls_given=given, tcls=tcls[t_at:t_at + n_t])
                records.append(rec)
                off, p_at, t_at = off + n_p, p_at + n_p, t_at + n_t
        return records

    def calculate_from_flags(self, units):
        """units: (flags (K,P) uint8 in rank order, sorted confidences, number of targets) -> metrics._do_calculate's result.
        Per unit this is what `metrics._process_one` returns, taken from the flags."""
        thresholds = self.iou_thresholds
        per_thr = {t: {'true_positives': [], 'false_positives': [], 'recall_300': []} for t in thresholds}
        confs, total = [], 0
        for flags, conf, n_tgt in units:
            tp = flags.to(torch.float32)
            fp = 1 - tp
            # (columns = thresholds: cumulative sums of 0/1 flags are exact, so the recall of every column is the 1-D routine's)
            _, rec = metrics.precision_and_recall(tp.t(), fp.t(), n_tgt)
            r300 = rec[:300][-1] if len(rec) > 0 else None
            for k, t in enumerate(thresholds):
                per_thr[t]['true_positives'].append(tp[k])
                per_thr[t]['false_positives'].append(fp[k])
                per_thr[t]['recall_300'].append(r300[k] if r300 is not None else 0)
            confs.append(conf)
            total += n_tgt
        return metrics._do_calculate(thresholds, per_thr, confs, total)

    def compute(self):
        """-> the dictionary `metrics.calculate_metrics` returns (with 'raw'), one unit per image."""
        if not self._batches:
            return metrics.calculate_metrics([], [], [], self.iou_thresholds)
        return self.calculate_from_flags([(r['tp'], r['conf'], r['n_tgt']) for r in self._fetch()])

    def compute_per_class(self, n_classes):
        """The grouping of `detection_eval.evaluate_detections`: one unit per (image, class) for every class present among the
        image's predictions or targets; class -1 (unknown label) only enters the pooled result.
        -> (per-class results for the classes 0..n_classes-1 that occur, pooled result), both without 'raw'."""
        if not self._labelled:
            if self._labelled is None:
                return {}, _strip(metrics.calculate_metrics([], [], [], self.iou_thresholds))
            raise ValueError('compute_per_class needs the class ids given to update()')
        return self.per_class_from_records(self._fetch(), n_classes)

    def per_class_from_records(self, records, n_classes):
        """The host half of `compute_per_class`.  records: per image a dict with 'tp' (K,P) uint8 flags in rank order, 'conf' sorted
        confidences, 'pcls' the predictions' class ids in rank order, 'pcls_given' the same in input order, 'tcls' the targets'."""
        pooled, by_class = [], {c: [] for c in range(n_classes)}
        for r in records:
            # (the host harness walks a Python set built this way; the same expression gives the same order of units)
            for c in {int(x) for x in r['pcls_given']} | {int(x) for x in r['tcls']}:
                mine = r['pcls'] == c
                unit = (r['tp'][:, mine], r['conf'][mine], int((r['tcls'] == c).sum()))
                pooled.append(unit)
                if c in by_class:
                    by_class[c].append(unit)
        per_class = {c: _strip(self.calculate_from_flags(units)) for c, units in by_class.items() if units}
        if not pooled:
            return per_class, _strip(metrics.calculate_metrics([], [], [], self.iou_thresholds))
        return per_class, _strip(self.calculate_from_flags(pooled))
