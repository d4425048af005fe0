"""The embed + match accuracy harness (`classification_eval.eval_dihe`) a window of shelf images at a time, compared on the device.

`ClassificationTally` is the opt-in counterpart of the per-image loop: `update` queues, for a whole window, one crop
pass straight to the embedder's bf16 input (`production.roi_crops`), one `embed_packed`, one `Classifier.match` and one launch of
`torch.ops.cvpce_amd.classeval_rank` (csrc/classeval.hip) into the window's slice of a record log that stays on the device;
`compute` brings the log back with one pinned copy and one synchronisation and counts on the host.  Labels are compared as ids of
the classifier's id space (`Classifier.label_ids`); the target strings never leave the host.  The crops, the schedule and the
matcher are the host path's bit for bit, so every count equals the loop's (tests/test_gpu_classeval.py).

A classifier without an id space (unhashable annotations), targets that do not hash, or an encoder object without an engine take the
per-image host path for that window (`host_routed` counts them) -- the rule of `PlanogramComparator(device_reclass=True)`.
"""
import torch

from . import datautils, ops
from .classification_eval import clip_boxes_to_image
from . import staging

LOG_ROWS = 4096           # records the log is first allocated for; it doubles when a window does not fit


class ClassificationTally:
    """classifier: a `production.Classifier` built with k = max(k); k: the knn values of the accuracy dict.

    update(images, boxes, targets)   one window: device images (either form), per-image integer xyxy boxes (T,4), per-image lists of
                                     T target annotations -- device work is queued, the host does not wait
    compute()                        -> {'accuracy': {knn: correct / total}, 'total', 'correct': {knn: n}, 'per_ann', 'missed',
                                     'confusion'}, keyed by annotation as the host loop keys them
    """

    def __init__(self, classifier, k=(1,)):
        self.classifier = classifier
        self.k = tuple(k)
        self.host_routed = 0                  # windows that took the per-image host path
        self._log = None                      # (rows, 2) int32 on the device: first rank, nearest label id
        self._rows = 0
        self._events = []                     # in window order: ('device', first row, end row, K, targets) | ('host', targets, predictions)
        self._reset_counts()

    def _reset_counts(self):
        self.total, self.correct = 0, {knn: 0 for knn in self.k}
        self.per_ann, self.missed, self.confusion = {}, {}, {}
        self._label_of = None                 # label id -> annotation, made at the first `reduce` after a reset

    # ------------------------------------------------------------------ update ------------------------------------------------
    def _slice(self, n, device):
        """the next n rows of the log (grown on the device, without a wait, when they do not fit)"""
        need = self._rows + n
        if self._log is None or need > self._log.shape[0]:
            rows = max(LOG_ROWS, 2 * need)
            log = torch.empty((rows, 2), dtype=torch.int32, device=device)
            if self._rows:
                log[:self._rows].copy_(self._log[:self._rows])
            self._log = log
        out = self._log[self._rows:need]
        self._rows = need
        return out

    def _host_window(self, images, boxes, targets):
        """the lines of `eval_dihe`'s loop, image by image"""
        clf = self.classifier
        for img, b, t in zip(images, boxes, targets):
            b = clip_boxes_to_image(b, datautils.image_hw(img))
            crops = ops.crop_resize(ops.input_image(img, clf.device), b.to(clf.device), datautils.CLASSIFICATION_IMAGE_SIZE, mode=0)
            self._events.append(('host', list(t), clf.classify(crops)))

    @torch.no_grad()
    def update(self, images, boxes, targets):
        from . import production, torch_ops_classeval  # noqa: F401  (registers torch.ops.cvpce_amd.classeval_rank)
        clf = self.classifier
        counts = [len(b) for b in boxes]
        if not len(images) == len(boxes) == len(targets) or [len(t) for t in targets] != counts:
            raise ValueError('one (T,4) box tensor and one list of T targets per image')
        total = sum(counts)
        if not total:
            return
        flat = [a for t in targets for a in t]
        ids = clf.expected_label_ids(flat) if hasattr(clf.encoder, 'engine') and getattr(clf, 'label_ids', None) is not None else None
        if ids is None:
            self.host_routed += 1
            return self._host_window(images, boxes, targets)
        device = clf.device
        n, per = len(images), max(counts)
        # ONE upload: the clipped boxes (as the bits of their float32 values), the counts, the compaction and the wanted ids
        fb = torch.zeros((n, per, 4), dtype=torch.float32)
        sel = []
        for i, (img, b, c) in enumerate(zip(images, boxes, counts)):
            if c:
                fb[i, :c] = clip_boxes_to_image(torch.as_tensor(b).cpu(), datautils.image_hw(img)).to(torch.float32)
                sel += range(i * per, i * per + c)
        small = staging.upload(torch.cat((fb.view(torch.int32).reshape(-1), torch.tensor(counts + sel + ids, dtype=torch.int32))), device)
        at = n * per * 4
        dev_boxes, dev_count = small[:at].view(torch.float32).view(n, per, 4), small[at:at + n]
        dev_sel, dev_ids = small[at + n:at + n + total], small[at + n + total:]
        crops, ext, const_in, partial = production.roi_crops(
            clf.encoder, device, [ops.input_image(img, device) if c else None for img, c in zip(images, counts)], dev_boxes, dev_count)
        if total != n * per:                    # (the embedder only runs over the valid crops, as BatchedPipeline._select has it)
            crops = crops.index_select(0, dev_sel)
            ext = ext.index_select(0, dev_sel) if ext is not None else None
        eng = clf.encoder.engine()
        emb = eng.embed_packed(crops, ext=ext, const_in=const_in, partial=partial) if ext is not None else eng.embed_packed(crops)
        indices = clf.match(emb).contiguous()
        first = self._rows
        torch.ops.cvpce_amd.classeval_rank(indices, clf.gallery_label_id, dev_ids, self._slice(total, device))
        self._events.append(('device', first, first + total, indices.shape[1], flat))

    # ------------------------------------------------------------------ compute -----------------------------------------------
    def reduce(self, targets, records, K):
        """The host's share of the comparison: targets (annotations) and their records [(first rank, nearest label id), ...] of a
        match with K columns are added to the counts -- per box `want in got[:knn]` is first rank < min(knn, K), `want != got[0]` is
        first rank != 0, and got[0] is the annotation behind the nearest label id."""
        if self._label_of is None:
            self._label_of = {i: a for a, i in (getattr(self.classifier, 'label_ids', None) or {}).items()}
        label_of = self._label_of
        self.total += len(targets)
        for want, (rank, nearest) in zip(targets, records):
            self.per_ann[want] = self.per_ann.get(want, 0) + 1
            for knn in self.k:
                self.correct[knn] += int(rank < min(knn, K))
            if rank != 0:
                got = label_of.get(nearest)
                self.missed[want] = self.missed.get(want, 0) + 1
                self.confusion.setdefault(want, {})
                self.confusion[want][got] = self.confusion[want].get(got, 0) + 1

    def _reduce_host(self, targets, predictions):
        """the same counts from the host path's label lists (`eval_dihe`'s own lines)"""
        self.total += len(targets)
        for want, got in zip(targets, predictions):
            self.per_ann[want] = self.per_ann.get(want, 0) + 1
            for knn in self.k:
                self.correct[knn] += int(want in got[:knn])
            if want != got[0]:
                self.missed[want] = self.missed.get(want, 0) + 1
                self.confusion.setdefault(want, {})
                self.confusion[want][got[0]] = self.confusion[want].get(got[0], 0) + 1

    def compute(self):
        """One pinned copy of the whole log, one synchronisation, then the counts on the host (callable again after more updates)."""
        self._reset_counts()
        records = []
        if self._rows:
            host = torch.empty((self._rows, 2), dtype=torch.int32).pin_memory()
            host.copy_(self._log[:self._rows], non_blocking=True)
            torch.cuda.current_stream(self._log.device).synchronize()
            records = host.tolist()
        for ev in self._events:
            if ev[0] == 'device':
                _, a, b, K, targets = ev
                self.reduce(targets, records[a:b], K)
            else:
                self._reduce_host(ev[1], ev[2])
        return self.result()

    def result(self):
        """the counts as they stand, in `compute`'s form"""
        accuracy = {knn: c / self.total for knn, c in self.correct.items()}
        return {'accuracy': accuracy, 'total': self.total, 'correct': dict(self.correct), 'per_ann': self.per_ann, 'missed': self.missed,
                'confusion': self.confusion}


def report(result):
    """The reference's report (classification_eval.py:50-55) of a `compute()` result, as a list of lines."""
    per_ann, missed, confusion = result['per_ann'], result['missed'], result['confusion']
    lines = [f'Total annotations: {result["total"]}, Correctly guessed: {result["correct"]}, Accuracy: {result["accuracy"]}']
    worst = sorted(((v / per_ann[a], v, a) for a, v in missed.items()), reverse=True)[:10]
    lines.append('Most missed: ' + ', '.join(f'{a} ({n}, {p * 100} %)' for p, n, a in worst))
    for _, n, want in worst[:3]:
        common = sorted(((v / n, v, a) for a, v in confusion[want].items()), reverse=True)[:3]
        lines.append(f'{want}: Commonly mistaken for ' + ', '.join(f'{a} ({c}, {p * 100} %)' for p, c, a in common))
    return lines
