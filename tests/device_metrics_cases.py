"""Inputs shared by test_device_metrics_cpu.py and test_gpu_device_metrics.py, and the plain-torch restatement of the closed
form the device kernel computes.  (Not a test module.)"""
import os

import torch

from cvpce_amd import metrics

# the known-answer images of tests/test_metrics_cpu.py (the reference's test/metrics_test.py)
TARGETS = [
    torch.tensor([[0, 0, 1, 1], [1, 0, 2, 1], [1, 1, 2, 2]], dtype=torch.float),
    torch.tensor([[1, 1, 2, 2], [3, 1, 4, 2], [5, 1, 6, 2], [7, 1, 8, 2]], dtype=torch.float),
    torch.tensor([[0, 0, 5, 5], [5, 5, 10, 10]], dtype=torch.float),
]
PREDICTIONS = [
    torch.tensor([[0, 0, .9, .9], [1.1, 0.1, 1.9, 0.9], [0, 0, 1, 1], [0.9, 0.9, 2.1, 2.1], [3, 3, 4, 4]], dtype=torch.float),
    torch.tensor([[1, 0, 2, 1], [1, 1, 2, 2], [5, 1, 6, 2], [7, 1.1, 8, 1.9], [9, 9, 10, 10]], dtype=torch.float),
    torch.tensor([[0, 0, 1, 1], [1, 1, 3, 3], [0.5, 0.5, 4.5, 4.5], [0, 0, 6, 6], [6, 6, 9, 9]], dtype=torch.float),
]
CONFIDENCES = [
    torch.tensor([1, 0.8, 0.6, 0.4, 0.2], dtype=torch.float),
    torch.tensor([0.9, 0.8, 0.7, 0.65, 0.5], dtype=torch.float),
    torch.tensor([0.85, 0.6, 0.4, 0.2, 0.1], dtype=torch.float),
]

THRESHOLD_SETS = ((0.5,), tuple(torch.linspace(.5, .95, 10)), (0.7, 0.95))


def known_answer_cases(golden_dir):
    """The seven known-answer inputs of tests/test_metrics_cpu.py as (name, targets, predictions, confidences): the three images
    together (calculate_metrics_kat), each alone (iou_matrices_kat / check_matches_kat use them one at a time), the two edge
    cases (no boxes at all; targets but no predictions) and the reference-made two-target case of the golden file."""
    g = torch.load(os.path.join(golden_dir, 'metrics.pt'), weights_only=False)
    two = g['two_targets']
    n2 = len(two['predictions'])
    cases = [('kat_all', TARGETS, PREDICTIONS, CONFIDENCES)]
    cases += [(f'kat_{i}', [TARGETS[i]], [PREDICTIONS[i]], [CONFIDENCES[i]]) for i in range(3)]
    cases += [('empty', [torch.zeros(0, 4)], [torch.zeros(0, 4)], [torch.zeros(0)]),
              ('none_found', [TARGETS[0]], [torch.zeros(0, 4)], [torch.zeros(0)]),
              ('two_targets', [two['targets']], [two['predictions']], [torch.linspace(1, 0.5, n2)])]
    return cases


def golden_cases(golden_dir):
    """The reference-made inputs of tests/golden/metrics.pt: its known-answer set, the random and the dense-overlap cases."""
    g = torch.load(os.path.join(golden_dir, 'metrics.pt'), weights_only=False)
    cases = [('golden_kat', g['targets'], g['predictions'], g['confidences'])]
    for kind in ('random', 'dense'):
        cases += [(f'{kind}_{i}', c['targets'], c['predictions'], c['confidences']) for i, c in enumerate(g[kind])]
    return cases


def closed_form(target, prediction, confidence, thresholds, target_labels=None, prediction_labels=None):
    """Plain torch on the host: a prediction is a true positive iff it is the first one, in stable descending confidence order,
    that covers some target at IoU >= threshold (and, with labels, has that target's class).
    -> (flags (K,P) uint8 in rank order, first (K,T) int64, sorted confidences, the order)."""
    conf, order = torch.sort(confidence, descending=True, stable=True)
    n_p, n_t = len(order), len(target)
    iou = metrics.box_iou(prediction[order].reshape(-1, 4), target.reshape(-1, 4))
    same = torch.ones(n_p, n_t, dtype=torch.bool)
    if target_labels is not None:
        same = prediction_labels[order][:, None] == target_labels[None, :]
    rank = torch.arange(n_p)[:, None].expand(n_p, n_t)
    flags = torch.zeros(len(thresholds), n_p, dtype=torch.uint8)
    first = torch.full((len(thresholds), n_t), -1, dtype=torch.long)
    for k, thr in enumerate(thresholds):
        cover = (iou >= thr) & same
        if n_p and n_t:
            f = torch.where(cover, rank, torch.full_like(rank, n_p)).min(dim=0).values
            first[k] = torch.where(f == n_p, torch.full_like(f, -1), f)
            flags[k, f[f < n_p]] = 1
    return flags, first, conf, order


def assert_results_equal(got, want, thresholds):
    """torch.equal on every field of the result dictionary, 'raw' included."""
    assert list(got) == list(want) or [float(t) for t in got] == [float(t) for t in want]
    for tg, tw in zip(got, want):
        for k in ('f', 'p', 'r', 'c', 'ap', 'ar_300'):
            a, b = torch.as_tensor(got[tg][k]), torch.as_tensor(want[tw][k])
            assert a.dtype == b.dtype and torch.equal(a, b), (float(tw), k, a, b)
        if 'raw' in want[tw]:
            for k in ('p', 'r', 'f', 'c'):
                assert torch.equal(got[tg]['raw'][k], want[tw]['raw'][k]), (float(tw), 'raw', k)
        else:
            assert 'raw' not in got[tg]
