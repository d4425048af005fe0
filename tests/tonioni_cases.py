"""Cases and a plain restatement for the Tonioni matcher (not a test module): the seeded case generator behind
tests/golden/tonioni.pt and `model_tonioni`, the device algorithm of DESIGN.md 4b ("the Tonioni rule") restated with numpy over
the [n][8] slot tables, beside `model_match` of planogram_device_cases.py.  test_tonioni_cpu.py pins the host `tonioni_mcs` to the
reference's recorded results and the model to the host; test_gpu_tonioni.py holds the kernels to the model."""
import os

import numpy as np
import torch

NAMES = tuple(f'name_{i:02d}' for i in range(12))
GENERATED = 40              # seeds 0 .. 39 of `generated`
NO_BOUND = 2 ** 31 - 1      # M of a start that took no step


def shelf(rows, cols, labels, pitch=(72, 120), size=(64, 96)):
    """A gridded planogram of rows x cols integer boxes, `labels` names assigned in row blocks: the grid in row-major order is
    cut into `labels` runs of (nearly) equal length, one name each."""
    n = rows * cols
    boxes = [[10 + c * pitch[0], 20 + r * pitch[1], 10 + c * pitch[0] + size[0], 20 + r * pitch[1] + size[1]] for r in range(rows) for c in range(cols)]
    return torch.tensor(boxes, dtype=torch.float32), [NAMES[i * labels // n] for i in range(n)]


def detections_of(boxes, labels, seed, names, drop=0.15, mislabel=0.20):
    """The boxes scaled 1.7x, shifted, jittered by 3 px; a fraction dropped and a fraction given the next of `names`."""
    g = torch.Generator().manual_seed(seed)
    n = len(labels)
    out = boxes * 1.7 + torch.tensor([30.0, 12.0, 30.0, 12.0]) + (torch.rand(n, 4, generator=g) * 2 - 1) * 3
    keep = (torch.rand(n, generator=g) >= drop).tolist()
    wrong = (torch.rand(n, generator=g) < mislabel).tolist()
    lab = [names[(names.index(l) + 1) % len(names)] if w else l for l, w in zip(labels, wrong)]
    idx = [i for i in range(n) if keep[i]] or [0]
    return out[idx].contiguous(), [lab[i] for i in idx]


def generated(seed):
    """Case `seed`: a grid between 2x5 and 4x8 with 2 to 7 labels, and its detections."""
    g = torch.Generator().manual_seed(1000 + seed)
    rows, cols, k = (int(torch.randint(lo, hi + 1, (1,), generator=g)) for lo, hi in ((2, 4), (5, 8), (2, 7)))
    b1, l1 = shelf(rows, cols, k)
    b2, l2 = detections_of(b1, l1, 2000 + seed, NAMES[:k])
    return {'name': f'grid{rows}x{cols}_k{k}_s{seed}', 'boxes1': b1, 'labels1': l1, 'boxes2': b2, 'labels2': l2, 'min_score': -0.2}


def special():
    """The hand-made cases: no equal labels, 1-node graphs, another min_score."""
    b1, l1 = shelf(2, 5, 2)
    b2, _ = detections_of(b1, l1, 7, NAMES[:2], drop=0.0, mislabel=0.0)
    out = [{'name': 'no_equal_labels', 'boxes1': b1, 'labels1': l1, 'boxes2': b2, 'labels2': [NAMES[5]] * len(b2), 'min_score': -0.2}]
    one = torch.tensor([[10.0, 20.0, 74.0, 116.0]])
    out.append({'name': 'one_node', 'boxes1': one, 'labels1': [NAMES[0]], 'boxes2': one * 1.7, 'labels2': [NAMES[0]], 'min_score': -0.2})
    out.append(dict(generated(3), name='min_score_half', min_score=-0.5))
    out.append(dict(generated(11), name='min_score_half_b', min_score=-0.5))
    return out


def cases():
    return [generated(s) for s in range(GENERATED)] + special()


def golden(golden_dir):
    return torch.load(os.path.join(golden_dir, 'tonioni.pt'), weights_only=False)


def window_scene(i):
    """Scene i of the comparator tests' window: a shelf of few products with many facings, and its detections."""
    rows, cols, k = ((3, 6, 3), (3, 7, 2), (4, 6, 4), (2, 8, 3), (4, 5, 2), (3, 8, 5), (4, 7, 3), (2, 6, 2))[i % 8]
    b1, l1 = shelf(rows, cols, k)
    b2, l2 = detections_of(b1, l1, 300 + i, NAMES[:k], drop=0.10, mislabel=0.10)
    return b1, l1, b2, l2


# ---------------------------------------------------------------------------------------------------------------------------------
def score8_limit(min_score):
    """The largest integer t for which t / 8 is NOT above min_score: a head whose score8 = -agree - 8 * bumps is above it ends a run."""
    t = int(np.floor(8 * min_score))
    while not (t + 1) / 8 > min_score:
        t += 1
    while t / 8 > min_score:
        t -= 1
    return t


def hypotheses_of(nb1, labels1, nb2, labels2):
    """The seed pairs in the match kernel's order -- agree descending, then n1, then n2 -> int64 arrays (agree, n1, n2)."""
    ids = {}
    l1 = np.array([ids.setdefault(l, len(ids)) for l in labels1], dtype=np.int64)
    l2 = np.array([ids.setdefault(l, len(ids)) for l in labels2], dtype=np.int64)
    nb1, nb2 = np.asarray(nb1, dtype=np.int64).reshape(-1, 8), np.asarray(nb2, dtype=np.int64).reshape(-1, 8)
    nl1 = np.where(nb1 >= 0, l1[np.clip(nb1, 0, None)], -1)
    nl2 = np.where(nb2 >= 0, l2[np.clip(nb2, 0, None)], -2)
    a, b = np.nonzero(l1[:, None] == l2[None, :])
    agree = (nl1[a] == nl2[b]).sum(axis=1) if len(a) else np.zeros(0, dtype=np.int64)
    order = np.lexsort((b, a, -agree))
    return agree[order].astype(np.int64), a[order].astype(np.int64), b[order].astype(np.int64)


def model_run(agree, x1, x2, nb1, nb2, limit):
    """One start over the hypotheses given (already the suffix) -> (pairs in growth order, M, whether the run ended on the
    min_score stop with hypotheses left).  The live hypotheses are kept as an (n1, n2) matrix of keys."""
    n1, n2 = len(nb1), len(nb2)
    big = np.iinfo(np.int64).max
    score = np.zeros((n1, n2), dtype=np.int64)
    alive = np.zeros((n1, n2), dtype=bool)
    score[x1, x2], alive[x1, x2] = -agree, True
    place = (np.arange(n1, dtype=np.int64)[:, None] << 10) | np.arange(n2, dtype=np.int64)[None, :]
    taken, low = [], NO_BOUND
    while alive.any():
        key = np.where(alive, ((score + (1 << 30)) << 20) | place, big)     # ascending key = ascending (score8, n1, n2)
        a, b = (int(v) for v in np.unravel_index(int(np.argmin(key)), key.shape))
        if score[a, b] > limit:
            return taken, low, True
        taken.append((a, b))
        alive[a, :], alive[:, b] = False, False
        key = np.where(alive, key, big)
        first = alive & (key == key.min(axis=1)[:, None]) & (key == key.min(axis=0)[None, :])   # first of its n1 AND of its n2, old order
        for e1, e2 in {(int(nb1[a][d]), int(nb2[b][d])) for d in range(8)}:                      # (a pair gains its point once)
            if e1 >= 0 and e2 >= 0 and alive[e1, e2]:
                score[e1, e2] -= 8
        low = min(low, len(taken) + int(first.sum()))
    return taken, low, False


def model_tonioni(t1, labels1, t2, labels2, min_score=-0.2, use_bound=True, starts=None):
    """The Tonioni rule over slot tables t = (nbr, weight, stamp) -> (pairs of the adopted start in growth order, {start: (M, F)},
    the adopted start or -1, whether its run ended on the min_score stop with hypotheses left).
    use_bound=False adopts every strictly larger run whatever its M.  starts: only these starts are run, and there is no choice
    (pairs = [], start = -1)."""
    nb1, nb2 = np.asarray(t1[0], dtype=np.int64).reshape(-1, 8), np.asarray(t2[0], dtype=np.int64).reshape(-1, 8)
    agree, x1, x2 = hypotheses_of(nb1, labels1, nb2, labels2)
    limit, h = score8_limit(min_score), len(agree)
    run = lambda i: model_run(agree[i:], x1[i:], x2[i:], nb1, nb2, limit)
    if starts is not None:
        return [], {i: (lambda r: (r[1], len(r[0])))(run(i)) for i in starts}, -1, False
    mf, best, arg, kept = {}, 0, -1, ([], NO_BOUND, False)
    for i in range(h):
        r = run(i)
        mf[i] = (r[1], len(r[0]))
    for i in range(h):
        if best > h - i:
            break
        m, f = mf[i]
        if (m >= best or not use_bound) and f > best:
            best, arg = f, i
    if arg >= 0:
        kept = run(arg)
    return kept[0], mf, arg, kept[2]


def choose(mf, h):
    """the scan alone over {start: (M, F)} of all h starts -> (adopted start or -1, its size)"""
    best, arg = 0, -1
    for i in range(h):
        if best > h - i:
            break
        if mf[i][0] >= best and mf[i][1] > best:
            best, arg = mf[i][1], i
    return arg, best


def tables_of_host(g):
    """A host DiGraph (`planograms.build_graph`) in table form -> (nbr int32, weight float32, stamp int32), each (n, 8); a node's
    stamps count its adjacency order."""
    from cvpce_amd.planograms import CARDINALS
    n = len(g)
    nbr, wgt, stp = torch.full((n, 8), -1, dtype=torch.int32), torch.zeros((n, 8), dtype=torch.float32), torch.full((n, 8), -1, dtype=torch.int32)
    for i in range(n):
        for k, nb in enumerate(g[i]):
            s = CARDINALS.index(g[i][nb]['dir'])
            nbr[i, s], wgt[i, s], stp[i, s] = int(nb), float(g[i][nb]['weight']), k
    return nbr, wgt, stp
