"""Cases and plain restatements for the device planogram comparator (not a test module): the scene generator, the tie-free
condition, the device rule of DESIGN.md 4b restated over torch's CPU fp32 arithmetic (`model_graph`) and the match rule restated
over the slot tables (`model_match`).  test_planograms_device_cpu.py pins the two restatements against the stock host functions;
test_gpu_planograms_device.py holds the kernels to them bit for bit."""
import math
import os

import torch

from cvpce_amd import planograms

NAMES = tuple(f'name_{i:02d}' for i in range(12))
TAN_PI_8 = torch.tensor(0.41421356, dtype=torch.float32)
TAN_3PI_8 = torch.tensor(2.41421356, dtype=torch.float32)
# the first tie-free seed of `scene` per size (searched by first_tie_free_seed; asserted in test_planograms_device_cpu.py)
TIE_FREE_SEEDS = {1: 0, 2: 0, 3: 0, 7: 0, 25: 0, 26: 0, 64: 0, 65: 0}


def scene(n, seed):
    """n boxes: integer top-left corners uniform in [0, 2000), even integer widths and heights in [40, 120), labels from 12 names."""
    g = torch.Generator().manual_seed(seed)
    xy = torch.randint(0, 2000, (n, 2), generator=g)
    wh = torch.randint(20, 60, (n, 2), generator=g) * 2
    labels = [NAMES[i] for i in torch.randint(0, len(NAMES), (n,), generator=g).tolist()]
    return torch.cat((xy, xy + wh), dim=1).to(torch.float32), labels


def centres(boxes):
    return (boxes[:, 0] + boxes[:, 2]) / 2, (boxes[:, 1] + boxes[:, 3]) / 2


def is_tie_free(boxes, margin=2e-5):
    """For every node the squared centre distances to all others are pairwise distinct (exact: the centres are integers), and no
    pair's direction is within `margin` rad of a sector boundary (an odd multiple of pi/8)."""
    cx, cy = (c.to(torch.int64) for c in centres(boxes))
    assert torch.equal(cx.to(torch.float32), centres(boxes)[0]) and torch.equal(cy.to(torch.float32), centres(boxes)[1])
    n = len(cx)
    dx, dy = cx[None, :] - cx[:, None], cy[None, :] - cy[:, None]
    sq = dx * dx + dy * dy
    off = ~torch.eye(n, dtype=torch.bool)
    for i in range(n):
        row = sq[i][off[i]]
        if len(row.unique()) != len(row) or bool((row == 0).any()):
            return False
    ang = torch.atan2(dy.double(), dx.double())[off]
    frac = torch.remainder(ang / (math.pi / 8) - 1, 2.0)                 # 0 (= 2) at the odd multiples of pi/8
    gap = torch.minimum(frac, 2.0 - frac) * (math.pi / 8)
    return not bool((gap < margin).any())


def first_tie_free_seed(n, limit=3000):
    return next(s for s in range(limit) if is_tie_free(scene(n, s)[0]))


def threshold(boxes, thresh_size):
    """build_graph's own expression (planograms.py:42-43) -> float32 0-dim tensor"""
    span = (torch.amax(boxes[:, 2]) - torch.amin(boxes[:, 0]) + torch.amax(boxes[:, 3]) - torch.amin(boxes[:, 1])) / 2
    return thresh_size * span


def exact_root(x):
    """The correctly rounded fp32 square root of a float32 tensor, whatever this machine's vector maths library does (torch.sqrt
    goes through it and is within 1 ulp on some CPUs, not correctly rounded): a first guess, then the neighbour test in exact
    arithmetic -- the midpoint between two adjacent floats has 25 bits, its square 50: exact in float64."""
    xd = x.double()
    r = torch.sqrt(xd).float()
    for _ in range(2):
        lo, hi = torch.nextafter(r, torch.full_like(r, -float('inf'))), torch.nextafter(r, torch.full_like(r, float('inf')))
        mlo, mhi = (r.double() + lo.double()) / 2, (r.double() + hi.double()) / 2
        r = torch.where((lo >= 0) & (xd < mlo * mlo), lo, torch.where(xd > mhi * mhi, hi, r))
    return r


def assert_same_as_stock(model_adj, host_adj, boxes):
    """Adjacency lists (neighbour, direction, weight) of the device rule against stock `planograms.build_graph` on a scene with
    integer centres: structure and order exactly; our weight is the exact root of the exact squared distance, bit for bit; the
    host's weight equals it wherever the host's own root is the correctly rounded one -- everywhere, on a machine whose torch.sqrt
    is -- and is otherwise off by the host's error, one ulp at the most.  -> the number of host weights that are not exact roots."""
    assert [[e[:2] for e in row] for row in model_adj] == [[e[:2] for e in row] for row in host_adj]
    cx, cy = centres(boxes.to(torch.float32))
    src = torch.tensor([i for i, row in enumerate(model_adj) for _ in row], dtype=torch.long)
    dst = torch.tensor([e[0] for row in model_adj for e in row], dtype=torch.long)
    dx, dy = cx[dst] - cx[src], cy[dst] - cy[src]
    exact = exact_root(dx * dx + dy * dy)
    ours = torch.tensor([e[2] for row in model_adj for e in row], dtype=torch.float32)
    host = torch.tensor([e[2] for row in host_adj for e in row], dtype=torch.float32)
    assert torch.equal(ours.view(torch.int32), exact.view(torch.int32))
    ulp = torch.nextafter(exact, torch.full_like(exact, float('inf'))) - exact
    assert bool(((host - exact).abs() <= ulp).all())
    return int((host != exact).sum())


def model_graph(boxes, thresh_size=0.5):
    """The device rule, plainly: -> (nbr int32, weight float32, stamp int32), each (n, 8); empty slot = (-1, 0, -1)."""
    boxes = boxes.to(torch.float32)
    n = len(boxes)
    thresh = float(threshold(boxes, thresh_size))
    cx, cy = centres(boxes)
    dx, dy = cx[None, :] - cx[:, None], cy[None, :] - cy[:, None]           # [i][j] = c_j - c_i
    d = exact_root(dx * dx + dy * dy)                                       # three roundings and a correctly rounded root
    ax, ay = dx.abs(), dy.abs()
    flat, steep = ay <= TAN_PI_8 * ax, ay > TAN_3PI_8 * ax
    diag = torch.where(dy > 0, torch.where(dx > 0, 1, 3), torch.where(dx > 0, 7, 5))
    sector = torch.where(flat, torch.where(dx > 0, 0, 4), torch.where(steep, torch.where(dy > 0, 2, 6), diag))
    by_dist, order = d.sort(dim=1, stable=True)                             # ascending (d, j)
    by_dist, order, sector = by_dist.tolist(), order.tolist(), sector.tolist()
    nbr = [[-1] * 8 for _ in range(n)]
    wgt = [[0.0] * 8 for _ in range(n)]
    stp = [[-1] * 8 for _ in range(n)]
    count = 0
    for i in range(n):
        wanted = {s for s in range(8) if nbr[i][s] < 0}
        for dist, j in zip(by_dist[i], order[i]):
            if dist > thresh or not wanted:
                break
            if j == i or not dist > 0:
                continue
            s = sector[i][j]
            if s not in wanted:
                continue
            back = (s + 4) % 8
            rival = nbr[j][back]
            if rival >= 0:
                if wgt[j][back] <= dist:
                    continue
                assert nbr[rival][s] == j
                nbr[rival][s], wgt[rival][s], stp[rival][s] = -1, 0.0, -1
            nbr[i][s], wgt[i][s], stp[i][s] = j, dist, count
            nbr[j][back], wgt[j][back], stp[j][back] = i, dist, count + 1
            count += 2
            wanted.remove(s)
    return (torch.tensor(nbr, dtype=torch.int32).reshape(n, 8), torch.tensor(wgt, dtype=torch.float32).reshape(n, 8),
            torch.tensor(stp, dtype=torch.int32).reshape(n, 8))


def adjacency_of_tables(nbr, weight, stamp):
    """per node: [(neighbour, direction name, weight as float)] in stamp order"""
    out = []
    for i in range(len(nbr)):
        slots = sorted((int(stamp[i, s]), s) for s in range(8) if int(nbr[i, s]) >= 0)
        out.append([(int(nbr[i, s]), planograms.CARDINALS[s], float(weight[i, s])) for _, s in slots])
    return out


def adjacency_of_host(g):
    """the same view of a stock `planograms.build_graph` DiGraph"""
    return [[(int(nb), g[i][nb]['dir'], float(g[i][nb]['weight'])) for nb in g[i]] for i in range(len(g))]


def model_match(t1, labels1, t2, labels2, min_score=-0.2, stop_at_fraction=1 / 2):
    """`build_hypotheses` + `large_common_subgraph` restated over slot tables t = (nbr, weight, stamp) -> list of pairs in grown order."""
    nb1, st1, nb2 = t1[0].tolist(), t1[2].tolist(), t2[0].tolist()
    n1, n2 = len(labels1), len(labels2)
    order1 = [[s for _, s in sorted((st1[a][s], s) for s in range(8) if nb1[a][s] >= 0)] for a in range(n1)]
    min_agree = next((a for a in range(9) if not -(a / 8) > min_score), 9)
    enough = int(min(n1, n2) * stop_at_fraction)
    levels = [[] for _ in range(9)]
    for a in range(n1):
        for b in range(n2):
            if labels1[a] != labels2[b]:
                continue
            agree = sum(1 for s in range(8) if nb1[a][s] >= 0 and nb2[b][s] >= 0 and labels1[nb1[a][s]] == labels2[nb2[b][s]])
            levels[agree].append((a, b))
    best = []
    for agree in range(8, -1, -1):
        for s1, s2 in levels[agree]:
            if agree < min_agree and best:
                return best
            grown, used1, used2, queue = [], set(), set(), [(s1, s2)]
            while queue:
                a, b = queue.pop(0)
                if a in used1 or b in used2:
                    continue
                grown.append((a, b)); used1.add(a); used2.add(b)
                queue += [(nb1[a][s], nb2[b][s]) for s in order1[a] if nb2[b][s] >= 0 and labels1[nb1[a][s]] == labels2[nb2[b][s]]]
            if len(grown) > enough:
                return grown
            if len(grown) > len(best):
                best = grown
    return best


def golden_cases(golden_dir):
    return torch.load(os.path.join(golden_dir, 'planograms.pt'), weights_only=False)


def grid(rows, cols, seed, pitch=(72, 120), size=(64, 96)):
    """A gridded planogram with exact ties: integer boxes, random labels from the 12 names."""
    g = torch.Generator().manual_seed(seed)
    boxes = [[10 + c * pitch[0], 20 + r * pitch[1], 10 + c * pitch[0] + size[0], 20 + r * pitch[1] + size[1]] for r in range(rows) for c in range(cols)]
    labels = [NAMES[i] for i in torch.randint(0, len(NAMES), (rows * cols,), generator=g).tolist()]
    return torch.tensor(boxes, dtype=torch.float32), labels


def detections_of(boxes, labels, seed, drop=0.05, mislabel=0.05):
    """The boxes scaled 1.7x, shifted, jittered by 3 px, a fraction dropped and a fraction given another name."""
    g = torch.Generator().manual_seed(seed)
    n = len(labels)
    out = boxes * 1.7 + torch.tensor([30.0, 12.0, 30.0, 12.0]) + (torch.rand(n, 4, generator=g) * 2 - 1) * 3
    keep = (torch.rand(n, generator=g) >= drop).tolist()
    wrong = (torch.rand(n, generator=g) < mislabel).tolist()
    lab = [NAMES[(NAMES.index(l) + 1) % len(NAMES)] if w else l for l, w in zip(labels, wrong)]
    idx = [i for i in range(n) if keep[i]] or [0]
    return out[idx].contiguous(), [lab[i] for i in idx]


def repeated_blocks(repeats):
    """A 3-row shelf made of `repeats` copies of one 3x3 label block side by side, one label changed per copy: many seed pairs agree
    in most directions, none grows past its own block's neighbourhood at once -- the search runs through several hypotheses."""
    block = [NAMES[i] for i in range(9)]
    boxes, labels = [], []
    for r in range(3):
        for k in range(repeats):
            for c in range(3):
                x, y = 10 + (k * 3 + c) * 72, 20 + r * 120
                boxes.append([x, y, x + 64, y + 96])
                labels.append(NAMES[9 + (k % 3)] if (r * 3 + c) == k % 9 else block[r * 3 + c])
    return torch.tensor(boxes, dtype=torch.float32), labels
