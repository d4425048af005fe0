"""The head-loss rule of DESIGN.md 4d on the host, and the cases the tests share (not a test module: test_headloss_cpu.py checks the
models and the conditions the cases must meet, test_gpu_headloss.py compares csrc/headloss.hip with them).

Two models of one image:
  * `model(..., F32)`: numpy, one fp32 operation at a time -- every intermediate is an np.float32 array, so nothing is contracted or kept
    wider.  Its matching is THE matching: the rule defines the IoU as an fp32 quantity (the expression of csrc/iou.h) and compares bit
    patterns, so the kernel must reproduce it on every anchor.
  * `model(..., F64)`: the same fp32 inputs and the same matching (it is a rule on fp32 bit patterns, not an approximation of
    something), every loss term and both sums in float64 -- what the losses are measured against.
Anchors come from oracle.gln.grid_anchors and scaled boxes from oracle.gln.resize_boxes."""
import numpy as np
import torch

from oracle import gln as og

F32, F64 = np.float32, np.float64
CHUNK = 1024                                  # CVPCE_HEADLOSS_CHUNK
# T_ref: the largest relative distance of the fp32 model from the float64 model over the cases below, as test_headloss_cpu.py measures
# it (the regression loss of seven_boxes_k3; the others lie between 3e-9 and 8e-8): the measured value, 1.0690905e-7, with its last digit
# shown rounded up.  The kernel does not enter it.
T_REF = 1.0690906e-7
LOSS_RTOL = 8 * T_REF                         # device losses against the float64 model (DESIGN.md 4d has the reason for the factor)

BOXES_128 = [[4, 6, 38, 41], [50, 10, 90, 92], [20, 60, 47, 120], [70, 70, 125, 100], [3, 90, 14, 126], [60, 2, 66, 9], [0, 0, 128, 128]]
BOXES_TIES = [[-16, -16, 16, 16], [-16, -16, 16, 16], [48, 48, 80, 80]]
GRIDS_128 = [(16, 16), (8, 8), (4, 4), (2, 2), (1, 1)]
GRIDS_96_160 = [(12, 20), (6, 10), (3, 5), (2, 3), (1, 2)]
NUM_ANCHORS = 9


def strides(padded, grids):
    return [(padded[0] // gh, padded[1] // gw) for gh, gw in grids]


def anchors(padded, grids):
    """(A_total,4) float32: level-major, cell-major, then anchor -- the order of the head outputs."""
    return torch.cat(og.grid_anchors(padded, grids)).numpy().astype(F32)


def scaled_boxes(boxes, original, transformed):
    boxes = torch.as_tensor(boxes, dtype=torch.float32).reshape(-1, 4)
    return og.resize_boxes(boxes, original, transformed).numpy().astype(F32)


def iou_matrix(anc, boxes):
    """(A,T) fp32: hg_iou of csrc/iou.h, every operation rounded on its own."""
    a, b = anc[:, None, :], boxes[None, :, :]
    area_a = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_b = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    w = np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])
    h = np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])
    inter = np.where(w < 0, F32(0), w) * np.where(h < 0, F32(0), h)
    out = inter / ((area_b + area_a) - inter)
    assert out.dtype == F32
    return out


def match(anc, boxes):
    """-> (m (A,) int32: box index, -1 background, -2 between; restored (A,) bool: below 0.5 and made foreground by the low-quality rule)."""
    n = anc.shape[0]
    if boxes.shape[0] == 0:
        return np.full(n, -1, np.int32), np.zeros(n, bool)
    iou = iou_matrix(anc, boxes)
    arg = np.argmax(iou, axis=1)                                  # (numpy documents the FIRST occurrence of the maximum)
    val = iou[np.arange(n), arg]
    m = np.where(val >= F32(0.5), arg, np.where(val >= F32(0.4), -2, -1))
    low = (iou == iou.max(axis=0)[None, :]).any(axis=1)           # (IoUs are >= 0 and never NaN here: value equality is bit equality)
    restored = low & (val < F32(0.5))
    m = np.where(low, arg, m)
    return m.astype(np.int32), restored


def model(anc, boxes, labels, logits, regs, D):
    """One image.  anc (A,4), boxes (T,4) scaled, logits (A,K), regs (A,4): fp32; labels (T,) ints; D: F32 or F64, the type of every
    loss operation.  -> dict(matched, counts (foreground, between, restored), classification, bbox_regression)."""
    m, restored = match(anc, boxes)
    fg = m >= 0
    nfg = int(fg.sum())
    den = D(max(1, nfg))
    x = logits.astype(D)
    t = np.zeros_like(x)
    t[np.nonzero(fg)[0], np.asarray(labels, dtype=np.int64)[m[fg]]] = 1
    one = D(1)
    p = one / (one + np.exp(-x))
    ce = (np.maximum(x, D(0)) - x * t) + np.log1p(np.exp(-np.abs(x)))
    p_t = p * t + (one - p) * (one - t)
    alpha_t = D(0.25) * t + D(0.75) * (one - t)
    q = one - p_t
    term = alpha_t * (ce * (q * q))
    assert term.dtype == D
    cls = term[m != -2].sum(dtype=D) / den
    reg = D(0)
    if nfg:
        a, g, r = anc[fg].astype(D), boxes[m[fg]].astype(D), regs[fg].astype(D)
        w, h = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1]
        cx, cy = a[:, 0] + D(0.5) * w, a[:, 1] + D(0.5) * h
        gw, gh = g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        gcx, gcy = g[:, 0] + D(0.5) * gw, g[:, 1] + D(0.5) * gh
        enc = np.stack([(gcx - cx) / w, (gcy - cy) / h, np.log(gw / w), np.log(gh / h)], axis=1)
        assert enc.dtype == D
        reg = np.abs(r - enc).sum(dtype=D) / den
    return {'matched': m, 'counts': (nfg, int((m == -2).sum()), int(restored.sum())), 'classification': float(cls), 'bbox_regression': float(reg)}


def _random_boxes(count, padded, seed):
    """`count` valid boxes with sides of 6 to 70 px whose corners lie on a quarter-pixel grid, all inside a little more than the image."""
    g = torch.Generator().manual_seed(seed)
    w = torch.randint(24, 281, (count,), generator=g).float() / 4
    h = torch.randint(24, 281, (count,), generator=g).float() / 4
    x1 = torch.randint(-32, 4 * padded[1] - 200, (count,), generator=g).float() / 4
    y1 = torch.randint(-32, 4 * padded[0] - 200, (count,), generator=g).float() / 4
    return torch.stack([x1, y1, x1 + w, y1 + h], dim=1).tolist()


def _image(boxes, original, transformed, num_classes, seed):
    labels = [(3 * i + seed) % num_classes for i in range(len(boxes))]
    return {'boxes': boxes, 'labels': labels, 'original': original, 'transformed': transformed}


def _heads(case, seed):
    """seeded head outputs, per level (N,gh,gw,A*K) and (N,gh,gw,A*4) float32: logits around the detector's prior, regressions around 0"""
    g = torch.Generator().manual_seed(seed)
    n, k = len(case['images']), case['num_classes']
    case['cls'] = [torch.randn((n, gh, gw, NUM_ANCHORS * k), generator=g) * 2 - 2 for gh, gw in case['grids']]
    case['reg'] = [torch.randn((n, gh, gw, NUM_ANCHORS * 4), generator=g) * 0.5 for gh, gw in case['grids']]
    return case


def cases():
    """name -> dict(padded, grids, num_classes, images: [dict(boxes, labels, original, transformed)], cls, reg)."""
    out = {}
    for k in (1, 3):
        out[f'seven_boxes_k{k}'] = {'padded': (128, 128), 'grids': GRIDS_128, 'num_classes': k,
                                    'images': [_image(BOXES_128, (128, 128), (128, 128), k, 1)]}
    out['ties'] = {'padded': (128, 128), 'grids': GRIDS_128, 'num_classes': 1, 'images': [_image(BOXES_TIES, (128, 128), (128, 128), 1, 0)]}
    out['no_boxes'] = {'padded': (128, 128), 'grids': GRIDS_128, 'num_classes': 3, 'images': [_image([], (128, 128), (128, 128), 3, 0)]}
    out['chunk_plus_one'] = {'padded': (96, 160), 'grids': GRIDS_96_160, 'num_classes': 2,
                             'images': [_image(_random_boxes(CHUNK + 1, (96, 160), 19), (96, 160), (96, 160), 2, 0)]}
    # a batch: scale factors that are not 1 (and differ per axis), the empty image in the middle
    shrink = lambda boxes, fy, fx: [[x1 / fx, y1 / fy, x2 / fx, y2 / fy] for x1, y1, x2, y2 in boxes]
    out['batch'] = {'padded': (128, 128), 'grids': GRIDS_128, 'num_classes': 3,
                    'images': [_image(shrink(BOXES_128, 1.25, 1.42), (100, 90), (125, 128), 3, 2),
                               _image([], (60, 60), (120, 120), 3, 0),
                               _image(shrink(BOXES_TIES, 2.0, 0.5), (64, 250), (128, 125), 3, 1)]}
    # (the seed 19 of the random boxes is one for which the last index, in the second chunk, is matched: test_headloss_cpu.py asserts it)
    return {name: _heads(c, 11 + i) for i, (name, c) in enumerate(out.items())}


def flat_heads(case, image):
    """(A_total,K) logits and (A_total,4) regressions of one image of a case, in anchor order."""
    k = case['num_classes']
    logits = torch.cat([c[image].reshape(-1, k) for c in case['cls']]).numpy()
    regs = torch.cat([r[image].reshape(-1, 4) for r in case['reg']]).numpy()
    return logits, regs


def run_model(case, D):
    """the model on every image of a case -> list of `model` results"""
    anc = anchors(case['padded'], case['grids'])
    out = []
    for i, img in enumerate(case['images']):
        logits, regs = flat_heads(case, i)
        out.append(model(anc, scaled_boxes(img['boxes'], img['original'], img['transformed']), img['labels'], logits, regs, D))
    return out


_memo = {}


def reference(name):
    """(case, fp32 results, float64 results) of a named case, computed once per process and shared."""
    if name not in _memo:
        case = cases()[name]
        _memo[name] = (case, run_model(case, F32), run_model(case, F64))
    return _memo[name]


CASE_NAMES = ('seven_boxes_k1', 'seven_boxes_k3', 'ties', 'no_boxes', 'chunk_plus_one', 'batch')
