"""The Gaussian-map scoring rule of DESIGN.md 4c in numpy, one fp32 operation at a time (not a test module: test_gaussians_cpu.py checks
it against vectors the reference's own `generate_gaussians` and `gaussian_loss` produced, tests/golden/gaussian_targets.pt;
test_gpu_gaussians.py compares csrc/gaussians.hip with it).  Every intermediate is an np.float32, so nothing is contracted or kept wider:
the kernel, built without contraction, performs the same operations and differs only where its expf rounds the last place otherwise.
Also the inputs of the golden file, shared with tests/golden/make_gaussian_golden.py."""
import numpy as np

F = np.float32
METHODS = {'multivariate_normal': 0, 'kant_method': 1, 'simple_and_scaled': 2}
JOINS = {'max': 0, 'addition': 1, 'replacement': 2}
DEFAULT_PARAMS = {'multivariate_normal': (1.0, 0.5, 0.0), 'kant_method': (120, 40), 'simple_and_scaled': (-1.0, 1.0, 6.0)}
LN2 = F(0.6931472)
# T_ref: the largest difference between this model and the reference over the golden cases, measured by test_gaussians_cpu.py
# (9.54e-7 = 8 units in the last place below 1: the reference normalises exp(log_prob) by its maximum, the rule is the closed form),
# rounded up.  The kernel does not enter it.
T_REF = 9.6e-7
TARGET_TOL = 4 * T_REF                      # device targets: the factor is for expf's different last-place rounding


def loss_tolerance(loss):
    """|p - t| <= 2 bounds a squared error's change under a target change of TARGET_TOL by 4 * TARGET_TOL, and with it the mean's; a
    fixed fp32 tree over <= 2^21 terms adds 2e-6 relative."""
    return 4 * TARGET_TOL + 2e-6 * abs(loss)


def kant_table(size=120, sigma=40):
    d = np.arange(size, dtype=np.int64) - size // 2
    d2 = (d[:, None] ** 2 + d[None, :] ** 2).astype(F)
    return np.exp((F(-4.0) * LN2) * d2 / F(sigma * sigma)).astype(F)


def bilinear_taps(out_size, in_size, scale=None):
    """F.interpolate(mode='bilinear', align_corners=False) along one axis -> (i0, i1, l0, l1) per output index."""
    scale = F(in_size) / F(out_size) if scale is None else F(scale)
    src = scale * (np.arange(out_size, dtype=F) + F(0.5)) - F(0.5)
    src = np.where(src < 0, F(0), src).astype(F)
    i0 = np.minimum(src.astype(np.int64), in_size - 1)
    i1 = i0 + (i0 < in_size - 1)
    l1 = (src - i0.astype(F)).astype(F)
    return i0, i1, (F(1) - l1).astype(F), l1


def blend(v00, v01, v10, v11, l0y, l1y, l0x, l1x):
    """the four taps of every output element -> its value (rows: y weights, columns: x weights)"""
    top = (l0x[None, :] * v00 + l1x[None, :] * v01).astype(F)
    bottom = (l0x[None, :] * v10 + l1x[None, :] * v11).astype(F)
    return (l0y[:, None] * top + l1y[:, None] * bottom).astype(F)


def resize(src, h, w):
    hs, ws = src.shape
    y0, y1, ly0, ly1 = bilinear_taps(h, hs)
    x0, x1, lx0, lx1 = bilinear_taps(w, ws)
    return blend(src[y0][:, x0], src[y0][:, x1], src[y1][:, x0], src[y1][:, x1], ly0, ly1, lx0, lx1)


def _min_dist2(c, lo, hi):
    f = np.floor(c)
    a = min(max(f, F(lo)), F(hi - 1))
    b = min(max(f + F(1), F(lo)), F(hi - 1))
    da, db = F(a - c), F(b - c)
    return min(F(da * da), F(db * db))


def render(w, h, boxes, size_reduction=1, method='multivariate_normal', params=None, join='max', tanh=False, table=None):
    """-> (map (h//r, w//r) f32, covered (h//r, w//r) bool: the pixels some box contributes to)."""
    r = int(size_reduction)
    ws, hs = w // r, h // r
    params = DEFAULT_PARAMS[method] if params is None else params
    img = np.full((hs, ws), -1 if tanh else 0, dtype=F)
    covered = np.zeros((hs, ws), dtype=bool)
    if method == 'kant_method' and table is None:
        table = kant_table(*params)
    for box in np.asarray(boxes, dtype=np.int64).reshape(-1, 4):
        x1, y1, x2, y2 = (int(c) // r for c in box)                 # Python's //: towards minus infinity
        xlo, xhi, ylo, yhi = max(x1, 0), min(x2, ws), max(y1, 0), min(y2, hs)
        if x1 == x2 or y1 == y2 or xlo >= xhi or ylo >= yhi:
            continue
        cx, cy = F(F(x1 + x2) * F(0.5)), F(F(y1 + y2) * F(0.5))
        wd, ht = F(abs(x2 - x1)), F(abs(y2 - y1))
        xs, ys = np.arange(xlo, xhi).astype(F), np.arange(ylo, yhi).astype(F)
        if method == 'multivariate_normal':
            peak, vscale = F(params[0]), F(params[1])
            sw, sh = F(wd * vscale), F(ht * vscale)
            vw, vh = F(sw * sw), F(sh * sh)
            dx, dy = (xs - cx).astype(F), (ys - cy).astype(F)
            ex = ((dx * dx - _min_dist2(cx, xlo, xhi)) / vw).astype(F)
            ey = ((dy * dy - _min_dist2(cy, ylo, yhi)) / vh).astype(F)
            val = (peak * np.exp((F(-0.5) * (ey[:, None] + ex[None, :])).astype(F))).astype(F)
        elif method == 'simple_and_scaled':
            lo, hi, div = F(params[0]), F(params[1]), F(params[2])
            sx, sy = F(wd / div), F(ht / div)
            px, py = F(F(2) * F(sx * sx)), F(F(2) * F(sy * sy))
            dx, dy = (xs - cx).astype(F), (ys - cy).astype(F)
            ex, ey = ((dx * dx) / px).astype(F), ((dy * dy) / py).astype(F)
            val = (F(hi - lo) * np.exp(-(ex[None, :] + ey[:, None]).astype(F)) + lo).astype(F)
        else:
            size = table.shape[0]
            i0, i1, li0, li1 = bilinear_taps(xhi - xlo, size, F(size) / F(xhi - xlo))      # x along the table's first axis
            j0, j1, lj0, lj1 = bilinear_taps(yhi - ylo, size, F(size) / F(yhi - ylo))
            # value[y][x] = li0[x] * (lj0[y] * T[i0][j0] + lj1[y] * T[i0][j1]) + li1[x] * (...)
            a = (lj0[:, None] * table[i0][:, j0].T + lj1[:, None] * table[i0][:, j1].T).astype(F)
            b = (lj0[:, None] * table[i1][:, j0].T + lj1[:, None] * table[i1][:, j1].T).astype(F)
            val = (li0[None, :] * a + li1[None, :] * b).astype(F)
        region = img[ylo:yhi, xlo:xhi]
        if join == 'max':
            region[...] = np.maximum(region, val)
        elif join == 'addition':
            region[...] = (region + val).astype(F)
        else:
            region[...] = val
        covered[ylo:yhi, xlo:xhi] = True
    return img, covered


def fused_targets(images, hb, wb, tanh=False, **method):
    """images: [(W0, H0, boxes, r, (h, w))] -> (targets (N,1,hb,wb) f32, touched (N,1,hb,wb) bool: elements with a covered tap)."""
    out = np.full((len(images), 1, hb, wb), -1 if tanh else 0, dtype=F)
    touched = np.zeros(out.shape, dtype=bool)
    for n, (w0, h0, boxes, r, (h, w)) in enumerate(images):
        src, cov = render(w0, h0, boxes, r, tanh=tanh, **method)
        h, w = min(h, hb), min(w, wb)
        if h < 1 or w < 1 or src.size == 0:
            continue
        out[n, 0, :h, :w] = resize(src, h, w)
        y0, y1, _, _ = bilinear_taps(h, src.shape[0])
        x0, x1, _, _ = bilinear_taps(w, src.shape[1])
        touched[n, 0, :h, :w] = cov[y0][:, x0] | cov[y0][:, x1] | cov[y1][:, x0] | cov[y1][:, x1]
    return out, touched


def loss(pred, target, negative_threshold=0.0, positive_threshold=0.1, min_negatives=1000, negatives_per_positive=3, extent=None):
    """One segment of the loss: se in fp32 as the kernel takes it, the sums in float64 -> dict(loss, pos_sum, pos_count, neg_sum,
    neg_count_used, tau_ties: how many negatives equal the threshold value).  extent (rows, cols): the counted corner of a (Hb,Wb) map."""
    pred, target = np.asarray(pred, dtype=F), np.asarray(target, dtype=F)
    if extent is not None:
        pred, target = pred[..., :extent[0], :extent[1]], target[..., :extent[0], :extent[1]]
    d = (pred - target).astype(F)
    se = (d * d).astype(F)
    pos, neg = se[target >= F(positive_threshold)], np.sort(se[target <= F(negative_threshold)])[::-1]
    m = min(max(int(min_negatives), int(negatives_per_positive) * len(pos)), len(neg))
    top = neg[:m].astype(np.float64)
    ps, ns = float(pos.astype(np.float64).sum()), float(top.sum())
    den = len(pos) + m
    return {'loss': (ps + ns) / den if den else float('nan'), 'pos_sum': ps, 'pos_count': len(pos), 'neg_sum': ns, 'neg_count_used': m,
            'tau_ties': int((neg == neg[m - 1]).sum()) if m else 0}


# ---- the golden file's inputs ---------------------------------------------------------------------------------------------------------
BIG = (203, 157)                                 # (W0, H0)
SMALL = (97, 75)
# overlapping, crossing every edge, negative odd coordinates; no zero reduced extent and no empty clip at r = 1 and r = 2
BOXES_BIG = [[10, 12, 60, 50], [40, 30, 120, 90], [-7, -5, 30, 40], [150, 100, 231, 181], [90, -3, 141, 25], [55, 60, 57, 121],
             [101, 71, 160, 131], [-13, 120, 22, 171]]
BOXES_SMALL = [[5, 6, 30, 25], [20, 15, 60, 45], [-7, -5, 15, 20], [70, 50, 111, 91], [45, -3, 71, 13], [27, 30, 29, 61],
               [50, 35, 80, 66], [-13, 60, 11, 85]]
# (simple_and_scaled only) wholly outside with an empty -- not reversed -- range: the reference's arange accepts those
OUTSIDE_SMALL = [[-30, 10, 0, 40], [97, 20, 130, 60], [10, 75, 40, 99]]


def target_cases():
    """-> [(name, dict(w, h, boxes, size_reduction, method, join, tanh))] the reference can run"""
    cases = [('big_mvn_max_r1', dict(w=BIG[0], h=BIG[1], boxes=BOXES_BIG, size_reduction=1, method='multivariate_normal', join='max', tanh=False)),
             ('big_mvn_max_r2', dict(w=BIG[0], h=BIG[1], boxes=BOXES_BIG, size_reduction=2, method='multivariate_normal', join='max', tanh=False))]
    for method in METHODS:
        for join in JOINS:
            if method == 'kant_method' and join == 'addition':
                continue                          # fails in the reference on a broadcast: left to this model
            boxes = BOXES_SMALL + (OUTSIDE_SMALL if method == 'simple_and_scaled' else [])
            for r in ((1, 2) if join == 'max' else (1,)):
                cases.append((f'{method}_{join}_r{r}', dict(w=SMALL[0], h=SMALL[1], boxes=boxes, size_reduction=r, method=method, join=join, tanh=False)))
            if method == 'simple_and_scaled' and join == 'max':
                cases.append((f'{method}_{join}_tanh', dict(w=SMALL[0], h=SMALL[1], boxes=boxes, size_reduction=1, method=method, join=join, tanh=True)))
    return cases


# losses: three images of different sizes in one padded (3,1,48,64) batch; maps = multivariate_normal / max at r = 1
LOSS_HB, LOSS_WB = 48, 64
LOSS_IMAGES = [dict(w=97, h=75, boxes=BOXES_SMALL, size=(96, 128)),
               dict(w=80, h=60, boxes=[[8, 8, 30, 40], [35, 10, 70, 30], [50, 35, 78, 58]], size=(80, 100)),
               dict(w=50, h=50, boxes=[[5, 5, 25, 25], [20, 22, 48, 47]], size=(64, 90))]
LOSS_PARAMS = {
    'defaults': dict(),
    'more_negatives_than_n': dict(min_negatives=10, negatives_per_positive=1),
    'fewer_negatives_than_n': dict(min_negatives=100000),
    'no_positives': dict(),                      # with all-zero maps
    'ties_at_tau': dict(min_negatives=500, negatives_per_positive=0),   # with a constant prediction over the padding
}


def loss_predictions(name):
    """the (3,1,48,64) prediction of a loss case: seeded values in [0, 0.4); 'ties_at_tau' holds 0.5 over every image's padding"""
    rng = np.random.RandomState(1234)
    pred = (rng.rand(len(LOSS_IMAGES), 1, LOSS_HB, LOSS_WB) * 0.4).astype(F)
    if name == 'ties_at_tau':
        for n, im in enumerate(LOSS_IMAGES):
            h, w = im['size'][0] // 2, im['size'][1] // 2
            pad = np.ones((LOSS_HB, LOSS_WB), dtype=bool)
            pad[:h, :w] = False
            pred[n, 0][pad] = F(0.5)
    return pred
