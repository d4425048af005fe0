"""Cases and a plain restatement of the comparator's tail rule (not a test module): `model_tail` restates
csrc/homography.hip in numpy float64 / float32 with elementwise operations only -- every sum whose order matters is an explicit
loop in the rule's order (no np.sum, np.dot or @ on floating-point data).  test_homography_device_cpu.py pins the restatement
against `planograms._dlt` and `planograms.finalize_via_ransac`; test_gpu_homography_device.py holds the kernels to it bit for bit.

The hypotheses are independent, so the restatement carries them as one array axis: an elementwise operation on an array of K
values is K separately rounded operations, exactly what K threads do."""
import math

import numpy as np
import torch

import planogram_device_cases as cases

OK, NONE, INVALID = 0, 1, 2
THREADS = 256
SQRT2 = 1.4142135623730951
DEGENERATE = 1e-12
PIVOT_MIN = 1e-12
THETA_MAX = 1e150
SWEEPS = 10
H_TRUE = np.array([[1.7, 0.05, 30.0], [-0.03, 1.6, 12.0], [1e-5, 2e-5, 1.0]])          # tests/test_planograms_cpu.py's perspective map
F32, F64 = np.float32, np.float64


# ---------------------------------------------------------------------------------------------------------------------
# the rule
# ---------------------------------------------------------------------------------------------------------------------
def hash32(seed, t, draw):
    """counter hash of (seed, t, draw): murmur3's finaliser over seed + 0x9E3779B9 * (4 t + draw + 1), all modulo 2^32; t: int array"""
    m = 0xFFFFFFFF
    x = (int(seed) + 0x9E3779B9 * (np.asarray(t, dtype=np.uint64) * 4 + draw + 1)) & m
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & m
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & m
    x ^= x >> 16
    return x


def sample(seed, t, n):
    """Floyd's method -> (len(t), 4) distinct indices below n, in drawing order"""
    t = np.asarray(t)
    s = np.zeros((len(t), 4), dtype=np.int64)
    for d in range(4):
        j = n - 4 + d
        v = (hash32(seed, t, d) % np.uint64(j + 1)).astype(np.int64)
        seen = np.zeros(len(t), dtype=bool)
        for e in range(d):
            seen |= s[:, e] == v
        s[:, d] = np.where(seen, j, v)
    return s


def points_of(pairs, b1, b2):
    """-> (src, dst), each (n, 2) float32: top-left corners, bottom-right corners, centres formed in fp32; m = 1 appends (x2, y1), (x0, y3)"""
    e, a = [p[0] for p in pairs], [p[1] for p in pairs]

    def three(b):
        centres = np.stack(((b[:, 0] + b[:, 2]) / F32(2), (b[:, 1] + b[:, 3]) / F32(2)), axis=1)
        pts = np.concatenate((b[:, :2], b[:, 2:], centres))
        return np.concatenate((pts, b[:, (2, 1)], b[:, (0, 3)])) if len(b) == 1 else pts
    return three(b1[e]), three(b2[a])


def _strided_sum(vals, mask):
    """thread j adds its elements j, j + 256, ... in that order; the 256 partial sums are then added in index order"""
    part = np.zeros(THREADS, dtype=F64)
    for r in range(0, len(vals), THREADS):
        seg, mk = vals[r:r + THREADS], mask[r:r + THREADS]
        part[:len(seg)] = np.where(mk, part[:len(seg)] + seg, part[:len(seg)])
    total = 0.0
    for j in range(THREADS):
        total = total + float(part[j])
    return total


def normalise(pts, mask=None):
    """Hartley normalisation of the masked points -> ((cx, cy, k), ok)"""
    mask = np.ones(len(pts), dtype=bool) if mask is None else mask
    x, y = pts[:, 0].astype(F64), pts[:, 1].astype(F64)
    count = float(int(mask.sum()))
    with np.errstate(all='ignore'):
        cx, cy = F64(_strided_sum(x, mask)) / F64(count), F64(_strided_sum(y, mask)) / F64(count)
        dx, dy = x - cx, y - cy
        s = F64(_strided_sum(np.sqrt(dx * dx + dy * dy), mask)) / F64(count)
        k = F64(SQRT2) / s
    return (cx, cy, k), bool(s >= DEGENERATE)


def denormalise(hn, na, nb):
    """hn: list of 9 arrays (or scalars) -> (h: list of 9, ok)"""
    (acx, acy, ak), (bcx, bcy, bk) = na, nb
    with np.errstate(all='ignore'):
        tx, ty = ak * acx, ak * acy
        m = [None] * 9
        for r in range(3):
            m[3 * r] = hn[3 * r] * ak
            m[3 * r + 1] = hn[3 * r + 1] * ak
            m[3 * r + 2] = (hn[3 * r + 2] - hn[3 * r] * tx) - hn[3 * r + 1] * ty
        h = [None] * 9
        for j in range(3):
            h[j] = m[j] / bk + bcx * m[6 + j]
            h[3 + j] = m[3 + j] / bk + bcy * m[6 + j]
            h[6 + j] = m[6 + j]
        d = h[8]
        ok = np.abs(d) >= DEGENERATE
        h = [v / d for v in h]
        for v in h:
            ok = ok & np.isfinite(v)
    return h, ok


def minimal(s, src, dst, na, nb):
    """the K homographies through the sampled correspondences s (K, 4) -> (h: list of 9 arrays of K, ok array)"""
    (acx, acy, ak), (bcx, bcy, bk) = na, nb
    k_ = len(s)
    zero, one = np.zeros(k_), np.ones(k_)
    a = [[None] * 9 for _ in range(8)]
    with np.errstate(all='ignore'):
        for i in range(4):
            x, y = (src[s[:, i], 0].astype(F64) - acx) * ak, (src[s[:, i], 1].astype(F64) - acy) * ak
            u, v = (dst[s[:, i], 0].astype(F64) - bcx) * bk, (dst[s[:, i], 1].astype(F64) - bcy) * bk
            a[2 * i] = [x, y, one, zero, zero, zero, -(u * x), -(u * y), u]
            a[2 * i + 1] = [zero, zero, zero, x, y, one, -(v * x), -(v * y), v]
        ok = np.ones(k_, dtype=bool)
        for c in range(8):
            for r in range(c + 1, 8):
                sw = np.abs(a[r][c]) > np.abs(a[c][c])
                for j in range(c, 9):
                    top, low = a[c][j], a[r][j]
                    a[c][j], a[r][j] = np.where(sw, low, top), np.where(sw, top, low)
            ok &= np.abs(a[c][c]) >= PIVOT_MIN
            for r in range(c + 1, 8):
                f = a[r][c] / a[c][c]
                for j in range(c + 1, 9):
                    a[r][j] = a[r][j] - f * a[c][j]
        hn = [None] * 9
        for i in range(7, -1, -1):
            acc = a[i][8]
            for j in range(i + 1, 8):
                acc = acc - a[i][j] * hn[j]
            hn[i] = acc / a[i][i]
        hn[8] = one
    h, fine = denormalise(hn, na, nb)
    return h, ok & fine


def errors(h, src, dst):
    """reprojection errors in pixels: h list of 9 arrays of K (or scalars) -> (K, n) (or (n,))"""
    x, y, u, v = (c.astype(F64) for c in (src[:, 0], src[:, 1], dst[:, 0], dst[:, 1]))
    h = [np.asarray(c, dtype=F64)[..., None] for c in h]
    with np.errstate(all='ignore'):
        px, py, pw = (h[0] * x + h[1] * y) + h[2], (h[3] * x + h[4] * y) + h[5], (h[6] * x + h[7] * y) + h[8]
        ex, ey = px / pw - u, py / pw - v
        return np.sqrt(ex * ex + ey * ey)


def ransac(src, dst, reproj_threshold, seed, hypotheses, chunk=4096):
    """-> (winner, its count, h of every hypothesis is not kept): highest count, lowest t at equal counts; no model counts 0"""
    n = len(src)
    na, oka = normalise(src)
    nb, okb = normalise(dst)
    counts = np.zeros(hypotheses, dtype=np.int64)
    if oka and okb:
        for t0 in range(0, hypotheses, chunk):
            t = np.arange(t0, min(t0 + chunk, hypotheses))
            h, ok = minimal(sample(seed, t, n), src, dst, na, nb)
            inl = errors(h, src, dst) < F64(reproj_threshold)
            counts[t] = np.where(ok, inl.sum(axis=1), 0)
    winner = int(np.argmax(counts))                                     # (the first of the largest)
    return winner, int(counts[winner]), (na, nb, oka and okb)


def hypothesis(src, dst, seed, t, norms):
    """hypothesis t alone -> (h as 9 floats, ok)"""
    na, nb, ok = norms
    h, fine = minimal(sample(seed, np.array([t]), len(src)), src, dst, na, nb)
    return [F64(c[0]) for c in h], bool(fine[0]) and ok


def jacobi_smallest(ata):
    """cyclic Jacobi with a fixed sweep count over a symmetric 9 x 9 matrix (list of lists of floats) -> the eigenvector of the
    smallest eigenvalue (the lowest index among equal ones)"""
    a = [[float(v) for v in row] for row in ata]
    vec = [[1.0 if i == j else 0.0 for j in range(9)] for i in range(9)]
    for _ in range(SWEEPS):
        for p in range(8):
            for q in range(p + 1, 9):
                apq = a[p][q]
                if apq == 0.0:
                    continue
                app, aqq = a[p][p], a[q][q]
                theta = (aqq - app) / (2.0 * apq)
                at = abs(theta)
                t = 0.5 / at if at > THETA_MAX else 1.0 / (at + math.sqrt(at * at + 1.0))
                t = -t if theta < 0.0 else t
                c = 1.0 / math.sqrt(t * t + 1.0)
                s = t * c
                for r in range(9):
                    vrp, vrq = vec[r][p], vec[r][q]
                    vec[r][p], vec[r][q] = c * vrp - s * vrq, s * vrp + c * vrq
                    if r != p and r != q:
                        arp, arq = a[r][p], a[r][q]
                        a[r][p] = a[p][r] = c * arp - s * arq
                        a[r][q] = a[q][r] = s * arp + c * arq
                a[p][p], a[q][q] = app - t * apq, aqq + t * apq
                a[p][q] = a[q][p] = 0.0
    imin = 0
    for i in range(1, 9):
        if a[i][i] < a[imin][imin]:
            imin = i
    return [vec[i][imin] for i in range(9)]


def refit(src, dst, mask):
    """the DLT over the masked correspondences, normalised over them -> (3 x 3 float64 array, ok)"""
    na, oka = normalise(src, mask)
    nb, okb = normalise(dst, mask)
    (acx, acy, ak), (bcx, bcy, bk) = na, nb
    acc = np.zeros((9, 9), dtype=F64)
    with np.errstate(all='ignore'):
        for k in np.nonzero(mask)[0].tolist():                                # index order
            x, y = (F64(src[k, 0]) - acx) * ak, (F64(src[k, 1]) - acy) * ak
            u, v = (F64(dst[k, 0]) - bcx) * bk, (F64(dst[k, 1]) - bcy) * bk
            r1 = np.array([-x, -y, -1.0, 0.0, 0.0, 0.0, u * x, u * y, u], dtype=F64)
            r2 = np.array([0.0, 0.0, 0.0, -x, -y, -1.0, v * x, v * y, v], dtype=F64)
            acc = acc + (r1[:, None] * r1[None, :] + r2[:, None] * r2[None, :])
        hn = jacobi_smallest(acc.tolist())
        h, ok = denormalise([F64(v) for v in hn], na, nb)
    return np.array([float(v) for v in h]).reshape(3, 3), bool(ok) and oka and okb


def project(h, b1):
    """every expected box through H rounded to fp32, in fp32 -> (n1, 4) float32"""
    f = h.astype(F32).reshape(9)
    with np.errstate(all='ignore'):
        def corner(x, y):
            w = (f[6] * x + f[7] * y) + f[8]
            return ((f[0] * x + f[1] * y) + f[2]) / w, ((f[3] * x + f[4] * y) + f[5]) / w
        x0, y0 = corner(b1[:, 0], b1[:, 1])
        x1, y1 = corner(b1[:, 2], b1[:, 3])
    return np.stack((x0, y0, x1, y1), axis=1).astype(F32)


def iou_matrix(a, b):
    """metrics.box_iou's expression in fp32, (P, 4), (T, 4) -> (P, T)"""
    with np.errstate(all='ignore'):
        area_a, area_b = (a[:, 2] - a[:, 0]) * (a[:, 3] - a[:, 1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        w = np.minimum(a[:, None, 2], b[None, :, 2]) - np.maximum(a[:, None, 0], b[None, :, 0])
        h = np.minimum(a[:, None, 3], b[None, :, 3]) - np.maximum(a[:, None, 1], b[None, :, 1])
        inter = np.where(w < 0, F32(0), w) * np.where(h < 0, F32(0), h)
        return inter / ((area_a[:, None] + area_b[None, :]) - inter)


def claim(positions, b2, lab1, lab2, iou_threshold):
    """detection j is matched iff some expected box of its label has IoU >= threshold with it, and is claimed by the lowest such
    box; an expected box is matched iff it claims a detection -> (matched_expected, matched_actual) bool"""
    lab1, lab2 = np.asarray(lab1), np.asarray(lab2)
    ok = (lab1[:, None] == lab2[None, :]) & (iou_matrix(positions, b2).astype(F64) >= F64(iou_threshold))
    matched_actual = ok.any(axis=0)
    first = ok.argmax(axis=0)
    matched_expected = np.zeros(len(lab1), dtype=bool)
    matched_expected[first[matched_actual]] = True
    return matched_expected, matched_actual


def label_ids(l1, l2):
    ids = {}
    return [ids.setdefault(l, len(ids)) for l in l1], [ids.setdefault(l, len(ids)) for l in l2]


def model_tail(b1, l1, b2, l2, pairs, reproj_threshold=10.0, iou_threshold=0.5, seed=0, hypotheses=2048):
    """The whole rule for one image.  b1, b2: (n, 4) float32 (tensor or array), l1, l2: labels, pairs: [(expected, actual)] in
    growth order -> dict: status, H (3 x 3 float64), winner, winner_count, final_count, matched_expected, matched_actual (bool),
    expected_positions (float32), and for the tests winner_mask, final_mask, points."""
    b1 = np.ascontiguousarray(np.asarray(b1, dtype=F32)).reshape(-1, 4)
    b2 = np.ascontiguousarray(np.asarray(b2, dtype=F32)).reshape(-1, 4)
    n1, n2 = len(b1), len(b2)
    res = {'status': OK, 'H': np.zeros((3, 3)), 'winner': 0, 'winner_count': 0, 'final_count': 0,
           'matched_expected': np.zeros(n1, dtype=bool), 'matched_actual': np.zeros(n2, dtype=bool),
           'expected_positions': np.zeros((n1, 4), dtype=F32), 'winner_mask': None, 'final_mask': None, 'points': None}

    def end(status):
        res['status'] = status
        return res
    pairs = [(int(e), int(a)) for e, a in pairs]
    if any(not (0 <= e < n1 and 0 <= a < n2) for e, a in pairs):
        return end(INVALID)
    if not pairs:
        return end(NONE)
    src, dst = points_of(pairs, b1, b2)
    res['points'] = (src, dst)
    if len(src) < 4 or not (np.isfinite(b1).all() and np.isfinite(b2).all()):
        return end(NONE)
    winner, _, norms = ransac(src, dst, reproj_threshold, seed, hypotheses)
    h, ok = hypothesis(src, dst, seed, winner, norms)
    mask = (errors(h, src, dst) < F64(reproj_threshold)) & ok
    if int(mask.sum()) < 4:
        return end(NONE)
    hr, ok = refit(src, dst, mask)
    if not ok:
        return end(NONE)
    final = errors(list(hr.reshape(9)), src, dst) < F64(reproj_threshold)
    pos = project(hr, b1)
    id1, id2 = label_ids(l1, l2)
    me, ma = claim(pos, b2, id1, id2, iou_threshold)
    res.update(H=hr, winner=winner, winner_count=int(mask.sum()), final_count=int(final.sum()), matched_expected=me, matched_actual=ma,
               expected_positions=pos, winner_mask=mask, final_mask=final)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------------------------------------------------
def through(h, boxes):
    """boxes (n, 4) float32 tensor mapped corner by corner through the 3 x 3 map h (float64) -> float32 tensor"""
    b = boxes.double().numpy()
    out = []
    for x, y in ((b[:, 0], b[:, 1]), (b[:, 2], b[:, 3])):
        w = h[2, 0] * x + h[2, 1] * y + h[2, 2]
        out += [(h[0, 0] * x + h[0, 1] * y + h[0, 2]) / w, (h[1, 0] * x + h[1, 1] * y + h[1, 2]) / w]
    return torch.tensor(np.stack(out, axis=1), dtype=torch.float32)


def tail_case(m, kind='clean', seed=0, extra=3):
    """An (expected, actual) pair with a matching of m pairs in a shuffled growth order.
      clean        the detections are the boxes scaled 1.7x, shifted and jittered by up to 1 px; pair k is (node, the same node)
      permuted     the same, 20 % of the pairs (at least one) point at another pair's detection
      perspective  the detections are the boxes through H_TRUE, jittered by up to 1 px
      overlap      a dense grid (pitch 40 x 60 under 80 x 120 boxes) with three labels: same-label neighbours overlap at IoU 0.33
    -> dict(b1, l1, b2, l2, pairs, wrong = the positions in `pairs` that were permuted)"""
    g = torch.Generator().manual_seed(1000 * seed + m)
    n = m + extra
    if kind == 'overlap':
        cols = max(2, int(math.ceil(math.sqrt(n))))
        b1, l1 = cases.grid(-(-n // cols), cols, seed, pitch=(40, 60), size=(80, 120))        # neighbours at IoU 0.33
        b1, l1 = b1[:n].contiguous(), [cases.NAMES[cases.NAMES.index(l) % 3] for l in l1[:n]]
    else:
        b1, l1 = cases.scene(n, seed)
    if kind == 'perspective':
        b2 = through(H_TRUE, b1)
    else:
        b2 = b1 * 1.7 + torch.tensor([30.0, 12.0, 30.0, 12.0])
    b2 = (b2 + (torch.rand(n, 4, generator=g) * 2 - 1)).contiguous()
    l2 = list(l1)
    order = torch.randperm(n, generator=g)[:m].tolist()
    actual = list(order)
    wrong = []
    if kind == 'permuted' and m >= 2:
        wrong = sorted(torch.randperm(m, generator=g)[:max(2, m // 5)].tolist())
        for a, b in zip(wrong, wrong[1:] + wrong[:1]):
            actual[a] = order[b]
    return {'b1': b1, 'l1': l1, 'b2': b2, 'l2': l2, 'pairs': list(zip(order, actual)), 'wrong': wrong}
