"""Plain restatements of the detections rule (include/cvpce_amd_actuals.h) and the inputs the actuals tests share.
(Not a test module: test_actuals_cpu.py pins the models to `production._nondegenerate` and `planograms_device.graph_threshold`,
test_gpu_actuals.py pins the kernels of csrc/actuals.hip to the models.)

numpy only, written from the header's text: truncation toward zero and integer differences for the kept test, an ordered copy for the
compaction, and np.float32 scalars -- every operation rounded to fp32 on its own -- for the threshold.
"""
import numpy as np

B, PER, G = 8, 300, 24
KS = (1, 3)
# the wave (64) and workgroup-loop (256) boundaries of the ordered compaction, none and all of the slots
COUNTS = (0, 1, 63, 64, 65, 256, 257, 300)
ALL_DEGENERATE = 2                                   # the image of 63 boxes keeps none
ANNOTATIONS = [f'sku{i % 6}' for i in range(G)]      # the gallery of the pipeline tests: 24 items under 6 labels
THRESH_SIZES = (0.5, 0.3)
# named boxes, planted at SPECIAL_SLOTS of every image of at least 64 boxes (the all-degenerate image aside)
SPECIAL = {'fraction_only': ((10.2, 5.0, 10.9, 9.0), False),         # x0 = 10.2, x2 = 10.9: both truncate to 10
           'around_zero': ((-0.5, 5.0, 0.4, 9.0), False),            # -0.5 ... 0.4: both truncate (toward zero) to 0
           'width_one': ((10.9, 5.0, 11.1, 9.0), True),              # 10 and 11 after truncation: a width of exactly 1 is kept
           'height_zero': ((3.0, 7.2, 30.0, 7.9), False),
           'negative': ((50.0, 5.0, 20.0, 9.0), False)}
SPECIAL_SLOTS = {'fraction_only': 3, 'around_zero': 17, 'width_one': 40, 'height_zero': 62, 'negative': 63}


def kept_mask(boxes):
    """boxes (n, 4) f32, finite -> bool (n,): the header's kept test"""
    t = np.trunc(np.asarray(boxes, dtype=np.float64)).astype(np.int64)
    return (t[:, 2] - t[:, 0] > 0) & (t[:, 3] - t[:, 1] > 0)


def model_count(boxes, count):
    per = boxes.shape[1]
    return np.array([int(kept_mask(boxes[i, :min(max(int(c), 0), per)]).sum()) for i, c in enumerate(count)], dtype=np.int32)


def threshold(boxes, thresh_size):
    """thresh_size * ((((max x2 - min x0) + max y3) - min y1) / 2) in fp32, every operation rounded on its own -> np.float32"""
    b = np.asarray(boxes, dtype=np.float32)
    span = (((b[:, 2].max() - b[:, 0].min()) + b[:, 3].max()) - b[:, 1].min()) / np.float32(2)
    assert span.dtype == np.float32
    return np.float32(thresh_size) * span


def model_pack(boxes, count, indices, gallery_label_id, off2, thresh_size):
    """-> (out_boxes (sum2, 4) f32, out_row, out_label (sum2,) i32, thresh (B,) f32, status (B,) i32, rows written (sum2,) bool,
    thresholds written (B,) bool).  Unwritten elements hold 0."""
    b, per = boxes.shape[:2]
    sum2, g = int(off2[-1]) if len(off2) else 0, len(gallery_label_id)
    sum2 = max(sum2, 0)
    out_boxes, out_row, out_label = np.zeros((sum2, 4), np.float32), np.zeros(sum2, np.int32), np.zeros(sum2, np.int32)
    thresh, status = np.zeros(b, np.float32), np.zeros(b, np.int32)
    rows, tw = np.zeros(sum2, bool), np.zeros(b, bool)
    for i in range(b):
        c = min(max(int(count[i]), 0), per)
        keep = np.nonzero(kept_mask(boxes[i, :c]))[0]
        a0 = min(max(int(off2[i]), 0), sum2)
        a1 = min(max(int(off2[i + 1]), a0), sum2)
        bad = False
        for slot, j in enumerate(keep):
            r = int(indices[i, j, 0])
            inside = 0 <= r < g
            bad = bad or not inside
            if slot < a1 - a0:
                out_boxes[a0 + slot], out_row[a0 + slot], rows[a0 + slot] = boxes[i, j], (r if inside else -1), True
                out_label[a0 + slot] = gallery_label_id[r] if inside else 0
        if len(keep):
            thresh[i], tw[i] = threshold(boxes[i, keep], thresh_size), True
        status[i] = 2 if bad else (1 if len(keep) != int(off2[i + 1]) - int(off2[i]) else 0)
    return out_boxes, out_row, out_label, thresh, status, rows, tw


def offsets(lengths):
    off = [0]
    for n in lengths:
        off.append(off[-1] + int(n))
    return np.array(off, dtype=np.int32)


def _degenerate(rng, kind):
    x, y = np.floor(rng.uniform(0, 1500)), np.floor(rng.uniform(0, 1100))
    if kind == 0:                                   # narrower than a pixel, inside one
        return x + 0.1, y, x + 0.8, y + rng.uniform(2, 300)
    if kind == 1:                                   # flatter than a pixel
        return x, y + 0.3, x + rng.uniform(2, 300), y + 0.6
    return x + 40.5, y, x + 2.25, y + 30.0          # x2 < x0


def make_boxes(seed=0):
    """-> (boxes (B, PER, 4) f32, count (B,) i32, degenerate (B, PER) bool as planted).  Slots beyond the count hold NaN."""
    rng = np.random.default_rng(seed)
    boxes = np.full((B, PER, 4), np.nan, dtype=np.float32)
    planted = np.zeros((B, PER), bool)
    for i, c in enumerate(COUNTS):
        for j in range(c):
            # irregular positions: about a fifth of the slots, by the generator
            if i == ALL_DEGENERATE or rng.uniform() < 0.2:
                boxes[i, j], planted[i, j] = _degenerate(rng, int(rng.integers(0, 3))), True
            else:
                x0, y1 = rng.uniform(0, 1500), rng.uniform(0, 1100)
                boxes[i, j] = (x0, y1, x0 + rng.uniform(2, 400), y1 + rng.uniform(2, 300))
        if c >= 64 and i != ALL_DEGENERATE:
            for name, slot in SPECIAL_SLOTS.items():
                boxes[i, slot], planted[i, slot] = SPECIAL[name][0], not SPECIAL[name][1]
    return boxes, np.array(COUNTS, dtype=np.int32), planted


def make_indices(k, seed=1):
    """(B, PER, k) i64: gallery rows in [0, G) inside the count, -1 beyond it"""
    rng = np.random.default_rng(seed + k)
    idx = rng.integers(0, G, size=(B, PER, k)).astype(np.int64)
    for i, c in enumerate(COUNTS):
        idx[i, c:] = -1
    return idx


def label_ids(annotations=ANNOTATIONS):
    """`Classifier._refresh_label_ids` restated: -> (dict annotation -> id, the id of every gallery row (G,) i32)"""
    ids = {}
    rows = [ids.setdefault(a, len(ids)) for a in annotations]
    return ids, np.array(rows, dtype=np.int32)


BOXES, COUNT, PLANTED = make_boxes()
KEPT = model_count(BOXES, COUNT)
OFF2 = offsets(KEPT)


def _threshold_variants(boxes, thresh_size):
    """the same expression re-associated in fp32, and evaluated exactly (float64 holds every intermediate) and rounded once"""
    b = np.asarray(boxes, dtype=np.float32)
    a, m, c, d = b[:, 2].max(), b[:, 0].min(), b[:, 3].max(), b[:, 1].min()
    re = np.float32(thresh_size) * (((a + c) - (m + d)) / np.float32(2))
    fused = np.float32(float(np.float32(thresh_size)) * ((float(a) - float(m) + float(c) - float(d)) / 2))
    return re, fused


def order_sensitive_images(thresh_size):
    """the images whose fp32 threshold is not the value of a re-associated or a fused evaluation"""
    out = []
    for i in range(B):
        keep = kept_mask(BOXES[i, :COUNTS[i]])
        if keep.any():
            want = threshold(BOXES[i, :COUNTS[i]][keep], thresh_size)
            if any(v.tobytes() != want.tobytes() for v in _threshold_variants(BOXES[i, :COUNTS[i]][keep], thresh_size)):
                out.append(i)
    return out


# what this module promises about its own data
assert KEPT[ALL_DEGENERATE] == 0 and KEPT[0] == 0 and all(KEPT[i] > 0 for i in range(B) if i not in (0, ALL_DEGENERATE)), KEPT
assert all(0 < KEPT[i] < COUNTS[i] for i in range(3, B)), KEPT
assert all(order_sensitive_images(t) for t in THRESH_SIZES), 'no threshold of the case set tells the evaluation orders apart'
