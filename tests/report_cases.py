"""Plain restatements of the comparator's report rule (include/cvpce_amd_report.h) and the inputs the tests share.
(Not a test module: test_report_cpu.py pins the numpy model against `PlanogramComparator.report`'s host path, test_gpu_report.py
pins the kernels against the model.)  The expected side of every scene is reclass_cases.py's."""
import numpy as np
import torch

import reclass_cases as rc
from reclass_cases import F32, INVALID, NONE, OK  # noqa: F401

DETECTED, RECOVERED, MISSING, OUT_OF_VIEW, UNCHECKED, PENDING = range(6)
MAX_NODES = 1024


# ---------------------------------------------------------------------------------------------------------------------
# the rule in numpy
# ---------------------------------------------------------------------------------------------------------------------
def iou_row(a, b):
    """hg_iou of one position a (4,) with the boxes b (n, 4), fp32, every operation rounded on its own: fminf / fmaxf drop a NaN,
    the two comparisons with 0 keep one"""
    a, b = np.asarray(a, dtype=F32), np.asarray(b, dtype=F32).reshape(-1, 4)
    with np.errstate(all='ignore'):
        area_a, area_b = (a[2] - a[0]) * (a[3] - a[1]), (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
        w = np.fmin(a[2], b[:, 2]) - np.fmax(a[0], b[:, 0])
        h = np.fmin(a[3], b[:, 3]) - np.fmax(a[1], b[:, 1])
        inter = np.where(w < 0, F32(0), w) * np.where(h < 0, F32(0), h)
        return (inter / ((area_a + area_b) - inter)).astype(F32)


def model_positions(status, matched_expected, matched_actual, positions, boxes, off1, off2, image, actual_row=None, iou_threshold=0.5):
    """-> dict(outcome, occupant, occupant_row (sumN1,) i32, occupant_iou (sumN1,) f32, stray (sumN2,) i32, rows1 (sumN1,) bool,
    rows2 (sumN2,) bool: the rows the rule writes)"""
    sum1, sum2 = len(matched_expected), len(matched_actual)
    out = {'outcome': np.zeros(sum1, dtype=np.int32), 'occupant': np.zeros(sum1, dtype=np.int32), 'occupant_iou': np.zeros(sum1, dtype=F32),
           'occupant_row': np.zeros(sum1, dtype=np.int32), 'stray': np.zeros(sum2, dtype=np.int32), 'rows1': np.zeros(sum1, dtype=bool),
           'rows2': np.zeros(sum2, dtype=bool)}
    for p in range(len(status)):
        a0, a1, b0, b1 = off1[p], off1[p + 1], off2[p], off2[p + 1]
        if status[p] != OK or a1 - a0 > MAX_NODES or b1 - b0 > MAX_NODES:
            continue
        h, w, enabled = image[p]
        free = np.asarray(matched_actual[b0:b1]) == 0
        taken = np.zeros(b1 - b0, dtype=bool)
        valid = rc.clamp_and_validity(positions[a0:a1], h, w)[1]
        for e in range(a1 - a0):
            code, occ, occ_iou = DETECTED, -1, F32(-1)
            if matched_expected[a0 + e] == 0:
                code = UNCHECKED if not enabled else PENDING if valid[e] else OUT_OF_VIEW
                iou = iou_row(positions[a0 + e], boxes[b0:b1])
                with np.errstate(invalid='ignore'):
                    ok = free & (iou.astype(np.float64) >= iou_threshold)                        # (false on NaN)
                if ok.any():
                    occ = int(np.nonzero(ok & (iou == iou[ok].max()))[0][0])                     # the lowest index among equals
                    occ_iou = iou[occ]
                    taken[occ] = True
            out['outcome'][a0 + e], out['occupant'][a0 + e], out['occupant_iou'][a0 + e] = code, occ, occ_iou
            out['occupant_row'][a0 + e] = actual_row[b0 + occ] if occ >= 0 and actual_row is not None else -1
        out['stray'][b0:b1] = free & ~taken
        out['rows1'][a0:a1], out['rows2'][b0:b1] = True, True
    return out


def model_reclass(expected_index, count, slot_row, indices, distances, gallery_label_id, expected_label_id, off1, status, cap, outcome):
    """-> (outcome (sumN1,) i32, seen_row (sumN1,) i32, seen_distance (sumN1,) f32, written (sumN1,) bool)"""
    sum1, m, g = len(outcome), len(indices), len(gallery_label_id)
    outcome = np.array(outcome, dtype=np.int32)
    seen_row, seen_distance, written = np.zeros(sum1, dtype=np.int32), np.zeros(sum1, dtype=F32), np.zeros(sum1, dtype=bool)
    for p in range(len(status)):
        a0, a1 = off1[p], off1[p + 1]
        if status[p] != OK or a1 - a0 > cap:
            continue
        first, recovered = {}, set()
        for s in range(min(max(int(count[p]), 0), cap)):
            e, row = int(expected_index[p][s]), int(slot_row[p][s])
            if not 0 <= e < a1 - a0 or not 0 <= row < m:
                continue
            j = int(indices[row][0])
            if not 0 <= j < g:
                continue
            first.setdefault(e, s)
            if expected_label_id[a0 + e] >= 0 and gallery_label_id[j] == expected_label_id[a0 + e]:
                recovered.add(e)
        for e in range(a1 - a0):
            seen_row[a0 + e], seen_distance[a0 + e] = -1, -1
            if outcome[a0 + e] == PENDING:
                if e in first:
                    row = int(slot_row[p][first[e]])
                    seen_row[a0 + e], seen_distance[a0 + e] = int(indices[row][0]), distances[row][0]
                outcome[a0 + e] = RECOVERED if e in recovered else MISSING
        written[a0:a1] = True
    return outcome, seen_row, seen_distance, written


# ---------------------------------------------------------------------------------------------------------------------
# inputs
# ---------------------------------------------------------------------------------------------------------------------
SPECIAL_POSITIONS = 6           # planted at the end of an image of at least 24 positions and 10 detections
SPECIAL_DETECTIONS = 10


def report_image(n1, n2, kind, h, w, seed, status=OK, enabled=1):
    """One image of a `report_positions` launch: reclass_cases.plan_image's expected side plus n2 detections -- jittered copies of
    the positions, about 40 % of them claimed.  Where the image is large enough (kind is not 'none_missing'), its last positions and
    detections are the rule's edge cases:
      * a detection at IoU exactly 0.5 with its position (the occupant) and one just below (a stray),
      * two positions sharing one occupant,
      * two identical detections on one position (the lower index is the occupant, the other a stray),
      * a detection with a NaN coordinate, two zero-area detections, a zero-area position under one of them (IoU 0 / 0),
      * a detection that would be the best occupant but is claimed."""
    im = rc.plan_image(n1, kind, h, w, seed, status, enabled)
    g = torch.Generator().manual_seed(seed + 2000)
    pos = im['positions']
    src = (torch.arange(n2) * 7) % n1
    base = torch.nan_to_num(pos[src], nan=50.0, posinf=float(w), neginf=0.0)
    boxes = (base + (torch.rand(n2, 4, generator=g) - 0.5) * 12 + 0.0).to(torch.float32)
    claimed = (torch.rand(n2, generator=g) < 0.4).to(torch.int32)
    if kind != 'none_missing' and n1 >= 24 and n2 >= SPECIAL_DETECTIONS:
        e, j = n1 - SPECIAL_POSITIONS, n2 - SPECIAL_DETECTIONS
        f = lambda *v: torch.tensor(v, dtype=torch.float32)
        pos[e], boxes[j], boxes[j + 1] = f(16, 16, 80, 48), f(16, 16, 48, 48), f(16, 16, 47.5, 48)
        pos[e + 1] = pos[e + 2] = f(100, 100, 160, 180)
        boxes[j + 2] = f(101, 101, 161, 181)
        pos[e + 3] = f(200, 50, 260, 130)
        boxes[j + 3] = boxes[j + 4] = f(202, 52, 262, 132)
        boxes[j + 5], boxes[j + 6], boxes[j + 7] = f(float('nan'), 10, 60, 60), f(30, 30, 30, 90), f(40, 40, 40, 40)
        pos[e + 4] = f(40, 40, 40, 40)
        pos[e + 5] = f(300, 200, 360, 280)
        boxes[j + 8], boxes[j + 9] = f(300, 200, 360, 280), f(302, 202, 362, 282)
        im['matched'][e:] = 0
        claimed[j:] = 0
        claimed[j + 8] = 1
    im.update(boxes=boxes.contiguous(), claimed=claimed)
    return im


def report_tables(images, with_rows=True):
    """-> the host tensors of one `report_positions` launch, in the op's order of inputs"""
    t, _ = rc.plan_tables(images)
    off = [0]
    for im in images:
        off.append(off[-1] + len(im['claimed']))
    g = torch.Generator().manual_seed(len(images))
    return {'status': t['status'], 'matched_expected': t['matched_expected'], 'matched_actual': torch.cat([im['claimed'] for im in images]),
            'expected_positions': t['expected_positions'], 'actual_boxes': torch.cat([im['boxes'] for im in images]).contiguous(),
            'off1': t['off1'], 'off2': torch.tensor(off, dtype=torch.int32), 'image': t['image'],
            'actual_row': torch.randint(0, 24, (off[-1],), generator=g).to(torch.int32) if with_rows else None}


def run_model_positions(t, iou_threshold=0.5):
    return model_positions(t['status'].tolist(), t['matched_expected'].numpy(), t['matched_actual'].numpy(), t['expected_positions'].numpy(),
                           t['actual_boxes'].numpy(), t['off1'].tolist(), t['off2'].tolist(), t['image'].tolist(),
                           None if t['actual_row'] is None else t['actual_row'].numpy(), iou_threshold)


def reclass_case(images, outcome, k, seed=0, gallery=24, labels=6):
    """The inputs of one `report_reclass` launch for the images of a `report_positions` launch whose outcomes are `outcome`: the
    model's own plan, a match result of k columns with distances, rows and indices outside their ranges, one position named by two
    slots, labels no gallery item has -> (host tensors in the op's order of inputs, cap)"""
    g = torch.Generator().manual_seed(seed)
    t, cap = rc.plan_tables(images)
    _, index, count, written = rc.model_plan(t['status'].numpy(), t['matched_expected'].numpy(), t['expected_positions'].numpy(), t['off1'].tolist(),
                                             t['image'].tolist(), cap)
    total = int(count.sum())
    m = max(total - 3, 0)                                                                  # the last three rows lie beyond the match result
    slot_row = np.full(index.shape, -1, dtype=np.int32)
    slot_row[written] = np.arange(total)
    indices = torch.randint(0, gallery, (m, k), generator=g, dtype=torch.int64)
    distances = torch.rand(m, k, generator=g).to(torch.float32)
    index = index.copy()
    busiest = int(np.argmax(count))
    if count[busiest] >= 8 and m > 8:
        indices[3, 0], indices[5, 0] = gallery, -1                                          # indices outside the gallery
        slot_row[busiest, 1] = -7                                                           # a negative row
        index[busiest, 0], index[busiest, 2] = MAX_NODES + 1, -1                            # indices outside the image
        index[busiest, 6] = index[busiest, 5]                                               # one position, two slots: the lower decides
    index[~written] = 0x5A5A5A5A
    sum1 = int(t['off1'][-1])
    expected_id = torch.randint(0, labels, (sum1,), generator=g).to(torch.int32)
    expected_id[::7] = -1                                                                  # labels no gallery item has
    host = {'expected_index': torch.from_numpy(index), 'count': torch.from_numpy(count), 'slot_row': torch.from_numpy(slot_row), 'indices': indices,
            'distances': distances, 'gallery_label_id': torch.tensor([i % labels for i in range(gallery)], dtype=torch.int32),
            'expected_label_id': expected_id, 'off1': t['off1'], 'status': t['status'], 'outcome': torch.as_tensor(outcome, dtype=torch.int32).clone()}
    return host, cap


RECLASS_ORDER = ('expected_index', 'count', 'slot_row', 'indices', 'distances', 'gallery_label_id', 'expected_label_id', 'off1', 'status')


def run_model_reclass(host, cap):
    return model_reclass(host['expected_index'].numpy(), host['count'].numpy(), host['slot_row'].numpy(), host['indices'].numpy(),
                         host['distances'].numpy(), host['gallery_label_id'].tolist(), host['expected_label_id'].tolist(), host['off1'].tolist(),
                         host['status'].tolist(), cap, host['outcome'].numpy())


# the windows the tests share: the wave (64), workgroup (256) and capacity (1024) edges on both sides, every status
WINDOW = ((1, 1, 'all_missing', 480, 640), (63, 65, 'mixed', 333, 517), (64, 64, 'all_missing', 480, 640), (65, 63, 'edges', 333, 517),
          (257, 257, 'mixed', 480, 640), (1024, 1, 'mixed', 480, 640), (1, 1024, 'all_missing', 480, 640), (64, 257, 'none_missing', 333, 517),
          (1024, 1024, 'edges', 2161, 3847), (30, 12, 'edges', 480, 640))
_CACHE = {}


def window_images():
    """WINDOW's images with an image without a homography, a disabled one and an invalid one among them; made once, never changed"""
    if 'images' not in _CACHE:
        images = [report_image(n1, n2, kind, h, w, 100 + k) for k, (n1, n2, kind, h, w) in enumerate(WINDOW)]
        images.insert(2, report_image(40, 40, 'all_missing', 480, 640, 7, status=NONE))
        images.insert(5, report_image(40, 40, 'mixed', 480, 640, 8, enabled=0))
        images.append(report_image(40, 40, 'all_missing', 480, 640, 9, status=INVALID))
        _CACHE['images'] = images
    return _CACHE['images']


def small_images():
    """the images of the window with at most 257 boxes on either side (the footprint test's)"""
    return [im for im in window_images() if len(im['matched']) <= 257 and len(im['claimed']) <= 257]


# ---------------------------------------------------------------------------------------------------------------------
# whole scenes for the comparator
# ---------------------------------------------------------------------------------------------------------------------
def comparator_scene(k, scale=1.7, cut=None, strays=True):
    """A gridded planogram of 24 boxes against detections made from it (synthetic.perturbed_detections, nothing dropped or mislabelled
    there): every 9th detection is withheld, every 7th carries a label of its own (it sits on its position unclaimed: an occupant),
    every 11th expected label is one no gallery item has, two detections lie below the shelf (strays), and with `cut` the detections
    beyond that x are withheld and the image ends there (their positions are out of view)
    -> (expected, actual, (h, w) of the image)"""
    from cvpce_amd import synthetic
    eb, el = synthetic.planogram_grid(4, 6, 100 + k)
    ab, al = synthetic.perturbed_detections(eb, el, 200 + k, scale=scale, drop=0.0, mislabel=0.0)
    assert len(al) == len(el) == 24
    far = ab[:, 2:].amax(dim=0)
    keep = [i for i in range(24) if i % 9 != 4 and (cut is None or float(ab[i, 0]) < cut)]
    al = [('a_product_of_its_own' if i % 7 == 3 else l) for i, l in enumerate(al)]
    boxes, labels = ab[keep], [al[i] for i in keep]
    if strays:
        y = float(far[1]) + 20
        boxes = torch.cat((boxes, torch.tensor([[40.0, y, 120.0, y + 110.0], [200.0, y, 280.0, y + 110.0]])))
        labels = labels + [el[0], 'a_product_of_its_own']
    expected = {'boxes': eb, 'labels': [('not_in_the_gallery' if i % 11 == 5 else l) for i, l in enumerate(el)]}
    h, w = int(far[1]) + 160, int(cut if cut is not None else far[0] + 8)
    return expected, {'boxes': boxes.contiguous(), 'labels': labels}, (h, w)
