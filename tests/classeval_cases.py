"""Cases for the classification harness's device comparison (not a test module): a few-line torch model of
`cvpce_classeval_rank` (include/cvpce_amd_classeval.h), the reference's string loop (cvpce/classification_eval.py:28-42) restated
literally, seeded label cases for the two to be compared on, and planted index tables for the kernel."""
import torch

NOWHERE = 'label-on-no-gallery-row'
LONE = 777                          # the label id only the last gallery row of a kernel case carries


def model_rank(indices, gallery_label_id, want):
    """indices (Q,K) int64, gallery_label_id (G,) int32, want (Q,) int32 -> records (Q,2) int32"""
    q, k = indices.shape
    g = gallery_label_id.numel()
    inside = (indices >= 0) & (indices < g)
    label = torch.where(inside, gallery_label_id.to(torch.int64)[indices.clamp(0, g - 1)], torch.full_like(indices, -1))
    hit = inside & (label == want.to(torch.int64)[:, None]) & (want[:, None] >= 0)
    first = torch.where(hit, torch.arange(k).expand(q, k), torch.full((q, k), k)).min(dim=1).values
    return torch.stack((first, label[:, 0]), dim=1).to(torch.int32)


def string_loop(targets, predictions, k):
    """classification_eval.py:12-48 over one flat list of boxes: a1 the wanted annotation, a2 the list of neighbours' annotations"""
    total, correct = 0, {knn: 0 for knn in k}
    missed, confusion, per_ann = {}, {}, {}
    total += len(targets)
    for a1, a2 in zip(targets, predictions):
        if a1 not in per_ann:
            per_ann[a1] = 0
        per_ann[a1] += 1
        for knn in k:
            if a1 in a2[:knn]:
                correct[knn] += 1
        if a1 != a2[0]:
            if a1 not in missed:
                missed[a1] = 0
                confusion[a1] = {}
            if a2[0] not in confusion[a1]:
                confusion[a1][a2[0]] = 0
            missed[a1] += 1
            confusion[a1][a2[0]] += 1
    return {'accuracy': {knn: c / total for knn, c in correct.items()}, 'total': total, 'correct': correct, 'per_ann': per_ann,
            'missed': missed, 'confusion': confusion}


def label_space(annotations):
    """`Classifier._refresh_label_ids`: annotation -> id, and every gallery row's id"""
    ids = {}
    rows = [ids.setdefault(a, len(ids)) for a in annotations]
    return ids, torch.tensor(rows, dtype=torch.int32)


GALLERY = ['a', 'b', 'a', 'c', 'd', 'e', 'b', 'f', 'g', 'h', 'a', 'i']          # rows 0, 2 and 10 share a label, as do 1 and 6


def label_case(seed, q=80, k=4):
    """A seeded window: every row's K nearest gallery rows (distinct, as a ranking has them) and a target chosen row by row -- the
    annotation at a rank of the row, one of the gallery's that the row does not hold, or one no gallery row has.
    -> (targets, indices (Q,K) int64, predictions as the host path's label lists)"""
    g = torch.Generator().manual_seed(seed)
    n = len(GALLERY)
    indices = torch.stack([torch.randperm(n, generator=g)[:k] for _ in range(q)]).to(torch.int64)
    predictions = [[GALLERY[j] for j in row] for row in indices.tolist()]
    targets = []
    for r, got in enumerate(predictions):
        kind = r % (k + 2)
        if kind < k:
            targets.append(got[kind])
        elif kind == k:
            absent = [a for a in GALLERY if a not in got]
            targets.append(absent[r % len(absent)])
        else:
            targets.append(NOWHERE)
    return targets, indices, predictions


def kernel_case(q, k, g, seed):
    """Planted rows for the kernel, where the case has them (row r exists iff r < q; the last gallery row alone carries LONE):
      0  the wanted label at rank 0                      1  LONE at rank K-1 only (the last, possibly partial, pass of the lanes)
      2  LONE twice, at K // 2 and K-1: K // 2 wins      3  LONE wanted, not among the neighbours
      4  want = -1                                       5  indices[5][0] = G and indices[5][K-1] = -1 (K > 1)
      6  LONE at the first rank of the last pass         7 ...  random
    -> (indices (Q,K) int64, gallery_label_id (G,) int32, want (Q,) int32, {row: the first rank it must get})"""
    gen = torch.Generator().manual_seed(seed)
    common = max(1, g - 1)                                        # rows 0 .. common-1 carry the shared labels
    gallery = torch.randint(0, max(1, common // 3), (g,), generator=gen).to(torch.int32)
    if g > 1:
        gallery[g - 1] = LONE
    indices = torch.randint(0, common, (q, k), generator=gen).to(torch.int64)
    want = gallery[torch.randint(0, common, (q,), generator=gen)].clone()
    planted = {}
    want[0] = gallery[indices[0, 0]]
    planted[0] = 0
    if g > 1:
        if q > 1:
            indices[1, k - 1], want[1], planted[1] = g - 1, LONE, k - 1
        if q > 2:
            indices[2, k - 1], indices[2, k // 2], want[2], planted[2] = g - 1, g - 1, LONE, k // 2
        if q > 3:
            want[3], planted[3] = LONE, k
        if q > 6:
            first_of_last_pass = (k - 1) // 64 * 64
            indices[6, first_of_last_pass], want[6], planted[6] = g - 1, LONE, first_of_last_pass
    if q > 4:
        want[4], planted[4] = -1, k
    if q > 5:
        indices[5, 0] = g
        if k > 1:
            indices[5, k - 1] = -1
    return indices, gallery, want, planted
