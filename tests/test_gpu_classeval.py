"""The classification harness's comparison on the GPU: the kernel of csrc/classeval.hip equals the torch model
(tests/classeval_cases.py, pinned against the reference's string loop in test_classeval_cpu.py), writes `records` and nothing
else, and `eval_dihe(..., device_eval=True)` / `ClassificationTally` / `dihe eval --device-eval` give the host path's counts exactly."""
import re

import pytest
import torch

import classeval_cases as cc
import footprint

pytestmark = pytest.mark.gpu

PREFILL = 0x5A5A5A5A
# (Q, K, G): the smallest case, an odd one, the wave boundary of the lanes' stride over K, the full ranking of a gallery of 130 (three
# passes of 64 lanes, the last one partial), and a K of the fused matcher; Q = 4 fills a workgroup's four rows, the others do not
SHAPES = ((1, 1, 1), (5, 3, 7), (4, 63, 130), (4, 64, 130), (4, 65, 130), (7, 130, 130), (9, 16, 40))
KNN = (1, 3, 5, 20)


def _launch(cuda, indices, gallery, want):
    records = torch.full((indices.shape[0], 2), PREFILL, dtype=torch.int32, device=cuda)
    torch.ops.cvpce_amd.classeval_rank(indices.to(cuda), gallery.to(cuda), want.to(cuda), records)
    return records.cpu()


# ---------------------------------------------------------------------------------------------------------------------
# 5. the kernel against the model
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('q, k, g', SHAPES)
def test_kernel_equals_the_model(cuda, q, k, g):
    from cvpce_amd import torch_ops_classeval  # noqa: F401
    indices, gallery, want, planted = cc.kernel_case(q, k, g, seed=q * 1000 + k)
    model = cc.model_rank(indices, gallery, want)
    for row, rank in planted.items():                                  # the model itself, on the rows whose answer is known by construction
        assert int(model[row, 0]) == rank, (row, rank)
    if q > 5:
        assert int(model[5, 1]) == -1 and int(indices[5, 0]) == g and (k == 1 or int(indices[5, k - 1]) == -1)
    got = _launch(cuda, indices, gallery, want)
    assert torch.equal(got, model), (got.tolist(), model.tolist())
    # indices outside the gallery change nothing else: the same table with them replaced gives the same other rows
    if q > 5:
        inside = indices.clone()
        inside[5] = 0
        again = _launch(cuda, inside, gallery, want)
        keep = [r for r in range(q) if r != 5]
        assert torch.equal(again[keep], got[keep])


def test_the_planted_ranks_cover_what_they_should():
    seen = {}
    for q, k, g in SHAPES:
        _, _, want, planted = cc.kernel_case(q, k, g, seed=q * 1000 + k)
        seen[(q, k, g)] = planted
        assert q <= 4 or int(want[4]) == -1
    assert seen[(7, 130, 130)] == {0: 0, 1: 129, 2: 65, 3: 130, 4: 130, 6: 128}          # rank 0, K-1, two hits, none, want -1, last pass
    assert seen[(4, 65, 130)][1] == 64 and seen[(4, 64, 130)][1] == 63 and seen[(4, 63, 130)][1] == 62
    assert {q % 4 == 0 for q, _, _ in SHAPES} == {True, False}


# ---------------------------------------------------------------------------------------------------------------------
# 6. footprint
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('q, k, g', ((4, 65, 130), (5, 3, 7)))
def test_footprint(cuda, q, k, g):
    """every element of `records` is written, nothing outside it, none of the inputs"""
    from cvpce_amd import torch_ops_classeval  # noqa: F401
    indices, gallery, want, _ = cc.kernel_case(q, k, g, seed=q * 1000 + k)
    ins = [footprint.put(t, cuda) for t in (indices, gallery, want)]
    out = footprint.out((q, 2), torch.int32, cuda)
    run = lambda: torch.ops.cvpce_amd.classeval_rank(ins[0][0], ins[1][0], ins[2][0], out[0])
    res = footprint.check(run, ins, [out])
    assert torch.equal(res[0].cpu(), cc.model_rank(indices, gallery, want))


# ---------------------------------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_the_op_refuses_bad_calls_before_any_launch(cuda):
    from cvpce_amd import torch_ops_classeval  # noqa: F401
    indices, gallery, want, _ = cc.kernel_case(5, 3, 7, seed=1)
    d = dict(indices=indices.to(cuda), gallery=gallery.to(cuda), want=want.to(cuda))
    records = torch.full((5, 2), PREFILL, dtype=torch.int32, device=cuda)
    rank = lambda **kw: torch.ops.cvpce_amd.classeval_rank(kw.get('indices', d['indices']), kw.get('gallery', d['gallery']),
                                                            kw.get('want', d['want']), kw.get('records', records))
    for bad in (dict(indices=d['indices'].to(torch.int32)), dict(want=d['want'].to(torch.int64)), dict(gallery=d['gallery'].float()),
                dict(records=records.to(torch.int64)), dict(indices=d['indices'].t().contiguous().t()), dict(want=d['want'][:-1]),
                dict(want=torch.cat((d['want'], d['want']))[::2]), dict(records=records[:-1]), dict(indices=d['indices'][:, 0]),
                dict(gallery=d['gallery'][:0])):
        with pytest.raises(RuntimeError, match='cvpce_classeval_rank'):
            rank(**bad)
    torch.cuda.synchronize()
    assert bool((records == PREFILL).all()), 'a refused call launched'
    rank()
    assert torch.equal(records.cpu(), cc.model_rank(indices, gallery, want))
    # Q = 0 launches nothing and is no error
    torch.ops.cvpce_amd.classeval_rank(torch.empty((0, 3), dtype=torch.int64, device=cuda), d['gallery'], torch.empty(0, dtype=torch.int32, device=cuda),
                                       torch.empty((0, 2), dtype=torch.int32, device=cuda))


# ---------------------------------------------------------------------------------------------------------------------
# 8. - 10. end to end
# ---------------------------------------------------------------------------------------------------------------------
ANNS = [f'p{i}' for i in range(12)]
ANNS[7] = ANNS[2]                                                       # two gallery items share an annotation
_WORLD = {}


def _paste(shelf, product, x, y, w, h):
    import torch.nn.functional as F
    shelf[:, y:y + h, x:x + w] = F.interpolate(((product + 1) / 2)[None], size=(h, w), mode='bilinear', align_corners=False)[0]
    return [x, y, x + w, y + h]


def _world(cuda):
    """a seeded MAC-VGG16, a gallery of 12 under 11 annotations, three shelf images of different sizes -- a float one with 4 boxes, an
    8-bit one with 5 (one of them reaching past the image's edge) and one without boxes -- and the host path's own label lists"""
    if _WORLD:
        return _WORLD
    from cvpce_amd import classification_eval, datautils, ops, production, synthetic
    enc = synthetic.synthetic_macvgg(seed=1).to(cuda)
    gal = synthetic.gallery_images(12, seed=5)
    g = torch.Generator().manual_seed(11)
    a = torch.full((3, 300, 840), 0.3) + 0.05 * torch.rand(3, 300, 840, generator=g)
    boxes_a = [_paste(a, gal[3], 10, 20, 256, 256), _paste(a, gal[2], 300, 40, 100, 180), _paste(a, gal[7], 450, 10, 60, 200),
               _paste(a, gal[9], 560, 150, 200, 90)]
    b = torch.full((3, 411, 530), 0.4) + 0.05 * torch.rand(3, 411, 530, generator=g)
    boxes_b = [_paste(b, gal[0], 5, 7, 128, 128), _paste(b, gal[11], 140, 30, 77, 211), _paste(b, gal[5], 230, 300, 190, 101),
               _paste(b, gal[1], 250, 10, 256, 256), _paste(b, gal[6], 431, 280, 99, 131)]
    boxes_b[4] = [431, 280, 530 + 25, 411 + 9]                          # reaches past the right and the lower edge: clipped to the image
    b = (b.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    c = synthetic.shelf_image(12, 200, 333)
    images = [a, b, c]
    boxes = [torch.tensor(boxes_a), torch.tensor(boxes_b), torch.zeros((0, 4), dtype=torch.int64)]
    sampleset = synthetic.TensorGallery(gal, ANNS)
    clf = production.Classifier(enc, sampleset, device=cuda, emb_device=cuda, batch_size=8, k=max(KNN))
    clf5 = production.Classifier.from_embedding(enc, clf.embedding, ANNS, device=cuda, emb_device=cuda, batch_size=8, k=5)

    def host_lists(classifier):
        out = []
        for img, bx in zip(images, boxes):
            bx = classification_eval.clip_boxes_to_image(bx, datautils.image_hw(img))
            out.append(classifier.classify(ops.crop_resize(ops.input_image(img, cuda), bx.to(cuda), datautils.CLASSIFICATION_IMAGE_SIZE, mode=0))
                       if len(bx) else [])
        return out

    top5 = host_lists(clf5)
    # each box's target from the host path's own k = 5 list: its rank 0, 1 or 4 entry, a gallery annotation outside the list, or a
    # string no gallery item has
    plan = [[0, 1, 4, 'none'], ['nowhere', 4, 'none', 1, 0]]
    targets, ranks = [], []
    for lists, kinds in zip(top5, plan):
        row = []
        for got, kind in zip(lists, kinds):
            if kind == 'nowhere':
                row.append(cc.NOWHERE)
            elif kind == 'none':
                row.append(next(x for x in ANNS if x not in got))
            else:
                row.append(got[kind])
            ranks.append(got.index(row[-1]) if row[-1] in got else None)
        targets.append(row)
    targets.append([])
    _WORLD.update(enc=enc, sampleset=sampleset, images=images, boxes=boxes, targets=targets, ranks=ranks, clf=clf, top5=top5,
                  host=host_lists(clf), testset=[(img, t, bx) for img, t, bx in zip(images, targets, boxes)])
    return _WORLD


def test_the_world_holds_the_ranks_it_is_meant_to(cuda):
    w = _world(cuda)
    print('first ranks in the host path\'s k = 5 lists:', w['ranks'])
    assert {0, 1, 4, None} <= set(w['ranks']) and w['ranks'].count(None) >= 3
    assert all(len(l) == 5 for lists in w['top5'] for l in lists) and all(len(l) == 12 for lists in w['host'] for l in lists)      # K = min(20, G)
    assert [len(b) for b in w['boxes']] == [4, 5, 0] and w['images'][1].dtype == torch.uint8
    assert int(w['boxes'][1][4, 2]) > w['images'][1].shape[1] and int(w['boxes'][1][4, 3]) > w['images'][1].shape[0]


@pytest.mark.parametrize('window', (2, 8))
def test_eval_dihe_with_the_switch_returns_the_host_paths_dict(cuda, window):
    from cvpce_amd import classification_eval
    w = _world(cuda)
    if 'off' not in w:
        w['off'] = classification_eval.eval_dihe(w['enc'], w['sampleset'], w['testset'], 8, k=KNN, device_eval=False)
    on = classification_eval.eval_dihe(w['enc'], w['sampleset'], w['testset'], 8, k=KNN, device_eval=True, window=window)
    print(f'window {window}: device {on}, host {w["off"]}')
    assert on == w['off']
    flat_t = [t for row in w['targets'] for t in row]
    flat_p = [p for lists in w['host'] for p in lists]
    assert on == cc.string_loop(flat_t, flat_p, KNN)['accuracy']
    assert 0 < on[1] < on[5] < on[20] < 1                                # ranks 0, 1 and 4 and the string nowhere all count


@pytest.mark.parametrize('window', (2, 8))
def test_the_tally_equals_the_string_loop(cuda, window):
    from cvpce_amd import ops
    from cvpce_amd.device_classification import ClassificationTally
    w = _world(cuda)
    tally = ClassificationTally(w['clf'], KNN)
    items = [(ops.input_image(img, cuda), bx, t) for img, t, bx in w['testset']]
    for s in range(0, len(items), window):
        tally.update(*zip(*items[s:s + window]))
    got = tally.compute()
    want = cc.string_loop([t for row in w['targets'] for t in row], [p for lists in w['host'] for p in lists], KNN)
    assert got == want
    assert tally.host_routed == 0 and want['missed'] and want['confusion'] and want['total'] == 9
    assert tally.compute() == want                                       # (callable again)


def test_eval_dihe_prints_the_references_report(cuda, capsys):
    from cvpce_amd import classification_eval
    w = _world(cuda)
    classification_eval.eval_dihe(w['enc'], w['sampleset'], w['testset'], 8, k=KNN, verbose=True, device_eval=True, window=2)
    out = capsys.readouterr().out
    assert 'Total annotations: 9, Correctly guessed: {' in out and 'Most missed: ' in out and out.count(': Commonly mistaken for ') >= 1


# ---- 9. no host synchronisation in update() ----------------------------------------------------------------------------
def test_update_does_not_synchronise_the_host(cuda):
    from cvpce_amd import ops
    from cvpce_amd.device_classification import ClassificationTally
    w = _world(cuda)
    items = [(ops.input_image(img, cuda), bx, t) for img, t, bx in w['testset']]
    windows = [items[0:1], items[1:2], items[2:3]]                       # the third one has no boxes: nothing is launched
    warm = ClassificationTally(w['clf'], KNN)
    for win in windows:
        warm.update(*zip(*win))                                          # (first use: allocator growth, the cached tables)
    want = warm.compute()
    tally = ClassificationTally(w['clf'], KNN)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        with pytest.raises(RuntimeError):
            torch.ones(1, device=cuda).sum().item()                      # the mode is armed
        for win in windows:
            tally.update(*zip(*win))
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert tally.compute() == want


# ---- 10. annotations that do not hash -----------------------------------------------------------------------------------
class _Key:
    """a hashable target that equals the one-element list annotation of the same name (the host loop keys its dicts by the target)"""

    def __init__(self, name):
        self.name = name

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return other == [self.name] if isinstance(other, list) else isinstance(other, _Key) and other.name == self.name


def test_unhashable_annotations_take_the_host_path(cuda):
    """list annotations leave the classifier without an id space: the window goes through `Classifier.classify` and the string
    comparison, as with the switch off (exact pastes: every box is its own product, so the loop never keys a dict by a list)"""
    from cvpce_amd import classification_eval, ops, production, synthetic
    from cvpce_amd.device_classification import ClassificationTally
    w = _world(cuda)
    gal = synthetic.gallery_images(12, seed=5)
    names = [f'q{i}' for i in range(12)]
    shelf = torch.full((3, 300, 1100), 0.3)
    boxes, targets = [], []
    for j, i in enumerate((3, 7, 0, 11)):
        boxes.append(_paste(shelf, gal[i], 10 + j * 270, 20, 256, 256))
        targets.append(_Key(names[i]))
    testset = [(shelf, targets, torch.tensor(boxes))]
    sampleset = synthetic.TensorGallery(gal, [[n] for n in names])
    off = classification_eval.eval_dihe(w['enc'], sampleset, testset, 8, k=(1, 3), device_eval=False)
    on = classification_eval.eval_dihe(w['enc'], sampleset, testset, 8, k=(1, 3), device_eval=True, window=2)
    assert on == off == {1: 1.0, 3: 1.0}
    odd = production.Classifier.from_embedding(w['enc'], w['clf'].embedding, [[n] for n in names], device=cuda, emb_device=cuda, batch_size=8, k=3)
    assert odd.label_ids is None
    tally = ClassificationTally(odd, (1, 3))
    tally.update([ops.input_image(shelf, cuda)], [torch.tensor(boxes)], [targets])
    assert tally.host_routed == 1 and tally.compute()['accuracy'] == off


# ---------------------------------------------------------------------------------------------------------------------
# 11. the command
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def tree(cuda, tmp_path_factory):
    """the GP-like file tree of tests/test_gpu_cli.py, the part `dihe eval` reads: six products, two test images of three boxes"""
    from PIL import Image
    from cvpce_amd import synthetic
    root = tmp_path_factory.mktemp('classeval_cli')
    to_img = lambda t: Image.fromarray((t.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy())
    torch.save({'model_state_dict': synthetic.synthetic_macvgg(seed=1).state_dict()}, root / 'dihe.tar')
    gal = (synthetic.gallery_images(6, seed=5) + 1) / 2
    names = []
    for i in range(6):
        d = root / 'Training' / 'Food' / f'Cat{i % 2}'
        d.mkdir(parents=True, exist_ok=True)
        to_img(gal[i]).save(d / f'{10 + i}.png')
        names.append(f'Food/Cat{i % 2}/{10 + i}')
    (root / 'Training' / 'Background').mkdir()
    to_img(gal[0]).save(root / 'Training' / 'Background' / 'bg.png')
    (root / 'Testing' / 'store1' / 'images').mkdir(parents=True)
    (root / 'ann').mkdir()
    for img_id, picks, wrong in ((15, (3, 1, 4), None), (16, (0, 5, 2), 1)):
        shelf = torch.full((3, 300, 840), 0.3)
        rows = []
        for j, i in enumerate(picks):
            x = 10 + j * 270
            shelf[:, 20:276, x:x + 256] = gal[i]
            named = names[(i + 1) % 6] if j == wrong else names[i]        # one annotation names another product: a miss at k = 1
            rows.append(f'{named}.jpg, {x}, 20, {x + 256}, 276')
        to_img(shelf).save(root / 'Testing' / 'store1' / 'images' / f'store1_{img_id}.jpg', format='PNG')
        (root / 'ann' / f's1_{img_id}.csv').write_text('\n'.join(rows) + '\n')
    return root


def test_the_command_prints_the_same_accuracy_with_the_switch(tree):
    from click.testing import CliRunner
    from cvpce_amd.cli import cli
    args = ['dihe', 'eval', '--img-dir', tree / 'Training', '--test-imgs', tree / 'Testing', '--annotations', tree / 'ann',
            '--enc-weights', tree / 'dihe.tar', '--knn', '1', '--knn', '3', '--knn', '6']
    outs = []
    for switch in ([], ['--device-eval']):
        r = CliRunner().invoke(cli, [str(a) for a in args + switch], catch_exceptions=False)
        assert r.exit_code == 0, r.output
        outs.append(r.output)
    lines = [re.search(r'--> accuracy (\{.*\})', o).group(0) for o in outs]
    print(lines)
    assert lines[0] == lines[1]
    acc = eval(re.search(r'--> accuracy (\{.*\})', outs[1]).group(1))
    assert acc[1] == 5 / 6 and acc[6] == 1.0
    assert 'Commonly mistaken for' in outs[1] and 'Commonly mistaken for' not in outs[0]
