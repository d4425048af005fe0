"""The compliance pictures on the GPU: csrc/render.hip equals the plain restatement of the picture rule (tests/render_cases.py,
pinned on the host in test_render_cpu.py) byte for byte and writes only the canvases' bytes; `SceneRenderer.render` is one launch and
no wait; the atlas holds the model's reductions; `pictures_batch` gives `report_batch`'s reports and the same pictures on every route."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import footprint
import render_cases as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN = ('canvases', 'base', 'box', 'src', 'colour', 'thickness', 'atlas', 'atlas_rows')
PREFILL = 0x5A


def _launch(cuda, t, background):
    """the kernel on plain tensors, the output prefilled with a pattern -> the flat output on the host"""
    from cvpce_amd import torch_ops_render  # noqa: F401
    d = {k: torch.from_numpy(t[k]).to(cuda) for k in IN}
    out = torch.full((t['out_bytes'],), PREFILL, dtype=torch.uint8, device=cuda)
    torch.ops.cvpce_amd.render_canvases(d['canvases'], t['total_tiles'], d['base'] if d['base'].numel() else None, d['box'], d['src'], d['colour'],
                                        d['thickness'], d['atlas'], d['atlas_rows'], background, out)
    return out.cpu().numpy()


def _covered(t):
    m = np.zeros(t['out_bytes'], dtype=bool)
    for off, h, w in t['spans']:
        m[off:off + h * w * 3] = True
    return m


def _assert_canvases(flat, t, want, what):
    for c, ((off, h, w), img) in enumerate(zip(t['spans'], want)):
        got = flat[off:off + h * w * 3].reshape(h, w, 3)
        bad = (got != img).any(axis=2)
        assert not bad.any(), (what, c, (h, w), int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), img[bad][:4].tolist())
    assert (flat[~_covered(t)] == PREFILL).all(), (what, 'a byte between the canvases was written')


@pytest.fixture(scope='module')
def window():
    win = rc.window()
    return win, rc.run_model(win)


def test_the_kernel_equals_the_model_byte_for_byte(cuda, window):
    win, want = window
    for align in (1, 4):                  # back to back (rows at odd addresses: the byte path) and at dword offsets (the dword stores)
        t = rc.tables(win, align=align)
        _assert_canvases(_launch(cuda, t, win['background']), t, want, f'align {align}')
    # another background colour changes the uncovered pixels alone
    t = rc.tables(win)
    other = rc.run_model(dict(win, background=0x010203))
    _assert_canvases(_launch(cuda, t, 0x010203), t, other, 'background')


def test_a_canvas_launched_alone_gives_the_bytes_it_gives_inside_the_window(cuda, window):
    win, want = window
    for c in range(len(win['canvases'])):
        t = rc.tables(win, only=[c])
        _assert_canvases(_launch(cuda, t, win['background']), t, [want[c]], f'canvas {c} alone')


def test_footprint_of_the_entry_point(cuda, window):
    """the output arena is prefilled: every canvas byte is written and no byte outside the canvases; the atlas, the bases, the items and
    both tables sit between guard bands whose fill never reaches a pixel -- the window holds the bad `src` rows, a canvas that asks for a
    base it does not have and boxes far outside the canvases"""
    from cvpce_amd import torch_ops_render  # noqa: F401
    win, want = window
    t = rc.tables(win, align=4)
    ins = {k: footprint.put(torch.from_numpy(t[k]), cuda) for k in IN}
    out = footprint.out((t['out_bytes'],), torch.uint8, cuda)
    run = lambda: torch.ops.cvpce_amd.render_canvases(ins['canvases'][0], t['total_tiles'], ins['base'][0], ins['box'][0], ins['src'][0], ins['colour'][0],
                                                      ins['thickness'][0], ins['atlas'][0], ins['atlas_rows'][0], win['background'], out[0])
    covered = _covered(t)
    assert not covered.all()                                        # (the padding between the canvases must stay unwritten)
    model = np.full(t['out_bytes'], PREFILL, dtype=np.uint8)
    for (off, h, w), img in zip(t['spans'], want):
        model[off:off + h * w * 3] = img.reshape(-1)
    # a byte whose value IS the prefill pattern cannot be told from an unwritten one: no claim there, the comparison below covers it
    must = torch.from_numpy(covered & (model != PREFILL))
    res = footprint.check(run, list(ins.values()), [out], written=[(must, torch.from_numpy(covered))])
    assert np.array_equal(res[0].cpu().numpy(), model)


def _counter():
    spec = importlib.util.spec_from_file_location('bench_planogram_compare', os.path.join(ROOT, 'tools', 'bench_planogram_compare.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Atlas:
    def __init__(self, images, device):
        from cvpce_amd import rendering as rd
        rows, _ = rd.atlas_layout([im.shape[:2] for im in images])
        self.data = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(device)
        self.rows = torch.tensor(rows, dtype=torch.int32).to(device)


def test_render_is_one_launch_and_no_wait(cuda, window):
    from cvpce_amd import rendering as rd
    win, want = window
    renderer = rd.SceneRenderer(_Atlas(win['atlas'], cuda))
    cs = win['canvases']
    lists = [rd.Items(*(torch.from_numpy(c[k]).to(cuda) for k in ('box', 'src', 'colour', 'thickness'))) for c in cs]
    hws = [c['hw'] for c in cs]
    bases = [None if c['base'] is None else torch.from_numpy(c['base']).to(cuda) for c in cs]
    renderer.render(lists, hws, bases, win['background'])            # (allocator)
    torch.cuda.synchronize()
    with _counter().WindowCounter() as n:
        views = renderer.render(lists, hws, bases, win['background'])
    print(f'render: {n.kernels} launches, {n.waits} waits, {n.torch_device_ops} other device operators')
    assert n.kernels == 1 and n.waits == 0
    assert len(views) == len(cs) and all(v.is_cuda and v.dtype == torch.uint8 and tuple(v.shape) == hw + (3,) for v, hw in zip(views, hws))
    assert len({v.untyped_storage().data_ptr() for v in views}) == 1                      # views of one flat buffer
    for c, (v, img) in enumerate(zip(views, want)):
        assert np.array_equal(v.cpu().numpy(), img), c
    # float planes as a base become bytes by floor(clamp(x, 0, 1) * 255 + 0.5); bases that are views of one allocation are read where they lie
    planes = torch.rand(3, 5, 7, generator=torch.Generator().manual_seed(3)) * 1.5 - 0.25
    got = renderer.render([lists[1]], [(5, 7)], [planes])[0].cpu()
    assert torch.equal(got, rd.float_image_bytes(planes))
    pool = torch.randint(0, 256, (2, 6, 9, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(4)).to(cuda)
    whole = rd._items(torch.tensor([[0.0, 0, 9, 6]]), rd.R.SRC_BASE, 0, 0)
    got = renderer.render([whole, whole], [(6, 9), (6, 9)], [pool[1], pool[0]])
    assert torch.equal(got[0], pool[1]) and torch.equal(got[1], pool[0])
    assert renderer.render([], []) == []


def test_the_atlas_holds_the_models_reductions(cuda):
    from cvpce_amd import rendering as rd, synthetic
    g = torch.Generator().manual_seed(9)
    sizes = ((256, 256), (200, 31), (128, 128), (17, 255), (1, 1))
    byte_items = [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g) for h, w in sizes]
    float_items = synthetic.gallery_images(5, seed=31)
    for name, images, as_bytes in (('bytes', byte_items, byte_items), ('float', float_items, [rd.gallery_float_bytes(im) for im in float_items])):
        gallery = synthetic.TensorGallery(images)
        atlas = rd.ThumbnailAtlas(gallery, gallery.annotations, cuda, max_side=128)
        assert len(atlas) == 5 and atlas.rows.dtype == torch.int32 and tuple(atlas.rows.shape) == (5, 3)
        for r, im in enumerate(as_bytes):
            h, w = rd.reduced_hw(im.shape[0], im.shape[1], 128)
            assert max(h, w) <= 128 and tuple(atlas.image(r).shape) == (h, w, 3)
            assert np.array_equal(atlas.image(r).cpu().numpy(), rc.resample(im.numpy(), h, w)), (name, r)
        kept = rd.ThumbnailAtlas(gallery, None, cuda, num_workers=2, max_side=None)
        assert all(torch.equal(kept.image(r).cpu(), im) for r, im in enumerate(as_bytes)), name
        assert kept.data.numel() == sum(im.numel() for im in as_bytes) and atlas.data.numel() < kept.data.numel()
    with pytest.raises(ValueError):
        rd.ThumbnailAtlas(synthetic.TensorGallery(byte_items), ['not', 'the', 'classifier', 's', 'rows'], cuda)


# ---------------------------------------------------------------------------------------------------------------------
# through the evaluator
# ---------------------------------------------------------------------------------------------------------------------
_PIPE = {}
SCALE, SHIFT, WINDOW, GALLERY, SIDE = 1.2, (30.3, 12.3), 3, 24, 512


def _pipeline(cuda):
    """A small synthetic pipeline and a planted window, made once: 3 images of 512^2 with 24 boxes each (a 4 x 6 grid photographed at
    another scale), every 9th detection withheld, every 11th expected label one no gallery item has.  The gallery's 24 annotations are
    all different, so a label's first gallery row is the row the matcher found.  The detections are the planogram's boxes scaled and
    shifted with no jitter, and the shift keeps every projected coordinate a tenth of a pixel from an integer: the host's homography
    and the device's refit the same exact correspondences, so their positions agree to rounding (the tail rule) and the
    integer extents of the picture rule are the same on every route -- with jittered detections the two estimators keep different
    inliers and the rings of the annotated picture move by a pixel between the host route and the device routes."""
    if 'clf' not in _PIPE:
        from cvpce_amd import production, rendering as rd, synthetic
        bench = _counter()
        det = synthetic.synthetic_gln(seed=0, detections_per_img=40).to(cuda)
        enc = synthetic.synthetic_macvgg(seed=1).to(cuda)
        gallery = synthetic.TensorGallery(synthetic.gallery_images(GALLERY, seed=17))
        clf = production.Classifier(enc, gallery, device=cuda, emb_device=cuda, batch_size=8)
        pg = production.ProposalGenerator(det, device=cuda, confidence_threshold=0.5)
        imgs = [synthetic.shelf_image(70 + k, SIDE, SIDE).to(cuda) for k in range(WINDOW)]
        grids = [synthetic.planogram_grid(4, 6, 100 + k, cell=(40, 60), gap=(6, 14)) for k in range(WINDOW)]
        full = [synthetic.perturbed_detections(eb, el, 200 + k, scale=SCALE, shift=SHIFT, jitter=0.0, drop=0.0, mislabel=0.0)[0] for k, (eb, el) in enumerate(grids)]
        assert all(float(b.max()) < SIDE for b in full)
        assert all(float(((b - b.round()).abs()).min()) > 0.05 for b in full)

        def planted(boxes):
            packed = torch.zeros((WINDOW, det.detections_per_img, 4))
            for k, b in enumerate(boxes):
                packed[k, :len(b)] = b
            return packed.to(cuda), torch.tensor([len(b) for b in boxes], dtype=torch.int32, device=cuda)

        def evaluator(cmp, boxes, **kw):
            ev = bench.PlantedDetectionsEvaluator(pg, clf, cmp, **kw)
            ev._pipeline().planted = planted(boxes)
            return ev
        all_dets = evaluator(production.PlanogramComparator(), full).detect_and_classify_batch(imgs)
        assert all(len(labels) == 24 for _, labels in all_dets)
        planos = [{'boxes': eb, 'labels': [('not_in_the_gallery' if i % 11 == 5 else l) for i, l in enumerate(labels)]}
                  for (eb, _), (_, labels) in zip(grids, all_dets)]
        withheld = [b[[i for i in range(24) if i % 9 != 4]].contiguous() for b in full]
        atlas = rd.ThumbnailAtlas(gallery, clf.annotations, cuda, max_side=64)
        _PIPE.update(clf=clf, imgs=imgs, planos=planos, withheld=withheld, evaluator=evaluator, atlas=atlas, bench=bench)
    return _PIPE


def test_pictures_batch_gives_the_reports_and_the_same_pictures_on_every_route(cuda):
    from cvpce_amd import production, rendering as rd
    from test_gpu_report import SEEN_DISTANCE_BOUND, _same_reports
    p = _pipeline(cuda)
    imgs, planos, atlas = p['imgs'], p['planos'], p['atlas']
    renderer = rd.SceneRenderer(atlas)
    on = dict(device_graphs=True, device_tail=True)
    routes = (('host', dict(), dict()), ('device_graphs + device_tail', on, dict()),
              ('all switches', dict(on, device_reclass=True), dict(device_detections=True)))
    first = None
    for name, switches, more in routes:
        ev = p['evaluator'](production.PlanogramComparator(**switches), p['withheld'], **more)
        want = ev.report_batch(imgs, planos)
        got = ev.pictures_batch(imgs, planos, renderer)
        assert len(got) == WINDOW and all(isinstance(pic, rd.CompliancePictures) for _, pic in got)
        _same_reports([rep for rep, _ in got], want, name, SEEN_DISTANCE_BOUND)
        if name == 'all switches':
            assert ev.detections_host_routed == 0
        pics = [[getattr(pic, n).cpu() for n in rd.CompliancePictures.NAMES] for _, pic in got]
        if first is None:
            first = pics
            reports = want
            assert all(r.status == 'ok' for r in reports)
            dets = ev.detect_and_classify_batch(imgs)
        else:
            for k in range(WINDOW):
                for n, a, b in zip(rd.CompliancePictures.NAMES, pics[k], first[k]):
                    assert torch.equal(a, b), (name, k, n, int((a != b).sum()))
        # the iterator yields the same, one window after another
        if name != 'device_graphs + device_tail':
            again = list(ev.pictures_iter(zip(imgs, planos), renderer, lookahead=WINDOW))
            _same_reports([rep for rep, _ in again], want, name + ' iter', SEEN_DISTANCE_BOUND)
            assert all(torch.equal(getattr(pic, n).cpu(), pics[k][i]) for k, (_, pic) in enumerate(again) for i, n in enumerate(rd.CompliancePictures.NAMES))
    # the model on the host route's report and detections
    table = rd.label_rows(p['clf'].annotations)
    images = [atlas.image(r).cpu().numpy() for r in range(len(atlas))]
    arrays = lambda it: (it.box.numpy(), it.src.numpy(), it.colour.numpy(), it.thickness.numpy())
    unknown = 0
    for k, (img, plano, rep, (boxes, labels)) in enumerate(zip(imgs, planos, reports, dets)):
        hw = (SIDE, SIDE)
        ehw = rd.expected_canvas_hw(plano['boxes'], SIDE)
        base = rd.float_image_bytes(img.cpu()).numpy()
        expected_rows = rd.rows_of_labels(plano['labels'], table)
        unknown += int((expected_rows < 0).sum())
        lists = (rd.annotation_items(rep, boxes, rd.ANNOTATION_THICKNESS, hw), rd.observed_items(boxes, rd.rows_of_labels(labels, table)),
                 rd.expected_items(plano['boxes'], expected_rows, ehw))
        for n, it, size, b, got in zip(rd.CompliancePictures.NAMES, lists, (hw, hw, ehw), (base, None, None), first[k]):
            want = rc.paint(size, *arrays(it), images, b, rd.WHITE)
            assert tuple(got.shape) == size + (3,) and np.array_equal(got.numpy(), want), (k, n, int((got.numpy() != want).sum()))
        assert not np.array_equal(first[k][0].numpy(), base) and (first[k][1].numpy() != 255).any()      # something was drawn
    assert unknown >= 3                               # the labels no gallery item has: empty rectangles in the expected pictures


def test_pictures_cost_one_launch_more_than_the_report_and_no_wait(cuda):
    from cvpce_amd import production, rendering as rd
    p = _pipeline(cuda)
    imgs, planos = p['imgs'], p['planos']
    renderer = rd.SceneRenderer(p['atlas'])
    ev = p['evaluator'](production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True), p['withheld'], device_detections=True)
    ev.report_batch(imgs, planos), ev.pictures_batch(imgs, planos, renderer)               # (caches, allocator)
    counts = {}
    for key, call in (('report', lambda: ev.report_batch(imgs, planos)), ('pictures', lambda: ev.pictures_batch(imgs, planos, renderer))):
        with p['bench'].WindowCounter() as c:
            call()
        counts[key] = c
    print(f'report {counts["report"].kernels} launches, {counts["report"].waits} waits; pictures {counts["pictures"].kernels} launches, '
          f'{counts["pictures"].waits} waits')
    assert counts['pictures'].kernels == counts['report'].kernels + 1 and counts['pictures'].waits == counts['report'].waits


def test_the_op_refuses_bad_calls_before_any_launch(cuda, window):
    from cvpce_amd import torch_ops_render  # noqa: F401
    win, _ = window
    t = rc.tables(win, only=[1, 2])
    d = {k: torch.from_numpy(t[k]).to(cuda) for k in IN}
    out = torch.empty(t['out_bytes'], dtype=torch.uint8, device=cuda)
    order = ('canvases', 'total_tiles', 'base', 'box', 'src', 'colour', 'thickness', 'atlas', 'atlas_rows', 'background', 'out')
    good = dict(d, total_tiles=t['total_tiles'], background=0, out=out)
    call = lambda **kw: torch.ops.cvpce_amd.render_canvases(*[dict(good, **kw)[k] for k in order])
    call()
    for bad in (dict(canvases=d['canvases'].to(torch.int32)), dict(canvases=d['canvases'][:, :9].contiguous()), dict(box=d['box'].double()),
                dict(box=d['box'][:-1]), dict(src=d['src'].to(torch.int64)), dict(colour=d['colour'][:-1]), dict(thickness=d['thickness'][:-1]),
                dict(atlas=d['atlas'].to(torch.int32)), dict(atlas_rows=d['atlas_rows'][:, :2].contiguous()), dict(out=out.view(-1, 3)),
                dict(base=d['base'].to(torch.int32)), dict(total_tiles=-1), dict(box=d['box'].t().contiguous().t())):
        with pytest.raises(RuntimeError, match='cvpce_render_canvases'):
            call(**bad)
    torch.cuda.synchronize()
