"""The product path with ops.U8_KERNELS on: an 8-bit image stays bytes from the upload to the last crop -- no float copy of it is
ever made (`ops.uint8_to_float` / `ops.device_image` raise here when handed one) -- and every entry point gives the bits its float
twin gives.  With the switch off the same entry points give the same results through the conversion.  Fixtures: those of
tests/test_gpu_uint8_input.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu


def _quantise(scene):
    """float scene (3,H,W) in [0,1] -> (8-bit image (H,W,3), its float twin (3,H,W) made on the CPU)."""
    u = (scene * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    return u, (u.permute(2, 0, 1).float() / 255).contiguous()


@pytest.fixture(scope='module')
def det(cuda):
    from cvpce_amd import synthetic
    return synthetic.synthetic_gln(seed=0, detections_per_img=64).to(cuda)


@pytest.fixture(scope='module')
def clf(cuda):
    from cvpce_amd import production, synthetic
    enc = synthetic.synthetic_macvgg(seed=1).to(cuda)
    gal = synthetic.gallery_images(24, seed=17)
    return production.Classifier(enc, synthetic.TensorGallery(gal, [f'sku{i % 6}' for i in range(24)]), device=cuda, emb_device=cuda,
                                 batch_size=8)


@pytest.fixture(scope='module')
def scenes():
    from cvpce_amd import synthetic
    return [_quantise(synthetic.shelf_image(s, h, w)) for s, h, w in ((70, 512, 512), (71, 640, 448), (72, 512, 512), (73, 512, 512))]


@pytest.fixture(scope='module')
def evaluator(cuda, det, clf):
    from cvpce_amd import production
    pg = production.ProposalGenerator(det, device=cuda, confidence_threshold=0.5)
    return production.PlanogramEvaluator(pg, clf, production.PlanogramComparator())


@pytest.fixture(scope='module')
def planted(cuda, det):
    """60 boxes per image on a grid, whatever the seeded detector emits (three 512 x 512 images)."""
    n, dpi = 3, det.detections_per_img
    g = torch.Generator().manual_seed(5)
    xy = torch.stack([torch.tensor([40.0 * (k % 10) + 8, 70.0 * (k // 10) + 6]) for k in range(60)])
    wh = torch.rand(60, 2, generator=g) * 30 + 40
    boxes = torch.zeros(n, dpi, 4)
    boxes[:, :60] = torch.cat([xy, xy + wh], dim=1)
    return boxes.to(cuda), torch.full((n,), 60, dtype=torch.int32, device=cuda)


def _detections(res):
    return [{k: r[k].clone() for k in ('boxes', 'scores', 'labels', 'gaussians')} for r in res]


def _pipeline(out):
    return {k: out[k].clone() for k in ('boxes', 'scores', 'count', 'indices', 'embeddings')}, list(out['counts_host'])


@pytest.fixture(scope='module')
def want(cuda, det, clf, evaluator, scenes, planted):
    """The float twins' results, computed once (float images never meet the switch)."""
    from cvpce_amd import production
    fs = [f for _, f in scenes]
    pg = evaluator.proposal_generator
    planos = []
    for k, f in enumerate(fs):              # each image's own detections, a third dropped, a few labels changed -> partial compliance
        boxes, crops = pg.generate_proposals_and_images(f)
        b, l = boxes.cpu(), [a[0] for a in clf.classify(crops)]
        keep = [i for i in range(len(b)) if i % 3 != k % 3]
        planos.append({'boxes': b[keep] * 0.5, 'labels': [('other' if i % 7 == 0 else l[i]) for i in keep]})
    pipe = production.BatchedPipeline(det, clf, 0.5)
    w = {
        'single': [_detections(det([f])) for f in fs[:2]],
        'mixed': _detections(det([fs[0], fs[2]])),
        'proposals': [pg.generate_proposals_and_images(f) for f in fs[:2]],
        'pipeline': _pipeline(pipe.run([fs[i].to(cuda) for i in (0, 2, 3)], proposals=planted)),
        'evaluate': [float(evaluator.evaluate(f, p)) for f, p in zip(fs, planos)],
        'planos': planos,
    }
    assert all(len(r['boxes']) > 0 for res in w['single'] for r in res) and w['pipeline'][1] == [60] * 3
    assert any(0.0 < v < 1.0 for v in w['evaluate']), w['evaluate']
    return w


def _same_detections(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        for k in ('boxes', 'scores', 'labels', 'gaussians'):
            assert torch.equal(x[k], y[k]), k


def _check_entry_points(cuda, det, clf, evaluator, scenes, planted, want):
    from cvpce_amd import production
    from cvpce_amd.feeding import ImageFeeder
    us, fs = [u for u, _ in scenes], [f for _, f in scenes]
    for u, w in zip(us[:2], want['single']):            # square and portrait
        _same_detections(det([u]), w)
        _same_detections(det([u]), w)                   # (the second call of a geometry replays the captured schedule)
        _same_detections(det([u.to(cuda)]), w)
    _same_detections(det([us[0], fs[2]]), want['mixed'])              # a list that mixes the forms
    _same_detections(det([fs[0], us[2]]), want['mixed'])
    pg = evaluator.proposal_generator
    for u, (bf, cf) in zip(us[:2], want['proposals']):
        bu, cu = pg.generate_proposals_and_images(u)
        assert len(bu) > 0 and torch.equal(bu, bf) and torch.equal(cu, cf)
    pipe = production.BatchedPipeline(det, clf, 0.5)
    for images in ([us[0], us[2], us[3]], [us[0].to(cuda), fs[2].to(cuda), us[3]]):
        out, counts = _pipeline(pipe.run(images, proposals=planted))
        assert counts == want['pipeline'][1] == [60] * 3
        for k, v in want['pipeline'][0].items():
            assert torch.equal(out[k], v), k
    planos = want['planos']
    assert [float(evaluator.evaluate(u, p)) for u, p in zip(us, planos)] == want['evaluate']
    assert [float(v) for v in evaluator.evaluate_batch(us, planos)] == want['evaluate']
    assert [float(v) for v in evaluator.evaluate_batch([us[0], fs[1], us[2], fs[3]], planos)] == want['evaluate']
    feeder = ImageFeeder(list(zip(us, planos)), workers=4, device=cuda)
    assert [float(v) for v in evaluator.evaluate_iter(feeder, lookahead=4)] == want['evaluate']
    assert feeder.bytes_uploaded == sum(u.numel() for u in us)


def test_bytes_all_the_way(cuda, det, clf, evaluator, scenes, planted, want, monkeypatch):
    from cvpce_amd import ops
    monkeypatch.setattr(ops, 'U8_KERNELS', True)
    made = []

    def refuse(real):
        def guarded(img, *args, **kwargs):
            if ops.is_uint8_image(img):
                made.append(tuple(img.shape))
                raise AssertionError('a float copy of an 8-bit image was asked for')
            return real(img, *args, **kwargs)
        return guarded

    monkeypatch.setattr(ops, 'uint8_to_float', refuse(ops.uint8_to_float))
    monkeypatch.setattr(ops, 'device_image', refuse(ops.device_image))
    _check_entry_points(cuda, det, clf, evaluator, scenes, planted, want)
    assert not made


def test_switch_off_is_the_conversion_path(cuda, det, clf, evaluator, scenes, planted, want, monkeypatch):
    from cvpce_amd import ops
    monkeypatch.setattr(ops, 'U8_KERNELS', False)
    converted = []
    real = ops.uint8_to_float
    monkeypatch.setattr(ops, 'uint8_to_float', lambda u: (converted.append(tuple(u.shape)), real(u))[1])
    _check_entry_points(cuda, det, clf, evaluator, scenes, planted, want)
    assert converted                                    # (the float kernels read converted images)
