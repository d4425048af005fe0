"""8-bit shelf images on the GPU: an (H,W,3) uint8 image gives, at every entry point, the very bits its float twin
`u.permute(2,0,1).float() / 255` (made on the CPU) gives -- the inputs are the same numbers, so every comparison is exact -- whether
it is uploaded by the entry point or read ahead and uploaded by `feeding.ImageFeeder`."""
import json
import re

import pytest
import torch

pytestmark = pytest.mark.gpu


def _quantise(scene):
    """float scene (3,H,W) in [0,1] -> (8-bit image (H,W,3), its float twin (3,H,W) made on the CPU)."""
    u = (scene * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()
    return u, (u.permute(2, 0, 1).float() / 255).contiguous()       # (contiguous: BatchedPipeline.run takes its float images as they are)


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


def _same_detections(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert len(x['boxes']) > 0
        for k in ('boxes', 'scores', 'labels', 'gaussians'):
            assert torch.equal(x[k], y[k]), k


def test_device_conversion_is_exact(cuda, scenes):
    from cvpce_amd import ops
    codes = torch.arange(256, dtype=torch.uint8).repeat(3, 1).t().contiguous().view(16, 16, 3)
    got = ops.device_image(codes, cuda)
    host = torch.arange(256, dtype=torch.float32) / 255.0
    assert got.is_cuda and got.dtype == torch.float32 and got.is_contiguous() and tuple(got.shape) == (3, 16, 16)
    for c in range(3):
        assert torch.equal(got[c].reshape(-1).cpu().view(torch.int32), host.view(torch.int32))
    assert torch.equal(ops.uint8_table(cuda).cpu().view(torch.int32), host.view(torch.int32))
    for u, f in scenes[:2]:
        d = ops.device_image(u, cuda)
        assert tuple(d.shape) == tuple(f.shape) and d.is_contiguous() and torch.equal(d.cpu(), f)
        assert torch.equal(ops.device_image(u.pin_memory(), cuda).cpu(), f)        # the non-blocking upload from pinned memory
        assert torch.equal(ops.device_image(u.to(cuda), cuda).cpu(), f)            # already on the device: converted where it is
        assert torch.equal(ops.device_image(f, cuda).cpu(), f)


def test_model_forward(cuda, det, scenes):
    (u0, f0), (u1, f1) = scenes[0], scenes[1]          # square and portrait
    for u, f in ((u0, f0), (u1, f1)):
        _same_detections(det([u]), det([f]))
        _same_detections(det([u]), det([f]))           # (the second call of a geometry replays the captured schedule)
    _same_detections(det([u0, scenes[2][1]]), det([f0, scenes[2][1]]))          # a list that mixes the forms
    _same_detections(det([f0, scenes[2][0]]), det([f0, scenes[2][1]]))
    _same_detections(det([u1.to(cuda)]), det([f1]))
    report = det.saturation_report([u0])
    assert report['stages'] == det.saturation_report([f0])['stages']


def test_proposals_and_resize(cuda, det, scenes):
    from cvpce_amd import datautils, production
    pg = production.ProposalGenerator(det, device=cuda, confidence_threshold=0.5)
    for u, f in scenes[:2]:
        bu, cu = pg.generate_proposals_and_images(u)
        bf, cf = pg.generate_proposals_and_images(f)
        assert len(bu) > 0 and torch.equal(bu, bf) and torch.equal(cu, cf)
        assert torch.equal(pg.generate_proposals(u), pg.generate_proposals(f))
        ru, rf = datautils.resize_for_classification(u.to(cuda)), datautils.resize_for_classification(f.to(cuda))
        assert tuple(ru.shape) == (3, 256, 256) and torch.equal(ru, rf)


def test_batched_pipeline(cuda, det, clf, scenes):
    from cvpce_amd import production
    pipe = production.BatchedPipeline(det, clf, 0.5)
    pairs = [scenes[0], scenes[2], scenes[3]]                       # three 512 x 512 images
    n, dpi = len(pairs), det.detections_per_img
    # planted proposals: 60 boxes per image on a grid, whatever the seeded detector emits
    g = torch.Generator().manual_seed(5)
    xy = torch.stack([torch.tensor([40.0 * (k % 10) + 8, 70.0 * (k // 10) + 6]) for k in range(60)])
    wh = torch.rand(60, 2, generator=g) * 30 + 40
    boxes = torch.zeros(n, dpi, 4)
    boxes[:, :60] = torch.cat([xy, xy + wh], dim=1)
    planted = (boxes.to(cuda), torch.full((n,), 60, dtype=torch.int32, device=cuda))
    for proposals in (planted, None):
        out_u = pipe.run([u for u, _ in pairs], proposals=proposals)
        out_f = pipe.run([f.to(cuda) for _, f in pairs], proposals=proposals)
        assert out_u['counts_host'] == out_f['counts_host'] and out_u['embeddings'].shape[0] == sum(out_u['counts_host']) > 0
        if proposals is not None:          # at least 50 crops per image reach the embedder: nothing here passes on empty results
            assert out_u['counts_host'] == [60] * n
        for k in ('boxes', 'scores', 'count', 'indices', 'embeddings'):
            assert torch.equal(out_u[k], out_f[k]), k
    # a list that mixes the forms (and an 8-bit image that is on the device already)
    mixed = pipe.run([pairs[0][0].to(cuda), pairs[1][1].to(cuda), pairs[2][0]], proposals=planted)
    want = pipe.run([f.to(cuda) for _, f in pairs], proposals=planted)
    for k in ('boxes', 'scores', 'count', 'indices', 'embeddings'):
        assert torch.equal(mixed[k], want[k]), k


@pytest.fixture(scope='module')
def evaluator(cuda, det, clf):
    from cvpce_amd import production
    pg = production.ProposalGenerator(det, device=cuda, confidence_threshold=0.5)
    return production.PlanogramEvaluator(pg, clf, production.PlanogramComparator())


@pytest.fixture(scope='module')
def planos(evaluator, scenes):
    """Each image's own detections, a third of them dropped and a few labels changed -> partial compliance (the planograms of
    tests/test_gpu_harness.py)."""
    out = []
    for k, (_, f) in enumerate(scenes):
        boxes, crops = evaluator.proposal_generator.generate_proposals_and_images(f)
        b, l = boxes.cpu(), [a[0] for a in evaluator.classifier.classify(crops)]
        keep = [i for i in range(len(b)) if i % 3 != k % 3]
        out.append({'boxes': b[keep] * 0.5, 'labels': [('other' if i % 7 == 0 else l[i]) for i in keep]})
    return out


def test_evaluator(cuda, evaluator, scenes, planos):
    from cvpce_amd.feeding import ImageFeeder
    ev = evaluator
    want = [float(ev.evaluate(f, p)) for (_, f), p in zip(scenes, planos)]
    assert any(0.0 < v < 1.0 for v in want), want
    us = [u for u, _ in scenes]
    assert [float(ev.evaluate(u, p)) for u, p in zip(us, planos)] == want
    assert [float(v) for v in ev.evaluate_batch(us, planos)] == want
    assert [float(v) for v in ev.evaluate_batch([us[0], scenes[1][1], us[2], scenes[3][1]], planos)] == want      # mixed forms
    for (bu, lu), (bf, lf) in zip(ev.detect_and_classify_batch(us), ev.detect_and_classify_batch([f for _, f in scenes])):
        assert len(bu) > 0 and torch.equal(bu, bf) and lu == lf
    pairs = list(zip(us, planos))
    feeder = ImageFeeder(pairs, workers=4, device=cuda)
    assert [float(v) for v in ev.evaluate_iter(feeder, lookahead=4)] == want
    assert feeder.bytes_uploaded == sum(u.numel() for u in us)
    # a second pass reuses the pinned ring (and, with depth 2 over four images, every slot within the pass): no stale buffer
    assert [float(v) for v in ev.evaluate_iter(feeder, lookahead=4)] == want
    assert [float(v) for v in ev.evaluate_iter(ImageFeeder(pairs, workers=2, depth=2, device=cuda), lookahead=2)] == want
    assert [float(v) for v in ev.evaluate_iter(iter(pairs), lookahead=4)] == want


def test_feeder_on_the_device(cuda, scenes):
    import threading
    from cvpce_amd import ops
    from cvpce_amd.feeding import ImageFeeder
    before = threading.active_count()
    items = [(u, {'i': i}) for i, (u, _) in enumerate(scenes)] * 3          # 12 items through a ring of 2 and of 4 slots
    for depth in (2, None):
        feeder = ImageFeeder(items, workers=4, depth=depth, device=cuda)
        for _ in range(2):                                                  # the second pass reuses nothing stale
            n = 0
            for (img, tag), (u, want_tag) in zip(feeder, items):
                assert img.is_cuda and img.dtype == torch.uint8 and tuple(img.shape) == tuple(u.shape) and tag is want_tag
                assert torch.equal(ops.device_image(img, cuda), ops.device_image(u, cuda))
                assert torch.equal(img.cpu(), u)
                n += 1
            assert n == len(items)
    # float images pass through as they are; workers = 0 uploads in the calling thread
    f = scenes[0][1]
    got = list(ImageFeeder([(f, 0), (scenes[1][0], 1)], workers=0, device=cuda))
    assert got[0][0] is f and got[1][0].is_cuda and torch.equal(got[1][0].cpu(), scenes[1][0])
    # leaving early joins the readers
    for k, _ in enumerate(ImageFeeder(items, workers=4, device=cuda)):
        if k == 2:
            break
    assert threading.active_count() == before


# ---- command line: the same printed lines whatever reads the files ----------------------------------------------------
@pytest.fixture(scope='module')
def world(cuda, tmp_path_factory):
    """The file fixtures of tests/test_gpu_cli.py, smaller: checkpoints, a six-product gallery, two GP-180-like shelf images with
    planograms, three SKU-110K-like images."""
    from PIL import Image
    from cvpce_amd import synthetic
    root = tmp_path_factory.mktemp('cli_uint8')
    to_img = lambda t: Image.fromarray((t.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy())
    torch.save({'model_state_dict': synthetic.synthetic_gln(seed=0, detections_per_img=60).state_dict()}, root / 'gln.tar')
    torch.save({'model_state_dict': synthetic.synthetic_macvgg(seed=1).state_dict()}, root / 'dihe.tar')
    gal = (synthetic.gallery_images(6, seed=5) + 1) / 2
    names = []
    for i in range(6):
        d = root / 'Training' / 'Food' / f'Cat{i % 2}'
        d.mkdir(parents=True, exist_ok=True)
        to_img(gal[i]).save(d / f'{10 + i}.png')
        names.append(f'Food/Cat{i % 2}/{10 + i}')
    (root / 'Testing' / 'store1' / 'images').mkdir(parents=True)
    (root / 'ann').mkdir(); (root / 'plano').mkdir()
    for img_id, picks in ((15, (3, 1, 4)), (16, (0, 5, 2)), (17, (2, 4, 1))):
        shelf = torch.full((3, 300, 840), 0.3)
        rows = []
        for j, i in enumerate(picks):
            x = 10 + j * 270
            shelf[:, 20:276, x:x + 256] = gal[i]
            rows.append(f'{names[i]}.jpg, {x}, 20, {x + 256}, 276')
        to_img(shelf).save(root / 'Testing' / 'store1' / 'images' / f'store1_{img_id}.jpg', format='PNG')
        (root / 'ann' / f's1_{img_id}.csv').write_text('\n'.join(rows) + '\n')
        graph = [{'ogg': j, 'n': -1, 's': -1, 'e': j + 1 if j < 2 else -1, 'w': j - 1, 'ne': -1, 'nw': -1, 'se': -1, 'sw': -1} for j in range(3)]
        objects = [{'width': 256, 'height': 256, 'img_path': names[i] + '.jpg'} for i in picks]
        (root / 'plano' / f's1_{img_id}.json').write_text(json.dumps({'graph': graph, 'objects': objects}))
    (root / 'sku').mkdir()
    rows = []
    for k in range(3):
        to_img(synthetic.shelf_image(30 + k, 384, 512)).save(root / 'sku' / f'test_{k}.jpg', quality=92)       # real JPEG files
        rows += [f'test_{k}.jpg,{20 + 60 * b},{30},{70 + 60 * b},{120},object,512,384' for b in range(4)]
    (root / 'sku' / 'annotations.csv').write_text('\n'.join(rows) + '\n')
    return root


def _run(args, env=None):
    from click.testing import CliRunner
    from cvpce_amd.cli import cli
    r = CliRunner().invoke(cli, [str(a) for a in args], catch_exceptions=False, env=env)
    assert r.exit_code == 0, r.output
    return r.output


def test_cli_prints_the_same_lines_with_and_without_reader_threads(world):
    from cvpce_amd import datautils, proposals_eval
    gln_eval = ['gln', 'eval', '--dataset', 'sku110k', '--imgs', world / 'sku', '--annotations', world / 'sku' / 'annotations.csv',
                '-t', '0.5', '-t', '0.75', '--no-plots', '--metric-workers', '0', '--batch-size', '2']
    serial = _run(gln_eval + ['--dataloader-workers', '0', world / 'gln.tar'])
    threaded = _run(gln_eval + ['--dataloader-workers', '4', world / 'gln.tar'])
    assert re.search(r'--> AP [0-9.e-]+', serial) and serial == threaded
    # ... and they are the float readers' figures (the parent's path), to the last digit
    data = datautils.SKU110KDataset(str(world / 'sku'), str(world / 'sku' / 'annotations.csv'))
    direct = proposals_eval.evaluate_gln(str(world / 'gln.tar'), data, thresholds=[0.5, 0.75], batch_size=2, num_metric_processes=0,
                                         trim_module_prefix=False)
    assert all(f'{t}:\t{direct[t]}' in serial for t in (0.5, 0.75))
    plano = ['eval-planograms', '--img-dir', world / 'Training', '--test-imgs', world / 'Testing', '--test-annotations', world / 'ann',
             '--planograms', world / 'plano', '--verbose', world / 'gln.tar', world / 'dihe.tar']
    serial = _run(plano, env={'CVPCE_DATALOADER_WORKERS': '0'})
    threaded = _run(plano, env={'CVPCE_DATALOADER_WORKERS': '4'})
    assert serial.count('Detected accuracy:') == 3 and re.search(r'--> MSE: [0-9.e-]+', serial) and serial == threaded
    dihe = ['dihe', 'eval', '--img-dir', world / 'Training', '--test-imgs', world / 'Testing', '--annotations', world / 'ann',
            '--enc-weights', world / 'dihe.tar', '--knn', '1']
    serial = _run(dihe + ['--dataloader-workers', '0'])
    assert '--> accuracy {1: 1.0}' in serial and serial == _run(dihe + ['--dataloader-workers', '4'])
