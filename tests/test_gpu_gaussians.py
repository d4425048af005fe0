"""Scoring the detector's Gaussian maps on the GPU: csrc/gaussians.hip against the vectors of the reference's own code
(tests/golden/gaussian_targets.pt) and against the fp32 host model of tests/gaussian_cases.py.

Tolerances (gaussian_cases): targets within TARGET_TOL = 4 * T_ref, T_ref being the host model's distance from the reference measured on
the host -- relative to max(1, |value|) under `addition`; losses within 4 * TARGET_TOL + 2e-6 * |loss|.  Wherever no box covers a tap the
device's bits are the model's."""
import os

import numpy as np
import pytest
import torch

import footprint as F
import gaussian_cases as gc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HB, WB = 48, 64
# four images in one padded batch: extents that are no multiple of the 16-pixel tile, a size reduction, an image without boxes and one
# whose extent has no rows
BATCH = [(97, 75, gc.BOXES_SMALL, 1, (37, 45)),
         (80, 60, [[8, 8, 30, 40], [35, 10, 70, 30], [50, 35, 78, 58], [-9, 41, 33, 75]], 2, (48, 64)),
         (50, 50, [], 1, (20, 30)),
         (64, 64, [[5, 5, 40, 40]], 1, (0, 10))]
PAIRS = [(m, j) for m in gc.METHODS for j in gc.JOINS]


@pytest.fixture(scope='module')
def golden():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'gaussian_targets.pt'), weights_only=False)


def _descriptors(method, join):
    from cvpce_amd import datautils as d
    return getattr(d, 'generate_via_' + method)(), getattr(d, 'join_via_' + join)


def _fused(cuda, images, hb, wb, method, join, tanh=False, resize=True):
    from cvpce_amd import device_gaussians as dg
    g, j = _descriptors(method, join)
    boxes = [torch.tensor(b, dtype=torch.int64).reshape(-1, 4) for _, _, b, _, _ in images]
    geom = [(h0, w0, r, h, w) for w0, h0, _, r, (h, w) in images]
    return dg.render_boxes(boxes, geom, hb, wb, g, j, tanh, resize, cuda)


def _close(got, want, join):
    d = np.abs(got.astype(np.float64) - want)
    if join == 'addition':
        d = d / np.maximum(1, np.abs(want))
    return float(d.max()) if d.size else 0.0


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def test_targets_match_the_reference(cuda, golden):
    from cvpce_amd import datautils
    for name, c in golden['targets'].items():
        g, j = _descriptors(c['method'], c['join'])
        got = datautils.generate_gaussians(c['w'], c['h'], torch.tensor(c['boxes']), c['size_reduction'], g, j, c['tanh'])
        assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == tuple(c['expected'].shape), name
        worst = _close(got.cpu().numpy(), c['expected'].numpy(), c['join'])
        print(f'{name}: max difference from the reference {worst:.3e}')
        assert worst <= gc.TARGET_TOL, name


@pytest.mark.parametrize('method,join', PAIRS)
def test_fused_batch_against_the_model(cuda, method, join):
    """Elements no box reaches (background between boxes, the padding, the box-less image, the image without rows) carry the model's
    bits; the others are within the tolerance.  kant + addition, which the reference cannot run, is held to the model alone."""
    for tanh in ((False, True) if method == 'simple_and_scaled' else (False,)):
        want, touched = gc.fused_targets(BATCH, HB, WB, tanh=tanh, method=method, join=join)
        got = _fused(cuda, BATCH, HB, WB, method, join, tanh).cpu().numpy()
        assert got.shape == want.shape
        assert np.array_equal(_bits(got[~touched]), _bits(want[~touched]))
        assert touched[:2].any() and not touched[2:].any()
        assert _close(got, want, join) <= gc.TARGET_TOL


@pytest.mark.parametrize('method,join', PAIRS)
def test_fused_equals_render_then_resize(cuda, method, join):
    from cvpce_amd import datautils, device_gaussians as dg
    g, j = _descriptors(method, join)
    fused = _fused(cuda, BATCH, HB, WB, method, join)
    maps = [datautils.generate_gaussians(w0, h0, torch.tensor(b, dtype=torch.int64).reshape(-1, 4), r, g, j) for w0, h0, b, r, _ in BATCH]
    for m, (w0, h0, b, r, _) in zip(maps, BATCH):
        want, _ = gc.render(w0, h0, b, r, method=method, join=join)
        assert tuple(m.shape) == want.shape and _close(m.cpu().numpy(), want, join) <= gc.TARGET_TOL
    two_step = dg.render_maps(maps, [e for *_, e in BATCH], HB, WB)
    assert torch.equal(fused.view(torch.int32), two_step.view(torch.int32))


@pytest.mark.parametrize('count', [255, 256, 257, 600])
@pytest.mark.parametrize('join', ['replacement', 'addition'])
def test_box_list_around_its_capacity(cuda, count, join):
    """Every box covers the single 16 x 16 tile: the list is one under, at and one over its LDS capacity (256), and several chunks.
    Both joins depend on the order of the boxes."""
    from cvpce_amd import torch_ops_gaussians as G
    assert G.LIST == 256 and G.TILE == 16
    boxes = [[-(i % 3), -(i % 5), 16 + i % 7, 17 + i % 4] for i in range(count)]
    for images, resize in (([(16, 16, boxes, 1, (16, 16))], False), ([(16, 16, boxes, 1, (11, 13))], True)):
        hb, wb = images[0][4]
        want, _ = gc.fused_targets(images, hb, wb, method='multivariate_normal', join=join) if resize else \
            (gc.render(16, 16, boxes, 1, method='multivariate_normal', join=join)[0][None, None], None)
        got = _fused(cuda, images, hb, wb, 'multivariate_normal', join, resize=resize).cpu().numpy()
        assert _close(got, want, join) <= gc.TARGET_TOL


def test_bad_arguments_are_refused(cuda):
    from cvpce_amd import device_gaussians as dg
    out = torch.empty((1, 1, 8, 8), device=cuda)
    geom = torch.tensor([[8, 8, 1, 8, 8]], dtype=torch.int32, device=cuda)
    off = torch.tensor([0, 0], dtype=torch.int32, device=cuda)
    boxes = torch.zeros((0, 4), dtype=torch.int32, device=cuda)
    with pytest.raises(RuntimeError, match='bad argument'):
        torch.ops.cvpce_amd.gauss_targets(boxes, off, None, geom, None, 7, 0, 1.0, 0.5, 0.0, 0, 1, out)
    with pytest.raises(RuntimeError, match='bad argument'):                       # kant without its table
        torch.ops.cvpce_amd.gauss_targets(boxes, off, None, geom, None, 1, 0, 0.0, 0.0, 0.0, 0, 1, out)
    with pytest.raises(RuntimeError):
        torch.ops.cvpce_amd.gauss_targets(boxes, off, None, geom[:, :4].contiguous(), None, 0, 0, 1.0, 0.5, 0.0, 0, 1, out)
    with pytest.raises(RuntimeError, match='bad argument'):
        torch.ops.cvpce_amd.gauss_loss(out, out.clone(), None, 0.0, 0.1, -1, 3, 0, torch.empty(1 << 16, dtype=torch.uint8, device=cuda),
                                       torch.empty((1, 3), device=cuda), torch.empty((1, 2), dtype=torch.int32, device=cuda))
    with pytest.raises(RuntimeError, match='bad argument'):                       # workspace too small
        torch.ops.cvpce_amd.gauss_loss(out, out.clone(), None, 0.0, 0.1, 10, 3, 0, torch.empty(16, dtype=torch.uint8, device=cuda),
                                       torch.empty((1, 3), device=cuda), torch.empty((1, 2), dtype=torch.int32, device=cuda))
    with pytest.raises(TypeError):
        dg.render_boxes([torch.tensor([[1.5, 2.0, 3.0, 4.0]])], [(8, 8, 1, 8, 8)], 8, 8)


# ---- loss -----------------------------------------------------------------------------------------------------------------------------
def _loss_inputs(golden, name, cuda):
    L = golden['losses']
    c = L['cases'][name]
    maps = [(m * (0 if c['zero_maps'] else 1)).to(cuda) for m in L['maps']]
    return L['predictions'][c['prediction']].to(cuda), maps, L['sizes'], c


@pytest.mark.parametrize('name', list(gc.LOSS_PARAMS))
def test_loss_matches_the_reference(cuda, golden, name):
    from cvpce_amd import device_gaussians as dg
    from cvpce_amd.models import proposals
    pred, maps, sizes, c = _loss_inputs(golden, name, cuda)
    got = proposals.gaussian_loss(pred, maps, sizes, **c['params'])
    assert got.is_cuda and got.dim() == 0
    want = float(c['expected'])
    print(f'{name}: {float(got)!r} against the reference\'s {want!r}')
    assert abs(float(got) - want) <= gc.loss_tolerance(want)
    # the parts, against the host model on its own targets: counts exact
    extents = [(s[0] // 2, s[1] // 2) for s in sizes]
    target = dg.render_maps(maps, extents, HB, WB)
    out_f, out_i = dg.loss(pred, target, None, **c['params'])
    model_target = np.zeros((len(maps), 1, HB, WB), dtype=np.float32)
    for n, (m, (h, w)) in enumerate(zip(maps, extents)):
        model_target[n, 0, :h, :w] = gc.resize(m.cpu().numpy(), h, w)
    assert np.array_equal(_bits(target.cpu().numpy()), _bits(model_target))            # a resize has no expf: the model's bits
    m = gc.loss(pred.cpu().numpy(), model_target, **c['params'])
    assert out_i.tolist() == [[m['pos_count'], m['neg_count_used']]]
    f = out_f[0].tolist()
    assert f[0] == float(got)
    for got_v, want_v in ((f[0], m['loss']), (f[1], m['pos_sum']), (f[2], m['neg_sum'])):
        assert abs(got_v - want_v) <= 2e-6 * abs(want_v) + 1e-12
    again_f, again_i = dg.loss(pred, target, None, **c['params'])                      # the same bits on a second run
    assert torch.equal(again_f.view(torch.int32), out_f.view(torch.int32)) and torch.equal(again_i, out_i)


def test_loss_per_image_scope(cuda, golden):
    from cvpce_amd import device_gaussians as dg
    pred, maps, sizes, _ = _loss_inputs(golden, 'defaults', cuda)
    extents = [(s[0] // 2, s[1] // 2) for s in sizes]
    target = dg.render_maps(maps, extents, HB, WB)
    counted = [(48, 64), (40, 64), (33, 45)]                                           # rows and columns that are no multiple of anything
    for params in (dict(), dict(min_negatives=10, negatives_per_positive=1), dict(min_negatives=100000)):
        ext = torch.tensor(counted, dtype=torch.int32, device=cuda)
        out_f, out_i = dg.loss(pred, target, ext, **params)
        assert tuple(out_f.shape) == (3, 3) and tuple(out_i.shape) == (3, 2)
        for n, e in enumerate(counted):
            m = gc.loss(pred[n].cpu().numpy(), target[n].cpu().numpy(), extent=e, **params)
            assert out_i[n].tolist() == [m['pos_count'], m['neg_count_used']]
            assert abs(float(out_f[n, 0]) - m['loss']) <= 2e-6 * abs(m['loss'])
        again, _ = dg.loss(pred, target, ext, **params)
        assert torch.equal(again.view(torch.int32), out_f.view(torch.int32))
    # a batch of one: the batch scope is the per-image scope over the whole tensor, bit for bit
    one_f, one_i = dg.loss(pred[:1], target[:1], None)
    own_f, own_i = dg.loss(pred[:1], target[:1], torch.tensor([[HB, WB]], dtype=torch.int32, device=cuda))
    assert torch.equal(one_f.view(torch.int32), own_f.view(torch.int32)) and torch.equal(one_i, own_i)
    # an image with nothing counted, and targets that are neither positive nor negative: 0 / 0 = NaN as in the reference
    none_f, none_i = dg.loss(pred, target, torch.tensor([[0, 64], [48, 0], [0, 0]], dtype=torch.int32, device=cuda))
    assert bool(torch.isnan(none_f[:, 0]).all()) and none_i.tolist() == [[0, 0]] * 3
    grey_f, grey_i = dg.loss(pred, torch.full_like(target, 0.05), None)
    assert bool(torch.isnan(grey_f[0, 0])) and grey_i.tolist() == [[0, 0]]


def test_loss_over_more_than_one_workgroup_per_image(cuda):
    """130 x 190 elements per image: 13 workgroups each, the last one partly past the end; values with many equal squared errors."""
    rng = np.random.RandomState(7)
    pred = (rng.randint(0, 64, size=(2, 1, 130, 190)) / 64.0).astype(np.float32)
    target = np.where(rng.rand(2, 1, 130, 190) < 0.3, 0.5, 0.0).astype(np.float32)
    from cvpce_amd import device_gaussians as dg
    p, t = torch.from_numpy(pred).to(cuda), torch.from_numpy(target).to(cuda)
    for params in (dict(), dict(min_negatives=777, negatives_per_positive=0), dict(min_negatives=1, negatives_per_positive=0)):
        out_f, out_i = dg.loss(p, t, None, **params)
        m = gc.loss(pred, target, **params)
        assert out_i.tolist() == [[m['pos_count'], m['neg_count_used']]]
        assert abs(float(out_f[0, 0]) - m['loss']) <= 2e-6 * abs(m['loss'])
        assert abs(float(out_f[0, 2]) - m['neg_sum']) <= 2e-6 * abs(m['neg_sum'])
        ext = torch.tensor([[130, 190], [129, 77]], dtype=torch.int32, device=cuda)
        per_f, per_i = dg.loss(p, t, ext, **params)
        for n, e in enumerate(ext.tolist()):
            m = gc.loss(pred[n], target[n], extent=e, **params)
            assert per_i[n].tolist() == [m['pos_count'], m['neg_count_used']]
            assert abs(float(per_f[n, 0]) - m['loss']) <= 2e-6 * abs(m['loss'])


# ---- footprints -----------------------------------------------------------------------------------------------------------------------
def test_footprint_of_the_targets_kernel(cuda):
    from cvpce_amd import device_gaussians as dg, torch_ops_gaussians as G
    for method, params in (('multivariate_normal', (1.0, 0.5, 0.0)), ('kant_method', (0.0, 0.0, 0.0))):
        boxes = torch.tensor([b for _, _, bs, _, _ in BATCH for b in bs], dtype=torch.int32)
        offsets = torch.tensor(np.cumsum([0] + [len(bs) for _, _, bs, _, _ in BATCH]), dtype=torch.int32)
        geom = torch.tensor([(h0, w0, r, h, w) for w0, h0, _, r, (h, w) in BATCH], dtype=torch.int32)
        table = dg._kant_table(cuda, 120, 40).cpu() if method == 'kant_method' else None
        ins = [F.put(t, cuda) for t in (boxes, offsets, geom, table)]
        out = F.out((len(BATCH), 1, HB, WB), torch.float32, cuda)
        run = lambda: torch.ops.cvpce_amd.gauss_targets(ins[0][0], ins[1][0], None, ins[2][0], ins[3][0] if ins[3] else None, G.METHODS[method], 0,
                                                        *params, 0, 1, out[0])
        got = F.check(run, ins, [out])[0]
        want, _ = gc.fused_targets(BATCH, HB, WB, method=method, join='max')
        assert _close(got.cpu().numpy(), want, 'max') <= gc.TARGET_TOL
    # the maps as the source
    maps = [torch.rand(h0 // r, w0 // r) for w0, h0, _, r, _ in BATCH]
    held = [F.put(m, cuda) for m in maps]
    ptrs = F.put(torch.tensor([v.data_ptr() for v, _ in held], dtype=torch.int64), cuda)
    geom = F.put(torch.tensor([(m.shape[0], m.shape[1], 1, h, w) for m, (*_, (h, w)) in zip(maps, BATCH)], dtype=torch.int32), cuda)
    out = F.out((len(BATCH), 1, HB, WB), torch.float32, cuda)
    run = lambda: torch.ops.cvpce_amd.gauss_targets(None, None, ptrs[0], geom[0], None, 0, 0, 0.0, 0.0, 0.0, 0, 1, out[0])
    got = F.check(run, held + [ptrs, geom], [out])[0].cpu().numpy()
    for n, (m, (*_, (h, w))) in enumerate(zip(maps, BATCH)):
        if h and w:
            assert np.array_equal(_bits(got[n, 0, :h, :w]), _bits(gc.resize(m.numpy(), h, w)))


def test_footprint_of_the_loss_kernels(cuda, golden):
    from cvpce_amd import device_gaussians as dg, torch_ops_gaussians as G
    pred, maps, sizes, _ = _loss_inputs(golden, 'defaults', cuda)
    target = dg.render_maps(maps, [(s[0] // 2, s[1] // 2) for s in sizes], HB, WB)
    for per_image in (0, 1):
        segments = 3 if per_image else 1
        ins = [F.put(pred.cpu(), cuda), F.put(target.cpu(), cuda), F.put(torch.tensor([[48, 64], [40, 50], [32, 45]], dtype=torch.int32), cuda)]
        outs = [F.out((G.loss_workspace_bytes(3, HB, WB),), torch.uint8, cuda), F.out((segments, 3), torch.float32, cuda),
                F.out((segments, 2), torch.int32, cuda)]
        run = lambda: torch.ops.cvpce_amd.gauss_loss(ins[0][0], ins[1][0], ins[2][0] if per_image else None, 0.0, 0.1, 1000, 3, per_image, outs[0][0],
                                                     outs[1][0], outs[2][0])
        _, out_f, out_i = F.check(run, ins, outs, written=[F.SCRATCH, None, None])
        want_f, want_i = dg.loss(pred, target, ins[2][0] if per_image else None)
        assert torch.equal(out_f.view(torch.int32), want_f.view(torch.int32)) and torch.equal(out_i, want_i)


# ---- the accumulator and the harness --------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def scene(cuda):
    from cvpce_amd import synthetic
    model = synthetic.synthetic_gln(seed=3, detections_per_img=20).to(cuda)
    images = [synthetic.shelf_image(40 + k, 384, 512) for k in range(4)]
    boxes = [torch.tensor([[20 + 110 * b + 7 * k, 30 + 9 * k, 95 + 110 * b + 7 * k, 170 + 40 * k] for b in range(4)]) for k in range(4)]
    return model, images, boxes


def test_gaussian_score_equals_the_loss_image_by_image(cuda, scene):
    from cvpce_amd import datautils, device_gaussians as dg
    from cvpce_amd.models import proposals
    model, images, boxes = scene
    score = dg.GaussianScore(model)
    assert score.loss_params == dict(negative_threshold=0.0, positive_threshold=0.1, min_negatives=1000, negatives_per_positive=3) and not score.tanh
    single = []
    for at in (0, 2):
        results = model([i.to(cuda) for i in images[at:at + 2]])
        score.update(results, boxes[at:at + 2], [(384, 512)] * 2)
        for r, b in zip(results, boxes[at:at + 2]):
            assert tuple(r['gaussians'].shape) == (1, 400, 544)
            full = datautils.generate_gaussians(512, 384, b)
            single.append(float(proposals.gaussian_loss(r['gaussians'][None], [full], [proposals.resized_hw(384, 512)])))
    assert score.host_copies == 0 and all(t.is_cuda for t in score._losses)
    out = score.compute()
    assert score.host_copies == 1 and not out['loss'].is_cuda and tuple(out['loss'].shape) == (4,)
    for got, want in zip(out['loss'].tolist(), single):
        assert abs(got - want) <= gc.loss_tolerance(want)
    assert abs(out['mean'] - float(np.mean(single))) <= gc.loss_tolerance(np.mean(single))
    assert abs(out['std'] - float(np.std(single, ddof=1))) <= 1e-5 + 4 * gc.TARGET_TOL
    assert out['outliers'] == [i for i, v in enumerate(out['loss'].tolist()) if v > out['mean'] + 3 * out['std']]
    # an image scored in a batch padded for a wider neighbour counts its own padded extent only: the reference's loss over that corner
    wide = torch.zeros(3, 384, 700)
    mixed = dg.GaussianScore(model)
    results = model([images[0].to(cuda), wide.to(cuda)])
    assert results[0]['gaussians'].shape[2] > 544
    mixed.update(results, [boxes[0], boxes[1]], [(384, 512), (384, 700)])
    corner = results[0]['gaussians'][:, :400, :544].contiguous()[None]
    want = float(proposals.gaussian_loss(corner, [datautils.generate_gaussians(512, 384, boxes[0])], [proposals.resized_hw(384, 512)]))
    assert abs(float(mixed.compute()['loss'][0]) - want) <= gc.loss_tolerance(want)


def test_evaluate_gln_with_and_without_a_score(cuda, scene):
    from cvpce_amd import device_gaussians as dg, proposals_eval
    model, images, boxes = scene
    data = [(img, {'boxes': b}) for img, b in zip(images, boxes)]
    plain = proposals_eval.evaluate_gln_sync(model, data, thresholds=(0.5,), batch_size=2, gaussian_score=None)
    assert list(plain) == [0.5] and 'gaussians' not in plain
    scored = proposals_eval.evaluate_gln_sync(model, data, thresholds=(0.5,), batch_size=2, gaussian_score=dg.GaussianScore(model))
    assert list(scored) == [0.5, 'gaussians'] and tuple(scored['gaussians']['loss'].shape) == (4,)
    assert {k: float(v) for k, v in scored[0.5].items()} == {k: float(v) for k, v in plain[0.5].items()}
    device = proposals_eval.evaluate_gln_sync(model, data, thresholds=(0.5,), batch_size=2, device_metrics=True, gaussian_score=dg.GaussianScore(model))
    assert torch.equal(device['gaussians']['loss'], scored['gaussians']['loss'])
