"""csrc/headloss.hip against the host models of tests/headloss_cases.py: the matching and the counts exactly, on every
anchor; the two losses within 8 x T_ref of the float64 model; identical bits on a second run; nothing read or written outside the
tensors given.  Then the model level: `GaussianLayerNetwork.losses`, the kept head outputs eagerly and under graph replay, and the
graph keys of a model that never asked for them."""
import pytest
import torch

import footprint as fp
import headloss_cases as hc

pytestmark = pytest.mark.gpu


def _base_anchors(dev):
    from cvpce_amd.models import proposals
    return proposals._base_anchors().to(dev)


def _run(case, dev):
    from cvpce_amd import device_headloss
    imgs = case['images']
    return device_headloss.head_losses([c.to(dev) for c in case['cls']], [r.to(dev) for r in case['reg']], case['grids'],
                                       hc.strides(case['padded'], case['grids']), _base_anchors(dev),
                                       [torch.tensor(i['boxes'], dtype=torch.float32).reshape(-1, 4) for i in imgs],
                                       [torch.tensor(i['labels'], dtype=torch.int64) for i in imgs],
                                       device_headloss.scale_factors([i['transformed'] for i in imgs], [i['original'] for i in imgs]))


@pytest.mark.parametrize('name', hc.CASE_NAMES)
def test_kernels_match_the_models(cuda, name):
    case, r32, r64 = hc.reference(name)
    out_f, out_i, matched = (t.cpu() for t in _run(case, cuda))
    again = [t.cpu() for t in _run(case, cuda)]
    for i, (m32, m64) in enumerate(zip(r32, r64)):
        got = matched[i].numpy()
        wrong = int((got != m32['matched']).sum())
        print(f'{name}[{i}]: counts {out_i[i].tolist()} (model {list(m32["counts"])}), {wrong} anchors matched otherwise')
        for k, key in enumerate(('classification', 'bbox_regression')):
            rel = abs(float(out_f[i, k]) - m64[key]) / abs(m64[key]) if m64[key] else abs(float(out_f[i, k]))
            print(f'    {key}: device {float(out_f[i, k])!r} float64 model {m64[key]!r} relative {rel:.3e} (bound {hc.LOSS_RTOL:.3e})')
        assert wrong == 0                                                           # exact, every anchor
        assert tuple(out_i[i].tolist()) == m32['counts']
        for k, key in enumerate(('classification', 'bbox_regression')):
            assert abs(float(out_f[i, k]) - m64[key]) <= hc.LOSS_RTOL * abs(m64[key]), key
    assert torch.equal(out_f.view(torch.int32), again[0].view(torch.int32)) and torch.equal(out_i, again[1]) and torch.equal(matched, again[2])


@pytest.mark.parametrize('name', hc.CASE_NAMES)
def test_kernels_stay_inside_their_tensors(cuda, name):
    """Guard bands around every input and output (tests/footprint.py), for every case: K = 1 (the detector's own class count) and
    K = 3 logits, a single partial chunk, a last partial chunk and anchor tile, an image without boxes inside a batch, and no boxes
    at all."""
    from cvpce_amd import device_headloss, torch_ops_headloss as H
    case, r32, _ = hc.reference(name)
    imgs, grids, n = case['images'], case['grids'], len(case['images'])
    counts = [len(i['boxes']) for i in imgs]
    boxes = torch.tensor([b for i in imgs for b in i['boxes']], dtype=torch.float32).reshape(-1, 4)
    labels = torch.tensor([l for i in imgs for l in i['labels']], dtype=torch.int32)
    offsets = torch.tensor([sum(counts[:i]) for i in range(n + 1)], dtype=torch.int32)
    scales = device_headloss.scale_factors([i['transformed'] for i in imgs], [i['original'] for i in imgs])
    total = hc.NUM_ANCHORS * sum(gh * gw for gh, gw in grids)
    cls = [fp.put(c, cuda) for c in case['cls']]
    reg = [fp.put(r, cuda) for r in case['reg']]
    # (an empty tensor has no address to put guards around: without boxes the op passes null pointers and the arena holds one unused row)
    rest = [fp.put(t, cuda) for t in (_base_anchors(cuda).cpu(), boxes if len(boxes) else torch.zeros((1, 4)),
                                      labels if len(labels) else torch.zeros(1, dtype=torch.int32), offsets, scales)]
    views = [v for v, _ in rest]
    if not len(boxes):
        views[1], views[2] = views[1][:0], views[2][:0]
    nbytes = H.workspace_bytes([g[0] for g in grids], [g[1] for g in grids], hc.NUM_ANCHORS, n, sum(counts))
    assert nbytes > 0
    outs = [fp.out((nbytes,), torch.uint8, cuda), fp.out((n, total), torch.int32, cuda), fp.out((n, 2), torch.float32, cuda),
            fp.out((n, 3), torch.int32, cuda)]
    st = hc.strides(case['padded'], grids)

    def run():
        torch.ops.cvpce_amd.headloss([v for v, _ in cls], [v for v, _ in reg], [g[0] for g in grids], [g[1] for g in grids],
                                     [s[0] for s in st], [s[1] for s in st], *views,
                                     hc.NUM_ANCHORS, case['num_classes'], outs[0][0], outs[1][0], outs[2][0], outs[3][0])

    _, matched, _, out_i = fp.check(run, cls + reg + rest, outs, written=[fp.SCRATCH, None, None, None])
    for i, m32 in enumerate(r32):
        assert (matched[i].cpu().numpy() == m32['matched']).all() and tuple(out_i[i].tolist()) == m32['counts']


def test_arguments_are_refused(cuda):
    from cvpce_amd import torch_ops_headloss as H
    assert H.workspace_bytes([16], [16], 9, 1, 0) > 0
    assert H.workspace_bytes([16], [16], 9, 0, 0) == 0 and H.workspace_bytes([0], [16], 9, 1, 0) == 0
    assert H.workspace_bytes([16] * 9, [16] * 9, 9, 1, 0) == 0                      # more than 8 levels
    assert H.workspace_bytes([4096], [4096], 9, 16, 0) == 0                         # N * A_total past int32
    case = hc.cases()['no_boxes']
    with pytest.raises(RuntimeError):                                               # a workspace that is too small: nothing is launched
        grids, st = case['grids'], hc.strides(case['padded'], case['grids'])
        torch.ops.cvpce_amd.headloss([c.to(cuda) for c in case['cls']], [r.to(cuda) for r in case['reg']], [g[0] for g in grids],
                                     [g[1] for g in grids], [s[0] for s in st], [s[1] for s in st], _base_anchors(cuda),
                                     torch.zeros((0, 4), device=cuda), torch.zeros(0, dtype=torch.int32, device=cuda),
                                     torch.zeros(2, dtype=torch.int32, device=cuda), torch.ones((1, 2), device=cuda), hc.NUM_ANCHORS, 3,
                                     torch.empty(16, dtype=torch.uint8, device=cuda), torch.empty((1, 3069), dtype=torch.int32, device=cuda),
                                     torch.empty((1, 2), device=cuda), torch.empty((1, 3), dtype=torch.int32, device=cuda))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------------
# model level: a seeded detector at a small transform size, two images
# ---------------------------------------------------------------------------------------------------------------------------------
def _model(cuda):
    from cvpce_amd import synthetic
    return synthetic.synthetic_gln(seed=0, detections_per_img=40, min_size=256, max_size=384).to(cuda)


@pytest.fixture(scope='module')
def world(cuda):
    from cvpce_amd import synthetic
    model = _model(cuda)
    images = [synthetic.shelf_image(3, 200, 260).to(cuda), synthetic.shelf_image(4, 180, 300).to(cuda)]
    targets = [{'boxes': torch.tensor([[10, 12, 60, 70], [100, 40, 190, 150], [30, 100, 75, 190]]), 'labels': torch.zeros(3, dtype=torch.long)},
               {'boxes': torch.tensor([[5, 5, 120, 90], [150, 60, 200, 110]]), 'labels': torch.zeros(2, dtype=torch.long)}]
    return model, images, targets


def _same(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))


def test_graph_keys_and_kept_head_outputs(world, cuda):
    """On a model of its own, which has never been asked for its head outputs: the graph keys and replay counts below do not depend
    on what the other tests did to the shared one."""
    _, images, _ = world
    model = _model(cuda)
    eng = model.engine()
    plain = [model(images) for _ in range(3)]                                       # eager, capture + replay, replay
    original, resized, padded = eng.batch_geometry(images, eng.min_size, eng.max_size)
    parent_key = (len(images), padded, tuple(resized), tuple(original), model.num_classes, model.detections_per_img, 0.5, eng.detect_options())
    assert list(eng._graphs) == [parent_key]                                        # the key of the parent commit, nothing appended
    assert model.head_outputs() is None
    model.keep_head_outputs(True)
    kept, results = [], []
    for _ in range(3):                                                              # eager, capture + replay, replay (another graph)
        results.append(model(images))
        kept.append(model.head_outputs())
        assert model.head_outputs() is None                                         # handed out once
    model.keep_head_outputs(False)
    assert list(eng._graphs) == [parent_key, parent_key + ('head_outputs',)]
    assert eng._graphs[parent_key + ('head_outputs',)]['replays'] == 1
    for h in kept:
        assert len(h['cls']) == len(h['reg']) == 5 and h['padded'] == tuple(padded) and h['sizes'] == list(resized)
        for a, b in zip(h['cls'] + h['reg'], kept[0]['cls'] + kept[0]['reg']):
            assert _same(a, b)
    _, inter = eng.detect(images, model.num_classes, model.detections_per_img, want_intermediates=True)
    for a, b in zip(kept[0]['cls'] + kept[0]['reg'], list(inter['cls']) + list(inter['reg'])):
        assert _same(a, b) and a.dtype == torch.float32
    for res in results + plain[1:]:
        for r, p in zip(res, plain[0]):
            assert all(_same(r[k], p[k]) for k in ('boxes', 'scores', 'labels', 'gaussians'))
    after = model(images)                                                           # the plain graph again
    assert eng._graphs[parent_key]['replays'] == 2 and model.head_outputs() is None
    assert all(_same(r[k], p[k]) for r, p in zip(after, plain[0]) for k in ('boxes', 'scores', 'labels', 'gaussians'))


def test_model_losses_are_head_losses_of_the_pass(world):
    from cvpce_amd import datautils, device_gaussians, device_headloss
    from cvpce_amd.models import proposals
    model, images, targets = world
    eng = model.engine()
    res = model.losses(images, targets)
    assert set(res) == {'classification', 'bbox_regression', 'gaussian'}
    assert all(v.is_cuda and v.dim() == 0 and v.dtype == torch.float32 for v in res.values())
    assert model.head_outputs() is None and model._keep_head_outputs is False
    out, inter = eng.detect(images, model.num_classes, model.detections_per_img, want_intermediates=True)
    original, resized, padded = eng.batch_geometry(images, eng.min_size, eng.max_size)
    grids = [(c.shape[1], c.shape[2]) for c in inter['cls']]
    strides = [(padded[0] // g[0], padded[1] // g[1]) for g in grids]
    out_f, out_i, _ = device_headloss.head_losses(inter['cls'], inter['reg'], grids, strides, eng.base_anchors, [t['boxes'] for t in targets],
                                                  [t['labels'] for t in targets], device_headloss.scale_factors(resized, original))
    assert int(out_i[:, 0].min()) > 0                                               # both images have foreground: the L1 loss is exercised
    assert _same(res['classification'], out_f[:, 0].mean()) and _same(res['bbox_regression'], out_f[:, 1].mean())
    assert bool(torch.isfinite(torch.stack(list(res.values()))).all()) and float(res['bbox_regression']) > 0
    # the Gaussian loss, both ways.  Maps rendered from the integer boxes: the targets launch and the batch-scope loss by hand on the same
    # pass's map ...
    gauss = out[5]
    hb, wb = gauss.shape[2:]
    geom = [(h0, w0, 1, rh // 2, rw // 2) for (h0, w0), (rh, rw) in zip(original, resized)]
    maps = device_gaussians.render_boxes([t['boxes'] for t in targets], geom, hb, wb, device=gauss.device)
    assert not _same(maps, torch.zeros_like(maps))
    by_hand = device_gaussians.loss(gauss.to(torch.float32), maps, None)[0][0, 0]
    assert _same(res['gaussian'], by_hand) and float(by_hand) > 0
    # ... and the reference's own route: full-resolution maps of generate_gaussians through gaussian_loss, which resizes them (the fused
    # launch has the bits of render-then-resize: test_gpu_gaussians.py).  Targets that carry 'gaussians' take that route in `losses`.
    full = [datautils.generate_gaussians(w0, h0, t['boxes']) for (h0, w0), t in zip(original, targets)]
    reference_way = proposals.gaussian_loss(gauss, full, resized)
    assert _same(res['gaussian'], reference_way)
    with_maps = model.losses(images, [dict(t, gaussians=m) for t, m in zip(targets, full)])
    assert set(with_maps) == set(res) and all(_same(with_maps[k], res[k]) for k in res)
    float_boxes = [dict(t, boxes=t['boxes'].float()) for t in targets]              # not integers, no maps given: nothing to score
    assert set(model.losses(images, float_boxes)) == {'classification', 'bbox_regression'}
    with_maps = model.losses(images, [dict(t, gaussians=m) for t, m in zip(float_boxes, full)])
    assert _same(with_maps['gaussian'], reference_way)                              # maps given: float boxes are no obstacle
    model.train()
    with pytest.raises(NotImplementedError):
        model(images, targets)
    model.eval()


def test_evaluate_gln_reports_head_losses(world):
    from cvpce_amd import device_headloss, proposals_eval
    model, images, targets = world
    data = [(img, t) for img, t in zip(images, targets)]
    plain = proposals_eval.evaluate_gln_sync(model, data, batch_size=2)
    score = device_headloss.HeadScore(model)
    scored = proposals_eval.evaluate_gln_sync(model, data, batch_size=2, head_score=score)
    assert 'head_losses' not in plain and set(scored) == set(plain) | {'head_losses'}
    assert all(scored[thr]['ap'] == plain[thr]['ap'] and scored[thr]['ar_300'] == plain[thr]['ar_300'] for thr in plain)
    assert score.host_copies == 1 and score.images == 2 and model._keep_head_outputs is False
    res = model.losses(images, targets)
    heads = scored['head_losses']
    assert tuple(heads['counts'].shape) == (2, 3) and int(heads['counts'][:, 0].min()) > 0
    for key in ('classification', 'bbox_regression'):
        assert tuple(heads[key]['loss'].shape) == (2,)
        assert _same(heads[key]['loss'].mean(), res[key].cpu())
