"""RetinaNet's inference keywords on the GPU (GaussianLayerNetwork(**kwargs)).

* the post-processing at the wide capacity (topk_candidates up to 4096, up to 20 480 candidates per image) against the oracle on
  identical logits, chunked and one-kernel decode bit-identical, one- and two-phase NMS bit-identical;
* the whole detector with non-default thresholds, transform sizes (int and tuple min_size, up to 1600 / 2667), mean / std and
  anchors against the fp32 oracle with tests/test_gpu_configs1.py's fp16 tolerances (the oracle's module constants are
  monkeypatched where it reads them);
* attributes changed after a geometry's graph was captured take effect on the next call;
* the defaults spelled out give the default model's outputs bit for bit."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


class Anchors:
    """Duck-typed torchvision AnchorGenerator."""

    def __init__(self, sizes, aspect_ratios):
        self.sizes, self.aspect_ratios = sizes, aspect_ratios


ANCHORS12 = tuple((s, int(s * 2 ** 0.25), int(s * 2 ** 0.5), int(s * 2 ** 0.75)) for s in (32, 64, 128, 256, 512))   # A = 4 x 3


def _random_head_outputs(n, grids, a, k, seed, spread=2.0, bias=-1.0, quantum=0.0):
    g = torch.Generator().manual_seed(seed)
    cls = [torch.randn(n, gh * gw * a * k, generator=g) * spread + bias for gh, gw in grids]
    if quantum:                        # logits on a coarse grid: exact ties at the top-k cuts and in the NMS order
        # (+ 0.0 turns -0.0 into +0.0: the kernels order by the logit's bit pattern, where -0.0 < +0.0, while torch.sort ties them)
        cls = [torch.round(c / quantum) * quantum + 0.0 for c in cls]
    reg = [torch.randn(n, gh * gw * a, 4, generator=g) * 0.5 for gh, gw in grids]
    return cls, reg


SMALL = ((512, 640), [(64, 80), (32, 40), (16, 20), (8, 10), (4, 5)], [(500, 640), (512, 600)], [(1000, 1280), (700, 820)])
LARGE = ((800, 832), [(100, 104), (50, 52), (25, 26), (13, 13), (7, 7)], [(800, 810), (790, 832)], [(2048, 2073), (1000, 1053)])


@pytest.mark.parametrize('geom,topk,dpi,k,seed,bias,quantum,score_thresh,nms_thresh', [
    (SMALL, 1500, 3000, 1, 0, 0.5, 0.25, 0.05, 0.5),     # chunked decode at the wide capacity (P3: 6 chunks)
    (SMALL, 4096, 3000, 2, 1, 1.0, 0.125, 0.2, 0.6),     # P3 12 chunks at k = 2: the one-kernel decode; ties
    (SMALL, 4096, 1000, 1, 2, 1.0, 0.0, 0.05, 0.1),      # NMS phase 1 keeps < dpi of its 8000: phase 2 over all candidates
    (LARGE, 4096, 3000, 1, 3, 0.0, 0.5, 0.05, 0.5),      # 14 000+ candidates per image, many exact ties
    (LARGE, 2048, 2500, 3, 4, -1.0, 0.0, 0.3, 0.45),
])
def test_postprocess_parity_at_the_wide_capacity(cuda, geom, topk, dpi, k, seed, bias, quantum, score_thresh, nms_thresh, monkeypatch):
    from cvpce_amd import ops
    from cvpce_amd.models import proposals as P
    from oracle import gln as og
    import detect_plan as dp
    padded, grids, resized, original = geom
    n = 2
    rc, plan = dp.query(grids, n, 9, k, topk, dpi)
    assert rc == 0 and plan['cap'] == 4096
    if (geom, topk, k) == (SMALL, 1500, 1):      # chunked decode at the wide capacity, P3 of 46 080 logits in 6 chunks
        assert (plan['chunked'], plan['chunk_first1']) == (1, 6)
    if (geom, topk, k) == (SMALL, 4096, 2):      # P3 of 92 160 logits: 12 chunks, one merge workgroup holds 8 runs of 4096
        assert (plan['chunked'], plan['why'], plan['chunk_first1']) == (0, dp.MERGE_LIMIT, 8)
    cls, reg = _random_head_outputs(n, grids, 9, k, seed, bias=bias, quantum=quantum)
    anchors = og.grid_anchors(padded, grids)
    strides = [(padded[0] // gh, padded[1] // gw) for gh, gw in grids]
    image_hw = torch.tensor(resized, dtype=torch.int32)
    ratios = torch.stack([torch.tensor(o, dtype=torch.float32) / torch.tensor(r, dtype=torch.float32)
                          for o, r in zip(original, resized)])

    def run():
        out = ops.detect_postprocess([c.to(cuda) for c in cls], [r.to(cuda) for r in reg], grids, strides, P._base_anchors().to(cuda),
                                     image_hw.to(cuda), ratios.to(cuda), 9, k, topk, score_thresh, nms_thresh, og.BBOX_XFORM_CLIP, dpi, 0.5)
        torch.cuda.synchronize()
        return out

    boxes, scores, labels, count, conf = out = run()
    for i in range(n):
        b, s, l = og.postprocess_image([c[i].view(-1, k) for c in cls], [r[i] for r in reg], anchors, resized[i], dpi,
                                       score_thresh=score_thresh, nms_thresh=nms_thresh, topk=topk)
        b = og.resize_boxes(b, resized[i], original[i])
        c = int(count[i])
        assert c == len(b), (c, len(b))
        torch.testing.assert_close(scores[i, :c].cpu(), s, rtol=0, atol=1e-6)
        torch.testing.assert_close(boxes[i, :c].cpu(), b, rtol=1e-5, atol=2e-3)
        assert torch.equal(labels[i, :c].cpu(), l)
        assert int(conf[i]) == int((s > 0.5).sum())
        assert bool((scores[i, c:] == 0).all())
    ncand = [sum(min(topk, int((torch.sigmoid(c[i]) > score_thresh).sum())) for c in cls) for i in range(n)]
    assert max(ncand) > 1024 * 5 // 2            # beyond what one 1024-entry segment per level could hold in places
    limit = max(1024, dpi * 8)
    if nms_thresh == 0.1:                        # the phase-2 case: phase 1 could not finish an image
        assert any(nc > limit and int(count[i]) < dpi for i, nc in enumerate(ncand)), (ncand, count.tolist())
    monkeypatch.setenv('CVPCE_DECODE_ONE_KERNEL', '1')
    for x, y in zip(run(), out):
        assert torch.equal(x, y)
    monkeypatch.delenv('CVPCE_DECODE_ONE_KERNEL')
    monkeypatch.setenv('CVPCE_NMS_ONE_PHASE', '1')
    for x, y in zip(run(), out):
        assert torch.equal(x, y)


def test_postprocess_rejects_topk_beyond_the_capacity(cuda):
    from cvpce_amd import ops
    from cvpce_amd.models import proposals as P
    grids = [(8, 8)]
    lg, reg = torch.zeros(1, 576, device=cuda), torch.zeros(1, 576, 4, device=cuda)
    args = ([lg], [reg], grids, [(8, 8)], P._base_anchors()[:1].contiguous().to(cuda), torch.tensor([[64, 64]], dtype=torch.int32).to(cuda),
            torch.ones(1, 2).to(cuda), 9, 1)
    with pytest.raises(RuntimeError):
        ops.detect_postprocess(*args, 4097, 0.05, 0.5, 4.0, 100, 0.5)


# ---------------------------------------------------------------------------
# whole detector
# ---------------------------------------------------------------------------
DPI = 1000


def _compare(det_out, orc, i=0, tol_scale=1.0, dscore_tol=1e-4):
    """tests/test_gpu_configs1.py's fp16 tolerances (box error in original pixels scaled by `tol_scale`)."""
    import accuracy
    boxes, scores, labels, count, conf, gauss = det_out
    n0 = int(count[i])
    hb, hs = boxes[i, :n0].cpu(), scores[i, :n0].cpu()
    assert abs(n0 - len(orc['boxes'])) <= 0.02 * len(orc['boxes']) + 2, (n0, len(orc['boxes']))
    pairs = accuracy.pair_boxes(hb, orc['boxes'])
    frac = len(pairs) / max(1, len(orc['boxes']))
    a, b = torch.tensor(pairs).t()
    dscore = (hs[a] - orc['scores'][b]).abs().mean()
    dbox = (hb[a] - orc['boxes'][b]).abs().max(dim=1).values.mean()
    dg = (gauss[i].cpu() - orc['gaussians']).norm() / orc['gaussians'].norm()
    assert frac >= 0.97 and dscore < dscore_tol and dbox < 0.5 * tol_scale and dg < 0.03, (frac, float(dscore), float(dbox), float(dg))
    s = scores[i, :n0]
    assert bool((s[:-1] >= s[1:]).all()) and int(conf[i]) == int((s > 0.5).sum())


def _detect_twice(det, imgs):
    """eager call, then the captured graph's first replay: bit-identical"""
    eng = det.engine()
    a = eng.detect(imgs, det.num_classes, det.detections_per_img)
    b = eng.detect(imgs, det.num_classes, det.detections_per_img)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    return a


@pytest.fixture(scope='module')
def default_scene(cuda):
    from cvpce_amd import synthetic
    from oracle import gln as og
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    img = synthetic.shelf_image(7, 1024, 1024)
    sd = {k: v.clone() for k, v in synthetic.synthetic_gln(seed=0, detections_per_img=DPI).state_dict().items()}
    res, inter = og.gln_forward([img], sd, detections_per_img=DPI, return_intermediates=True)
    return img, res[0], inter


def test_thresholds_and_topk(cuda, default_scene):
    from cvpce_amd import synthetic
    from oracle import gln as og
    img, _, inter = default_scene
    opts = dict(score_thresh=0.3, nms_thresh=0.4, topk_candidates=2000)
    det = synthetic.synthetic_gln(seed=0, detections_per_img=1500, **opts).to(cuda)
    out = _detect_twice(det, [img.to(cuda)])
    hw = inter['image_sizes'][0]
    b, s, l = og.postprocess_image([c[0] for c in inter['cls']], [r[0] for r in inter['reg']], inter['anchors'], hw, 1500,
                                   score_thresh=0.3, nms_thresh=0.4, topk=2000)
    orc = {'boxes': og.resize_boxes(b, hw, tuple(img.shape[-2:])), 'scores': s, 'gaussians': inter['gaussians'][0]}
    assert len(s) > 300 and float(s.min()) > 0.3
    _compare(out, orc)


@pytest.fixture(scope='module')
def large_scene(cuda):
    """min_size 1024, max_size 1707 on a 1536 x 2048 image (the oracle reads MIN_SIZE / MAX_SIZE as module constants)"""
    from cvpce_amd import synthetic
    from oracle import gln as og
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    img = synthetic.shelf_image(8, 1536, 2048)
    sd = {k: v.clone() for k, v in synthetic.synthetic_gln(seed=0, detections_per_img=DPI).state_dict().items()}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(og, 'MIN_SIZE', 1024)
        mp.setattr(og, 'MAX_SIZE', 1707)
        orc = og.gln_forward([img], sd, detections_per_img=DPI)[0]
    return img, orc


def test_min_size_max_size(cuda, large_scene):
    from cvpce_amd import synthetic
    img, orc = large_scene
    det = synthetic.synthetic_gln(seed=0, detections_per_img=DPI, min_size=1024, max_size=1707).to(cuda)
    out = _detect_twice(det, [img.to(cuda)])
    assert out[-1].shape == (1, 1, 512, 688)                # the Gaussian map of the padded 1024 x 1376 batch
    assert orc['gaussians'].shape == (1, 512, 688)
    _compare(out, orc, tol_scale=1.5)
    # a tuple min_size resizes to its last entry: the same detector, bit for bit
    det_t = synthetic.synthetic_gln(seed=0, detections_per_img=DPI, min_size=(640, 800, 1024), max_size=1707).to(cuda)
    for x, y in zip(_detect_twice(det_t, [img.to(cuda)]), out):
        assert torch.equal(x, y)
    # and through the public forward
    res = det([img.to(cuda)])[0]
    assert res['gaussians'].shape == (1, 512, 688) and len(res['boxes']) == int(out[3][0])


def test_largest_transform_size(cuda):
    """min_size 1600, max_size 2667 (the largest maps the HIP path is checked for: padded 1600 x 2688) against the oracle"""
    from cvpce_amd import synthetic
    from oracle import gln as og
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    img = synthetic.shelf_image(9, 1200, 2000)
    det = synthetic.synthetic_gln(seed=0, detections_per_img=DPI, min_size=1600, max_size=2667).to(cuda)
    out = _detect_twice(det, [img.to(cuda), img.flip(-1).to(cuda)])
    assert out[-1].shape == (2, 1, 800, 1344)
    sd = {k: v.clone() for k, v in synthetic.synthetic_gln(seed=0, detections_per_img=DPI).state_dict().items()}
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(og, 'MIN_SIZE', 1600)
        mp.setattr(og, 'MAX_SIZE', 2667)
        orc = og.gln_forward([img], sd, detections_per_img=DPI)[0]
    _compare(out, orc, tol_scale=1.0)


def test_image_mean_std(cuda, monkeypatch):
    from cvpce_amd import synthetic
    from oracle import gln as og
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    mean, std = (0.4, 0.5, 0.6), (0.3, 0.2, 0.25)
    img = synthetic.shelf_image(10, 900, 1100)
    det = synthetic.synthetic_gln(seed=0, detections_per_img=DPI, image_mean=mean, image_std=std).to(cuda)
    out = _detect_twice(det, [img.to(cuda)])
    sd = {k: v.clone() for k, v in synthetic.synthetic_gln(seed=0, detections_per_img=DPI).state_dict().items()}
    monkeypatch.setattr(og, 'IMAGE_MEAN', mean)
    monkeypatch.setattr(og, 'IMAGE_STD', std)
    _compare(out, og.gln_forward([img], sd, detections_per_img=DPI)[0])


def test_custom_anchor_generator(cuda, monkeypatch):
    from cvpce_amd import synthetic
    from oracle import gln as og
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    img = synthetic.shelf_image(11, 1024, 1024)
    model = synthetic.synthetic_gln(seed=0, detections_per_img=DPI, anchor_generator=Anchors(ANCHORS12, (0.5, 1.0, 2.0)))
    assert model.head.regression_head.bbox_reg.out_channels == 48
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    out = _detect_twice(model.to(cuda), [img.to(cuda)])
    monkeypatch.setattr(og, 'ANCHOR_SIZES', ANCHORS12)      # (grid_anchors reads it; base_anchors' ratios stay (0.5, 1, 2))
    # (mean score error 1.07e-4 measured: a third more anchors than the configs1 detector, the same fp16 storage)
    _compare(out, og.gln_forward([img], sd, detections_per_img=DPI)[0], dscore_tol=2e-4)


def test_changing_attributes_after_capture(cuda):
    from cvpce_amd import synthetic
    img = synthetic.shelf_image(12, 800, 1000).to(cuda)
    det = synthetic.synthetic_gln(seed=0, detections_per_img=DPI).to(cuda)
    before = [det([img])[0] for _ in range(3)]              # eager, capture, replay
    torch.cuda.synchronize()
    det.score_thresh, det.nms_thresh, det.topk_candidates = 0.6, 0.3, 1200
    after = det([img])[0]
    fresh = synthetic.synthetic_gln(seed=0, detections_per_img=DPI, score_thresh=0.6, nms_thresh=0.3, topk_candidates=1200).to(cuda)([img])[0]
    torch.cuda.synchronize()
    assert len(after['boxes']) != len(before[-1]['boxes'])
    assert float(after['scores'].min()) > 0.6
    for key in ('boxes', 'scores', 'labels', 'gaussians'):
        assert torch.equal(before[0][key], before[2][key])
        assert torch.equal(after[key], fresh[key])
    again = det([img])[0]                                   # the new options' geometry: captured on its second call
    det.score_thresh, det.nms_thresh, det.topk_candidates = 0.05, 0.5, 1000
    back = det([img])[0]                                    # the first options' graph is still cached: replayed
    for key in ('boxes', 'scores', 'labels', 'gaussians'):
        assert torch.equal(again[key], after[key])
        assert torch.equal(back[key], before[0][key])
    det.nms_thresh = 1.5
    with pytest.raises(ValueError):
        det([img])


def test_defaults_spelled_out_are_bit_identical(cuda):
    from cvpce_amd import synthetic
    from cvpce_amd.models import proposals as P
    imgs = [synthetic.shelf_image(13, 700, 900).to(cuda), synthetic.shelf_image(14, 700, 900).to(cuda)]
    default = synthetic.synthetic_gln(seed=0, detections_per_img=DPI).to(cuda)
    explicit = synthetic.synthetic_gln(seed=0, detections_per_img=DPI, min_size=800, max_size=1333, image_mean=P.IMAGE_MEAN,
                                       image_std=P.IMAGE_STD, score_thresh=0.05, nms_thresh=0.5, topk_candidates=1000,
                                       anchor_generator=Anchors(P.ANCHOR_SIZES, (P.ASPECT_RATIOS,) * 5), fg_iou_thresh=0.5,
                                       bg_iou_thresh=0.4).to(cuda)
    a, b = _detect_twice(default, imgs), _detect_twice(explicit, imgs)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
