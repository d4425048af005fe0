"""GaussianLayerNetwork accepts torchvision 0.9 RetinaNet's inference keywords (the reference passes **kwargs on to RetinaNet,
/root/reference/cvpce/models/proposals.py:162-166): validation, storage under torchvision's attribute names, head widths that
follow the anchors, and the host side of the post-processing's larger top-k capacity.  No GPU needed."""
import hashlib

import pytest
import torch

# sha256 over "key:shape;..." of a default-built model's state dict (num_classes 1 and 3), as the code before these options built it
DEFAULT_SD = {1: (327, '2cfce99fedbb232fc7373fef97db97b79cc28771e0c273048571205ffd4406fe'),
              3: (327, '116dbf9c321f8ac504470a95c3004fe889fe3bc034a7160ce690bafe7894f10a')}


class Anchors:
    """Duck-typed torchvision AnchorGenerator (torchvision is not installed)."""

    def __init__(self, sizes, aspect_ratios):
        self.sizes, self.aspect_ratios = sizes, aspect_ratios


def _model(num_classes=1, **kw):
    from cvpce_amd.models import proposals as P
    return P.GaussianLayerNetwork(P.gln_backbone(4, pretrained=False), num_classes, **kw)


def _fingerprint(model):
    sd = model.state_dict()
    return len(sd), hashlib.sha256(';'.join(f'{k}:{tuple(v.shape)}' for k, v in sd.items()).encode()).hexdigest()


@pytest.mark.parametrize('num_classes', [1, 3])
def test_default_state_dict_is_unchanged(num_classes):
    assert _fingerprint(_model(num_classes)) == DEFAULT_SD[num_classes]


def test_defaults_are_torchvision_s():
    from cvpce_amd.models import proposals as P
    m = _model()
    assert m.transform.min_size == (800,) and m.transform.max_size == 1333
    assert tuple(m.transform.image_mean) == P.IMAGE_MEAN and tuple(m.transform.image_std) == P.IMAGE_STD
    assert (m.score_thresh, m.nms_thresh, m.topk_candidates, m.detections_per_img) == (0.05, 0.5, 1000, 1000)
    assert m.anchor_generator.sizes == P.ANCHOR_SIZES
    assert all(tuple(r) == P.ASPECT_RATIOS for r in m.anchor_generator.aspect_ratios)
    assert torch.equal(P._base_anchors(*P._anchor_spec(m.anchor_generator)), P._base_anchors())
    assert P.resized_hw(600, 900) == P.resized_hw(600, 900, 800, 1333) == (800, 1200)


def test_every_keyword_is_stored_under_torchvision_s_name():
    gen = Anchors(((16, 24), (32, 48), (64, 96), (128, 192), (256, 384)), ((0.5, 1.0, 2.0),) * 5)
    m = _model(min_size=1024, max_size=1707, image_mean=[0.5, 0.4, 0.3], image_std=(0.2, 0.25, 0.3), score_thresh=0.2,
               nms_thresh=0.6, topk_candidates=3000, detections_per_img=2500, anchor_generator=gen, fg_iou_thresh=0.6,
               bg_iou_thresh=0.3)
    assert m.transform.min_size == (1024,) and m.transform.max_size == 1707
    assert list(m.transform.image_mean) == [0.5, 0.4, 0.3] and list(m.transform.image_std) == [0.2, 0.25, 0.3]
    assert (m.score_thresh, m.nms_thresh, m.topk_candidates, m.detections_per_img) == (0.2, 0.6, 3000, 2500)
    assert m.anchor_generator is gen
    assert (m.fg_iou_thresh, m.bg_iou_thresh) == (0.6, 0.3)
    assert m._detect_options() == (3000, 0.2, 0.6)
    m2 = _model(min_size=(640, 672, 704), max_size=1333)
    assert m2.transform.min_size == (640, 672, 704)


def test_tuple_min_size_resizes_to_its_last_entry():
    from cvpce_amd.models import proposals as P
    m = _model(min_size=(800, 1024), max_size=1707)
    assert P.resized_hw(1536, 2048, m.transform.min_size[-1], m.transform.max_size) == (1024, 1365)
    assert P.resized_hw(1000, 3000, 1024, 1707) == (569, 1706)     # the long side caps the scale (floor of 1706.99...)


@pytest.mark.parametrize('kw', [dict(min_size=0), dict(min_size=1601), dict(min_size=(800, 0)), dict(min_size=()), dict(min_size=800.5),
                                dict(max_size=0), dict(max_size=2668), dict(image_mean=(0.5, 0.5)), dict(image_std=(0.2, 0.0, 0.2)),
                                dict(image_std=(0.2, -0.1, 0.2)), dict(image_mean=(0.1, float('nan'), 0.2)), dict(score_thresh=-0.01),
                                dict(score_thresh=1.0), dict(nms_thresh=0.0), dict(nms_thresh=1.01), dict(topk_candidates=0),
                                dict(topk_candidates=4097), dict(topk_candidates=2.0), dict(detections_per_img=0),
                                dict(detections_per_img=8193), dict(topk_candidates=4096, detections_per_img=20481)])
def test_out_of_range_values_raise_value_error(kw):
    with pytest.raises(ValueError):
        _model(**kw)


def test_bounds_themselves_are_accepted():
    m = _model(min_size=1600, max_size=2667, score_thresh=0.0, nms_thresh=1.0, topk_candidates=4096, detections_per_img=20480)
    assert m.transform.min_size == (1600,) and m.topk_candidates == 4096
    assert _model(topk_candidates=1, detections_per_img=8192).detections_per_img == 8192


@pytest.mark.parametrize('name', ['head', 'proposal_matcher', 'batch_size_per_image', 'not_an_option'])
def test_unsupported_keywords_raise_type_error_naming_them(name):
    with pytest.raises(TypeError, match=name):
        _model(**{name: object()})


@pytest.mark.parametrize('a,sizes,ratios', [
    (12, tuple((s, int(s * 1.26), int(s * 1.59), s * 2) for s in (32, 64, 128, 256, 512)), (0.5, 1.0, 2.0)),
    (15, ((32, 40, 50),) * 5, ((0.25, 0.5, 1.0, 2.0, 4.0),) * 5),
])
@pytest.mark.parametrize('num_classes', [1, 3])
def test_custom_anchor_generator_sets_head_widths(a, sizes, ratios, num_classes):
    from cvpce_amd.models import proposals as P
    m = _model(num_classes, anchor_generator=Anchors(sizes, ratios))
    sd = m.state_dict()
    assert tuple(sd['head.classification_head.cls_logits.weight'].shape) == (a * num_classes, 256, 3, 3)
    assert tuple(sd['head.classification_head.cls_logits.bias'].shape) == (a * num_classes,)
    assert tuple(sd['head.regression_head.bbox_reg.weight'].shape) == (4 * a, 256, 3, 3)
    assert tuple(sd['head.regression_head.bbox_reg.bias'].shape) == (4 * a,)
    assert sorted(sd) == sorted(_model(num_classes).state_dict())        # the same keys
    base = P._base_anchors(*P._anchor_spec(m.anchor_generator))
    assert tuple(base.shape) == (5, a, 4)
    # torchvision's cell anchors: ratios outer, scales inner, rounded half sizes
    r = torch.tensor(P._anchor_spec(m.anchor_generator)[1][0])
    s = torch.tensor(P._anchor_spec(m.anchor_generator)[0][0], dtype=torch.float32)
    ws = ((1 / r.sqrt())[:, None] * s[None, :]).reshape(-1)
    assert torch.equal(base[0, :, 2], (ws / 2).round())


@pytest.mark.parametrize('gen,num_classes', [
    (Anchors(((32,), (64,), (128,), (256,)), ((1.0,),) * 4), 1),                        # 4 levels
    (Anchors(((32, 40), (64,), (128,), (256,), (512,)), ((1.0,),) * 5), 1),             # unequal A
    (Anchors(((32, 40, 50, 64),) * 5, ((0.5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0, 7.0, 8.0),) * 5), 1),   # 4A = 144 > 128
    (Anchors(((32, 40, 50),) * 5, ((0.5, 1.0, 2.0),) * 5), 15),                          # A * K = 135 > 128
    (Anchors(((32, -40, 50),) * 5, ((0.5, 1.0, 2.0),) * 5), 1),                          # negative size
])
def test_bad_anchor_generators_raise_value_error(gen, num_classes):
    with pytest.raises(ValueError):
        _model(num_classes, anchor_generator=gen)


def test_flat_sequences_are_normalised_like_torchvision():
    from cvpce_amd.models import proposals as P
    sizes, ratios = P._anchor_spec(Anchors((32, 64, 128, 256, 512), (0.5, 1.0, 2.0)))
    assert sizes == ((32,), (64,), (128,), (256,), (512,)) and ratios == ((0.5, 1.0, 2.0),) * 5
    assert tuple(_model(anchor_generator=Anchors((32, 64, 128, 256, 512), (0.5, 1.0, 2.0))).state_dict()[
        'head.regression_head.bbox_reg.bias'].shape) == (12,)


def test_detection_attributes_are_checked_when_read():
    m = _model()
    m.score_thresh, m.topk_candidates = 0.3, 2000
    assert m._detect_options() == (2000, 0.3, 0.5)
    m.nms_thresh = 0.0
    with pytest.raises(ValueError):
        m._detect_options()


def test_synthetic_gln_passes_options_through():
    from cvpce_amd import synthetic
    base = synthetic.synthetic_gln(seed=0, calibrate=False)
    m = synthetic.synthetic_gln(seed=0, calibrate=False, min_size=1024, max_size=1707, score_thresh=0.1)
    assert m.transform.min_size == (1024,) and m.score_thresh == 0.1
    a, b = base.state_dict(), m.state_dict()
    assert all(torch.equal(a[k], b[k]) for k in a)          # the same weights: only the options differ


@pytest.mark.parametrize('n,L,topk,ws', [(1, 5, 1000, 3972604), (4, 5, 1000, 15878128), (2, 5, 1024, 8114232), (3, 8, 1024, 28905592),
                                         (1, 1, 1, 104744)])
def test_default_capacity_workspace_is_unchanged(n, L, topk, ws):
    from cvpce_amd._lib import lib
    assert lib.cvpce_detect_workspace_bytes(n, L, topk) == ws


@pytest.mark.parametrize('n,topk', [(1, 1025), (1, 4096), (4, 1500), (2, 4096)])
def test_wide_capacity_workspace_holds_the_mask(n, topk):
    from cvpce_amd._lib import lib
    tmax = (5 * topk + 63) // 64 * 64
    ws = lib.cvpce_detect_workspace_bytes(n, 5, topk)
    assert ws >= n * tmax * tmax // 8 + n * 5 * 12 * 4096 * 8         # the IoU bit matrix and 4096-entry chunk runs
    assert ws > lib.cvpce_detect_workspace_bytes(n, 5, 1024)
