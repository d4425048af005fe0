"""GLN dense-product detector on MI355X -- drop-in for
/root/reference/cvpce/models/proposals.py (`gln`, `gln_backbone`,
`GaussianLayerNetwork`; inference only).

The reference builds the detector by subclassing torchvision 0.9's RetinaNet
(proposals.py:162-168) over ResNet-50(FrozenBN)+FPN(+P6,P7) and adds a Gaussian
branch fed by C2 and P3 (proposals.py:109-139).  Here the nn.Modules are only
*parameter containers* that reproduce the reference's state-dict key names
 so released checkpoints load unchanged; the forward pass is a
fixed schedule of hand-written HIP kernels (cvpce_amd/csrc) over NHWC bf16
activations -- transform gather, MFMA implicit-GEMM convolutions with folded
FrozenBN/BN and fused residual / upsample-add / ReLU epilogues, LDS radix-select
top-k, bitmask NMS.  There is no CPU path: tensors must live on a HIP device.
"""
import math
import numbers
import os
import weakref
from collections import OrderedDict

import torch
from torch import nn

from .. import ops
from ..datautils import image_hw

# ---- torchvision 0.9 RetinaNet / transform constants ----
MIN_SIZE, MAX_SIZE, SIZE_DIVISIBLE = 800, 1333, 32
IMAGE_MEAN = (0.485, 0.456, 0.406)
IMAGE_STD = (0.229, 0.224, 0.225)
SCORE_THRESH, NMS_THRESH, TOPK_CANDIDATES = 0.05, 0.5, 1000
BBOX_XFORM_CLIP = math.log(1000.0 / 16)
ANCHOR_SIZES = tuple((x, int(x * 2 ** (1.0 / 3)), int(x * 2 ** (2.0 / 3))) for x in (32, 64, 128, 256, 512))
ASPECT_RATIOS = (0.5, 1.0, 2.0)
FPN_CHANNELS = 256
NUM_LEVELS = len(ANCHOR_SIZES)   # P3 .. P7
# bounds of torchvision RetinaNet's inference keywords on the HIP path (GaussianLayerNetwork(**kwargs))
MAX_MIN_SIZE, MAX_MAX_SIZE = 1600, 2667   # largest transform sizes the kernels' index arithmetic is checked for
MAX_TOPK_CANDIDATES = 4096                # csrc/detect.hip: per-level top-k capacity (L * topk <= 20 480)
MAX_HEAD_OUT_CHANNELS = 128               # A * num_classes and 4 * A: the head's output convs
USE_HEAD_ATLAS = True   # head towers on ONE atlas of the 5 pyramid levels (one launch per tower layer) instead of per level
N_SIDE_STREAMS = 4   # head towers of the 5 levels run concurrently on side HIP streams (0 = everything on one stream)
USE_DETECT_GRAPH = os.environ.get('CVPCE_DETECT_GRAPH', '1') != '0'   # replay the static launch schedule of a batch shape from a hipGraph (captured on the shape's 2nd call)
MAX_DETECT_GRAPHS = 4     # batch shapes kept captured (each graph keeps its intermediates alive: ~0.4 GB per 2048^2 image); LRU
CAPTURE_ON_SIGHT = 2      # a geometry is captured on its 2nd call (the 1st runs eagerly and fills the host-side caches) ...
MAX_CAPTURE_ON_SIGHT = 16  # ... and later, up to this many sights, once captured graphs start being evicted barely used (many geometries)
MAX_SIGHT_COUNTS = 512    # geometries whose call counts are remembered (LRU)
USE_SIDE_BRANCHES = os.environ.get('CVPCE_SIDE_BRANCHES', '1') != '0'   # Gaussian branch beside the heads, projection shortcuts beside conv1 -> conv2
# the fp16 storage mode checks its first batch for saturated activations once per engine and warns (CVPCE_FP16_GUARD=0 switches the check off)
FP16_SATURATION_GUARD = os.environ.get('CVPCE_FP16_GUARD', '1') != '0'
USE_ATLAS_COPY = os.environ.get('CVPCE_ATLAS_COPY', '1') != '0'       # levels <-> atlas in one launch each way (15 slice copies otherwise)
USE_BATCHED_TRANSFORM = os.environ.get('CVPCE_BATCHED_TRANSFORM', '1') != '0'   # the input transform of a whole batch in one launch
USE_FUSED_STEM = os.environ.get('CVPCE_FUSED_GLN_STEM', '1') != '0'     # conv1 + bn1 + relu + maxpool in one launch (csrc/gln_stem.hip); False: generic conv + pool kernels


# ---------------------------------------------------------------------------
# parameter containers (state-dict compatible with the reference checkpoints)
# ---------------------------------------------------------------------------
class FrozenBatchNorm2d(nn.Module):
    """Buffers only, like torchvision.ops.misc.FrozenBatchNorm2d (eps 1e-5)."""
    eps = 1e-5

    def __init__(self, n):
        super().__init__()
        self.register_buffer('weight', torch.ones(n))
        self.register_buffer('bias', torch.zeros(n))
        self.register_buffer('running_mean', torch.zeros(n))
        self.register_buffer('running_var', torch.ones(n))

    def _load_from_state_dict(self, state_dict, prefix, *args):
        state_dict.pop(prefix + 'num_batches_tracked', None)
        super()._load_from_state_dict(state_dict, prefix, *args)

    def affine(self):
        scale = self.weight * (self.running_var + self.eps).rsqrt()
        return scale, self.bias - self.running_mean * scale


def _conv(cin, cout, k, stride=1, pad=0, bias=True):
    return nn.Conv2d(cin, cout, k, stride=stride, padding=pad, bias=bias)


class _Bottleneck(nn.Module):
    def __init__(self, inplanes, planes, stride, downsample):
        super().__init__()
        self.conv1, self.bn1 = _conv(inplanes, planes, 1, bias=False), FrozenBatchNorm2d(planes)
        self.conv2, self.bn2 = _conv(planes, planes, 3, stride, 1, bias=False), FrozenBatchNorm2d(planes)
        self.conv3, self.bn3 = _conv(planes, planes * 4, 1, bias=False), FrozenBatchNorm2d(planes * 4)
        if downsample:
            self.downsample = nn.Sequential(_conv(inplanes, planes * 4, 1, stride, bias=False),
                                            FrozenBatchNorm2d(planes * 4))
        else:
            self.downsample = None
        self.stride = stride


class _ResNet50(nn.Module):
    """torchvision resnet50(norm_layer=FrozenBatchNorm2d) without avgpool/fc forward use."""
    inplanes = 2048

    def __init__(self):
        super().__init__()
        self.conv1, self.bn1 = _conv(3, 64, 7, 2, 3, bias=False), FrozenBatchNorm2d(64)
        inpl = 64
        for li, (planes, blocks) in enumerate(zip((64, 128, 256, 512), (3, 4, 6, 3))):
            layer = []
            for bi in range(blocks):
                stride = 2 if (bi == 0 and li > 0) else 1
                layer.append(_Bottleneck(inpl, planes, stride, downsample=(bi == 0)))
                inpl = planes * 4
            setattr(self, f'layer{li + 1}', nn.Sequential(*layer))
        self.fc = nn.Linear(2048, 1000)  # present in torchvision's resnet50; dropped by IntermediateLayerGetter
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.kaiming_normal_(m.weight, mode='fan_out', nonlinearity='relu')


class _P6P7(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.p6, self.p7 = _conv(cin, cout, 3, 2, 1), _conv(cout, cout, 3, 2, 1)
        for m in (self.p6, self.p7):
            nn.init.kaiming_uniform_(m.weight, a=1)
            nn.init.constant_(m.bias, 0)
        self.use_P5 = cin == cout


class _FPN(nn.Module):
    def __init__(self, in_channels_list, out_channels):
        super().__init__()
        self.inner_blocks = nn.ModuleList(_conv(c, out_channels, 1) for c in in_channels_list)
        self.layer_blocks = nn.ModuleList(_conv(out_channels, out_channels, 3, 1, 1) for _ in in_channels_list)
        for m in list(self.inner_blocks) + list(self.layer_blocks):
            nn.init.kaiming_uniform_(m.weight, a=1)
            nn.init.constant_(m.bias, 0)
        self.extra_blocks = _P6P7(out_channels, out_channels)


class _ConvNorm(nn.Module):
    """keys `.conv.*`, `.norm.*` (GaussianLayerBlock, proposals.py:51-63)."""

    def __init__(self, cin, cout):
        super().__init__()
        self.conv, self.norm = _conv(cin, cout, 3, 1, 1), nn.BatchNorm2d(cout)
        nn.init.kaiming_normal_(self.conv.weight, nonlinearity='relu')
        nn.init.constant_(self.conv.bias, 0)


class GaussianLayer(nn.Module):
    """Containers for proposals.py:65-79: lateral 1x1 on C2 + up2(P3), two conv+BN+ReLU blocks, up2."""

    def __init__(self, c_channels, p_channels):
        super().__init__()
        self.lateral = _conv(c_channels, p_channels, 1)
        self.block1 = _ConvNorm(p_channels, p_channels // 2)
        self.block2 = _ConvNorm(p_channels // 2, p_channels // 4)
        nn.init.xavier_normal_(self.lateral.weight)
        nn.init.constant_(self.lateral.bias, 0)


class _ConvAct(nn.Module):
    def __init__(self, cin, cout, k, tanh=False):
        super().__init__()
        self.conv = _conv(cin, cout, k, 1, 1 if k > 1 else 0)
        if tanh:
            nn.init.xavier_normal_(self.conv.weight, gain=nn.init.calculate_gain('tanh'))
        else:
            nn.init.kaiming_normal_(self.conv.weight, nonlinearity='relu')
        nn.init.constant_(self.conv.bias, 0)


class GaussianSubnet(nn.Module):
    """Containers for proposals.py:96-107: 3x3 c->c/2, 3x3, 3x3 ->c/4, 1x1, 1x1 ->1 (ReLU; last Tanh iff tanh)."""

    def __init__(self, in_channels, tanh=False):
        super().__init__()
        c = in_channels
        self.blocks = nn.Sequential(_ConvAct(c, c // 2, 3), _ConvAct(c // 2, c // 2, 3), _ConvAct(c // 2, c // 4, 3),
                                    _ConvAct(c // 4, c // 4, 1), _ConvAct(c // 4, 1, 1, tanh))
        self.tanh = tanh


class BackboneWithFPNAndGaussians(nn.Module):
    """proposals.py:109-139: body -> (C2 | C3..C5 -> FPN+P6,P7) + Gaussian branch on (C2, P3)."""

    def __init__(self, backbone, tanh=False):
        super().__init__()
        self.body = backbone
        if hasattr(self.body, 'fc'):
            del self.body.fc  # IntermediateLayerGetter keeps modules up to layer4 only
        in_channels_list = [(backbone.inplanes // 8) * 2 ** (i - 1) for i in (2, 3, 4)]
        self.fpn = _FPN(in_channels_list, FPN_CHANNELS)
        self.out_channels = FPN_CHANNELS
        self.gaussian_layer = GaussianLayer(256, FPN_CHANNELS)
        self.gaussian_subnet = GaussianSubnet(FPN_CHANNELS // 4, tanh)
        self.gaussians = None

    def get_gaussians(self):
        g = self.gaussians
        self.gaussians = None
        return g


class _HeadTower(nn.Module):
    def __init__(self, channels, out_name, out_channels):
        super().__init__()
        layers = []
        for _ in range(4):
            layers += [_conv(channels, channels, 3, 1, 1), nn.ReLU()]
        self.conv = nn.Sequential(*layers)  # conv keys 0,2,4,6
        setattr(self, out_name, _conv(channels, out_channels, 3, 1, 1))
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, std=0.01)
                nn.init.constant_(m.bias, 0)


class _RetinaNetHead(nn.Module):
    def __init__(self, channels, num_anchors, num_classes, prior_probability=0.01):
        super().__init__()
        self.classification_head = _HeadTower(channels, 'cls_logits', num_anchors * num_classes)
        nn.init.constant_(self.classification_head.cls_logits.bias, -math.log((1 - prior_probability) / prior_probability))
        self.regression_head = _HeadTower(channels, 'bbox_reg', num_anchors * 4)
        nn.init.zeros_(self.regression_head.bbox_reg.bias)


# ---------------------------------------------------------------------------
# the HIP execution plan
# ---------------------------------------------------------------------------
def _base_anchors(anchor_sizes=None, aspect_ratios=None):
    """torchvision AnchorGenerator.cell_anchors -> (L, A, 4).  anchor_sizes: one tuple of sizes per level (default ANCHOR_SIZES);
    aspect_ratios: one tuple per level (default ASPECT_RATIOS on every level); every level must give the same A."""
    anchor_sizes = ANCHOR_SIZES if anchor_sizes is None else anchor_sizes
    if aspect_ratios is None:
        aspect_ratios = (ASPECT_RATIOS,) * len(anchor_sizes)
    out = []
    for sizes, level_ratios in zip(anchor_sizes, aspect_ratios):
        scales = torch.as_tensor(sizes, dtype=torch.float32)
        ratios = torch.as_tensor(level_ratios, dtype=torch.float32)
        h_r = torch.sqrt(ratios)
        w_r = 1 / h_r
        ws = (w_r[:, None] * scales[None, :]).view(-1)
        hs = (h_r[:, None] * scales[None, :]).view(-1)
        out.append((torch.stack([-ws, -hs, ws, hs], dim=1) / 2).round())
    return torch.stack(out)  # (L, A, 4)


def resized_hw(h, w, min_size=None, max_size=None):
    """GeneralizedRCNNTransform.resize (eval): the short side to min_size unless the long side would exceed max_size
    (defaults MIN_SIZE, MAX_SIZE)."""
    min_size = MIN_SIZE if min_size is None else min_size
    max_size = MAX_SIZE if max_size is None else max_size
    scale = float(min_size) / float(min(h, w))
    if float(max(h, w)) * scale > max_size:
        scale = float(max_size) / float(max(h, w))
    return int(math.floor(float(h) * scale)), int(math.floor(float(w) * scale))


def padded_hw(h, w, size_divisible=SIZE_DIVISIBLE):
    """GeneralizedRCNNTransform.batch_images: an extent rounded up to the size divisor."""
    return (int(math.ceil(h / size_divisible) * size_divisible), int(math.ceil(w / size_divisible) * size_divisible))


class GLNEngine:
    """Weights packed for the HIP kernels (bf16 [Cout][K], FrozenBN/BN folded) + the launch schedule."""

    def __init__(self, model, device, precision=ops.DEFAULT_DETECTOR_PRECISION):
        """precision: storage type of the detector's weights and inter-layer activations -- 'fp16' (default: 10 mantissa bits, the
        mode that meets the 0.1 pt tolerance) or 'bf16' (opt-in: 7 mantissa bits at the same MFMA rate; head logits, box
        regressions and gaussians are fp32 in both)."""
        if precision not in ops.STORAGE_TYPES:
            raise ValueError(f'precision must be one of {sorted(ops.STORAGE_TYPES)}, got {precision!r}')
        self.precision = precision
        self.dtype = dt = ops.STORAGE_TYPES[precision]
        P = lambda conv, **kw: ops.PackedConv(conv.weight, conv.bias, conv.stride[0], conv.padding[0], device=device, dtype=dt, **kw)
        body = model.backbone.body

        def fold(conv, bn):
            s, b = bn.affine()
            return P(conv, scale=s, shift=b)

        self.stem = fold(body.conv1, body.bn1)
        self.stem_fused = ops.PackedGlnStem(body.conv1.weight, *body.bn1.affine(), device=device, dtype=dt) if tuple(body.conv1.weight.shape) == (64, 3, 7, 7) else None
        self.layers = []
        for li in range(4):
            blocks = []
            for blk in getattr(body, f'layer{li + 1}'):
                blocks.append((fold(blk.conv1, blk.bn1), fold(blk.conv2, blk.bn2), fold(blk.conv3, blk.bn3),
                               fold(blk.downsample[0], blk.downsample[1]) if blk.downsample is not None else None))
            self.layers.append(blocks)
        fpn = model.backbone.fpn
        self.inner = [P(m) for m in fpn.inner_blocks]
        self.outer = [P(m) for m in fpn.layer_blocks]
        self.p6, self.p7 = P(fpn.extra_blocks.p6), P(fpn.extra_blocks.p7)
        self.pack_gaussian(model.backbone.gaussian_layer, model.backbone.gaussian_subnet, device)
        ch, rh = model.head.classification_head, model.head.regression_head
        self.cls_tower = [P(ch.conv[i]) for i in (0, 2, 4, 6)]
        self.cls_out = P(ch.cls_logits)
        self.reg_tower = [P(rh.conv[i]) for i in (0, 2, 4, 6)]
        self.reg_out = P(rh.bbox_reg)
        # RetinaNet's transform and anchor options are fixed at the model's construction; the thresholds and top-k are read from
        # the model on every detect (detect_options)
        tf, ag = getattr(model, 'transform', None), getattr(model, 'anchor_generator', None)
        self.min_size = tf.min_size[-1] if tf is not None else MIN_SIZE
        self.max_size = tf.max_size if tf is not None else MAX_SIZE
        self.image_mean = tuple(tf.image_mean) if tf is not None else IMAGE_MEAN
        self.image_std = tuple(tf.image_std) if tf is not None else IMAGE_STD
        self.base_anchors = (_base_anchors(*_anchor_spec(ag)) if ag is not None else _base_anchors()).to(device)
        self._model = weakref.ref(model)
        self.side_streams = [torch.cuda.Stream(device=device) for _ in range(4)] if N_SIDE_STREAMS else []
        self.num_anchors = self.base_anchors.shape[1]
        self.device = device
        # opt-in (GaussianLayerNetwork.keep_head_outputs): a pass also returns its per-level head outputs, set aside for `take_heads`
        self.keep_heads = False
        self.kept_heads = None

    def detect_options(self):
        """(topk_candidates, score_thresh, nms_thresh) of the model as they are now (validated), torchvision's defaults without
        a model."""
        model = self._model()
        if model is None:
            return TOPK_CANDIDATES, SCORE_THRESH, NMS_THRESH
        return model._detect_options()

    def pack_gaussian(self, gl, subnet, device, dtype=None):
        """Gaussian branch weights (proposals.py:65-107): eval-mode BatchNorm folded into block1/block2."""
        dt = dtype if dtype is not None else getattr(self, 'dtype', ops.BF16)
        P = lambda conv, **kw: ops.PackedConv(conv.weight, conv.bias, conv.stride[0], conv.padding[0], device=device, dtype=dt, **kw)

        def fold_bn(blk):
            bn = blk.norm
            s = bn.weight * (bn.running_var + bn.eps).rsqrt()
            return P(blk.conv, scale=s, shift=bn.bias - bn.running_mean * s)

        self.g_lateral = P(gl.lateral)
        self.g_block1, self.g_block2 = fold_bn(gl.block1), fold_bn(gl.block2)
        self.g_subnet = [P(b.conv) for b in subnet.blocks]
        self.tanh = subnet.tanh

    def _keep(self, obj):
        """A captured hipGraph holds raw pointers to engine-owned tensors (level masks, tile maps, atlas buffers, per-geometry
        constants) that live in bounded caches: while a capture is being recorded every such object is also referenced from
        the graph's entry, so that a cache eviction can never free memory a later replay reads."""
        refs = self.__dict__.get('_capture_refs')
        if refs is not None:
            refs.append(obj)

    # -- stages ---------------------------------------------------------------
    @staticmethod
    def batch_geometry(images, min_size=None, max_size=None):
        """-> (original sizes, resized sizes, padded (Hp, Wp)) of GeneralizedRCNNTransform for this list of images
        (min_size, max_size: resized_hw's)."""
        sizes = [image_hw(i) for i in images]               # (either form: float (3,H,W) or uint8 (H,W,3))
        rs = [resized_hw(h, w, min_size, max_size) for h, w in sizes]
        return sizes, rs, padded_hw(max(r[0] for r in rs), max(r[1] for r in rs))

    def transform(self, images, out=None):
        sizes, rs, (hp, wp) = self.batch_geometry(images, self.min_size, self.max_size)
        batch = out if out is not None else torch.empty((len(images), hp, wp, 8), dtype=self.dtype, device=self.device)
        assert tuple(batch.shape) == (len(images), hp, wp, 8) and batch.dtype == self.dtype
        if USE_BATCHED_TRANSFORM:
            ops.gln_transform_batch(images, batch, rs, self.image_mean, self.image_std)
        else:
            for i, (img, (h, w)) in enumerate(zip(images, rs)):
                if ops.is_uint8_image(img):                 # (bytes are read by the batch kernel only)
                    ops.gln_transform_batch([img], batch[i:i + 1], [(h, w)], self.image_mean, self.image_std)
                else:
                    ops.gln_transform_into(img.contiguous(), batch, i, h, w, self.image_mean, self.image_std)
        return batch, sizes, rs

    def body(self, x):
        if USE_FUSED_STEM and self.stem_fused is not None:
            x = ops.gln_stem(x, self.stem_fused)
        else:
            x = ops.conv2d(x, self.stem, act=1)
            x = ops.maxpool2d(x, 3, 2, 1)
        feats = []
        for blocks in self.layers:
            for c1, c2, c3, ds in blocks:
                # the projection shortcut of a stage's first block is independent of conv1 -> conv2: beside them
                if ds is None and ops.can_fuse_bottleneck(x, c1, c2, c3, x):
                    x = ops.bottleneck(x, c1, c2, c3, x)           # identity block: one launch, intermediates in LDS
                    continue
                if ds is not None and ops.can_fuse_bottleneck(x, c1, c2, c3, (x.shape[0], x.shape[1], x.shape[2], c3.cout)):
                    x = ops.bottleneck(x, c1, c2, c3, ops.conv2d(x, ds))   # layer1's first block (stride 1): shortcut conv, then one launch
                    continue
                identity, joined = self._beside(2, lambda: ops.conv2d(x, ds)) if ds is not None else (x, None)
                y = ops.conv2d(x, c1, act=1)
                y = ops.conv2d(y, c2, act=1)
                if joined is not None:
                    torch.cuda.current_stream().wait_event(joined)
                x = ops.conv2d(y, c3, act=1, residual=identity)
            feats.append(x)
        return feats  # C2..C5

    def fpn(self, c3, c4, c5):
        # the top-down chain i5 -> i4 -> i3 -> p3 is the critical path; the output convs of the coarser levels and P6 / P7
        # (small maps, latency-bound launches) hang off it and run beside it
        def coarse(i5):
            p5 = ops.conv2d(i5, self.outer[2])
            p6 = ops.conv2d(p5, self.p6)
            return p5, p6, ops.conv2d(ops.relu(p6), self.p7)

        i5 = ops.conv2d(c5, self.inner[2])
        (p5, p6, p7), coarse_done = self._beside(2, lambda: coarse(i5))
        i4 = ops.conv2d(c4, self.inner[1], residual=i5, res_mode=2)
        p4, p4_done = self._beside(3, lambda: ops.conv2d(i4, self.outer[1]))
        i3 = ops.conv2d(c3, self.inner[0], residual=i4, res_mode=2)
        p3 = ops.conv2d(i3, self.outer[0])
        for ev in (coarse_done, p4_done):
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
        return [p3, p4, p5, p6, p7]

    def _beside(self, k, fn):
        """Run `fn` (launches whose inputs are ready on the current stream) on side stream k, concurrently with what the
        caller enqueues next.  -> (result, event the consumer stream must wait on | None when side streams are off).  Works
        the same eagerly and inside a hipGraph capture (the fork / join become graph dependencies)."""
        if not (self.side_streams and USE_SIDE_BRANCHES):
            return fn(), None
        main, side = torch.cuda.current_stream(), self.side_streams[k % len(self.side_streams)]
        ready = torch.cuda.Event()
        ready.record(main)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            out = fn()
            for t in (out if isinstance(out, tuple) else (out,)):
                t.record_stream(main)
            done = torch.cuda.Event()
            done.record(side)
        return out, done

    def gaussian_branch(self, c2, p3):
        x = ops.conv2d(c2, self.g_lateral, residual=p3, res_mode=2)       # lateral(C2) + up2(P3)
        x = ops.conv2d(x, self.g_block1, act=1)
        x = ops.conv2d(x, self.g_block2, act=1)
        if ops.can_fuse_gauss_subnet(x, self.g_subnet):
            # the whole subnet (proposals.py:81-107) over up2(x) in one launch: no intermediate layer reaches memory (csrc/gauss_subnet.hip)
            return ops.gauss_subnet(x, self.g_subnet, 2 if self.tanh else 1)
        x = ops.conv2d(x, self.g_subnet[0], act=1, in_up_shift=1)         # conv over up2(x), never materialised
        x = ops.conv2d(x, self.g_subnet[1], act=1)
        x = ops.conv2d(x, self.g_subnet[2], act=1)
        if ops.can_fuse_gauss_tail(x, self.g_subnet[3], self.g_subnet[4]):
            return ops.gauss_tail(x, self.g_subnet[3], self.g_subnet[4], 2 if self.tanh else 1)   # the two 1x1 layers in one launch
        x = ops.conv2d(x, self.g_subnet[3], act=1)
        return ops.conv2d(x, self.g_subnet[4], act=2 if self.tanh else 1, out_f32=True)  # (N,H/2,W/2,1) f32

    @staticmethod
    def atlas_layout(shapes):
        """Placement of the pyramid levels [(H, W), ...] on one canvas: the largest level at the origin, the others in a
        column to its right, one zero pixel between neighbours.  -> (Hc, Wc, [(oy, ox), ...])"""
        (h0, w0), rest = shapes[0], shapes[1:]
        offs, y = [(0, 0)], 0
        for (h, w) in rest:
            offs.append((y, w0 + 1))
            y += h + 1
        hc = max(h0, y - 1 if rest else 0)
        wc = w0 + ((1 + max(w for _, w in rest)) if rest else 0)
        return hc, wc, offs

    def heads_atlas(self, feats):
        """RetinaNetHead on all levels at once.  The head's weights are shared by the levels (torchvision RetinaNetHead
        loops over the features with the same modules), so the levels are packed into one zero-separated atlas and every
        tower layer is ONE launch of the masked halo kernel; the gaps between the levels are its zero padding."""
        n = feats[0].shape[0]
        shapes = [(f.shape[1], f.shape[2]) for f in feats]
        key = tuple(shapes)
        cache = self.__dict__.setdefault('_atlas_cache', {})
        if key not in cache:                 # (never inside a graph capture: the first call of a shape always runs eagerly)
            if len(cache) > 64:              # datasets with thousands of distinct image sizes: keep the cache bounded
                cache.clear()
            hc, wc, offs = self.atlas_layout(shapes)
            mask = torch.zeros(hc, wc, dtype=torch.uint8)
            for (h, w), (oy, ox) in zip(shapes, offs):
                mask[oy:oy + h, ox:ox + w] = 1
            cache[key] = (hc, wc, offs, mask.to(self.device), ops.atlas_tile_map(mask).to(self.device), int(mask.sum()))
        hc, wc, offs, mask, tile_map, npix = cache[key]
        self._keep(cache[key])
        # Atlas buffers live in the engine, zero-filled ONCE: the kernels write level pixels (and zeros on the gap pixels of
        # the tiles they compute) and skip the tiles that lie wholly in a gap, so the gaps stay zero -- no memset, and about
        # 1/7 of the canvas tiles (the empty ones) are never scheduled.
        bufs = self.__dict__.setdefault('_atlas_bufs', {})
        bkey = (n, hc, wc)
        if bkey not in bufs:
            if len(bufs) >= MAX_DETECT_GRAPHS:
                bufs.pop(next(iter(bufs)))
            bufs[bkey] = [torch.zeros(n, hc, wc, FPN_CHANNELS, dtype=self.dtype, device=self.device) for _ in range(5)]
        atlas, cls_a, cls_b, reg_a, reg_b = bufs[bkey]
        self._keep(bufs[bkey])
        if USE_ATLAS_COPY:
            ops.atlas_pack(feats, atlas, offs)               # the five levels into the canvas, one launch
        else:
            for f, (h, w), (oy, ox) in zip(feats, shapes, offs):
                atlas[:, oy:oy + h, ox:ox + w] = f

        def chain(tower, final, ping, pong):
            t = atlas
            for pc in tower:
                t = ops.conv3x3_atlas(t, pc, mask, act=1, tile_map=tile_map, out=ping, mask_pixels=npix)
                ping, pong = pong, ping
            o = ops.conv2d(t, final, out_f32=True)           # gap pixels hold junk here; they are never read
            if USE_ATLAS_COPY:
                return ops.atlas_unpack(o, shapes, offs)
            return [o[:, oy:oy + h, ox:ox + w].contiguous() for (h, w), (oy, ox) in zip(shapes, offs)]

        main = torch.cuda.current_stream()
        if not self.side_streams:
            return chain(self.cls_tower, self.cls_out, cls_a, cls_b), chain(self.reg_tower, self.reg_out, reg_a, reg_b)
        # the two towers are independent: the second one runs on a side stream and fills the first one's tail
        side = self.side_streams[0]
        ready = torch.cuda.Event()
        ready.record(main)
        with torch.cuda.stream(side):
            side.wait_event(ready)
            reg = chain(self.reg_tower, self.reg_out, reg_a, reg_b)
            for r in reg:
                r.record_stream(main)
            done = torch.cuda.Event()
            done.record(side)
        cls = chain(self.cls_tower, self.cls_out, cls_a, cls_b)
        main.wait_event(done)
        return cls, reg

    def heads(self, feats):
        """cls / reg towers on the 5 pyramid levels: 10 independent conv chains.  The small levels (25x25 .. 7x7) launch
        only a handful of workgroups each, so the chains are spread over side streams to run concurrently."""
        n_levels = len(feats)
        cls, reg = [None] * n_levels, [None] * n_levels

        def chain(f, tower, final):
            t = f
            for pc in tower:
                t = ops.conv2d(t, pc, act=1)
            return ops.conv2d(t, final, out_f32=True)

        main = torch.cuda.current_stream()
        if not self.side_streams:
            for i, f in enumerate(feats):
                cls[i] = chain(f, self.cls_tower, self.cls_out)
                reg[i] = chain(f, self.reg_tower, self.reg_out)
            return cls, reg
        ready = torch.cuda.Event()
        ready.record(main)
        jobs = [(i, kind) for i in range(n_levels) for kind in ('cls', 'reg')]
        done = []
        for k, (i, kind) in enumerate(jobs):
            stream = self.side_streams[k % len(self.side_streams)]
            with torch.cuda.stream(stream):
                stream.wait_event(ready)
                out = chain(feats[i], self.cls_tower if kind == 'cls' else self.reg_tower,
                            self.cls_out if kind == 'cls' else self.reg_out)
                out.record_stream(main)          # consumed by the post-processing kernels on the main stream
                (cls if kind == 'cls' else reg)[i] = out
                ev = torch.cuda.Event()
                ev.record(stream)
                done.append(ev)
        for ev in done:
            main.wait_event(ev)
        return cls, reg

    def postprocess(self, cls, reg, padded_hw, resized, original, num_classes, detections_per_img, conf_thresh, options=None):
        """options: (topk_candidates, score_thresh, nms_thresh); None = torchvision's defaults."""
        topk, score_thresh, nms_thresh = options if options is not None else (TOPK_CANDIDATES, SCORE_THRESH, NMS_THRESH)
        n = cls[0].shape[0]
        grids = [(c.shape[1], c.shape[2]) for c in cls]
        strides = [(padded_hw[0] // g[0], padded_hw[1] // g[1]) for g in grids]
        logits = [c.view(n, -1) for c in cls]
        regs = [r.view(n, -1, 4) for r in reg]
        # per-batch-shape constants, cached: an H2D copy here would block the host behind the whole detector
        key = (tuple(resized), tuple(original))
        cache = self.__dict__.setdefault('_pp_cache', {})
        if key not in cache:
            if len(cache) > 64:
                cache.clear()
            image_hw = torch.tensor(resized, dtype=torch.int32).to(self.device)
            ratios = torch.stack([torch.tensor(o, dtype=torch.float32) / torch.tensor(r, dtype=torch.float32)
                                  for o, r in zip(original, resized)]).to(self.device)
            torch.cuda.current_stream().synchronize()
            cache[key] = (image_hw, ratios)
        image_hw, ratios = cache[key]
        self._keep(cache[key])
        return ops.detect_postprocess(logits, regs, grids, strides, self.base_anchors, image_hw, ratios,
                                      self.num_anchors, num_classes, topk, score_thresh, nms_thresh,
                                      BBOX_XFORM_CLIP, detections_per_img, conf_thresh)

    def detect(self, images, num_classes, detections_per_img, conf_thresh=0.5, want_intermediates=False):
        """-> (boxes (N,dpi,4), scores, labels, count, conf_count, gaussians (N,1,H/2,W/2)) all on device.

        The launch schedule after the transform depends only on the batch geometry, so from the second call of a geometry on
        it is captured into a hipGraph and replayed: ~140 kernel launches become one graph launch (the host cost of the
        Python -> dispatcher -> ctypes path per launch disappears; the kernels and their results are the same, bit for bit).
        The model's topk_candidates, score_thresh and nms_thresh are read on every call."""
        options = self.detect_options()
        _check_detections_per_img(detections_per_img, options[0])
        if USE_DETECT_GRAPH and not want_intermediates and ops.PROFILE is None:
            return self._set_heads_aside(self._detect_graphed(images, num_classes, detections_per_img, conf_thresh, options), images)
        batch, original, resized = self.transform(images)
        res = self._detect_tail(batch, original, resized, num_classes, detections_per_img, conf_thresh, want_intermediates, options)
        if want_intermediates:
            return self._set_heads_aside(res[0], images), res[1]
        return self._set_heads_aside(res, images)

    def _set_heads_aside(self, res, images):
        """With `keep_heads` a pass returns its head outputs (L cls, then L reg tensors) behind its six results: they are kept, with
        the batch's geometry, until `take_heads` hands them out; the caller gets the six results it always got."""
        if len(res) == 6:
            return res
        levels = (len(res) - 6) // 2
        _, resized, padded = self.batch_geometry(images, self.min_size, self.max_size)
        self.kept_heads = {'cls': list(res[6:6 + levels]), 'reg': list(res[6 + levels:]), 'padded': tuple(padded), 'sizes': list(resized)}
        return res[:6]

    def take_heads(self):
        kept, self.kept_heads = self.kept_heads, None
        return kept

    def _detect_graphed(self, images, num_classes, detections_per_img, conf_thresh, options):
        """Graph cache policy (round-2 advisor finding): captured graphs live in an LRU of MAX_DETECT_GRAPHS entries; how often
        a geometry has been seen is counted in a separate (bounded) table, so first sights never push a captured graph out.
        A geometry is captured on its `_capture_on_sight`-th call (2 to begin with).  When a graph is evicted after fewer than
        4 replays -- the mark of a dataset with many image geometries, where capture (synchronise + private pool + eviction
        churn) costs more than it saves -- the threshold doubles (up to MAX_CAPTURE_ON_SIGHT): only geometries that keep
        coming back are then captured, everything else runs eagerly."""
        original, resized, padded = self.batch_geometry(images, self.min_size, self.max_size)
        # (the post-processing options are kernel arguments baked into the capture: a change of one is another graph)
        key = (len(images), padded, tuple(resized), tuple(original), num_classes, detections_per_img, float(conf_thresh), options)
        if self.keep_heads:                                 # (the kept tensors are outputs of that capture: another graph)
            key += ('head_outputs',)
        graphs = self.__dict__.setdefault('_graphs', OrderedDict())
        entry = graphs.get(key)
        if entry is not None:                               # captured: replay
            graphs.move_to_end(key)
            entry['replays'] += 1
            self.transform(images, out=entry['static_in'])
            entry['graph'].replay()
            # a graph that earns its keep lowers the capture threshold again (it is only ever raised when graphs are evicted barely
            # used: one burst of mixed geometries must not leave a later, stable geometry waiting 16 calls for its capture)
            if entry['replays'] == 4 and self.__dict__.get('_capture_on_sight', CAPTURE_ON_SIGHT) > CAPTURE_ON_SIGHT:
                self._capture_on_sight = max(CAPTURE_ON_SIGHT, self._capture_on_sight // 2)
            # results leave the graph's private memory: a later replay must not overwrite what the caller still holds
            return ops.clone_views(entry['static_out'])
        sights = self.__dict__.setdefault('_sights', OrderedDict())
        seen = sights.pop(key, 0) + 1
        sights[key] = seen
        while len(sights) > MAX_SIGHT_COUNTS:
            sights.popitem(last=False)
        need = self.__dict__.setdefault('_capture_on_sight', CAPTURE_ON_SIGHT)
        if seen < need:                                     # not yet: eager (the first call also fills the host-side caches)
            batch, original, resized = self.transform(images)
            return self._detect_tail(batch, original, resized, num_classes, detections_per_img, conf_thresh, False, options)
        static_in = torch.empty((len(images), padded[0], padded[1], 8), dtype=self.dtype, device=self.device)
        self.transform(images, out=static_in)
        torch.cuda.current_stream().synchronize()
        g = torch.cuda.CUDAGraph()
        self._capture_refs = []            # engine-owned tensors the captured kernels point at (see _keep)
        try:
            # (thread-local capture mode: other threads -- e.g. an RCCL watchdog polling its events -- may keep issuing HIP calls)
            with torch.cuda.graph(g, capture_error_mode='thread_local'):
                static_out = self._detect_tail(static_in, original, resized, num_classes, detections_per_img, conf_thresh, False, options)
        except Exception:
            # e.g. a host-side cache was evicted since the first call and would have to be refilled (an upload) inside the
            # capture: run this call eagerly -- which refills the caches -- and try the capture again next time
            self.__dict__.pop('_capture_refs', None)
            torch.cuda.synchronize()
            return self._detect_tail(static_in, original, resized, num_classes, detections_per_img, conf_thresh, False, options)
        while len(graphs) >= MAX_DETECT_GRAPHS:            # least recently used captured graph goes
            _, old = graphs.popitem(last=False)
            if old['replays'] < 4:
                self._capture_on_sight = min(MAX_CAPTURE_ON_SIGHT, 2 * self._capture_on_sight)
        graphs[key] = {'graph': g, 'static_in': static_in, 'static_out': static_out, 'keepalive': self.__dict__.pop('_capture_refs'),
                       'replays': 0}
        sights.pop(key, None)
        g.replay()
        return ops.clone_views(static_out)

    def _saturation_guard(self, tensors):
        """The automatic guard of the fp16 storage mode (round-5 review: fp16 stores SATURATE at +-65504 silently).  ONCE per engine, on the
        first eager pass (the first call of a geometry is never a graph replay): the largest magnitude of C2 ... C5 and of the five FPN maps
        of that batch (nine small reductions and one host read).  At the saturation value a warning names the remedy
        (`set_precision('bf16')`: 8 exponent bits); `GaussianLayerNetwork.saturation_report` gives the per-stage figures.  The result is
        kept in `self._saturation` ({'max_abs', 'saturated'})."""
        m = float(torch.stack([t.abs().amax().float() for t in tensors]).max())
        self._saturation = {'max_abs': m, 'saturated': m >= 65504.0}
        if self._saturation['saturated']:
            import warnings
            warnings.warn('cvpce_amd GLN detector (fp16 storage, the default): an activation of the backbone / FPN reached the fp16 saturation value '
                          '65504 on the first batch -- results of this checkpoint are clipped.  Use model.set_precision("bf16") (8 exponent bits, same '
                          'speed) or gln(..., precision="bf16"); model.saturation_report(images) lists the stages.', RuntimeWarning, stacklevel=3)

    def _detect_tail(self, batch, original, resized, num_classes, detections_per_img, conf_thresh, want_intermediates, options=None):
        c2, c3, c4, c5 = self.body(batch)
        feats = self.fpn(c3, c4, c5)
        if self.dtype == ops.F16 and FP16_SATURATION_GUARD and '_saturation' not in self.__dict__ and not torch.cuda.is_current_stream_capturing():
            self._saturation_guard((c2, c3, c4, c5) + tuple(feats))
        # the Gaussian branch (8 small convs, proposals.py:65-107) depends on C2 and P3 only: it runs beside the heads
        gauss, gauss_done = self._beside(1, lambda: self.gaussian_branch(c2, feats[0]))
        cls, reg = self.heads_atlas(feats) if USE_HEAD_ATLAS else self.heads(feats)
        out = self.postprocess(cls, reg, tuple(batch.shape[1:3]), resized, original, num_classes,
                               detections_per_img, conf_thresh, options)
        if gauss_done is not None:
            torch.cuda.current_stream().wait_event(gauss_done)
        gauss = gauss.permute(0, 3, 1, 2)  # (N,1,h,w) view of the NHWC buffer (C == 1)
        kept = tuple(cls) + tuple(reg) if self.keep_heads else ()
        if want_intermediates:
            return out + (gauss,) + kept, {'batch': batch, 'c': (c2, c3, c4, c5), 'features': feats, 'cls': cls, 'reg': reg}
        return out + (gauss,) + kept


# ---------------------------------------------------------------------------
# RetinaNet inference options (torchvision 0.9 keywords, eval semantics)
# ---------------------------------------------------------------------------
class TransformOptions:
    """The eval-mode settings of torchvision's GeneralizedRCNNTransform under its attribute names (min_size is a tuple; the
    eval resize uses min_size[-1])."""

    def __init__(self, min_size, max_size, image_mean, image_std, size_divisible=SIZE_DIVISIBLE):
        self.min_size, self.max_size = min_size, max_size
        self.image_mean, self.image_std = image_mean, image_std
        self.size_divisible = size_divisible

    def __repr__(self):
        return (f'TransformOptions(min_size={self.min_size}, max_size={self.max_size}, image_mean={self.image_mean}, '
                f'image_std={self.image_std})')


class AnchorOptions:
    """Stand-in for torchvision's AnchorGenerator (not installed here): `.sizes` and `.aspect_ratios`, one tuple per level."""

    def __init__(self, sizes=ANCHOR_SIZES, aspect_ratios=(ASPECT_RATIOS,) * NUM_LEVELS):
        self.sizes, self.aspect_ratios = sizes, aspect_ratios

    def num_anchors_per_location(self):
        return [len(s) * len(a) for s, a in zip(self.sizes, self.aspect_ratios)]

    def __repr__(self):
        return f'AnchorOptions(sizes={self.sizes}, aspect_ratios={self.aspect_ratios})'


_TRAINING_KEYWORDS = ('fg_iou_thresh', 'bg_iou_thresh')
_INFERENCE_KEYWORDS = ('min_size', 'max_size', 'image_mean', 'image_std', 'score_thresh', 'nms_thresh', 'topk_candidates',
                       'anchor_generator')


def _is_int(v):
    return isinstance(v, numbers.Integral) and not isinstance(v, bool)


def _is_real(v):
    return isinstance(v, numbers.Real) and not isinstance(v, bool) and math.isfinite(float(v))


def _anchor_spec(anchor_generator):
    """(sizes, aspect_ratios) of an AnchorGenerator-like object, normalised as torchvision does (a flat sequence of sizes is
    one size per level; a flat sequence of ratios applies to every level)."""
    sizes, ratios = anchor_generator.sizes, anchor_generator.aspect_ratios
    sizes = tuple(tuple(s) if isinstance(s, (list, tuple)) else (s,) for s in sizes)
    if len(ratios) and not isinstance(ratios[0], (list, tuple)):
        ratios = (tuple(ratios),) * len(sizes)
    return sizes, tuple(tuple(r) for r in ratios)


def _check_anchor_generator(anchor_generator, num_classes):
    if not (hasattr(anchor_generator, 'sizes') and hasattr(anchor_generator, 'aspect_ratios')):
        raise TypeError('anchor_generator needs .sizes and .aspect_ratios (torchvision AnchorGenerator)')
    sizes, ratios = _anchor_spec(anchor_generator)
    if len(sizes) != NUM_LEVELS or len(ratios) != NUM_LEVELS:
        raise ValueError(f'anchor_generator: one entry of sizes and aspect_ratios per FPN level ({NUM_LEVELS}), '
                         f'got {len(sizes)} and {len(ratios)}')
    for v in [x for level in sizes + ratios for x in level]:
        if not (_is_real(v) and v > 0):
            raise ValueError(f'anchor_generator: sizes and aspect ratios must be positive, got {v!r}')
    per_level = [len(s) * len(r) for s, r in zip(sizes, ratios)]
    if len(set(per_level)) != 1 or per_level[0] < 1:
        raise ValueError(f'anchor_generator: the HIP head needs the same number of anchors per location on every level, got {per_level}')
    a = per_level[0]
    if a * num_classes > MAX_HEAD_OUT_CHANNELS or 4 * a > MAX_HEAD_OUT_CHANNELS:
        raise ValueError(f'anchor_generator: {a} anchors per location give head outputs of {a * num_classes} and {4 * a} channels; '
                         f'the HIP head supports up to {MAX_HEAD_OUT_CHANNELS}')
    return a


def _check_detections_per_img(detections_per_img, topk_candidates):
    # the post-processing holds up to 8192 candidates per image at topk <= 1024 and 20 480 above (csrc/detect.hip)
    cap = 8192 if topk_candidates <= 1024 else NUM_LEVELS * MAX_TOPK_CANDIDATES
    if not (_is_int(detections_per_img) and 1 <= detections_per_img <= cap):
        raise ValueError(f'detections_per_img must be an int in [1, {cap}] at topk_candidates {topk_candidates}, got {detections_per_img!r}')


def _check_detect_options(topk_candidates, score_thresh, nms_thresh, detections_per_img):
    if not (_is_int(topk_candidates) and 1 <= topk_candidates <= MAX_TOPK_CANDIDATES):
        raise ValueError(f'topk_candidates must be an int in [1, {MAX_TOPK_CANDIDATES}], got {topk_candidates!r}')
    if not (_is_real(score_thresh) and 0 <= score_thresh < 1):
        raise ValueError(f'score_thresh must be in [0, 1), got {score_thresh!r}')
    if not (_is_real(nms_thresh) and 0 < nms_thresh <= 1):
        raise ValueError(f'nms_thresh must be in (0, 1], got {nms_thresh!r}')
    _check_detections_per_img(detections_per_img, topk_candidates)


def _transform_options(min_size, max_size, image_mean, image_std):
    min_size = tuple(min_size) if isinstance(min_size, (list, tuple)) else (min_size,)
    if not min_size or not all(_is_int(m) and 1 <= m <= MAX_MIN_SIZE for m in min_size):
        raise ValueError(f'min_size must be a positive int (or a tuple of them) up to {MAX_MIN_SIZE}, got {min_size!r}')
    if not (_is_int(max_size) and 1 <= max_size <= MAX_MAX_SIZE):
        raise ValueError(f'max_size must be a positive int up to {MAX_MAX_SIZE}, got {max_size!r}')
    stats = []
    for name, v in (('image_mean', image_mean), ('image_std', image_std)):
        v = [float(x) if _is_real(x) else None for x in v] if isinstance(v, (list, tuple)) or torch.is_tensor(v) else None
        if v is None or len(v) != 3 or None in v:
            raise ValueError(f'{name} must be 3 finite floats, got {v!r}')
        stats.append(v)
    if min(stats[1]) <= 0:
        raise ValueError(f'image_std must be positive, got {stats[1]}')
    return TransformOptions(min_size, int(max_size), stats[0], stats[1])


# ---------------------------------------------------------------------------
# public API
# ---------------------------------------------------------------------------
def _image_list(images):
    """The images of a forward call as a list, each in one of the two accepted forms (ops.IMAGE_FORMS; a list may mix them):
    a TypeError for anything else comes before the device check.  One tensor is a batch of float images (N,3,H,W), or ONE
    8-bit image (H,W,3)."""
    if torch.is_tensor(images):
        images = [images] if images.dtype == torch.uint8 else list(images)
    images = list(images)
    for i in images:
        ops.check_image_form(i)
    return images


class GaussianLayerNetwork(nn.Module):
    """Drop-in for proposals.py:162-181 (eval mode): `model(list[Tensor(3,H,W)])` ->
    `list[dict(boxes, scores, labels, gaussians)]`, boxes in original pixels, scores descending.  An image may also be 8-bit
    (H,W,3) as a decoder produces it: it is converted on the device to the float image `to_tensor` makes of it, bit for bit.

    `**kwargs` are torchvision 0.9 RetinaNet's inference keywords, stored under its attribute names: `min_size`, `max_size`,
    `image_mean`, `image_std` (-> `self.transform`) and `anchor_generator` are fixed at construction; `score_thresh`,
    `nms_thresh`, `topk_candidates` and `detections_per_img` are read on every forward.  `fg_iou_thresh` / `bg_iou_thresh`
    (training only) are stored and have no effect.  Bounds: DESIGN.md 1."""

    def __init__(self, resnet, num_classes, gaussian_loss_params={}, tanh=False, detections_per_img=1000, precision=None, **kwargs):
        super().__init__()
        if precision is None:       # (the CLI commands keep the reference's options: the environment selects the mode there)
            precision = os.environ.get('CVPCE_DETECTOR_PRECISION', ops.DEFAULT_DETECTOR_PRECISION)
        if precision not in ops.STORAGE_TYPES:
            raise ValueError(f'precision must be one of {sorted(ops.STORAGE_TYPES)}, got {precision!r}')
        self.precision = precision
        unsupported = sorted(k for k in kwargs if k not in _INFERENCE_KEYWORDS + _TRAINING_KEYWORDS)
        if unsupported:
            raise TypeError(f'unsupported RetinaNet overrides on the HIP path: {unsupported}')
        self.transform = _transform_options(kwargs.get('min_size', MIN_SIZE), kwargs.get('max_size', MAX_SIZE),
                                            kwargs.get('image_mean', IMAGE_MEAN), kwargs.get('image_std', IMAGE_STD))
        self.anchor_generator = kwargs['anchor_generator'] if kwargs.get('anchor_generator') is not None else AnchorOptions()
        num_anchors = _check_anchor_generator(self.anchor_generator, num_classes)
        self.score_thresh = kwargs.get('score_thresh', SCORE_THRESH)
        self.nms_thresh = kwargs.get('nms_thresh', NMS_THRESH)
        self.topk_candidates = kwargs.get('topk_candidates', TOPK_CANDIDATES)
        _check_detect_options(self.topk_candidates, self.score_thresh, self.nms_thresh, detections_per_img)
        self.fg_iou_thresh = kwargs.get('fg_iou_thresh', 0.5)
        self.bg_iou_thresh = kwargs.get('bg_iou_thresh', 0.4)
        self.backbone = BackboneWithFPNAndGaussians(resnet, tanh=tanh)
        self.head = _RetinaNetHead(FPN_CHANNELS, num_anchors, num_classes)
        self.num_classes = num_classes
        self.detections_per_img = detections_per_img
        self.gaussian_loss_params = gaussian_loss_params
        self._engine = None
        self._keep_head_outputs = False
        self.eval()

    def _detect_options(self):
        """-> (topk_candidates, score_thresh, nms_thresh) as set now; ValueError when one was set out of range."""
        _check_detect_options(self.topk_candidates, self.score_thresh, self.nms_thresh, self.detections_per_img)
        return int(self.topk_candidates), float(self.score_thresh), float(self.nms_thresh)

    def image_geometry(self, original_sizes):
        """-> [(transformed (h, w), the same padded to the size divisor)] of images of these (H, W), by this model's transform: the
        sizes the reference's transform records in `image_sizes`, and the extent a batch of that image alone is padded to."""
        rs = [resized_hw(int(h), int(w), self.transform.min_size[-1], self.transform.max_size) for h, w in original_sizes]
        return [(r, padded_hw(*r)) for r in rs]

    def load_state_dict(self, *args, **kwargs):
        self._engine = None
        return super().load_state_dict(*args, **kwargs)

    def set_precision(self, precision):
        """'fp16' (default) | 'bf16' (opt-in): storage type of the detector's weights / activations on the GPU.  The
        parameters themselves stay fp32 (checkpoint format unchanged); the engine is re-packed on the next forward."""
        if precision not in ops.STORAGE_TYPES:
            raise ValueError(f'precision must be one of {sorted(ops.STORAGE_TYPES)}, got {precision!r}')
        if precision != self.precision:
            self.precision = precision
            self._engine = None
        return self

    def _apply(self, fn, *a, **k):
        self._engine = None
        return super()._apply(fn, *a, **k)

    @torch.no_grad()
    def saturation_report(self, images):
        """Diagnostic for the fp16 storage mode (the default): fp16 stores SATURATE at +-65504 instead of overflowing, silently.  Runs one
        eager pass over `images` and reports, per stage the schedule keeps in 16-bit storage (C2 ... C5 of the body, the five FPN maps),
        the largest magnitude and the fraction of elements at the saturation value.  A checkpoint whose activations come near 65504
        should run with `set_precision('bf16')` (8 exponent bits).  Seeded and fitted weights here stay below 1e3.
        -> {'precision', 'stages': {name: {'max_abs', 'saturated_fraction'}}, 'saturated': bool}"""
        images = _image_list(images)
        eng = self.engine()
        images = [ops.input_image(i, eng.device) for i in images]
        _, inter = eng.detect(images, self.num_classes, self.detections_per_img, want_intermediates=True)
        self.backbone.gaussians = None
        limit = 65504.0 if self.precision == 'fp16' else float(torch.finfo(torch.bfloat16).max)
        stages = {}
        for name, t in list(zip(('c2', 'c3', 'c4', 'c5'), inter['c'])) + [(f'fpn{i}', f) for i, f in enumerate(inter['features'])]:
            a = t.float().abs()
            stages[name] = {'max_abs': float(a.max()), 'saturated_fraction': float((a >= limit).float().mean())}
        return {'precision': self.precision, 'stages': stages, 'saturated': any(v['saturated_fraction'] > 0 for v in stages.values())}

    def engine(self):
        dev = next(self.parameters()).device
        if dev.type != 'cuda':
            raise RuntimeError('GaussianLayerNetwork runs on an MI355X (HIP) device only: call .cuda() first. '
                               'No CPU fallback exists in cvpce_amd (the CPU restatement lives in oracle/ for tests).')
        if self._engine is None:
            self._engine = GLNEngine(self, dev, self.precision)
        self._engine.keep_heads = self._keep_head_outputs
        return self._engine

    def keep_head_outputs(self, flag=True):
        """Opt-in: every following forward pass also keeps its head outputs -- the per-level classification logits and box
        regressions the post-processing reads -- for `head_outputs`.  Off (the default), a pass launches, captures and replays
        exactly what it always did; on, the kept tensors are outputs of the pass (of its captured graph too: the flag is part of
        the graph key)."""
        self._keep_head_outputs = bool(flag)
        if self._engine is not None:
            self._engine.keep_heads = self._keep_head_outputs
        return self

    def head_outputs(self):
        """The head outputs of the last forward pass run with `keep_head_outputs(True)`, handed out once like `get_gaussians`:
        {'cls': per-level (N,gh,gw,A*K) float32, 'reg': per-level (N,gh,gw,A*4) float32, 'padded': the batch's (Hp, Wp),
        'sizes': the transformed (h, w) of every image}; None when there are none."""
        return self._engine.take_heads() if self._engine is not None else None

    @torch.no_grad()
    def losses(self, images, targets):
        """The reference's training-mode forward (proposals.py:169-181: RetinaNet's two head losses plus gaussian_loss) in
        EVAL-mode statistics, forward only -> {'classification', 'bbox_regression', 'gaussian'} as 0-dim float32 device tensors;
        nothing is copied to the host.

        targets: one dict per image with 'boxes' (T,4) float xyxy in original pixels, 'labels' (T,) integers in
        [0, num_classes) and optionally 'gaussians', a full-resolution (H,W) map.  Where no target has 'gaussians' the maps are
        rendered from the boxes when those are integers (datautils.generate_gaussians' defaults); otherwise 'gaussian' is
        omitted.  A ValueError for degenerate boxes, labels out of range or a length mismatch comes before anything is queued."""
        from .. import device_gaussians, device_headloss
        images = _image_list(images)
        targets = list(targets)
        if len(targets) != len(images):
            raise ValueError('one target dict per image')
        device_headloss.check_targets(targets, self.num_classes)
        eng = self.engine()
        images = [ops.input_image(i, eng.device) for i in images]
        before = self._keep_head_outputs
        self.keep_head_outputs(True)
        try:
            gauss = eng.detect(images, self.num_classes, self.detections_per_img)[5]
        finally:
            self.keep_head_outputs(before)
        heads = eng.take_heads()
        original = [image_hw(i) for i in images]
        grids = [(c.shape[1], c.shape[2]) for c in heads['cls']]
        strides = [(heads['padded'][0] // g[0], heads['padded'][1] // g[1]) for g in grids]
        out_f, _, _ = device_headloss.head_losses(heads['cls'], heads['reg'], grids, strides, eng.base_anchors, [t['boxes'] for t in targets],
                                                  [t['labels'] for t in targets], device_headloss.scale_factors(heads['sizes'], original))
        res = {'classification': out_f[:, 0].mean(), 'bbox_regression': out_f[:, 1].mean()}
        params = dict(self.gaussian_loss_params or {})
        tanh = bool(params.pop('tanh', self.backbone.gaussian_subnet.tanh))
        if all('gaussians' in t for t in targets):
            res['gaussian'] = gaussian_loss(gauss, [t['gaussians'] for t in targets], heads['sizes'], tanh=tanh, **params)
        elif not any('gaussians' in t for t in targets) and not any(torch.as_tensor(t['boxes']).is_floating_point() for t in targets):
            hb, wb = gauss.shape[2:]
            geom = [(h0, w0, 1, rh // 2, rw // 2) for (h0, w0), (rh, rw) in zip(original, heads['sizes'])]
            maps = device_gaussians.render_boxes([torch.as_tensor(t['boxes']) for t in targets], geom, hb, wb, tanh=tanh, device=eng.device)
            res['gaussian'] = device_gaussians.loss(gauss.to(torch.float32), maps, None, **params)[0][0, 0]
        return res

    @torch.no_grad()
    def forward(self, images, targets=None):
        if self.training:
            raise NotImplementedError('training is out of scope of the MI355X inference path (SURVEY.md 2)')
        images = _image_list(images)
        eng = self.engine()
        images = [ops.input_image(i, eng.device) for i in images]
        boxes, scores, labels, count, _, gauss = eng.detect(images, self.num_classes, self.detections_per_img)
        self.backbone.gaussians = gauss
        counts = count.tolist()
        res = [{'boxes': boxes[i, :c], 'scores': scores[i, :c], 'labels': labels[i, :c]} for i, c in enumerate(counts)]
        for r, g in zip(res, self.backbone.get_gaussians()):
            r['gaussians'] = g
        return res


def gaussian_loss(predictions, targets, sizes, tanh=False, negative_threshold=0.0, positive_threshold=0.1, min_negatives=1000,
                  negatives_per_positive=3):
    """proposals.py:141-160 on the GPU (forward only) -> a 0-dim float32 device tensor; nothing is copied to the host.

    predictions: (N,1,Hb,Wb) float32 on the device; targets: N full-resolution maps (H_i, W_i) float32 (uploaded when on the host);
    sizes: the transformed (h, w) of every image -- its map is resized to (h // 2, w // 2) into a batch tensor whose padding holds the
    background value (-1 with `tanh`, else 0).  One loss over the whole tensor, padding included: the sum of the positives' squared
    errors and of the max(min_negatives, negatives_per_positive * positives) largest negatives', over their count."""
    from .. import device_gaussians
    return device_gaussians.reference_loss(predictions, targets, sizes, tanh, negative_threshold, positive_threshold, min_negatives,
                                           negatives_per_positive)


def gln_backbone(trainable_layers=5, pretrained=True):
    """proposals.py:183-191.  No network here: `pretrained=True` cannot download and is rejected."""
    if pretrained:
        raise RuntimeError('pretrained ImageNet weights cannot be downloaded here; build with '
                           'pretrained_backbone=False and load a checkpoint via load_state_dict')
    backbone = _ResNet50()
    layers_to_train = ['layer4', 'layer3', 'layer2', 'layer1', 'conv1'][:trainable_layers]
    for name, parameter in backbone.named_parameters():
        if all(not name.startswith(layer) for layer in layers_to_train):
            parameter.requires_grad_(False)
    return backbone


def gln(num_classes=1, trainable_layers=4, pretrained_backbone=True, tanh=False, gaussian_loss_params={},
        detections_per_img=1000, precision=None):
    """proposals.py:202-203 (+ `precision`, keyword-only in spirit: 'fp16' | 'bf16' storage of the detector on the GPU; None = the
    CVPCE_DETECTOR_PRECISION environment variable, else ops.DEFAULT_DETECTOR_PRECISION = 'fp16')"""
    return GaussianLayerNetwork(gln_backbone(trainable_layers, pretrained_backbone), num_classes, tanh=tanh,
                                gaussian_loss_params=gaussian_loss_params, detections_per_img=detections_per_img, precision=precision)
