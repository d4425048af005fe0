"""Scoring the detector's Gaussian maps on the device -- the counterpart of the reference's `gaussian_loss` over
`generate_gaussians` targets (cvpce/models/proposals.py:141-160, cvpce/datautils.py:18-85; its `gln seek-sku110k-outliers` ranks
images by that loss).  The rule is DESIGN.md 4c; the kernels are csrc/gaussians.hip.

The reference renders a target with a Python loop over boxes on the CPU at full image resolution, resizes it and sorts every
negative pixel.  Here a batch's targets are rendered AND resized by one launch straight from the boxes, and the loss is found by
a radix select: a memset and six launches, whatever the number of boxes or pixels.  `GaussianScore.update` queues device work
only -- the per-image sizes are known from the shapes, every upload goes through pinned memory, nothing is read back -- and
`compute` brings the accumulated per-image losses to the host in one copy, like `device_metrics.DetectionMetrics` and
`device_classification.ClassificationTally`.
"""
import torch

from . import datautils, torch_ops_gaussians as G   # (registers torch.ops.cvpce_amd.gauss_*)
from . import staging

# stream operations `GaussianScore.update` queues per batch, whatever the number of boxes and pixels:
#   launches: the stack of the predictions, the targets launch, the loss (a memset, five passes, the finish)     1 + 1 + 7
#   uploads (pinned, asynchronous): boxes, box offsets, geometry, extents                                        4 copies
# (boxes that already live on the device are packed there instead: one cat and a cast in place of the first upload)
LAUNCHES_PER_BATCH = 9
UPLOADS_PER_BATCH = 4
HOST_WAITS_PER_BATCH = 0

_tables = {}


def _kant_table(device, size, sigma):
    """The kant method's table, built once per (device, size, sigma) on the device."""
    key = (str(device), size, sigma)
    if key not in _tables:
        t = torch.empty((size, size), dtype=torch.float32, device=device)
        torch.ops.cvpce_amd.gauss_kant_table(t, sigma)
        _tables[key] = t
    return _tables[key]


def _methods(generate_method, join_method):
    generate_method = datautils.generate_via_multivariate_normal() if generate_method is None else generate_method
    join_method = datautils.join_via_max if join_method is None else join_method
    if not isinstance(generate_method, datautils.GenerateMethod):
        raise TypeError('generate_method is what datautils.generate_via_* returns (the reference\'s closures run per box on the host)')
    if not isinstance(join_method, datautils.JoinMethod):
        raise TypeError('join_method is one of datautils.join_via_max, join_via_addition, join_via_replacement')
    return generate_method, join_method


def _int_boxes(boxes):
    out = []
    for b in boxes:
        b = torch.as_tensor(b)
        if b.is_floating_point() or b.dtype == torch.bool:
            raise TypeError('Gaussian targets are rendered from INTEGER boxes (the reference floor-divides them); got ' + str(b.dtype))
        if b.numel() % 4:
            raise ValueError('boxes are (B,4) xyxy')
        out.append(b)
    return out


def render_boxes(boxes, geom, hb, wb, generate_method=None, join_method=None, tanh=False, resize=True, device=None):
    """One launch: the (N,1,hb,wb) target tensor of N images from their boxes.  boxes: N integer (B_i,4) tensors; geom: N tuples
    (H0, W0, size_reduction, h, w) (include/cvpce_amd_gaussians.h).  Device work only."""
    generate_method, join_method = _methods(generate_method, join_method)
    boxes = _int_boxes(boxes)
    if len(boxes) != len(geom):
        raise ValueError('one box tensor and one geometry per image')
    if device is None:
        device = next((b.device for b in boxes if b.is_cuda), torch.device('cuda', torch.cuda.current_device()))
    out = torch.empty((len(boxes), 1, hb, wb), dtype=torch.float32, device=device)
    if out.numel() == 0:
        return out
    if any(int(g[2]) < 1 for g in geom):
        raise ValueError('size_reduction is a positive integer')
    if any(b.is_cuda for b in boxes):
        packed = staging.pack(boxes, torch.int32, device, (4,))
    else:                                                        # host boxes: packed on the host, one upload
        packed = torch.empty((0, 4), dtype=torch.int32, device=device) if not sum(b.numel() for b in boxes) else \
            torch.cat([b.reshape(-1, 4) for b in boxes]).to(torch.int32).pin_memory().to(device, non_blocking=True)
    offsets = staging.upload_values(staging.offsets([b.numel() // 4 for b in boxes]), torch.int32, device)
    g = staging.upload_values([[int(v) for v in row] for row in geom], torch.int32, device).reshape(len(geom), G.GEOM)
    table = _kant_table(device, *generate_method.table) if generate_method.table else None
    torch.ops.cvpce_amd.gauss_targets(packed, offsets, None, g, table, G.METHODS[generate_method.name], G.JOINS[join_method.name],
                                      *generate_method.params, int(bool(tanh)), int(bool(resize)), out)
    return out


def render_maps(maps, extents, hb, wb, tanh=False):
    """One launch: full-resolution maps (H_i, W_i) f32 on the device resized to `extents` (h_i, w_i) into a (N,1,hb,wb) tensor whose
    remainder holds the background value.  The maps must stay alive until the launch has run (the caller's references do that)."""
    device = maps[0].device
    out = torch.empty((len(maps), 1, hb, wb), dtype=torch.float32, device=device)
    if out.numel() == 0:
        return out
    for m in maps:
        if m.dim() != 2 or m.dtype != torch.float32 or not m.is_contiguous() or m.device != device:
            raise ValueError('targets are contiguous (H,W) float32 maps on one device')
    ptrs = staging.upload_values([m.data_ptr() for m in maps], torch.int64, device)
    g = staging.upload_values([[m.shape[0], m.shape[1], 1, int(h), int(w)] for m, (h, w) in zip(maps, extents)], torch.int32, device).reshape(len(maps), G.GEOM)
    torch.ops.cvpce_amd.gauss_targets(None, None, ptrs, g, None, 0, 0, 0.0, 0.0, 0.0, int(bool(tanh)), 1, out)
    return out


def render_full(w, h, boxes, size_reduction=1, generate_method=None, join_method=None, tanh=False):
    """`datautils.generate_gaussians`: the full-resolution map (h // r, w // r) of one image, no resize."""
    r = int(size_reduction)
    if r < 1:
        raise ValueError('size_reduction is a positive integer')
    hs, ws = int(h) // r, int(w) // r
    boxes = torch.as_tensor(boxes)
    return render_boxes([boxes], [(int(h), int(w), r, hs, ws)], hs, ws, generate_method, join_method, tanh, resize=False)[0, 0]


def loss(predictions, targets, extents=None, negative_threshold=0.0, positive_threshold=0.1, min_negatives=1000, negatives_per_positive=3):
    """The loss kernels: `extents` None -> one segment over the whole tensor (the reference), else (N,2) int32 on the device -> one
    segment per image over its own corner.  -> (out_f (S,3) f32: loss, pos_sum, neg_sum; out_i (S,2) i32: pos_count,
    neg_count_used), on the device.  A memset and six launches, no host wait."""
    if predictions.dim() != 4 or predictions.shape[1] != 1 or predictions.shape != targets.shape:
        raise ValueError('predictions and targets are (N,1,Hb,Wb)')
    n, _, hb, wb = predictions.shape
    segments = n if extents is not None else 1
    nbytes = G.loss_workspace_bytes(n, hb, wb)
    if nbytes == 0:
        raise ValueError(f'gaussian loss: unsupported shape {tuple(predictions.shape)} (empty, or 2^31 elements and more)')
    device = predictions.device
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
    out_f = torch.empty((segments, 3), dtype=torch.float32, device=device)
    out_i = torch.empty((segments, 2), dtype=torch.int32, device=device)
    torch.ops.cvpce_amd.gauss_loss(predictions.contiguous(), targets, extents, float(negative_threshold), float(positive_threshold),
                                   int(min_negatives), int(negatives_per_positive), int(extents is not None), workspace, out_f, out_i)
    return out_f, out_i


def reference_loss(predictions, targets, sizes, tanh=False, negative_threshold=0.0, positive_threshold=0.1, min_negatives=1000,
                   negatives_per_positive=3):
    """`models.proposals.gaussian_loss`."""
    if not predictions.is_cuda:
        raise RuntimeError('gaussian_loss runs on an MI355X (HIP) device only (no CPU fallback)')
    if not len(targets) == len(sizes) == predictions.shape[0]:
        raise ValueError('one target map and one size per image of the batch')
    device = predictions.device
    maps = [t.to(device=device, dtype=torch.float32, non_blocking=True).contiguous() for t in targets]
    extents = [(int(s[0]) // 2, int(s[1]) // 2) for s in sizes]
    hb, wb = predictions.shape[2:]
    if any(h > hb or w > wb for h, w in extents):
        raise ValueError('a target does not fit the predictions (the reference fails on the same assignment)')
    batch_targets = render_maps(maps, extents, hb, wb, tanh)
    out_f, _ = loss(predictions.to(torch.float32), batch_targets, None, negative_threshold, positive_threshold, min_negatives,
                    negatives_per_positive)
    return out_f[0, 0]


def summarise(values, outlier_threshold):
    """Per-image losses (n,) on the host -> {'loss', 'mean', 'std' (unbiased, the reference's torch.std), 'outliers': indices with
    loss > mean + outlier_threshold * std}: the reference's outlier rule, shared with device_headloss."""
    if not values.numel():
        return {'loss': values, 'mean': float('nan'), 'std': float('nan'), 'outliers': []}
    mean = float(values.mean())
    std = float(values.std()) if values.numel() > 1 else float('nan')
    outliers = [int(i) for i in (values > mean + outlier_threshold * std).nonzero().flatten()] if values.numel() > 1 else []
    return {'loss': values, 'mean': mean, 'std': std, 'outliers': outliers}


class GaussianScore:
    """Device-resident accumulator of per-image Gaussian losses: `update` per batch, `compute` once at the end.

    Every image is scored over its OWN padded extent (its transformed size rounded up to the size divisor, halved): the pixel
    set the reference scores at batch size 1, whatever batch it arrives in here."""

    def __init__(self, model, generate_method=None, join_method=None, outlier_threshold=3, **loss_params):
        self.model = model
        self.generate_method, self.join_method = _methods(generate_method, join_method)
        self.tanh = bool(model.backbone.gaussian_subnet.tanh) if 'tanh' not in loss_params else bool(loss_params.pop('tanh'))
        params = dict(negative_threshold=0.0, positive_threshold=0.1, min_negatives=1000, negatives_per_positive=3)
        given = dict(getattr(model, 'gaussian_loss_params', None) or {})
        given.update(loss_params)
        if 'tanh' in given:
            self.tanh = bool(given.pop('tanh'))
        unknown = sorted(set(given) - set(params))
        if unknown:
            raise TypeError(f'unknown gaussian_loss parameters: {unknown}')
        params.update(given)
        self.loss_params = params
        self.outlier_threshold = outlier_threshold
        self._losses = []
        self.images = 0
        self.host_copies = 0

    def update(self, results, target_boxes, original_sizes):
        """Queue the scoring of one batch the detector just ran.  results: its list of dicts (their 'gaussians' are (1,Hb,Wb) maps of
        one padded batch); target_boxes: one integer (T,4) tensor per image; original_sizes: one (H, W) per image."""
        if not len(results) == len(target_boxes) == len(original_sizes):
            raise ValueError('one result, one box tensor and one size per image')
        if not results:
            return
        pred = torch.stack([r['gaussians'] for r in results]).to(torch.float32)
        if pred.dim() != 4 or pred.shape[1] != 1:
            raise ValueError("r['gaussians'] is a (1,Hb,Wb) map")
        hb, wb = pred.shape[2:]
        geometry = self.model.image_geometry(original_sizes)
        geom = [(int(h0), int(w0), 1, rh // 2, rw // 2) for (h0, w0), ((rh, rw), _) in zip(original_sizes, geometry)]
        extents = [[min(ph // 2, hb), min(pw // 2, wb)] for _, (ph, pw) in geometry]
        targets = render_boxes(target_boxes, geom, hb, wb, self.generate_method, self.join_method, self.tanh, True, pred.device)
        ext = staging.upload_values(extents, torch.int32, pred.device).reshape(len(extents), 2)
        out_f, _ = loss(pred, targets, ext, **self.loss_params)
        self._losses.append(out_f)
        self.images += len(results)

    def device_losses(self):
        """The accumulated per-image losses (n,) still on the device, in the order given; None before the first update.  For a
        caller that brings them to the host together with something else (device_headloss.compute_together); no copy is made here."""
        return torch.cat(self._losses)[:, 0] if self._losses else None

    def compute(self):
        """The single device-to-host copy -> {'loss': (n,) per-image losses in the order given, 'mean', 'std' (unbiased, the
        reference's torch.std), 'outliers': indices with loss > mean + outlier_threshold * std}."""
        values = self.device_losses()
        if values is None:
            return summarise(torch.zeros(0), self.outlier_threshold)
        values = values.cpu()
        self.host_copies += 1
        return summarise(values, self.outlier_threshold)
