"""Scoring the detector's classification and regression heads on the device -- the counterpart of the first two losses of the
reference's `GaussianLayerNetwork.compute_loss` (cvpce/models/proposals.py:169-175: torchvision 0.9's RetinaNet losses), by which its
`gln seek-sku110k-outliers` ranks images.  The rule is DESIGN.md 4d; the kernels are csrc/headloss.hip.

Through torch ops the matching materialises an (anchors x boxes) IoU matrix per image -- about 190 000 x 700 floats for a SKU-110K
shelf -- and passes over it three times.  Here the matrix is never stored: a memset and three launches per batch, whatever the
number of boxes.  `HeadScore.update` queues device work only -- every upload goes through pinned memory, nothing is read back --
and `compute` brings the accumulated per-image losses and counts to the host in one copy, like `device_gaussians.GaussianScore`.
"""
import torch

from . import torch_ops_headloss as H   # (registers torch.ops.cvpce_amd.headloss)
from .device_gaussians import summarise
from . import staging

# stream operations `HeadScore.update` queues per batch, whatever the number of boxes and anchors:
#   launches: the memset of the boxes' best IoUs, headloss_match, headloss_terms, headloss_finish, the batch's result row   4 + 1
#   uploads (pinned, asynchronous): boxes, labels, box offsets, scale factors                                              4 copies
# (boxes or labels that already live on the device are packed there instead: a cat and a cast in place of that upload)
LAUNCHES_PER_BATCH = 5
UPLOADS_PER_BATCH = 4
HOST_WAITS_PER_BATCH = 0


def check_targets(targets, num_classes):
    """What torchvision's RetinaNet.forward checks of its targets, before anything is queued: a ValueError for a box with x2 <= x1 or
    y2 <= y1, a label outside [0, num_classes), boxes that are not (T,4) or a boxes / labels length mismatch.  Only host tensors are
    inspected: reading a device tensor here would make the host wait."""
    for i, t in enumerate(targets):
        boxes, labels = torch.as_tensor(t['boxes']), torch.as_tensor(t['labels'])
        if boxes.numel() % 4 or (boxes.numel() and (boxes.dim() != 2 or boxes.shape[1] != 4)):
            raise ValueError(f'target {i}: boxes are (T,4) xyxy, got {tuple(boxes.shape)}')
        if labels.is_floating_point() or labels.dtype == torch.bool:
            raise ValueError(f'target {i}: labels are integers, got {labels.dtype}')
        if labels.numel() != boxes.numel() // 4:
            raise ValueError(f'target {i}: {boxes.numel() // 4} boxes and {labels.numel()} labels')
        # (host values are read through numpy: no tensor op, so nothing here can be mistaken for -- or become -- a device read)
        if boxes.numel() and not boxes.is_cuda:
            b = boxes.detach().reshape(-1, 4).numpy()
            bad = ~((b[:, 2] > b[:, 0]) & (b[:, 3] > b[:, 1]))
            if bad.any():
                k = int(bad.nonzero()[0][0])
                raise ValueError(f'target {i}: all bounding boxes should have positive height and width, found {b[k].tolist()} at index {k}')
        if labels.numel() and not labels.is_cuda:
            v = labels.detach().numpy()
            if int(v.min()) < 0 or int(v.max()) >= num_classes:
                raise ValueError(f'target {i}: labels lie in [0, {num_classes}), found {int(v.min())} .. {int(v.max())}')


def scale_factors(transformed_sizes, original_sizes):
    """(N,2) float32 host tensor of `resize_boxes`' ratios (ratio_h, ratio_w) = float32(transformed) / float32(original)."""
    new = torch.tensor([[int(h), int(w)] for h, w in transformed_sizes], dtype=torch.float32).reshape(-1, 2)
    old = torch.tensor([[int(h), int(w)] for h, w in original_sizes], dtype=torch.float32).reshape(-1, 2)
    return new / old


def head_losses(cls, reg, grids, strides, base_anchors, boxes, labels, scales):
    """The memset and the three launches of one batch -> (out_f (N,2) f32: classification, bbox_regression per image; out_i (N,3)
    i32: foreground, between, restored anchors; matched (N,A_total) i32: box index, -1 background, -2 between), all on the device.

    cls, reg: the per-level head outputs of the eval-mode pass, (N,gh,gw,A*K) and (N,gh,gw,A*4) float32, as the post-processing
    reads them; grids, strides: (gh, gw) and (stride_h, stride_w) per level; base_anchors (L,A,4) on the device; boxes, labels: one
    (T_i,4) float xyxy tensor in original pixels and one (T_i,) integer tensor per image (host or device); scales: (N,2) ratio_h,
    ratio_w (`scale_factors`).  Device work only, no host wait."""
    n, device = cls[0].shape[0], cls[0].device
    num_anchors = base_anchors.shape[1]
    if not len(boxes) == len(labels) == n:
        raise ValueError('one box tensor and one label tensor per image of the batch')
    if len(cls) != len(reg) or len(cls) != len(grids) or len(cls) != len(strides) or base_anchors.shape[0] != len(cls):
        raise ValueError('one cls, reg, grid, stride and base-anchor entry per level')
    cells = [int(g[0]) * int(g[1]) * num_anchors for g in grids]
    if cls[0].numel() % (n * cells[0]):
        raise ValueError('the logits of a level are (N,gh,gw,A*K)')
    num_classes = cls[0].numel() // (n * cells[0])
    boxes = [torch.as_tensor(b) for b in boxes]
    labels = [torch.as_tensor(l) for l in labels]
    counts = [int(b.numel()) // 4 for b in boxes]
    if any(int(l.numel()) != c for l, c in zip(labels, counts)):
        raise ValueError('one label per box')
    sum_t = sum(counts)
    nbytes = H.workspace_bytes([g[0] for g in grids], [g[1] for g in grids], num_anchors, n, sum_t)
    if nbytes == 0:
        raise ValueError(f'head losses: unsupported shape ({n} images, {sum(cells)} anchors, {sum_t} boxes: empty, or 2^31 elements and more)')
    packed = staging.pack_once(boxes, torch.float32, device, (4,))
    packed_labels = staging.pack_once(labels, torch.int32, device)
    offsets = staging.upload_values(staging.offsets(counts), torch.int32, device)
    scales = torch.as_tensor(scales, dtype=torch.float32).reshape(n, 2)
    if not scales.is_cuda:
        scales = staging.upload(scales, device)
    workspace = torch.empty(nbytes, dtype=torch.uint8, device=device)
    matched = torch.empty((n, sum(cells)), dtype=torch.int32, device=device)
    out_f = torch.empty((n, 2), dtype=torch.float32, device=device)
    out_i = torch.empty((n, 3), dtype=torch.int32, device=device)
    torch.ops.cvpce_amd.headloss([c.contiguous() for c in cls], [r.contiguous() for r in reg], [int(g[0]) for g in grids],
                                 [int(g[1]) for g in grids], [int(s[0]) for s in strides], [int(s[1]) for s in strides],
                                 base_anchors.contiguous(), packed, packed_labels, offsets, scales.contiguous(), num_anchors, num_classes,
                                 workspace, matched, out_f, out_i)
    return out_f, out_i, matched


class HeadScore:
    """Device-resident accumulator of per-image head losses: `update` per batch with what `model.head_outputs()` hands out, `compute`
    once at the end.  Every image is scored over the anchors of the padded batch it arrives in, as the reference's compute_loss does:
    at batch size 1 (the reference's command) that is the image's own padded extent, in a larger batch the anchors over the extra
    padding count as background."""

    def __init__(self, model, outlier_threshold=3):
        self.model = model
        self.outlier_threshold = outlier_threshold
        self._rows = []
        self.images = 0
        self.host_copies = 0

    def update(self, head_outputs, targets, original_sizes):
        """Queue the scoring of one batch the detector just ran.  head_outputs: `model.head_outputs()` of that pass; targets: one
        dict with 'boxes' (T,4) and 'labels' (T,) per image; original_sizes: one (H, W) per image."""
        if head_outputs is None:
            raise RuntimeError('no head outputs were kept: call model.keep_head_outputs(True) before the forward pass')
        if not len(targets) == len(original_sizes) == len(head_outputs['sizes']):
            raise ValueError('one target and one size per image of the batch')
        if not targets:
            return
        check_targets(targets, self.model.num_classes)
        cls, reg = head_outputs['cls'], head_outputs['reg']
        padded = head_outputs['padded']
        grids = [(c.shape[1], c.shape[2]) for c in cls]
        strides = [(padded[0] // g[0], padded[1] // g[1]) for g in grids]
        out_f, out_i, _ = head_losses(cls, reg, grids, strides, self.model.engine().base_anchors, [t['boxes'] for t in targets],
                                      [t['labels'] for t in targets], scale_factors(head_outputs['sizes'], original_sizes))
        self._rows.append(torch.cat([out_f, out_i.view(torch.float32)], dim=1))     # (bit patterns: one tensor, one copy at the end)
        self.images += len(targets)

    def compute(self):
        """The single device-to-host copy -> {'classification': {...}, 'bbox_regression': {...}, 'counts': (n,3) int32 foreground,
        between, restored per image}; each loss entry holds 'loss' (n,) per-image values in the order given, 'mean', 'std' (unbiased,
        the reference's torch.std) and 'outliers': indices with loss > mean + outlier_threshold * std."""
        if not self._rows:
            return self._result(torch.zeros((0, 5)))
        rows = torch.cat(self._rows).cpu()
        self.host_copies += 1
        return self._result(rows)

    def _result(self, rows):
        return {'classification': summarise(rows[:, 0].contiguous(), self.outlier_threshold),
                'bbox_regression': summarise(rows[:, 1].contiguous(), self.outlier_threshold),
                'counts': rows[:, 2:5].contiguous().view(torch.int32)}


def compute_together(head_score, gaussian_score):
    """`head_score.compute()` and `gaussian_score.compute()` of the same images with ONE device-to-host copy between them (counted in
    `head_score.host_copies`) -> the head score's dict plus 'gaussian': the Gaussian score's."""
    if head_score.images != gaussian_score.images:
        raise ValueError('the two scores saw different images')
    gauss = gaussian_score.device_losses()
    if gauss is None:
        return dict(head_score.compute(), gaussian=gaussian_score.compute())
    rows = torch.cat([torch.cat(head_score._rows), gauss[:, None]], dim=1).cpu()
    head_score.host_copies += 1
    return dict(head_score._result(rows), gaussian=summarise(rows[:, 5].contiguous(), gaussian_score.outlier_threshold))
