"""Pipeline objects on MI355X -- drop-in for /root/reference/cvpce/production.py
(`ProposalGenerator` :8-20, `Classifier` :22-74, `PlanogramEvaluator` :118-129).

Differences from the reference, all on the device-boundary side:
  * crops / embeddings stay on the GPU (the reference builds crops on the CPU in a Python loop);
  * `BatchedPipeline` runs detect -> crop -> embed -> match for a whole batch of shelf images with a
    single host synchronisation at the end (the reference: one image, one box at a time);
  * degenerate (zero-area after `.to(long)`) boxes make the reference raise inside
    `resize_for_classification`; here they are dropped (documented divergence).
"""
import itertools
import os

import torch

from . import datautils, ops
from .staging import offsets, upload
from .models.classification import TANH_MEAN, TANH_STD


# Crops / gallery images handed to the encoder per call.  The reference's `batch_size` (8 in cvpce/cli/eval.py, 32 by default) bounds
# the memory of ONE forward pass on its GPU; here a pass over 8 crops would leave 7/8 of the chip idle (a conv5 layer is two
# workgroups per crop), and the per-crop results do not depend on what else is in the batch (no batch statistics; tests assert
# bit-identical embeddings), so `batch_size` is treated as a lower bound and calls are coalesced up to this many images.
ENGINE_BATCH = 1024
INDEX_BATCH = 64      # build_index: gallery images per pass (the host side -- reading and staging f32 images -- dominates there)
PINNED_STAGING = True  # build_index: persistent pinned double buffer instead of torch.stack + pin_memory per pass
# build_index: gallery byte images (uint8 (h,w,3) items) are uploaded as bytes and packed by csrc/gallery.hip; off (an A/B
# switch), they become float items on the host (`datautils.gallery_float`) and take the float path.  Same embeddings, bit for bit.
GALLERY_U8 = os.environ.get('CVPCE_GALLERY_U8', '1') != '0'
_INDEX_GENERATIONS = itertools.count(1)         # Classifier.index_generation: a new number at every refresh of a classifier's index


def is_gallery_bytes(img):
    """Whether a gallery item's image is a gallery byte image: a uint8 (h,w,3) tensor."""
    return torch.is_tensor(img) and img.dtype == torch.uint8 and img.dim() == 3 and img.shape[2] == 3


def pack_gallery_bytes(images, buf, geom, size=datautils.CLASSIFICATION_IMAGE_SIZE):
    """The host side of a byte pass: copies every image's bytes ONCE, back to back with no alignment between images, into the flat
    uint8 buffer `buf` and writes (byte offset, h, w) per image into geom (>= len(images),3) int32 -> the bytes used.
    images: uint8 (h,w,3) tensors with 1 <= h, w <= size (anything else: ValueError, before anything is copied)."""
    for img in images:
        if not is_gallery_bytes(img) or not (1 <= img.shape[0] <= size and 1 <= img.shape[1] <= size):
            raise ValueError(f'a gallery byte image is a uint8 (h,w,3) tensor with 1 <= h, w <= {size}, got {img.dtype} {tuple(img.shape)}')
    total = sum(img.numel() for img in images)
    if total > buf.numel() or len(images) > geom.shape[0]:
        raise ValueError(f'{len(images)} images of {total} bytes do not fit the staging buffers ({buf.numel()} bytes, {geom.shape[0]} rows)')
    off, rows = 0, []
    for img in images:
        k = img.numel()
        buf[off:off + k].copy_(img.reshape(-1))
        rows.append((off, int(img.shape[0]), int(img.shape[1])))
        off += k
    if rows:
        geom[:len(rows)].copy_(torch.tensor(rows, dtype=torch.int32))
    return off


def _nondegenerate(boxes):
    b = boxes.to(torch.long)
    return ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)


class ProposalGenerator:
    def __init__(self, detector, device=torch.device('cuda'), confidence_threshold=0.5):
        self.detector = detector
        self.device = device
        self.condfidence_threshold = confidence_threshold  # (sic) production.py:12

    def generate_proposals(self, image):
        """image: float (3,H,W) or 8-bit (H,W,3) (uploaded as bytes; read as bytes by the detector's transform with ops.U8_KERNELS on,
        converted on the device with it off or for a detector that is not ours)."""
        if ops.is_uint8_image(image):
            image = self._upload(image)
        if ops.is_uint8_image(image):
            res = self.detector([image])[0]
        else:
            res = self.detector(image[None].to(self.device))[0]
        return res['boxes'][res['scores'] > self.condfidence_threshold]

    def _upload(self, image):
        """ops.input_image for our detector (its transform reads bytes); any other detector object gets the float image, as before."""
        if hasattr(self.detector, 'engine'):
            return ops.input_image(image, self.device)
        return ops.device_image(image, self.device)

    def _confident_boxes(self, img):
        """The confident, non-degenerate boxes of one image with ONE host synchronisation: the detector's kept boxes are sorted by
        score, so `scores > threshold` is a prefix whose length the post-processing kernel already counted (conf_count); the
        prefix length and the <= detections_per_img boxes come to the host in one small copy, where the degenerate-box test
        (production.py:20 `.to(long)` slices of zero area) costs nothing.  The generic path (boolean masks on the device) costs
        three synchronisations and ~10 tiny launches per image."""
        det = self.detector
        boxes, scores, labels, count, conf, gauss = det.engine().detect([img], det.num_classes, det.detections_per_img, self.condfidence_threshold)
        det.backbone.gaussians = None
        dpi = boxes.shape[1]
        host = self.__dict__.get('_pin')                     # pinned staging buffer: dpi boxes + the prefix length, reused across calls
        if host is None or host.numel() != dpi * 4 + 1:
            host = self._pin = torch.empty(dpi * 4 + 1, dtype=torch.float32).pin_memory()
        packed = torch.cat((boxes[0].reshape(-1), conf[:1].to(torch.float32)))
        host.copy_(packed, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        c = int(host[-1])
        b = host[:c * 4].view(c, 4).to(torch.long)
        ok = ((b[:, 2] - b[:, 0]) > 0) & ((b[:, 3] - b[:, 1]) > 0)
        if bool(ok.all()):
            return boxes[0, :c]
        return boxes[0].index_select(0, ok.nonzero().flatten().to(boxes.device))

    def generate_proposals_and_images(self, image):
        size = datautils.CLASSIFICATION_IMAGE_SIZE
        img = self._upload(image)                            # (either form; uploaded once, detected and cropped from)
        if hasattr(self.detector, 'engine') and not getattr(self.detector, 'training', False):
            boxes = self._confident_boxes(img)
        else:                                   # any other detector object with the reference's call signature
            boxes = self.generate_proposals(img if ops.is_uint8_image(image) else image)
            if len(boxes):
                boxes = boxes[_nondegenerate(boxes)]
        if not len(boxes):
            return boxes, torch.empty((0, 3, size, size), device=self.device)
        return boxes, ops.crop_resize(img, boxes, size, mode=0)


class Classifier:
    """production.py:22-74.  `match_dtype`: operand type of the distance GEMM.  float32 (default) is the reference's
    arithmetic (classification.py:87-95 runs in fp32) on the exact-f32 matrix pipe; bfloat16 is the opt-in fast path
    (bench.py / BatchedPipeline pass it explicitly; its top-1 agreement with the fp32 matcher on real embeddings is measured
    by tools/accuracy.py and bounded in tests/test_gpu_accuracy.py)."""

    def __init__(self, encoder, sample_set, device=torch.device('cuda'), emb_device=torch.device('cuda'),
                 batch_size=32, num_workers=8, k=1, load=None, verbose=False, match_dtype=torch.float32):
        self.batch_size = batch_size
        self.num_workers = num_workers  # reader threads of build_index (the reference's DataLoader workers)
        self.device = device
        self.emb_device = emb_device
        self.k = k
        self.encoder = encoder
        self.match_dtype = match_dtype
        if load is None:
            self.embedding, self.annotations = self.build_index(sample_set, verbose)
        else:
            self.embedding, self.annotations = self.load_index(load)
        self._refresh_gallery()

    @classmethod
    def from_embedding(cls, encoder, embedding, annotations, device=torch.device('cuda'), emb_device=torch.device('cuda'),
                       batch_size=32, k=1, match_dtype=torch.float32):
        """Classifier over an index that already exists (e.g. embedded sharded across GPUs and all_gathered)."""
        self = cls.__new__(cls)
        self.batch_size, self.num_workers, self.device, self.emb_device = batch_size, 0, device, emb_device
        self.k, self.encoder, self.match_dtype = k, encoder, match_dtype
        self.set_index(embedding, annotations)
        return self

    def _refresh_gallery(self):
        """Device-resident gallery operand of the distance GEMM (+ its row norms), built once."""
        g = ops.pad_features(self.embedding.to(device=self.device, dtype=self.match_dtype))
        self._gallery = g
        self._gallery_norms = ops.row_norms(g)
        self._refresh_label_ids()

    def _refresh_label_ids(self):
        """The label-id space the comparator's device re-classification compares in: `label_ids` maps an annotation to an id >= 0 (equal
        annotations, equal id), `gallery_label_id` [G] int32 on the device holds every gallery row's id, and `index_generation` counts
        the refreshes, so that an id vector cached elsewhere (`expected_label_ids`) is known to be stale.  An unhashable annotation
        leaves no id space (`label_ids` None): such a classifier's windows are re-classified per image, as before."""
        self.index_generation = next(_INDEX_GENERATIONS)        # (one counter for all classifiers: no two indices share a number)
        ids = {}
        try:
            rows = [ids.setdefault(a, len(ids)) for a in self.annotations]
        except TypeError:
            self.label_ids, self.gallery_label_id = None, None
            return
        self.label_ids = ids
        self.gallery_label_id = torch.tensor(rows, dtype=torch.int32).to(self.device)

    def expected_label_ids(self, labels):
        """labels (a planogram's expected labels) -> their ids as a list, -1 for a label no gallery item has; None where there is no
        id space or a label is unhashable."""
        if self.label_ids is None:
            return None
        try:
            return [self.label_ids.get(l, -1) for l in labels]
        except TypeError:
            return None

    def set_index(self, embedding, annotations):
        self.embedding, self.annotations = embedding, annotations
        self._refresh_gallery()

    def _gallery_items(self, sample_set):
        """sample_set[0], sample_set[1], ... in order, read by `num_workers` threads a bounded window ahead -- the counterpart of
        the reference's DataLoader(num_workers=..., pin_memory=True) (production.py:37-39): decoding and resizing a product
        photo (PIL releases the GIL) would otherwise serialise with the GPU, which embeds > 5 000 gallery images/s."""
        n = len(sample_set)
        if self.num_workers <= 0 or n < 2:
            for i in range(n):
                yield sample_set[i]
            return
        from collections import deque
        from concurrent.futures import ThreadPoolExecutor
        window = max(2 * self.num_workers, self.batch_size)
        with ThreadPoolExecutor(self.num_workers) as pool:
            pending, nxt = deque(), 0
            while nxt < n or pending:
                while nxt < n and len(pending) < window:
                    pending.append(pool.submit(sample_set.__getitem__, nxt))
                    nxt += 1
                yield pending.popleft().result()

    def build_index(self, sample_set, verbose=False):
        """production.py:36-48.  Gallery images are already in [-1,1] (datautils.py:446): no scale_to_tanh.
        An item's image is either that float (3,256,256) tensor or a gallery byte image, uint8 (h,w,3) (a reader with
        image_format='uint8'): byte images are staged, uploaded and packed as bytes (`flush_bytes`), with the same
        embeddings bit for bit; a sample set may mix the two forms."""
        chunks, annotations, imgs = [], [], []
        step = max(self.batch_size, INDEX_BATCH)
        staging = []          # two pinned host buffers (step, C, H, W) + the event after which each may be refilled
        staging_u8 = []       # byte passes: two [pinned bytes (step * S * S * 3,), pinned geom (step, 3) int32, event]
        S = datautils.CLASSIFICATION_IMAGE_SIZE
        use_bytes = GALLERY_U8 and hasattr(self.encoder, 'engine')      # (any other encoder object: float items, as before)

        def flush_bytes():
            """A pass over gallery byte images: one copy of each image's bytes into pinned memory, two non-blocking uploads (the
            bytes and their geometry), one launch that makes the embedder's input pixels and the content extents; with the work-list
            schedule the constant padding is neither written nor computed on."""
            eng = self.encoder.engine()
            n = len(imgs)
            if not staging_u8:
                staging_u8[:] = [[torch.empty(step * S * S * 3, dtype=torch.uint8).pin_memory(),
                                  torch.empty((step, 3), dtype=torch.int32).pin_memory(), None] for _ in range(2)]
            staging_u8.append(staging_u8.pop(0))
            buf, geom, ev = staging_u8[0]
            if ev is not None:
                ev.synchronize()
            used = pack_gallery_bytes(imgs, buf, geom, S)
            data = buf[:used].to(device=eng.device, non_blocking=True)
            geom_dev = geom[:n].to(device=eng.device, non_blocking=True)
            staging_u8[0][2] = torch.cuda.Event()
            staging_u8[0][2].record()
            mean, std = getattr(self.encoder, 'input_mean', TANH_MEAN), getattr(self.encoder, 'input_std', TANH_STD)
            channels = 4 if getattr(eng, 'stem', None) is not None else 8       # (as BatchedPipeline._crops: the fused stem reads 8-byte pixels)
            if hasattr(eng, 'skip_plan') and eng.will_skip(S):
                packed, ext = ops.gallery_pack_u8(data, geom_dev, n, S, channels, mean, std, content_only=True)
                emb = eng.embed_packed(packed, ext=ext, const_in=eng.const_crop(mean, std, channels, S), partial=True)
            else:
                packed, _ = ops.gallery_pack_u8(data, geom_dev, n, S, channels, mean, std, content_only=False)
                emb = eng.embed_packed(packed)
            chunks.append(emb.detach().to(device=self.emb_device))
            imgs.clear()

        def flush():
            if not imgs:
                return
            first = imgs[0]
            if is_gallery_bytes(first):
                return flush_bytes()
            if first.is_cuda or not torch.cuda.is_available() or not PINNED_STAGING:
                batch = torch.stack(imgs).to(device=self.device)
            else:
                # one pass from the dataset's tensors into a persistent pinned buffer, async upload; the two buffers alternate
                # so that the host fills one while the other's upload / encoder pass is in flight
                if not staging or staging[0][0].shape[1:] != first.shape or staging[0][0].dtype != first.dtype:
                    staging[:] = [[torch.empty((step,) + tuple(first.shape), dtype=first.dtype).pin_memory(), None] for _ in range(2)]
                staging.append(staging.pop(0))
                buf, ev = staging[0]
                if ev is not None:
                    ev.synchronize()
                torch.stack(imgs, out=buf[:len(imgs)])
                batch = buf[:len(imgs)].to(device=self.device, non_blocking=True)
                staging[0][1] = torch.cuda.Event()
                staging[0][1].record()
            chunks.append(self.encoder(batch).detach().to(device=self.emb_device))
            imgs.clear()

        for i, item in enumerate(self._gallery_items(sample_set)):
            img = item[0]
            if is_gallery_bytes(img) and not use_bytes:
                img = datautils.gallery_float(img, S)
            if imgs and is_gallery_bytes(img) != is_gallery_bytes(imgs[0]):
                flush()                                        # a change of form ends the pass: order is kept, mixed sets work
            imgs.append(img)
            annotations.append(item[-1])
            if verbose and (i + 1) % self.batch_size == 0 and (i // self.batch_size) % 100 == 0:
                print(i // self.batch_size)
            if len(imgs) >= step:
                flush()
        flush()
        if chunks:
            embedding = torch.cat(chunks)
        else:
            embedding = torch.empty((0, self.encoder.embedding_size), dtype=torch.float, device=self.emb_device)
        return embedding, annotations

    def save_index(self, pth):
        torch.save({'embedding': self.embedding, 'annotations': self.annotations}, pth)

    def load_index(self, pth):
        idx = torch.load(pth)
        return idx['embedding'], idx['annotations']

    def match(self, emb, return_distance=False):
        """(P,1024) f32 unit-norm on device -> (P,min(k,G)) int64 gallery indices, nearest first (any k: ops.match_topk);
        return_distance: -> (indices, their cosine distances (P,min(k,G)) float32 as the match kernel emits them)."""
        q = ops.pad_features(emb.to(self.match_dtype))
        return ops.match_topk(q, self._gallery, self.k, g_norms=self._gallery_norms, return_distance=return_distance)

    def _embed(self, batch):
        """images (n,3,S,S) in [0,1] on the device -> their embeddings: one pass of the encoder's engine"""
        eng = self.encoder.engine()
        mean, std = getattr(self.encoder, 'input_mean', TANH_MEAN), getattr(self.encoder, 'input_std', TANH_STD)
        packed = ops.pack_embed_input(batch, True, mean, std)  # scale_to_tanh + the encoder's own normalisation, fused
        if hasattr(eng, 'skip_plan') and batch.dim() == 4 and batch.shape[2] == batch.shape[3] and eng.skip_plan(batch.shape[2]) is not None:
            # crops made by resize_for_classification carry a constant 0.5 border below / right of the box content
            # (datautils.py:232-239): the embedder skips the tiles that lie in it -- the extents are read off the crops
            b32 = batch.to(torch.float32).contiguous()
            return eng.embed_packed(packed, ext=ops.pad_extents(b32, 0.5), const_in=eng.const_crop(mean, std, 8, batch.shape[2]))
        return eng.embed_packed(packed)

    def classify_positions(self, image, boxes):
        """The comparator's re-classification of one image's positions, with what the matcher saw: boxes (P,4) xyxy inside `image`
        (either form) are cropped, embedded and matched as `PlanogramComparator._finish` has them classified
        -> (the nearest gallery row of every box: list of P ints, its cosine distance as the match kernel emitted it: (P,) float32
        on the host)."""
        img = ops.input_image(image, self.device)
        crops = ops.crop_resize(img, boxes.to(self.device), datautils.CLASSIFICATION_IMAGE_SIZE, mode=0)
        rows, dist = [], [torch.empty(0, dtype=torch.float32)]
        step = max(self.batch_size, ENGINE_BATCH)
        for i in range(0, len(crops), step):
            idx, d = self.match(self._embed(crops[i:i + step].to(device=self.device)), return_distance=True)
            # one blocking copy per batch, as `classify` has one: the rows, and the distances' bits beside them
            both = torch.stack((idx[:, 0], d[:, 0].contiguous().view(torch.int32).to(torch.int64))).cpu()
            rows += both[0].tolist()
            dist.append(both[1].to(torch.int32).view(torch.float32))
        return rows, torch.cat(dist)

    def classify(self, images, return_embedding=False):
        """production.py:57-74: images (P,3,256,256) in [0,1] -> list[list[str]] (P x k).  (One device-to-host copy of the
        (P,k) indices per batch -- `.tolist()` -- whatever k is.)"""
        res, embs = [], []
        step = max(self.batch_size, ENGINE_BATCH)
        for i in range(0, len(images), step):
            emb = self._embed(images[i:i + step].to(device=self.device))
            if return_embedding:
                embs.append(emb.to(device=self.emb_device))
            nearest = self.match(emb).tolist()
            res += [[self.annotations[j] for j in n] for n in nearest]
        if return_embedding:
            if embs:
                return res, torch.cat(embs)
            return res, torch.empty((0, self.encoder.embedding_size), dtype=torch.float, device=self.emb_device)
        return res


class ComplianceReport:
    """What `PlanogramComparator.report` says about one shelf image (the report rule of DESIGN.md 4b) -- the reference's
    `# TODO: Also return which were actually missing` (production.py:105,116).
      compliance          what `compare` returns for the same inputs, value and type
      status              'ok' | 'no_detections' | 'no_matching' | 'no_homography'; every field below is None unless 'ok'
      outcomes            (n1,) int8: DETECTED 0, RECOVERED 1 (by the re-classification), MISSING 2, OUT_OF_VIEW 3 (the projected
                          position does not lie in the image), UNCHECKED 4 (no classifier or no image)
      expected_positions  (n1, 4) float32: every expected box projected into the image
      seen_labels         per position: the annotation of the nearest gallery row where it was re-classified, else None
      seen_distance       (n1,) float32: that row's cosine distance as the match kernel emitted it, else -1
      occupant            (n1,) int32: the unclaimed detection that sits on an undetected position (IoU >= the claim's threshold, the
                          largest, the lowest index among equals), else -1; occupant_iou (n1,) float32 that IoU, else -1;
                          occupant_labels per position: the occupant's label, else None
      stray               (m,) int64: the unclaimed detections that are no position's occupant -- products the planogram does not know"""
    FIELDS = ('outcomes', 'expected_positions', 'seen_labels', 'seen_distance', 'occupant', 'occupant_iou', 'occupant_labels', 'stray')
    OUTCOMES = ('detected', 'recovered', 'missing', 'out_of_view', 'unchecked')

    def __init__(self, compliance, status, outcomes=None, expected_positions=None, seen_labels=None, seen_distance=None, occupant=None,
                 occupant_iou=None, occupant_labels=None, stray=None):
        self.compliance, self.status = compliance, status
        self.outcomes, self.expected_positions, self.seen_labels, self.seen_distance = outcomes, expected_positions, seen_labels, seen_distance
        self.occupant, self.occupant_iou, self.occupant_labels, self.stray = occupant, occupant_iou, occupant_labels, stray

    def missing(self):
        """the expected positions that hold no product of theirs (MISSING, OUT_OF_VIEW or UNCHECKED) -> list of indices"""
        return [] if self.outcomes is None else torch.where(self.outcomes >= 2)[0].tolist()

    def substituted(self):
        """the missing positions on which an unclaimed detection sits -> list of indices"""
        return [i for i in self.missing() if int(self.occupant[i]) >= 0]

    def to_dict(self):
        """plain JSON-able types (a value that is not finite becomes None; labels go as they are)"""
        def plain(v):
            if torch.is_tensor(v):
                v = v.tolist()
            if isinstance(v, (list, tuple)):
                return [plain(x) for x in v]
            if isinstance(v, float) and (v != v or v in (float('inf'), float('-inf'))):
                return None
            return v
        d = {'compliance': float(self.compliance), 'status': self.status}
        d.update({name: plain(getattr(self, name)) for name in self.FIELDS})
        d.update(missing=self.missing(), substituted=self.substituted())
        return d


class ComparisonSteps:
    """What the step pictures need of one comparison beside its report (`PlanogramComparator.steps`): the two neighbour graphs as
    `nbr` [n][8] int32 tables (-1 = empty; `planograms_device.Graph.nbr`) and the nodes the matcher paired, bool (n1,) and (n2,) --
    each on the device where the route left it (the device routes never copy them back), on the host from the host routes."""
    __slots__ = ('expected_nbr', 'actual_nbr', 'matched_expected', 'matched_actual')

    def __init__(self, expected_nbr, actual_nbr, matched_expected, matched_actual):
        self.expected_nbr, self.actual_nbr, self.matched_expected, self.matched_actual = expected_nbr, actual_nbr, matched_expected, matched_actual

    @classmethod
    def of_host(cls, ge, ga, matching):
        """from the host's networkx graphs and its set of (expected node, actual node) pairs"""
        from . import planograms_device as pd
        return cls(pd.nbr_table(ge), pd.nbr_table(ga), *pd.matched_of_pairs(matching, ge.number_of_nodes(), ga.number_of_nodes()))


class PlanogramComparator:
    """production.py:76-116: graph matching -> RANSAC homography -> per-label IoU matching -> optional re-classification
    of the expected-but-undetected positions (a second trip through the crop / embed / match kernels)."""

    MATCHERS = ('large', 'tonioni')

    def __init__(self, graph_threshold=0.5, device_graphs=False, device_tail=False, device_reclass=False, matcher='large'):
        """matcher: 'large' -- `planograms.large_common_subgraph`, the first sufficiently large common subgraph, the default -- or
        'tonioni' -- `planograms.tonioni_mcs`, the largest of the greedy runs from every hypothesis on: a larger matching on shelves
        with many facings of few products, at a much higher cost on the host (the Tonioni rule of DESIGN.md 4b).  On every device
        route the matching then comes from the Tonioni kernels; an image with more hypotheses (equal-label node pairs; with device
        detections: the bound n2 x the largest multiplicity of an expected label) than `planograms_device.TONIONI_MAX_HYPOTHESES`
        takes the host path and counts in `host_routed`.
        device_graphs (opt-in): the neighbour graphs and the common subgraph come from the kernels of `planograms_device` (its
        documented rule at equal distances); the homography and everything after it stay the host's.  `host_routed`
        counts the images that took the host path with the switch on (a graph of more than 1024 nodes).
        device_tail (opt-in, needs device_graphs): the homography, the projection and the per-label claim run on the device too
        (`planograms_device.finalize_batch`, the tail rule of DESIGN.md 4b): a window's graphs, matchings and tails are launched back
        to back and one copy brings back what the verdict needs; the re-classification runs per image through the host.
        device_reclass (opt-in, needs device_tail): the re-classification of a window's expected-but-undetected positions is one
        device pass too (`planograms_device.reclassify_batch`, the re-classification rule of DESIGN.md 4b): the positions are
        planned behind the tail, cropped to bf16 embedder input, embedded by one schedule, matched by one GEMM and compared as label
        ids; a window costs two waits.  `reclass_host_routed` counts the windows that took the per-image re-classification with the
        switch on (an annotation or an expected label that cannot be hashed into the id space)."""
        if matcher not in self.MATCHERS:
            raise ValueError(f'matcher is one of {self.MATCHERS}, got {matcher!r}')
        if device_tail and not device_graphs:
            raise ValueError('device_tail needs device_graphs: the tail kernels read the matching where the match kernel left it')
        if device_reclass and not device_tail:
            raise ValueError('device_reclass needs device_tail: the plan kernel reads the positions where the tail kernel left them')
        self.graph_threshold = graph_threshold
        self.device_graphs = device_graphs
        self.device_tail = device_tail
        self.device_reclass = device_reclass
        self.matcher = matcher
        self.host_routed = 0
        self.reclass_host_routed = 0

    def compare(self, expected, actual, image=None, classifier=None):
        if self.device_graphs:
            return self.compare_batch([expected], [actual], [image], classifier)[0]
        return self._compare_host(expected, actual, image, classifier)

    def _compare_host(self, expected, actual, image, classifier):
        from . import planograms
        if not len(actual['boxes']):
            return 0 if len(expected['boxes']) else 1
        ge = expected['graph'] if 'graph' in expected else planograms.build_graph(expected['boxes'], expected['labels'],
                                                                                  self.graph_threshold)
        ga = planograms.build_graph(actual['boxes'], actual['labels'], self.graph_threshold)
        return self._finish(self._host_matching(ge, ga), expected, actual, image, classifier)

    def _host_matching(self, ge, ga):
        from . import planograms
        return planograms.tonioni_mcs(ge, ga) if self.matcher == 'tonioni' else planograms.large_common_subgraph(ge, ga)

    def _over_limit(self, hypotheses):
        """whether a pair of `hypotheses` hypotheses (or that bound) has no device form under this comparator's matcher"""
        from . import planograms_device as pd
        return self.matcher == 'tonioni' and hypotheses > pd.TONIONI_MAX_HYPOTHESES

    def compare_batch(self, expecteds, actuals, images=None, classifier=None):
        """[compare(e, a, img, classifier) for ...] with the graph stages of the whole batch in two launches (all graphs, all matchings)
        and one copy back; the host tail (homography, per-label claim, re-classification) runs per image -- with `device_tail` the
        homography and the claim are two more launches of the window and only the re-classification stays per image; with
        `device_reclass` that is one pass of the window as well (`_device_window`: two waits, whatever the number of images with
        positions to classify).  With `device_graphs` off it is the plain loop.  `actuals` may be a `planograms_device.DeviceActuals` --
        a window's detections as `BatchedPipeline.run(actuals=True)` left them on the device -- where `device_graphs` and `device_tail`
        are on (`_compare_device_actuals`)."""
        return self._batch(expecteds, actuals, images, classifier)

    def report(self, expected, actual, image=None, classifier=None):
        """`compare` with its reasons -> `ComplianceReport`: `.compliance` is what `compare` returns, the other fields say which
        expected positions were detected, recovered by the re-classification, missing, out of view or unchecked, what the matcher saw
        there, which unclaimed detection sits on an undetected position and which sit on none (the report rule of DESIGN.md 4b)."""
        if self.device_graphs:
            return self.report_batch([expected], [actual], [image], classifier)[0]
        return self._report_host(expected, actual, image, classifier)

    def report_batch(self, expecteds, actuals, images=None, classifier=None):
        """[report(e, a, img, classifier) for ...] on the route `compare_batch` takes with the same switches, at its number of waits:
        with `device_tail` the outcomes, occupants and strays come from `report_positions` behind the tail and travel in the tail's own
        copy; with `device_reclass` `report_reclass` runs behind the verdict and its rows travel in the verdict's copy; an image that
        `compare_batch` sends through the host gets the host report."""
        return self._batch(expecteds, actuals, images, classifier, report=True)

    def steps(self, expected, actual, image=None, classifier=None):
        """`report` with what the step pictures draw -> (`ComplianceReport`, `ComparisonSteps`, or None for an image without
        detections: it has no graph to draw)."""
        return self.steps_batch([expected], [actual], [image], classifier)[0]

    def steps_batch(self, expecteds, actuals, images=None, classifier=None):
        """[steps(e, a, img, classifier) for ...] on the route `report_batch` takes with the same switches, its reports, launches and
        waits: the graphs and the matching are kept where the route has them anyway -- the device routes' stay on the device."""
        kept = [None] * len(expecteds)
        return list(zip(self._batch(expecteds, actuals, images, classifier, report=True, steps=kept), kept))

    def _host(self, expected, actual, image, classifier, report, steps=None, at=None):
        """steps, at: the list `steps_batch` fills and this image's place in it (report on)"""
        if not report:
            return self._compare_host(expected, actual, image, classifier)
        return self._report_host(expected, actual, image, classifier, steps=steps, at=at)

    def _batch(self, expecteds, actuals, images, classifier, report=False, steps=None):
        """`compare_batch` (report off: verdicts) and `report_batch` (report on: `ComplianceReport`s) on one route.  steps: a list with
        one place per image where `steps_batch` wants the graphs and the matching kept (`ComparisonSteps`)."""
        images = [None] * len(expecteds) if images is None else images
        if not isinstance(actuals, (list, tuple)):
            from . import planograms_device
            if isinstance(actuals, planograms_device.DeviceActuals):          # (detections that never left the device)
                return self._compare_device_actuals(expecteds, actuals, images, classifier, report, steps)
        if not self.device_graphs:
            return [self._host(e, a, img, classifier, report, steps, i) for i, (e, a, img) in enumerate(zip(expecteds, actuals, images))]
        from . import planograms_device as pd
        results, todo = [None] * len(expecteds), []
        for i, (e, a, img) in enumerate(zip(expecteds, actuals, images)):
            if not len(a['boxes']):
                results[i] = self._no_detections(e, report)
            elif (not 1 <= len(e['boxes']) <= pd.MAX_NODES or len(a['boxes']) > pd.MAX_NODES
                  or (self.matcher != 'large' and self._over_limit(pd.hypothesis_count(e['labels'], a['labels'])))):
                self.host_routed += 1
                results[i] = self._host(e, a, img, classifier, report, steps, i)
            else:
                todo.append(i)
        if todo:
            have = {i: pd.cached(expecteds[i], self.graph_threshold) for i in todo}
            build = [expecteds[i] for i in todo if have[i] is None] + [actuals[i] for i in todo]
            built = pd.build_graphs([(g['boxes'], g['labels']) for g in build], self.graph_threshold)
            fresh = iter(built[:len(build) - len(todo)])
            ge = [have[i] if have[i] is not None else next(fresh) for i in todo]
            ga = built[len(build) - len(todo):]
            if self.device_tail:                # graphs -> match -> tail back to back: the matching never leaves the device in between
                ids = self._window_label_ids([expecteds[i] for i in todo], classifier) if self.device_reclass else None
                return self._device_window(results, todo, ge, ga, expecteds, actuals, images, classifier, ids, report, steps=steps)
            matchings = pd.common_subgraphs(ge, ga, matcher=self.matcher)
            for p, (i, matching) in enumerate(zip(todo, matchings)):
                if steps is not None:
                    steps[i] = ComparisonSteps(ge[p].nbr, ga[p].nbr, *pd.matched_of_pairs(matching, len(ge[p]), len(ga[p])))
                if report:
                    results[i] = self._report_host(expecteds[i], actuals[i], images[i], classifier, matching)
                else:
                    results[i] = self._finish(matching, expecteds[i], actuals[i], images[i], classifier)
        return results

    @staticmethod
    def _no_detections(expected, report):
        verdict = 0 if len(expected['boxes']) else 1
        return ComplianceReport(verdict, 'no_detections') if report else verdict

    @staticmethod
    def _image_row(image, classifier):
        """an image's {h, w, enabled} row of the plan and report kernels: enabled where there is something to classify with and in"""
        on = classifier is not None and image is not None
        return datautils.image_hw(image) + (1,) if on else (0, 0, 0)

    # ---- the compliance report (the report rule) --------------------------------------------------------------
    def _report_host(self, expected, actual, image, classifier, matching=None, steps=None, at=None):
        """`_compare_host` with its reasons: the host tail with both of its optional returns, then `planograms.report_positions`.
        matching: the common subgraph where it was found elsewhere (`device_graphs` alone).  steps, at: the list `steps_batch` fills and this
        image's place in it: it takes the `ComparisonSteps` of the graphs and the matching made here."""
        from . import planograms
        if not len(actual['boxes']):
            return self._no_detections(expected, True)
        if matching is None:
            ge = expected['graph'] if 'graph' in expected else planograms.build_graph(expected['boxes'], expected['labels'], self.graph_threshold)
            ga = planograms.build_graph(actual['boxes'], actual['labels'], self.graph_threshold)
            matching = self._host_matching(ge, ga)
            if steps is not None:
                steps[at] = ComparisonSteps.of_host(ge, ga, matching)
        if not len(matching):
            return ComplianceReport(0, 'no_matching')
        tail = planograms.finalize_via_ransac(matching, expected['boxes'], actual['boxes'], expected['labels'], actual['labels'],
                                              reproj_threshold=self._reproj_threshold(image), return_matched_actual=True,
                                              return_expected_positions=True)
        if tail[0] is None:                     # no homography (production.py:98-99)
            return ComplianceReport(len(matching) / len(expected['boxes']), 'no_homography')
        matched_expected, matched_actual, positions = tail[:3]
        hw = datautils.image_hw(image) if classifier is not None and image is not None else None
        outcome, occupant, occupant_iou, stray = planograms.report_positions(matched_expected, matched_actual, positions, actual['boxes'], hw)
        return self._report_finish(outcome, positions, occupant, occupant_iou, stray, [actual['labels'][j] if j >= 0 else None for j in occupant.tolist()],
                                   expected, image, classifier)

    def _report_record(self, rec, expected, actual_labels, image, classifier, final=None, annotations=None):
        """A record of `planograms_device.finalize_batch(..., report=...)` as a `ComplianceReport`.  final: (outcome, seen_row,
        seen_distance) where the window's re-classification decided the pending positions on the device; else they are decided here,
        per image.  actual_labels: the detections' labels, or None where `annotations` names them by the occupants' gallery rows."""
        if not rec['matching']:
            return ComplianceReport(0, 'no_matching')
        if rec['status'] == 'invalid':
            raise RuntimeError('finalize_batch: the matching does not belong to the graphs')
        if rec['status'] != 'ok':
            return ComplianceReport(rec['matching'] / len(expected['boxes']), 'no_homography')
        occupant = rec['occupant']
        if actual_labels is not None:
            labels = [actual_labels[j] if j >= 0 else None for j in occupant.tolist()]
        else:
            labels = [annotations[r] if j >= 0 else None for j, r in zip(occupant.tolist(), rec['occupant_row'].tolist())]
        return self._report_finish(rec['outcome'], rec['expected_positions'], occupant, rec['occupant_iou'], rec['stray'], labels, expected, image,
                                   classifier, final)

    def _report_finish(self, outcome, positions, occupant, occupant_iou, stray, occupant_labels, expected, image, classifier, final=None):
        """The second half of the report rule and the report itself.  Positions that are still PENDING are re-classified here, through
        `classifier.classify_positions`, as `_finish` has them classified; final: what the device made of them instead."""
        from . import planograms
        n1 = len(outcome)
        if final is not None:
            outcome, seen_row, seen_distance = final
        else:
            outcome = outcome.clone()
            seen_row, seen_distance = torch.full((n1,), -1, dtype=torch.int32), torch.full((n1,), -1.0, dtype=torch.float32)
            pending = torch.where(outcome == planograms.PENDING)[0]
            if len(pending):
                h, w = datautils.image_hw(image)
                rows, dist = classifier.classify_positions(image, planograms.clamp_positions(positions[pending], h, w)[0])
                seen_row[pending], seen_distance[pending] = torch.tensor(rows, dtype=torch.int32), dist.to(torch.float32)
                same = torch.tensor([expected['labels'][i] == classifier.annotations[r] for i, r in zip(pending.tolist(), rows)])
                outcome[pending] = torch.where(same, planograms.RECOVERED, planograms.MISSING).to(outcome.dtype)
        found = outcome <= planograms.RECOVERED
        seen = [classifier.annotations[r] if r >= 0 else None for r in seen_row.tolist()]
        return ComplianceReport(found.sum() / len(found), 'ok', outcome.to(torch.int8), positions, seen, seen_distance, occupant.to(torch.int32),
                                occupant_iou, occupant_labels, torch.where(stray)[0])

    def _compare_device_actuals(self, expecteds, actuals, images, classifier, report=False, steps=None):
        """`compare_batch` on detections that never left the device (`planograms_device.DeviceActuals`; the detections rule of
        DESIGN.md 4b): the graph, match and tail kernels read the pack's boxes, label ids and thresholds where `actuals_pack` left
        them; the host knows the box counts alone.  An image without detections is decided here; an image whose expected or actual
        graph has no device form comes back through `to_host` and takes `_compare_host` (`host_routed`); so does a window whose
        expected labels have no ids (a label that cannot be hashed)."""
        from . import planograms_device as pd
        if not (self.device_graphs and self.device_tail):
            raise ValueError('device detections need device_graphs and device_tail: the kernels read the detections where they lie')
        if classifier is None or len(actuals) != len(expecteds):
            raise ValueError('one image of the pack per planogram, and the classifier whose id space the pack was labelled in')
        if actuals.thresh_size != self.graph_threshold:
            raise ValueError(f'the detections carry thresholds for graph_threshold {actuals.thresh_size}, the comparator has {self.graph_threshold}')
        results, todo, routed = [None] * len(expecteds), [], []
        for i, (e, n2) in enumerate(zip(expecteds, actuals.n2)):
            if not n2:
                results[i] = self._no_detections(e, report)
            elif not 1 <= len(e['boxes']) <= pd.MAX_NODES or n2 > pd.MAX_NODES:
                routed.append(i)
            else:
                todo.append(i)
        ids = pd.expected_label_ids([expecteds[i] for i in todo], classifier) if todo else None
        if ids is None:
            routed, todo = sorted(routed + todo), []
        elif self.matcher != 'large':           # (the launch is sized by the bound n2 x largest multiplicity: that is what must fit)
            over = [self._over_limit(actuals.n2[i] * e[1]) for i, e in zip(todo, ids)]
            routed = sorted(routed + [i for i, o in zip(todo, over) if o])
            todo, ids = [i for i, o in zip(todo, over) if not o], [e for e, o in zip(ids, over) if not o]
        for i in routed:
            self.host_routed += 1
            boxes, labels = actuals.to_host(i, classifier.annotations)
            results[i] = self._host(expecteds[i], {'boxes': boxes, 'labels': labels}, images[i], classifier, report, steps, i)
        if not todo:
            return results
        pack = actuals.select(todo)
        es = [expecteds[i] for i in todo]
        have = [pd.cached(e, self.graph_threshold) for e in es]
        fresh = iter(pd.build_graphs([(e['boxes'], e['labels']) for e, h in zip(es, have) if h is None], self.graph_threshold))
        ge = [h if h is not None else next(fresh) for h in have]
        ga = pd.build_graphs(pack, self.graph_threshold)
        # (two id vectors on purpose: `ids` above numbers a label outside the gallery len(space) + rank for the match and claim kernels,
        # these give it -1 for the verdict kernel -- merging them would change what a kernel reads)
        reclass_ids = self._window_label_ids(es, classifier) if self.device_reclass else None
        return self._device_window(results, todo, ge, ga, expecteds, pack, images, classifier, reclass_ids, report, expected_ids=ids, steps=steps)

    def _device_window(self, results, todo, ge, ga, expecteds, actuals, images, classifier, reclass_ids, report, expected_ids=None, steps=None):
        """The device window of the images `todo`: match -> tail (-> plan) back to back on the graphs `ge` / `ga` and
        the first wait; where the plan holds positions, crops -> embedder -> match -> verdict and the second wait
        (`planograms_device.reclassify_batch`) -> `results`, filled at `todo`.
        actuals: the host dicts of all images, or the `DeviceActuals` of the images `todo` with expected_ids, `expected_label_ids`' of
        their planograms.  reclass_ids: `_window_label_ids`' where the window is to be re-classified on the device, else None: no plan
        is asked for, and the re-classification runs per image in `_finish` / `_report_finish`.
        The verdict of an image with a homography in a re-classified window is found_count / n1 -- the value and dtype of `_finish`'s
        found.sum() / len(found); every other image, and a window without positions, ends in `_finish`."""
        from . import planograms_device as pd
        on_host = not isinstance(actuals, pd.DeviceActuals)
        if on_host:
            matching = pd.match_on_device(ge, ga, matcher=self.matcher)
        else:
            matching = pd.match_on_device(ge, ga, actuals=actuals, expected_ids=expected_ids, matcher=self.matcher)
        if steps is not None:                   # (views and a few device operators: nothing is copied back, nothing waited for)
            for p, i in enumerate(todo):
                steps[i] = ComparisonSteps(ge[p].nbr, ga[p].nbr, *pd.matched_nodes(matching, p))
        table = [self._image_row(images[i], classifier) for i in todo] if report or reclass_ids is not None else None
        out = pd.finalize_batch(ge, ga, matching, [pd.expected_boxes_on_device(expecteds[i], ga[0].nbr.device) for i in todo],
                                [actuals[i]['boxes'] for i in todo] if on_host else actuals, [self._reproj_threshold(images[i]) for i in todo],
                                reclass=table if reclass_ids is not None else None, report=table if report else None)
        records, plan = out if reclass_ids is not None else (out, None)
        found = None
        if plan is not None and sum(plan.counts):
            found = pd.reclassify_batch(plan, [images[i] for i in todo], classifier, reclass_ids, report=report)
        if report:
            return self._window_reports(results, todo, records, found, expecteds, actuals if on_host else None, images, classifier)
        for p, (i, rec) in enumerate(zip(todo, records)):
            if found is not None and rec['status'] == 'ok':
                results[i] = torch.tensor(found[p]) / len(expecteds[i]['boxes'])
            else:                               # (`_finish` reads the actual side only where it has to compute the tail itself)
                tail = pd.finalize_result(rec, expecteds[i]['labels']) if rec['matching'] else None
                results[i] = self._finish(rec['matching'], expecteds[i], actuals[i] if on_host else None, images[i], classifier, tail)
        return results

    LABEL_IDS_KEY = 'reclass_label_ids'           # a planogram dict's cached id vector, beside planograms_device.CACHE_KEY

    def _window_label_ids(self, planograms, classifier):
        """The expected labels of a window as ids of the classifier's id space, one list per planogram -- cached in the planogram's
        dict with the classifier's index generation, so a `set_index` invalidates it.  No classifier: nothing will be classified, no
        ids are needed ([None, ...]).  -> None where a label or an annotation cannot be hashed: the window is re-classified per
        image (`reclass_host_routed`)."""
        if classifier is None:
            return [None] * len(planograms)
        generation = getattr(classifier, 'index_generation', None)
        out = []
        for plano in planograms:
            cached = plano.get(self.LABEL_IDS_KEY) if isinstance(plano, dict) else None
            if cached is not None and generation is not None and cached[0] == generation and len(cached[1]) == len(plano['labels']):
                ids = cached[1]
            else:
                ids = classifier.expected_label_ids(plano['labels']) if generation is not None else None
                if ids is None:
                    self.reclass_host_routed += 1
                    return None
                if isinstance(plano, dict):
                    plano[self.LABEL_IDS_KEY] = (generation, ids)
            out.append(ids)
        return out

    def _window_reports(self, results, todo, records, found, expecteds, actuals, images, classifier):
        """The reports of a device window.  found: `reclassify_batch(..., report=True)`'s tuple, or None where the window had no
        position to classify (then no outcome is pending) or the re-classification runs per image.  actuals None: the detections are
        a `DeviceActuals`, their labels are the annotations of the occupants' gallery rows."""
        off = [0]
        for i in todo:
            off.append(off[-1] + len(expecteds[i]['boxes']))
        for p, (i, rec) in enumerate(zip(todo, records)):
            final = None
            if found is not None and rec['status'] == 'ok':
                a = slice(off[p], off[p + 1])
                final = (found[1][a].clone(), found[2][a].clone(), found[3][a].clone())
            results[i] = self._report_record(rec, expecteds[i], actuals[i]['labels'] if actuals is not None else None, images[i], classifier, final,
                                             None if classifier is None else classifier.annotations)
        return results

    @staticmethod
    def _reproj_threshold(image):
        return 10 if image is None else min(datautils.image_hw(image)) * 0.01

    def _finish(self, matching, expected, actual, image, classifier, tail=None):
        """matching: the common subgraph, or its size where `tail` -- `finalize_via_ransac`'s tuple, computed elsewhere -- comes along."""
        from . import planograms
        size = matching if isinstance(matching, int) else len(matching)
        if not size:
            return 0
        if tail is None:
            tail = planograms.finalize_via_ransac(matching, expected['boxes'], actual['boxes'], expected['labels'], actual['labels'],
                                                  reproj_threshold=self._reproj_threshold(image))
        found, missing_indices, missing_positions, missing_labels = tail
        if found is None:                       # no homography (production.py:98-99)
            return size / len(expected['boxes'])
        if classifier is not None and image is not None and len(missing_positions):
            h, w = datautils.image_hw(image)
            pos = missing_positions.clone()
            pos[:, 0::2] = pos[:, 0::2].clamp(min=0, max=w)
            pos[:, 1::2] = pos[:, 1::2].clamp(min=0, max=h)
            valid = (pos[:, 2] - pos[:, 0] > 1) & (pos[:, 3] - pos[:, 1] > 1)
            if not valid.any():
                return found.sum() / len(found)
            idx, pos = missing_indices[valid], pos[valid]
            lbls = [l for l, v in zip(missing_labels, valid) if v]
            img = ops.input_image(image, classifier.device)
            crops = ops.crop_resize(img, pos.to(classifier.device), datautils.CLASSIFICATION_IMAGE_SIZE, mode=0)
            for i, want, got in zip(idx, lbls, classifier.classify(crops)):
                if want == got[0]:
                    found[i] = True
        return found.sum() / len(found)


class PlanogramEvaluator:
    """production.py:118-129 glue; `planogram_comparator` is any object with `.compare(expected, actual, image, classifier)`."""

    def __init__(self, proposal_generator, classifier, planogram_comparator, device_detections=False):
        """device_detections (opt-in, needs a comparator with device_graphs and device_tail): a window's detections are never copied
        to the host before the verdict (the detections rule of DESIGN.md 4b): `BatchedPipeline.run(actuals=True)` counts and packs
        the confident, non-degenerate boxes with their label ids on the device, and the comparator's kernels read them there -- two
        blocking copies and a Python lookup per detection less per size group.  `detections_host_routed` counts the windows that
        took the host route with the switch on (a classifier without an id space)."""
        if device_detections and not (getattr(planogram_comparator, 'device_graphs', False) and getattr(planogram_comparator, 'device_tail', False)):
            raise ValueError('device_detections needs a comparator with device_graphs and device_tail: its kernels read the detections where they lie')
        self.proposal_generator = proposal_generator
        self.classifier = classifier
        self.planogram_comparator = planogram_comparator
        self.device_detections = device_detections
        self.detections_host_routed = 0

    def _float_image(self, image):
        """An 8-bit image becomes the device image here, ONCE (`ops.input_image`: the bytes themselves with ops.U8_KERNELS on, the float
        image with it off): detection, the crops and the comparator's re-classification all read that one.  A float image goes on as it
        came (the callees upload it as before)."""
        if ops.is_uint8_image(image):
            pg = self.proposal_generator
            device = getattr(pg, 'device', self.classifier.device)
            return pg._upload(image) if hasattr(pg, '_upload') else ops.device_image(image, device)
        return image

    def evaluate(self, image, planogram):
        return self._evaluate(image, planogram, False)

    def report(self, image, planogram):
        """`evaluate` with its reasons -> `ComplianceReport` (`PlanogramComparator.report` on the image's detections)."""
        return self._evaluate(image, planogram, True)

    def report_batch(self, images, planograms):
        """[report(image, planogram) for ...] on the route `evaluate_batch` takes with the same switches."""
        return self._evaluate_batch(images, planograms, True)

    def report_iter(self, pairs, lookahead=4):
        """`report(image, planogram)` over an iterable of pairs, windowed as `evaluate_iter` windows them."""
        return self._evaluate_iter(pairs, lookahead, True)

    def pictures(self, image, planogram, renderer):
        """`report` with its pictures -> (`ComplianceReport`, `rendering.CompliancePictures`): the photo with the report drawn on it,
        the observed planogram (every detection's product image where it was detected) and the expected planogram rebuilt the same way,
        composed on the device by `renderer` (a `rendering.SceneRenderer` over the `ThumbnailAtlas` of this classifier's gallery)."""
        return self.pictures_batch([image], [planogram], renderer)[0]

    def pictures_batch(self, images, planograms, renderer):
        """[pictures(image, planogram, renderer) for ...] on the route `report_batch` takes with the same switches; the reports are
        `report_batch`'s, and all pictures of the window come from ONE `renderer.render` call: one launch, no wait.  With
        `device_detections` the detections' boxes and gallery rows are read from the window's device pack and never visit the host;
        on the host routes a label becomes the first gallery row that carries it (`rendering.label_rows`), -1 -- an empty rectangle --
        where the gallery has none."""
        from . import rendering
        images, planograms = [self._float_image(img) for img in images], list(planograms)
        if not images:
            return []
        table = self._label_rows()
        if self._on_device():
            reports, dets = self._device_window(images, planograms, True)
        else:
            host = self.detect_and_classify_batch(images)
            reports = self._compare_all(images, planograms, host, True)
            dets = [(b, rendering.rows_of_labels(labels, table)) for b, labels in host]
        lists, sizes, bases = [], [], []
        for img, plano, rep, (boxes, rows) in zip(images, planograms, reports, dets):
            hw = datautils.image_hw(img)
            ehw = rendering.expected_canvas_hw(plano['boxes'], hw[1])
            lists += [rendering.annotation_items(rep, boxes, rendering.ANNOTATION_THICKNESS, hw), rendering.observed_items(boxes, rows),
                      rendering.expected_items(plano['boxes'], rendering.rows_of_labels(plano['labels'], table), ehw)]
            sizes += [hw, hw, ehw]
            bases += [img, None, None]
        views = renderer.render(lists, sizes, bases)
        return [(rep, rendering.CompliancePictures(*views[3 * k:3 * k + 3])) for k, rep in enumerate(reports)]

    def pictures_iter(self, pairs, renderer, lookahead=4):
        """`pictures(image, planogram, renderer)` over an iterable of pairs, windowed as `report_iter` windows them: one `render` call
        per window."""
        window = []
        for image, planogram in pairs:
            image = self._float_image(image)
            if window and (len(window) >= max(1, lookahead) or datautils.image_hw(image) != datautils.image_hw(window[0][0])):
                yield from self.pictures_batch([img for img, _ in window], [plano for _, plano in window], renderer)
                window.clear()
            window.append((image, planogram))
        if window:
            yield from self.pictures_batch([img for img, _ in window], [plano for _, plano in window], renderer)

    def step_pictures(self, image, planogram, renderer):
        """`pictures` step by step -> (`ComplianceReport`, `rendering.StepPictures`): the detections and the projected positions on
        the photo, the two neighbour graphs and the common subgraph the matcher found drawn over the rebuilt planograms, and the three
        pictures of `pictures` -- what the reference's `plot-planogram-eval` and `misc pipeline-demo` show in matplotlib windows."""
        return self.step_pictures_batch([image], [planogram], renderer)[0]

    def step_pictures_batch(self, images, planograms, renderer):
        """[step_pictures(image, planogram, renderer) for ...] on the route `report_batch` takes with the same switches; the reports are
        `report_batch`'s, the last three pictures `pictures_batch`'s byte for byte, and all pictures of the window come from ONE
        `renderer.render` call: the compositor's launch and the stroke launch over its output, no wait.  The graphs and the matching
        are drawn from where the comparator's route left them (`PlanogramComparator.steps_batch`); an image whose report says
        'no_detections' or 'no_matching' has no strokes, one that is not 'ok' no rings on `positions`."""
        from . import rendering
        images, planograms = [self._float_image(img) for img in images], list(planograms)
        if not images:
            return []
        if not hasattr(self.planogram_comparator, 'steps_batch'):
            raise TypeError('step pictures need a comparator that keeps its graphs and its matching (`PlanogramComparator.steps_batch`)')
        table = self._label_rows()
        if self._on_device():
            both, dets = self._device_window(images, planograms, True, steps=True)
        else:
            host = self.detect_and_classify_batch(images)
            both = self._compare_all(images, planograms, host, True, steps=True)
            dets = [(b, rendering.rows_of_labels(labels, table)) for b, labels in host]
        # the photos as bytes, each made once (float planes by `render`'s own rule) and joined into ONE allocation: `render` reads bases that
        # are views of one allocation where they lie, so a photo that is the base of three canvases is not copied three times
        photos = [(img if img.dtype == torch.uint8 else rendering.float_image_bytes(img.to(renderer.device))).to(renderer.device) for img in images]
        pool, at = torch.cat([p.reshape(-1) for p in photos]), 0
        lists, sizes, bases, strokes = [], [], [], []
        for img, photo, plano, (rep, steps), (boxes, rows) in zip(images, photos, planograms, both, dets):
            base, at = pool[at:at + photo.numel()].view(photo.shape), at + photo.numel()
            hw = datautils.image_hw(img)
            ehw = rendering.expected_canvas_hw(plano['boxes'], hw[1])
            # (a list that several canvases share goes to the device once, not once per canvas)
            annotated = rendering.annotation_items(rep, boxes, rendering.ANNOTATION_THICKNESS, hw).to(renderer.device)
            observed = rendering.observed_items(boxes, rows).to(renderer.device)
            expected = rendering.expected_items(plano['boxes'], rendering.rows_of_labels(plano['labels'], table), ehw).to(renderer.device)
            ringed = lambda b, colour: rendering.ring_items(b, colour, rendering.ANNOTATION_THICKNESS, hw, boxes.device).to(renderer.device)
            lists += [ringed(boxes, rendering.DETECTION_COLOUR), ringed(rep.expected_positions if rep.status == 'ok' else None, rendering.POSITION_COLOUR),
                      expected, observed, expected, observed, annotated, observed, expected]
            sizes += [hw, hw, ehw, hw, ehw, hw, hw, hw, ehw]
            bases +=[base, base, None, None, None, None, base, None, None]
            if steps is None or rep.status in ('no_detections', 'no_matching'):
                strokes += [None] * 9
            else:
                on_canvas = rendering.expected_boxes_on_canvas(plano['boxes'], ehw)
                ge, ga = rendering.graph_strokes(steps.expected_nbr, on_canvas), rendering.graph_strokes(steps.actual_nbr, boxes)
                strokes += [None, None, ge, ga, rendering.matched_strokes(steps.expected_nbr, on_canvas, steps.matched_expected, whole=ge),
                            rendering.matched_strokes(steps.actual_nbr, boxes, steps.matched_actual, whole=ga), None, None, None]
        views = renderer.render(lists, sizes, bases, strokes=strokes)
        return [(rep, rendering.StepPictures(*views[9 * k:9 * k + 9])) for k, (rep, _) in enumerate(both)]

    def step_pictures_iter(self, pairs, renderer, lookahead=4):
        """`step_pictures(image, planogram, renderer)` over an iterable of pairs, windowed as `pictures_iter` windows them."""
        window = []
        for image, planogram in pairs:
            image = self._float_image(image)
            if window and (len(window) >= max(1, lookahead) or datautils.image_hw(image) != datautils.image_hw(window[0][0])):
                yield from self.step_pictures_batch([img for img, _ in window], [plano for _, plano in window], renderer)
                window.clear()
            window.append((image, planogram))
        if window:
            yield from self.step_pictures_batch([img for img, _ in window], [plano for _, plano in window], renderer)

    def _label_rows(self):
        """`rendering.label_rows` of the classifier's annotations, made once per index (`index_generation`)"""
        from . import rendering
        generation = getattr(self.classifier, 'index_generation', None)
        cached = self.__dict__.get('_label_rows_cache')
        if cached is None or generation is None or cached[0] != generation:
            cached = self._label_rows_cache = (generation, rendering.label_rows(self.classifier.annotations))
        return cached[1]

    def _evaluate(self, image, planogram, report):
        image = self._float_image(image)
        if self._on_device():
            return self._evaluate_on_device([image], [planogram], report)[0]
        boxes, images = self.proposal_generator.generate_proposals_and_images(image)
        classes = [ann[0] for ann in self.classifier.classify(images)]
        cmp = self.planogram_comparator
        return (cmp.report if report else cmp.compare)(planogram, {'boxes': boxes.detach().cpu(), 'labels': classes}, image, self.classifier)

    def detect_and_classify_batch(self, images):
        """[(boxes (P,4) cpu, labels list[str])] for a list of images -- what `evaluate` hands to the comparator, per image, but
        computed for the whole list at once: images of one size go through `BatchedPipeline` together (one detector pass, one
        embedder schedule, one distance GEMM).  Per-image results are the ones `evaluate` gets: neither the detector's nor the
        embedder's result for an image depends on what it is batched with (tests/test_gpu_harness.py), images of different
        sizes are never mixed in a batch (the padded batch shape enters the anchors, like in torchvision), and the zero-area
        boxes `generate_proposals_and_images` drops are dropped here too."""
        pg = self.proposal_generator
        pipe = self._pipeline()
        out = [None] * len(images)
        for idxs in self._size_groups(images):
            res = pipe.run([ops.input_image(images[i], pg.device) for i in idxs])
            boxes, indices = res['boxes'].cpu(), res['indices'][:, :, 0].cpu()
            for j, i in enumerate(idxs):
                c = res['counts_host'][j]
                b, ix = boxes[j, :c], indices[j, :c]
                if c:
                    ok = _nondegenerate(b)
                    b, ix = b[ok], ix[ok]
                out[i] = (b, [self.classifier.annotations[k] for k in ix.tolist()])
        return out

    def _pipeline(self):
        pg = self.proposal_generator
        pipe = self.__dict__.get('_pipe')
        if pipe is None or pipe.detector is not pg.detector or pipe.classifier is not self.classifier:
            pipe = self._pipe = BatchedPipeline(pg.detector, self.classifier, pg.condfidence_threshold)
        pipe.confidence_threshold = pg.condfidence_threshold
        return pipe

    @staticmethod
    def _size_groups(images):
        """the indices of the images of each size, in order of first appearance (images of different sizes never share a batch)"""
        groups = {}
        for i, img in enumerate(images):
            groups.setdefault(datautils.image_hw(ops.check_image_form(img)), []).append(i)
        return list(groups.values())

    def _on_device(self):
        """Whether this window's detections stay on the device: the switch, and a classifier with an id space to label them in."""
        if not self.device_detections:
            return False
        if getattr(self.classifier, 'label_ids', None) is None:
            self.detections_host_routed += 1
            return False
        return True

    def _evaluate_on_device(self, images, planograms, report=False):
        """A window with `device_detections`: `run(actuals=True)` per size group, the packs joined on the device, ONE `compare_batch`
        on them (in group order; the verdicts go back to the images' order)."""
        return self._device_window(images, planograms, report)[0]

    def _device_window(self, images, planograms, report, steps=False):
        """`_evaluate_on_device`'s window -> (the verdicts in the images' order, per image the (boxes, gallery rows) of its detections
        as views of the window's device pack: what the pictures are made of, never copied to the host).  steps: the verdicts are
        `PlanogramComparator.steps_batch`'s pairs."""
        from . import planograms_device as pd
        pg, cmp = self.proposal_generator, self.planogram_comparator
        pipe = self._pipeline()
        pipe.actuals_thresh_size = cmp.graph_threshold
        planograms = list(planograms)
        if not images:
            return [], []
        order, packs = [], []
        for idxs in self._size_groups(images):
            packs.append(pipe.run([ops.input_image(images[i], pg.device) for i in idxs], actuals=True)['actuals'])
            order += idxs
        pack = pd.DeviceActuals.concat(packs)
        compare = cmp.steps_batch if steps else cmp.report_batch if report else cmp.compare_batch
        verdicts = compare([planograms[i] for i in order], pack, [images[i] for i in order], self.classifier)
        out, dets, at = [None] * len(images), [None] * len(images), 0
        for i, v, n in zip(order, verdicts, pack.n2):
            out[i], dets[i] = v, (pack.boxes[at:at + n], pack.row[at:at + n])
            at += n
        return out, dets

    def evaluate_batch(self, images, planograms):
        """[evaluate(image, planogram) for image, planogram in zip(...)] with the detect / crop / embed / match half batched
        (`detect_and_classify_batch`); the comparator (CPU graph matching, RANSAC, re-classification of missing positions) runs
        per image as in production.py:123-129.  With `device_detections` the detections go from the matcher to the comparator's
        kernels on the device (`_evaluate_on_device`)."""
        return self._evaluate_batch(images, planograms, False)

    def _evaluate_batch(self, images, planograms, report):
        images = [self._float_image(img) for img in images]
        if self._on_device():
            return self._evaluate_on_device(images, planograms, report)
        dets = self.detect_and_classify_batch(images)
        return self._compare_all(images, planograms, dets, report)

    def _compare_all(self, images, planograms, dets, report=False, steps=False):
        """The comparator over a window: per image, or -- a comparator with `device_graphs` on -- its `compare_batch` (report on:
        `report` and `report_batch`; steps on: `steps` and `steps_batch`)."""
        cmp = self.planogram_comparator
        actuals = [{'boxes': b, 'labels': labels} for b, labels in dets]
        if getattr(cmp, 'device_graphs', False) and hasattr(cmp, 'compare_batch'):
            batch = cmp.steps_batch if steps else cmp.report_batch if report else cmp.compare_batch
            return batch(list(planograms), actuals, list(images), self.classifier)
        one = cmp.steps if steps else cmp.report if report else cmp.compare
        return [one(plano, actual, img, self.classifier) for img, plano, actual in zip(images, planograms, actuals)]


    def evaluate_iter(self, pairs, lookahead=4):
        """`evaluate(image, planogram)` over an ITERABLE of (image, planogram) pairs, yielding the results in order -- the per-image
        calling pattern of production.py:118-129 (one shelf photo at a time, e.g. a camera feed or a dataset loop) without its cost:
        a single image is a 1.9 ms latency chain through the detector and 200 crops do not fill the embedder's passes (171 images/s
        against 275 batched).  The iterator reads up to `lookahead` pairs ahead and sends consecutive images of one size through
        `detect_and_classify_batch` together; the comparator runs per image as before.  Every yielded value equals what
        `evaluate(image, planogram)` returns for that pair (tests/test_gpu_harness.py): an image's detections and labels do not depend
        on what it is batched with.  lookahead = 1 is the serial loop.  `pairs` may be a `feeding.ImageFeeder` over such pairs: its
        device-resident 8-bit images are converted where they are, never copied again."""
        return self._evaluate_iter(pairs, lookahead, False)

    def _evaluate_iter(self, pairs, lookahead, report):
        window = []

        def flush():
            if self._on_device():
                yield from self._evaluate_on_device([img for img, _ in window], [plano for _, plano in window], report)
                window.clear()
                return
            dets = self.detect_and_classify_batch([img for img, _ in window])
            if getattr(self.planogram_comparator, 'device_graphs', False):
                yield from self._compare_all([img for img, _ in window], [plano for _, plano in window], dets, report)
            else:
                one = self.planogram_comparator.report if report else self.planogram_comparator.compare
                for (img, plano), (b, labels) in zip(window, dets):
                    yield one(plano, {'boxes': b, 'labels': labels}, img, self.classifier)
            window.clear()

        for image, planogram in pairs:
            image = self._float_image(image)
            if window and (len(window) >= max(1, lookahead) or datautils.image_hw(image) != datautils.image_hw(window[0][0])):
                yield from flush()
            window.append((image, planogram))
        if window:
            yield from flush()


CROP_CONTENT_ONLY = os.environ.get('CVPCE_CROP_CONTENT', '1') != '0'   # A/B switch: the crop kernel leaves the constant padding unwritten for the work-list embedder


def roi_crops(encoder, device, images, boxes, count, content_only=True):
    """The embedder's input for the first count[i] of the boxes[i] of every image, launched WITHOUT knowing the counts on the host --
    what `BatchedPipeline._crops` does for the detector's confident boxes and `planograms_device.reclassify_batch` for a window's
    positions to re-classify.  images: device images (either form); an entry may be None: nothing is launched for it and its slots
    stay unwritten (the caller knows its count to be 0).  boxes (n,per,4) f32 and count (n,) int32 on `device`.
    -> (crops (n * per,S,S,4|8) bf16, their content extents | None, the encoder's all-padding crop | None, partial), as `_crops`
    documents them."""
    emb_eng = encoder.engine()
    n, dpi = boxes.shape[0], boxes.shape[1]
    size = datautils.CLASSIFICATION_IMAGE_SIZE
    # the fused VGG stem reads 4- or 8-channel pixels: 8-byte pixels halve what the crop kernel writes and the stem re-reads
    narrow = getattr(emb_eng, 'stem', None) is not None
    mean, std = getattr(encoder, 'input_mean', TANH_MEAN), getattr(encoder, 'input_std', TANH_STD)
    crops = torch.empty((n * dpi, size, size, 4 if narrow else 8), dtype=torch.bfloat16, device=device)
    # content extents of the crops (the part of a crop beyond them is the pad constant of datautils.py:232-239: the embedder
    # skips the tiles that lie in it) -- only for an encoder whose engine has the work-list schedule
    skip = hasattr(emb_eng, 'skip_plan') and emb_eng.skip_plan(size) is not None
    ext = torch.empty((n * dpi, 2), dtype=torch.int32, device=device) if skip else None
    hw = [None if img is None else datautils.image_hw(img) for img in images]    # (either form)
    same_size = all(s is not None and s == hw[0] for s in hw)
    partial = bool(content_only and skip and CROP_CONTENT_ONLY and emb_eng.will_skip(size))
    if skip and same_size:                   # (images of one size: the extents of the whole batch in one launch)
        ops.crop_extents(boxes.reshape(n * dpi, 4), count, hw[0][0], hw[0][1], size, out=ext, per_image=dpi)
    for i, img in enumerate(images):
        if img is None:
            continue
        if skip and not same_size:
            ops.crop_extents(boxes[i], count[i:i + 1], hw[i][0], hw[i][1], size, out=ext[i * dpi:(i + 1) * dpi])
        ops.crop_resize(img, boxes[i], size, mode=2 if narrow else 1, mean=mean, std=std, count=count[i:i + 1],
                        out=crops[i * dpi:(i + 1) * dpi], content_ext=ext[i * dpi:(i + 1) * dpi] if partial else None)
    return crops, ext, (emb_eng.const_crop(mean, std, crops.shape[3], size) if skip else None), partial


class BatchedPipeline:
    """detect -> RoI crop -> embed -> match for a batch of shelf images, device-resident end to end.

    Same arithmetic as ProposalGenerator.generate_proposals_and_images + Classifier.classify per image
    (production.py:13-20,57-74) but: one detector pass for the whole batch, the crop kernel reads the
    kept boxes and the confidence-prefix count straight from device memory and writes normalised
    NHWC bf16 embedder input (no f32 crop tensor, no host round trip), one distance GEMM per batch.
    """

    def __init__(self, detector, classifier, confidence_threshold=0.5):
        self.detector = detector
        self.classifier = classifier
        self.confidence_threshold = confidence_threshold

    def _crops(self, images, det_out, content_only=True):
        """RoI crops of every image's confident boxes, launched WITHOUT knowing the counts on the host: the crop kernel reads
        the boxes and the confidence-prefix count from device memory and skips the slots beyond it.
        -> (crops, their content extents | None, the encoder's all-padding crop | None, partial).
        partial (content_only and an encoder that runs the work-list schedule): only the crops' content was written -- the constant
        padding beyond the extents is never read by that schedule (it reads the constant crop instead), so it is not produced either;
        `embed_packed(..., partial=True)` refuses to run any other schedule on such crops."""
        boxes, scores, labels, count, conf_count, gauss = det_out
        return roi_crops(self.classifier.encoder, self.detector.engine().device, images, boxes, conf_count, content_only)

    def _select(self, crops, counts, ext=None):
        """The embedder only runs over the valid crops (compaction = a gather of row indices; their extents go along)."""
        n, dpi = len(counts), self.detector.detections_per_img
        eng = self.detector.engine()
        if sum(counts) == n * dpi:
            valid, sel = crops, None
        else:
            sel = torch.cat([torch.arange(i * dpi, i * dpi + c, device=eng.device) for i, c in enumerate(counts)])
            valid = crops.index_select(0, sel)
            if ext is not None:
                ext = ext.index_select(0, sel)
        return valid, sel, ext

    def _crop_embed_match(self, images, det_out, counts, embed_batch=None):
        """(kept for the dev tools) crops + selection with counts already on the host."""
        crops, ext, const_in, _ = self._crops(images, det_out, content_only=False)     # (whole crops: the tools embed them without lists too)
        valid, sel, ext = self._select(crops, counts, ext)
        return crops, valid, sel

    def _finish(self, images, det_out, counts, emb, idx, sel):
        boxes, scores, labels, count, conf_count, gauss = det_out
        n, dpi = len(images), self.detector.detections_per_img
        k = idx.shape[1] if idx.numel() else self.classifier.k
        indices = torch.full((n * dpi, k), -1, dtype=torch.int64, device=boxes.device)
        if sel is None:
            indices = idx
        elif idx.numel():
            indices.index_copy_(0, sel, idx)
        return {'boxes': boxes, 'scores': scores, 'labels': labels, 'count': conf_count, 'det_count': count,
                'indices': indices.view(n, dpi, k), 'gaussians': gauss, 'embeddings': emb, 'counts_host': counts}

    @torch.no_grad()
    def run(self, images, stage_events=None, proposals=None, actuals=False):
        """images: list of (3,H,W) f32 cuda tensors (or 8-bit (H,W,3) images: `ops.input_image`) -> dict of device tensors:
        boxes (N,dpi,4), scores (N,dpi), count (N,) = #scores > confidence, indices (N,dpi,k) (-1 beyond count).
        stage_events: optional list that receives (stage name, start event, end event) for detect / crop / embed / match.
        proposals: optional (boxes (N,dpi,4) f32, counts (N,) int32) device tensors that REPLACE the detector's confident boxes after
        the detector has run (stage-isolated benchmarks accept planted proposals, which pins P and the box shapes
        whatever the detector's weights emit); the detector's pass is still executed and timed.
        actuals (opt-in; the detections rule of DESIGN.md 4b): the dict gains 'actuals', a `planograms_device.DeviceActuals` -- the
        confident, non-degenerate boxes of every image with their label ids and graph thresholds (`actuals_thresh_size`), packed on the
        device for the comparator: two more launches (csrc/actuals.hip), no further wait.  Off, the call launches what it always did.
        (Queueing the detector of call i + 1 on its own stream beside the embedder of call i was measured: +1.3 % at best, and
        the two stages' queues do not actually make progress side by side on this stack -- profiles/r03_rejected_experiments.md.)"""
        def mark():
            if stage_events is None:
                return None
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            return e

        det = self.detector
        if any(ops.is_uint8_image(i) for i in images):
            for i in images:
                ops.check_image_form(i)
            device = det.engine().device
            images = [ops.input_image(i, device) if ops.is_uint8_image(i) else i for i in images]
        t0 = mark()
        if ops.PROFILE is not None:
            ops.PROFILE.records.stage = 'detect'           # (per-launch profile: the detector's 3x3 halo launches are filed apart)
        det_out = det.engine().detect(images, det.num_classes, det.detections_per_img, self.confidence_threshold)
        if ops.PROFILE is not None:
            ops.PROFILE.records.stage = 'embed'
        if proposals is not None:
            pb, pc = proposals
            assert pb.shape == det_out[0].shape and pb.dtype == torch.float32 and pc.dtype == torch.int32 and pc.shape == det_out[4].shape
            det_out = (pb, det_out[1], det_out[2], det_out[3], pc, det_out[5])
        t1 = mark()
        # The one host synchronisation of a step -- the confidence-prefix counts, which size the embedder's batch -- is
        # taken BESIDE the crop kernels, not before them: the counts go to pinned host memory right behind the detector,
        # the crops (which read the counts on the device) are launched behind that copy, and the host wakes up as soon as
        # the copy has landed, i.e. while the crops still run, and queues the embedder's launches behind them.
        n = len(images)
        pin = self.__dict__.setdefault('_count_pins', {})
        if actuals:
            # the kept counts -- how many of each image's confident boxes are non-degenerate -- are counted right behind the detector
            # and travel in the same pinned copy as the confidence counts: still one wait
            if getattr(self.classifier, 'gallery_label_id', None) is None:
                raise ValueError('actuals=True needs a classifier with an id space (Classifier.label_ids)')
            from . import torch_ops_actuals  # noqa: F401  (registers torch.ops.cvpce_amd.actuals_*)
            det_boxes = det_out[0].contiguous()
            both = torch.empty(2 * n, dtype=torch.int32, device=det_boxes.device)
            both[:n].copy_(det_out[4])
            torch.ops.cvpce_amd.actuals_count(det_boxes, both[:n], both[n:])
            if ('actuals', n) not in pin:
                pin['actuals', n] = torch.empty(2 * n, dtype=torch.int32).pin_memory()
            pinned = pin['actuals', n]
            pinned.copy_(both, non_blocking=True)
        else:
            if n not in pin:
                pin[n] = torch.empty(n, dtype=torch.int32).pin_memory()
            pinned = pin[n]
            pinned.copy_(det_out[4], non_blocking=True)
        copied = torch.cuda.Event()
        copied.record()
        crops, ext, const_in, partial = self._crops(images, det_out)
        copied.synchronize()
        counts = pinned.tolist()
        counts, kept = counts[:n], counts[n:]
        valid, sel, ext = self._select(crops, counts, ext)
        t2 = mark()
        if ext is not None:         # (an encoder with the work-list schedule: the tiles in the crops' constant padding are skipped)
            emb = self.classifier.encoder.engine().embed_packed(valid, ext=ext, const_in=const_in, partial=partial)
        else:
            emb = self.classifier.encoder.engine().embed_packed(valid)
        t3 = mark()
        idx = self.classifier.match(emb)
        t4 = mark()
        if stage_events is not None:
            stage_events += [('detect', t0, t1), ('crop', t1, t2), ('embed', t2, t3), ('match', t3, t4)]
        res = self._finish(images, det_out, counts, emb, idx, sel)
        if actuals:
            res['actuals'] = self._pack_actuals(det_boxes, both[:n], res['indices'], kept)
        return res

    actuals_thresh_size = 0.5          # the comparator's graph_threshold the packed thresholds are computed for

    def _pack_actuals(self, boxes, count, indices, kept):
        """`actuals_pack` behind the matcher: the kept boxes, their gallery rows, label ids and graph thresholds, packed on the device
        with the host's prefix sums of the kept counts -> `planograms_device.DeviceActuals`.  Nothing is waited for."""
        from . import planograms_device as pd
        device, total = boxes.device, sum(kept)
        off2 = upload(torch.tensor(offsets(kept), dtype=torch.int32), device)
        out_boxes = torch.empty((total, 4), dtype=torch.float32, device=device)
        small = torch.empty(2 * total + 2 * len(kept), dtype=torch.int32, device=device)
        row, label, status = small[:total], small[total:2 * total], small[2 * total + len(kept):]
        thresh = small[2 * total:2 * total + len(kept)].view(torch.float32)
        torch.ops.cvpce_amd.actuals_pack(boxes, count, indices.contiguous(), self.classifier.gallery_label_id, off2, float(self.actuals_thresh_size),
                                         out_boxes, row, label, thresh, status)
        return pd.DeviceActuals(out_boxes, row, label, thresh, status, off2, kept, self.actuals_thresh_size)
