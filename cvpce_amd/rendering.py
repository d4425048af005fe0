"""Compliance pictures on the device: the rebuilt scene and the annotated shelf of the reference's `rebuild-scene`,
`plot-planogram-eval` and `misc pipeline-demo` (cvpce/utils.py:205-228 `build_rebuild`; cvpce/cli/eval.py:73-108), composed by one
launch of csrc/render.hip by the picture rule of DESIGN.md 4b instead of one matplotlib `imshow` per product in a blocking window.

  * `ThumbnailAtlas`    the gallery's product images on the device, row r = gallery row r: the matcher's indices are atlas rows;
  * `observed_items`, `expected_items`, `annotation_items`    the item lists of the three pictures, pure tensor code that runs where
                        its inputs live;
  * `SceneRenderer`     any number of canvases in one launch and no wait;
  * `CompliancePictures`    the three pictures of a shelf image, `.save(prefix)` writes them as PNG (a host copy and a host encode).

The step pictures of `plot-planogram-eval` and `misc pipeline-demo` (cvpce/utils.py:181-189 `draw_planograph`: `nx.draw` at the box
centres) add straight strokes over those canvases, drawn in place by one launch of csrc/strokes.hip by the stroke rule of DESIGN.md 4b:

  * `Strokes`, `graph_strokes`, `matched_strokes`    the stroke lists of a neighbour graph and of the subgraph its matched nodes induce,
                        pure tensor code that runs where the graph's table lives; every size is known to the host;
  * `SceneRenderer.render(..., strokes=...)`    the second launch, over the same flat buffer;
  * `StepPictures`      the nine pictures of a shelf image, the last three `CompliancePictures`' own.
"""
import types

import torch

from . import torch_ops_render as R
from . import torch_ops_strokes as S

BLACK = 0x000000
WHITE = 0xFFFFFF


def rgb(r, g, b):
    """an item's colour: R | G<<8 | B<<16"""
    return int(r) | (int(g) << 8) | (int(b) << 16)


# one colour per ComplianceReport.OUTCOMES entry (out-of-view positions are not drawn, the colour names them in a legend) and one for
# the stray detections
OUTCOME_COLOURS = {'detected': rgb(0, 170, 0), 'recovered': rgb(0, 200, 200), 'missing': rgb(230, 0, 0), 'out_of_view': rgb(128, 128, 128),
                   'unchecked': rgb(240, 160, 0)}
STRAY_COLOUR = rgb(200, 0, 200)
OUT_OF_VIEW = 3                    # the code of 'out_of_view' in ComplianceReport.outcomes
ANNOTATION_THICKNESS = 3           # the rings of the annotated picture, in pixels
ATLAS_MAX_BYTES = 2 ** 31 - 1      # the atlas rows' offsets are int32
# the step pictures: the rings of the `detections` and `positions` pictures, and the graph drawings in networkx's default colours
# (black edges under blue nodes).  A stroke's radius is in HALF pixels: a stroke of radius t is t pixels thick.
DETECTION_COLOUR = rgb(255, 0, 0)
POSITION_COLOUR = rgb(0, 0, 255)
GRAPH_EDGE_COLOUR = BLACK
GRAPH_NODE_COLOUR = rgb(31, 120, 180)
GRAPH_EDGE_RADIUS = 2              # a 2-pixel line
GRAPH_NODE_RADIUS = 10             # a disc 10 pixels across


class Items:
    """An item list of the picture rule: `box` (n, 4) float32 x1 y1 x2 y2 in canvas pixels, `src`, `colour`, `thickness` (n,) int32,
    all on one device."""
    __slots__ = ('box', 'src', 'colour', 'thickness')

    def __init__(self, box, src, colour, thickness):
        self.box, self.src, self.colour, self.thickness = box, src, colour, thickness

    def __len__(self):
        return int(self.src.numel())

    def to(self, device):
        return Items(*(getattr(self, n).to(device) for n in self.__slots__))

    @staticmethod
    def cat(lists):
        lists = list(lists)
        return Items(*(torch.cat([getattr(l, n) for l in lists]) for n in Items.__slots__))


def _items(box, src, colour, thickness):
    """box (n, 4) any float; src, colour, thickness: (n,) tensors or Python integers -> Items on the boxes' device"""
    box = box.to(torch.float32).reshape(-1, 4).contiguous()
    n, dev = box.shape[0], box.device
    col = lambda v: (v.to(device=dev, dtype=torch.int32) if torch.is_tensor(v) else torch.full((n,), int(v), dtype=torch.int32, device=dev)).contiguous()
    return Items(box, col(src), col(colour), col(thickness))


def observed_items(boxes, rows):
    """The "observed planogram" of the reference's rebuild (utils.py:205-228): one item per detection, in order, the product image of
    gallery row rows[i] pasted into boxes[i].  A detection whose row is -1 (a label the gallery does not have) gets nothing inside and
    a 1-pixel black ring: the reference's empty rectangle.  boxes (n, 4), rows (n,) integers, on any one device."""
    rows = rows.to(device=boxes.device, dtype=torch.int32)
    known = rows >= 0
    return _items(boxes, torch.where(known, rows, torch.full_like(rows, R.SRC_NONE)), BLACK, torch.where(known, torch.zeros_like(rows), torch.ones_like(rows)))


def label_rows(annotations):
    """annotation -> its FIRST gallery row: how the host routes turn a label into an atlas row"""
    rows = {}
    for r, a in enumerate(annotations):
        try:
            rows.setdefault(a, r)
        except TypeError:           # an annotation that cannot be hashed names no row
            pass
    return rows


def rows_of_labels(labels, rows):
    """labels -> (n,) int32 atlas rows by `label_rows`' table, -1 for a label the gallery does not have (or one that cannot be hashed)"""
    def row(l):
        try:
            return rows.get(l, -1)
        except TypeError:
            return -1
    return torch.tensor([row(l) for l in labels], dtype=torch.int32)


def expected_canvas_hw(planogram_boxes, width):
    """The canvas of the expected picture: `width` wide and as high as keeps the planogram's aspect ratio -- ceil(width * eh / ew) with
    ew x eh the planogram's extents, at least 1 (host integers; an empty or flat planogram: width x width)."""
    b = planogram_boxes.detach().cpu().to(torch.float64).reshape(-1, 4)
    width = max(1, int(width))
    if not len(b):
        return width, width
    ew, eh = float(b[:, 2].max() - b[:, 0].min()), float(b[:, 3].max() - b[:, 1].min())
    if not (ew > 0 and eh > 0 and ew < float('inf') and eh < float('inf')):
        return width, width
    return max(1, min(R.MAX_SIDE, -int(-(width * eh) // ew))), width


def expected_items(planogram_boxes, rows, canvas_hw):
    """`observed_items` for the planogram itself: its boxes are mapped into the (H, W) canvas by `(b - origin) * scale`, two separately
    rounded fp32 operations, with origin = (min x1, min y1) of the planogram and scale = min(W / ew, H / eh) of its extents ew x eh (the
    aspect ratio is kept; fp32).  rows: the first gallery row of each expected label, -1 where the gallery has none."""
    return observed_items(expected_boxes_on_canvas(planogram_boxes, canvas_hw), rows)


def expected_boxes_on_canvas(planogram_boxes, canvas_hw):
    """`expected_items`' mapping alone: the planogram's boxes in the pixels of the (H, W) canvas, float32 (n, 4) where the boxes live --
    what the expected picture pastes into and what the expected graph is drawn between."""
    b = planogram_boxes.to(torch.float32).reshape(-1, 4)
    if not b.shape[0]:
        return b
    h, w = canvas_hw
    origin = torch.stack([b[:, 0].min(), b[:, 1].min()])
    ext = torch.stack([b[:, 2].max(), b[:, 3].max()]) - origin
    scale = torch.minimum(torch.tensor(float(w), dtype=torch.float32, device=b.device) / ext[0],
                          torch.tensor(float(h), dtype=torch.float32, device=b.device) / ext[1])
    return (b - origin.repeat(2)) * scale


def annotation_items(report, actual_boxes, thickness=3, canvas_hw=None):
    """The annotated shelf: first the base image over the whole (H, W) canvas, then the stray detections (`STRAY_COLOUR`), then the
    expected positions grouped by outcome in the order of `ComplianceReport.OUTCOMES` (`OUTCOME_COLOURS`; the positions of a group in
    index order; out-of-view positions left out), all as rings of `thickness` with nothing inside.  A report whose status is not 'ok'
    yields the base item alone.  The items live where `actual_boxes` lives."""
    if canvas_hw is None:
        raise ValueError('annotation_items needs the canvas size: the base item covers the whole canvas')
    h, w = canvas_hw
    dev = actual_boxes.device if torch.is_tensor(actual_boxes) else torch.device('cpu')
    base = _items(torch.tensor([[0.0, 0.0, float(w), float(h)]], device=dev), R.SRC_BASE, BLACK, 0)
    if report.status != 'ok':
        return base
    stray = _items(actual_boxes.to(torch.float32).reshape(-1, 4)[report.stray.to(dev)], R.SRC_NONE, STRAY_COLOUR, thickness)
    outcomes = report.outcomes.to(torch.int64)
    order = torch.cat([torch.where(outcomes == code)[0] for code, name in enumerate(report.OUTCOMES) if code != OUT_OF_VIEW])
    colours = torch.tensor([OUTCOME_COLOURS[name] for name in report.OUTCOMES], dtype=torch.int32)[outcomes[order]]
    positions = _items(report.expected_positions[order].to(dev), R.SRC_NONE, colours, thickness)
    return Items.cat([base, stray, positions])


def ring_items(boxes, colour, thickness=3, canvas_hw=None, device=None):
    """The photo with boxes ringed (`utils.show(img, boxes)`): the base image over the whole (H, W) canvas, then every box as a ring of
    `colour` with nothing inside.  boxes None: the base alone.  The items live where the boxes live (`device` where there are none)."""
    h, w = canvas_hw
    dev = boxes.device if torch.is_tensor(boxes) else torch.device('cpu' if device is None else device)
    base = _items(torch.tensor([[0.0, 0.0, float(w), float(h)]], device=dev), R.SRC_BASE, BLACK, 0)
    if boxes is None or not boxes.numel():
        return base
    return Items.cat([base, _items(boxes, R.SRC_NONE, colour, thickness)])


class Strokes:
    """A stroke list of the stroke rule: `ends` (n, 4) float32 ax ay bx by in canvas pixels, `colour`, `radius` (n,) int32 (the radius
    in half pixels, <= 0: the stroke is skipped), all on one device."""
    __slots__ = ('ends', 'colour', 'radius')

    def __init__(self, ends, colour, radius):
        self.ends, self.colour, self.radius = ends, colour, radius

    def __len__(self):
        return int(self.radius.numel())

    def to(self, device):
        return Strokes(*(getattr(self, n).to(device) for n in self.__slots__))

    @staticmethod
    def cat(lists):
        lists = list(lists)
        return Strokes(*(torch.cat([getattr(l, n) for l in lists]) for n in Strokes.__slots__))


def graph_strokes(graph, boxes, keep=None, edge_colour=GRAPH_EDGE_COLOUR, node_colour=GRAPH_NODE_COLOUR, edge_radius=GRAPH_EDGE_RADIUS,
                  node_radius=GRAPH_NODE_RADIUS):
    """The drawing of a neighbour graph over its boxes (`utils.draw_planograph`): one stroke slot per (node, direction slot) of the
    graph's `nbr` [n][8] table, node-major, then one disc -- a stroke of length zero -- per node, so the nodes lie over the edges and
    the list has 9 n strokes whatever the graph holds: the host knows every size and no count is read back.  An empty slot (-1, or a
    neighbour outside the graph) carries radius 0 and zero ends.  A node's position is its box's centre, ((x1 + x2) / 2, (y1 + y2) / 2)
    in fp32.  graph: a `planograms_device.Graph` or its `nbr` table; boxes (n, 4) in canvas pixels -- the expected side's through
    `expected_boxes_on_canvas`.  keep (n,) bool: only these nodes' discs and the edges between two of them (`matched_strokes`).  Pure
    tensor code where the table lives (the boxes are brought there), without a wait."""
    nbr = getattr(graph, 'nbr', graph)
    dev = nbr.device
    b = boxes.to(device=dev, dtype=torch.float32).reshape(-1, 4)
    n = b.shape[0]
    nbr = nbr.to(torch.int64).reshape(-1, 8)
    if nbr.shape[0] != n:
        raise ValueError(f'one box per node: {n} boxes for a graph of {nbr.shape[0]} nodes')
    centre = torch.stack([(b[:, 0] + b[:, 2]) / 2, (b[:, 1] + b[:, 3]) / 2], dim=1)
    filled = (nbr >= 0) & (nbr < n)
    to = nbr.clamp(0, max(n - 1, 0))
    nodes = torch.ones(n, dtype=torch.bool, device=dev) if keep is None else keep.to(device=dev, dtype=torch.bool).reshape(n)
    if keep is not None:
        filled = filled & nodes[:, None] & nodes[to]
    edges = torch.cat([centre[:, None, :].expand(n, 8, 2), centre[to]], dim=2)
    edges = torch.where(filled[:, :, None], edges, torch.zeros_like(edges)).reshape(-1, 4)
    i32 = lambda mask, value: torch.where(mask, int(value), 0).to(torch.int32).reshape(-1)
    ends = torch.cat([edges, centre.repeat(1, 2)]).contiguous()
    colour = torch.cat([torch.full((8 * n,), int(edge_colour), dtype=torch.int32, device=dev),
                        torch.full((n,), int(node_colour), dtype=torch.int32, device=dev)])
    return Strokes(ends, colour, torch.cat([i32(filled, edge_radius), i32(nodes, node_radius)]))


def matched_strokes(graph, boxes, matched, whole=None, **style):
    """`graph_strokes` of the subgraph the matched nodes induce (`ge.subgraph(nodes_e)`, cli/eval.py:335-342): the edges whose two ends
    are matched and the matched nodes' discs, in the same 9 n slots.  matched (n,) bool, on any device
    (`planograms_device.matched_nodes` makes it from a `DeviceMatching` without a wait).
    whole: `graph_strokes(graph, boxes, **style)` where the caller has it -- the list is then that one with the radii of the slots that
    leave the matched set zeroed (the same strokes painted; a slot of radius 0 keeps its ends)."""
    if whole is None:
        return graph_strokes(graph, boxes, keep=matched, **style)
    nbr = getattr(graph, 'nbr', graph).to(torch.int64).reshape(-1, 8)
    n = nbr.shape[0]
    if len(whole) != 9 * n:
        raise ValueError(f'the strokes of another graph: {len(whole)} for {n} nodes')
    nodes = matched.to(device=nbr.device, dtype=torch.bool).reshape(n)
    inside = nodes[:, None] & nodes[nbr.clamp(0, max(n - 1, 0))]          # (an empty slot has radius 0 in `whole` already)
    return Strokes(whole.ends, whole.colour, torch.where(torch.cat([inside.reshape(-1), nodes]), whole.radius, torch.zeros_like(whole.radius)))


def float_image_bytes(planes):
    """float planes (3, H, W) with values in [0, 1] -> uint8 (H, W, 3): floor(clamp(x, 0, 1) * 255 + 0.5), torch float32 operations
    where the planes live (a byte b read as b / 255 comes back as b)."""
    return (planes.to(torch.float32).clamp(0, 1) * 255 + 0.5).floor().to(torch.uint8).permute(1, 2, 0).contiguous()


def gallery_float_bytes(img):
    """a gallery float item (3, S, S) in [-1, 1] -> uint8 (S, S, 3): clamp(floor((x * 0.5 + 0.5) * 255 + 0.5), 0, 255), every operation a
    torch float32 operation rounded on its own"""
    return ((img.to(torch.float32) * 0.5 + 0.5) * 255 + 0.5).floor().clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous()


def reduced_hw(h, w, max_side):
    """The size an h x w product image is kept at: unchanged where max_side is None or max(h, w) <= max_side, else with m = max(h, w)
    (max(1, (h * max_side + m // 2) // m), max(1, (w * max_side + m // 2) // m)): integer arithmetic, the larger side becomes max_side."""
    h, w = int(h), int(w)
    m = max(h, w)
    if max_side is None or m <= max_side:
        return h, w
    return max(1, (h * max_side + m // 2) // m), max(1, (w * max_side + m // 2) // m)


def atlas_layout(hws):
    """[(h, w), ...] -> ([(byte offset, h, w), ...], total bytes) of images laid back to back (production.pack_gallery_bytes' layout);
    ValueError where the atlas would pass 2^31 - 1 bytes: the offsets are int32."""
    rows, off = [], 0
    for h, w in hws:
        rows.append((off, int(h), int(w)))
        off += int(h) * int(w) * 3
    if off > ATLAS_MAX_BYTES:
        raise ValueError(f'an atlas of {off} bytes passes {ATLAS_MAX_BYTES}: its offsets are int32 (reduce the images with max_side)')
    return rows, off


class ThumbnailAtlas:
    """The gallery's product images on the device: `data`, a flat uint8 buffer, and `rows` (G, 3) int32 (byte offset, h, w) -- row r is
    the product image of gallery row r, so the matcher's indices are atlas rows with no lookup.

    The set is read the way `Classifier._gallery_items` reads it (`num_workers` reader threads, in order).  An item's image is a
    gallery byte image, uint8 (h, w, 3), or the float (3, 256, 256) form in [-1, 1], quantised by
    clamp(floor((x * 0.5 + 0.5) * 255 + 0.5), 0, 255) (`gallery_float_bytes`).  float_items='unit': a float item is (3, h, w) of any size
    in [0, 1] instead -- what `datautils.SimpleFolderSet(train=False)` yields -- quantised by floor(clamp(x, 0, 1) * 255 + 0.5)
    (`float_image_bytes`).  annotations: the classifier's, where given the set's must equal them row by row (ValueError).

    max_side: an image whose larger side exceeds it is reduced on the device by the compositor itself, rendered as one item into a
    canvas of `reduced_hw(h, w, max_side)` = (max(1, (h * max_side + m // 2) // m), max(1, (w * max_side + m // 2) // m)), m = max(h, w);
    None keeps the images as read.  Memory: at most 128 * 128 * 3 = 49 KB per product at max_side=128, so at most 157 MB at G = 3 200;
    at most 256 * 256 * 3 = 197 KB per product, 629 MB at G = 3 200, with max_side=None.  An atlas that would pass 2^31 - 1 bytes raises
    ValueError (`atlas_layout`)."""
    PASS = 256          # images reduced per launch

    FLOAT_ITEMS = ('tanh', 'unit')

    def __init__(self, sample_set, annotations=None, device=torch.device('cuda'), num_workers=0, max_side=128, float_items='tanh'):
        from .production import Classifier, is_gallery_bytes
        self.device, self.max_side = torch.device(device), max_side
        if max_side is not None and max_side < 1:
            raise ValueError('max_side is None or at least 1')
        if float_items not in self.FLOAT_ITEMS:
            raise ValueError(f'float_items is one of {self.FLOAT_ITEMS}, got {float_items!r}')
        to_bytes = gallery_float_bytes if float_items == 'tanh' else float_image_bytes
        reader = types.SimpleNamespace(num_workers=num_workers, batch_size=self.PASS)
        chunks, hws, pending = [], [], []

        def flush():
            if pending:
                chunks.append(self._reduce(pending))
                pending.clear()

        for r, item in enumerate(Classifier._gallery_items(reader, sample_set)):
            img = item[0]
            if annotations is not None and (r >= len(annotations) or item[-1] != annotations[r]):
                raise ValueError(f'gallery item {r} is not the classifier\'s row {r}: the atlas rows are the matcher\'s indices')
            if not is_gallery_bytes(img):
                if not (torch.is_tensor(img) and img.is_floating_point() and img.dim() == 3 and img.shape[0] == 3):
                    raise TypeError(f'a gallery item is a uint8 (h,w,3) or a float (3,S,S) image, got {type(img).__name__} {tuple(getattr(img, "shape", ()))}')
                img = to_bytes(img)
            if img.shape[0] < 1 or img.shape[1] < 1:
                raise ValueError(f'gallery item {r} is empty')
            hws.append(reduced_hw(img.shape[0], img.shape[1], max_side))
            atlas_layout(hws)                                   # (fails before the image that passes the limit is uploaded)
            pending.append(img)
            if len(pending) >= self.PASS:
                flush()
        flush()
        if annotations is not None and len(hws) != len(annotations):
            raise ValueError(f'{len(hws)} gallery items for {len(annotations)} annotations')
        rows, total = atlas_layout(hws)
        self.data = torch.cat(chunks) if chunks else torch.empty(0, dtype=torch.uint8, device=self.device)
        assert self.data.numel() == total
        self.rows = torch.tensor(rows, dtype=torch.int32).reshape(-1, 3).to(self.device)
        self.sizes = hws

    def __len__(self):
        return len(self.sizes)

    @property
    def nbytes(self):
        return self.data.numel() + self.rows.numel() * 4

    def image(self, r):
        """row r as a uint8 (h, w, 3) view of the atlas"""
        off, h, w = (int(v) for v in self.rows[r].tolist())
        return self.data[off:off + h * w * 3].view(h, w, 3)

    def _reduce(self, images):
        """one pass: the images' bytes uploaded back to back; where any is larger than max_side, one launch renders each as one item
        into a canvas of its reduced size -> the flat bytes of the pass's atlas rows"""
        raw_rows, _ = atlas_layout([(im.shape[0], im.shape[1]) for im in images])
        raw = torch.cat([im.reshape(-1) for im in images]).to(self.device)
        sizes = [reduced_hw(im.shape[0], im.shape[1], self.max_side) for im in images]
        if all(s == (im.shape[0], im.shape[1]) for s, im in zip(sizes, images)):
            return raw
        raw_atlas = types.SimpleNamespace(data=raw, rows=torch.tensor(raw_rows, dtype=torch.int32).to(self.device))
        lists = [_items(torch.tensor([[0.0, 0.0, float(w), float(h)]]), k, BLACK, 0) for k, (h, w) in enumerate(sizes)]
        return SceneRenderer(raw_atlas, align=1)._launch(lists, sizes, None, BLACK)[0]      # (align 1: the canvases lie back to back)


class SceneRenderer:
    """Canvases from item lists, by one launch of csrc/render.hip.  atlas: a `ThumbnailAtlas` (anything with `.data` and `.rows`)."""

    def __init__(self, atlas, align=4):
        self.atlas = atlas
        self.device = atlas.data.device
        self.align = align          # canvases start at multiples of this many bytes of the flat output (4: dword stores where W * 3 allows)

    def render(self, item_lists, canvas_hws, bases=None, background=WHITE, strokes=None):
        """item_lists[c] (`Items`, on any device) painted into a canvas of canvas_hws[c] = (H, W), over `background` -> a list of device
        uint8 (H, W, 3) views of ONE flat buffer.  One launch, no wait: the host knows every size.  bases[c]: the base image `src = -2`
        names, or None.  A byte image (H, W, 3) is used where it lies when all bases of the call are views of one allocation (else
        their bytes are joined by one copy); float planes (3, H, W) become bytes first by floor(clamp(x, 0, 1) * 255 + 0.5)
        (`float_image_bytes`, torch operations on the device).
        strokes[c] (`Strokes`, on any device, or None): drawn over canvas c by a second launch on the same flat buffer
        (csrc/strokes.hip), again without a wait; None, or no stroke in any list: exactly the call above."""
        out, table = self._launch(item_lists, canvas_hws, bases, background)
        if strokes is not None:
            self._draw(out, table, strokes)
        return [out[row[1]:row[1] + row[2] * row[3] * 3].view(row[2], row[3], 3) for row in table]

    def _draw(self, out, table, strokes):
        """the stroke launch over the canvases of `table` that have strokes: only their tiles are in its grid"""
        if len(strokes) != len(table):
            raise ValueError('one stroke list or None per canvas')
        rows, lists, tile, k = [], [], 0, 0
        for row, s in zip(table, strokes):
            if s is not None and len(s):
                rows.append((tile, row[1], row[2], row[3], k, k + len(s)))
                lists.append(s if s.radius.device == self.device else s.to(self.device))
                tile, k = tile + S.tiles(row[2], row[3]), k + len(s)
        if not rows:
            return
        every = Strokes.cat(lists)
        canvases = torch.tensor(rows, dtype=torch.int64).to(self.device, non_blocking=True)
        self.last_strokes = (canvases, tile, every.ends, every.colour, every.radius)   # (the op's inputs: tools/bench_step_pictures.py times the launch alone)
        torch.ops.cvpce_amd.strokes_draw(*self.last_strokes, out)

    def _launch(self, item_lists, canvas_hws, bases, background):
        """-> (the flat output, the canvas table as host rows)"""
        n = len(item_lists)
        if len(canvas_hws) != n or (bases is not None and len(bases) != n):
            raise ValueError('one size, and one base or None, per item list')
        dev = self.device
        base_buf, base_rows = self._bases(bases, n)
        table, tile, off, k = [], 0, 0, 0
        for c, (items, (h, w)) in enumerate(zip(item_lists, canvas_hws)):
            h, w = int(h), int(w)
            if not (1 <= h <= R.MAX_SIDE and 1 <= w <= R.MAX_SIDE):
                raise ValueError(f'a canvas is 1 ... {R.MAX_SIDE} pixels a side, got {h} x {w}')
            off = -(-off // self.align) * self.align
            table.append((tile, off, h, w) + base_rows[c] + (k, k + len(items), 0))
            tile, off, k = tile + R.tiles(h, w), off + h * w * 3, k + len(items)
        out = torch.empty(off, dtype=torch.uint8, device=dev)
        if not n:
            return out, table
        items = Items.cat([l if l.src.device == dev else l.to(dev) for l in item_lists])
        canvases = torch.tensor(table, dtype=torch.int64).to(dev, non_blocking=True)
        self.last_launch = (canvases, tile, base_buf, items.box, items.src, items.colour, items.thickness, self.atlas.data, self.atlas.rows,
                            int(background))                   # (the op's inputs: tools/bench_scene_render.py times the launch alone with them)
        torch.ops.cvpce_amd.render_canvases(*self.last_launch, out)
        return out, table

    def _bases(self, bases, n):
        """-> (the flat base buffer or None, per canvas (byte offset or -1, h, w))"""
        none = (-1, 0, 0)
        if bases is None or all(b is None for b in bases):
            return None, [none] * n
        imgs = []
        for b in bases:
            if b is None:
                imgs.append(None)
                continue
            if b.dtype != torch.uint8:
                b = float_image_bytes(b.to(self.device))
            if b.dim() != 3 or b.shape[2] != 3:
                raise TypeError(f'a base image is uint8 (H,W,3) or float (3,H,W), got {tuple(b.shape)}')
            imgs.append(b.to(self.device).contiguous())
        have = [b for b in imgs if b is not None]
        store = have[0].untyped_storage()
        if all(b.untyped_storage().data_ptr() == store.data_ptr() for b in have):
            buf = torch.empty(0, dtype=torch.uint8, device=self.device).set_(store)        # the allocation itself, as flat bytes
            offs = [b.data_ptr() - store.data_ptr() for b in have]
        else:
            buf = torch.cat([b.reshape(-1) for b in have])
            offs, at = [], 0
            for b in have:
                offs.append(at)
                at += b.numel()
        it = iter(offs)
        return buf, [none if b is None else (next(it), int(b.shape[0]), int(b.shape[1])) for b in imgs]


class CompliancePictures:
    """The three pictures of one shelf image, device uint8 (H, W, 3): `annotated` (the photo with the report drawn on it), `observed`
    (every detection's product image where it was detected) and `expected` (the planogram rebuilt the same way)."""
    NAMES = ('annotated', 'observed', 'expected')

    def __init__(self, annotated, observed, expected):
        self.annotated, self.observed, self.expected = annotated, observed, expected

    def save(self, prefix):
        """writes <prefix>_annotated.png, <prefix>_observed.png and <prefix>_expected.png with PIL: a blocking copy to the host and a
        host encode per picture, by far the dearest step of a picture -> the three paths"""
        from PIL import Image
        paths = []
        for name in self.NAMES:
            path = f'{prefix}_{name}.png'
            Image.fromarray(getattr(self, name).cpu().numpy(), 'RGB').save(path)
            paths.append(path)
        return paths


class StepPictures(CompliancePictures):
    """The comparison of one shelf image step by step, device uint8 (H, W, 3), in the order `plot-planogram-eval` and
    `misc pipeline-demo` show them: `detections` (the photo with every detection ringed), `positions` (the photo with every projected
    expected position ringed: `utils.show(img, expected_positions)`), `expected_graph` and `observed_graph` (the rebuilt planograms with
    their neighbour graphs drawn over them), `expected_matched` and `observed_matched` (the same with the common subgraph the matcher
    found), then `CompliancePictures`' three, byte for byte.  An image without a matching has no strokes on its graph pictures, and one
    without a homography no rings on `positions`."""
    NAMES = ('detections', 'positions', 'expected_graph', 'observed_graph', 'expected_matched', 'observed_matched') + CompliancePictures.NAMES

    def __init__(self, *pictures):
        if len(pictures) != len(self.NAMES):
            raise ValueError(f'{len(self.NAMES)} pictures: {", ".join(self.NAMES)}')
        for name, picture in zip(self.NAMES, pictures):
            setattr(self, name, picture)
