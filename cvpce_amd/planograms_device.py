"""The comparator's two graph stages on the device -- the opt-in counterpart of `planograms.build_graph` and
`planograms.large_common_subgraph` (which stay as they are: host logic over networkx).

  build_graphs       8-direction nearest-neighbour graphs of a batch of box sets: one launch (csrc/planogram.hip)
  common_subgraphs   hypothesis-seeded common subgraph of a batch of (expected, actual) graph pairs: one launch, one copy back;
                     matcher='tonioni': `planograms.tonioni_mcs` instead (csrc/tonioni.hip, the Tonioni rule of DESIGN.md 4b), three
                     launches, the same copy back
  match_on_device    the same launch without the copy back: the matchings stay on the device for `finalize_batch`
  finalize_batch     RANSAC homography, refit, projection and per-label claim of a batch (csrc/homography.hip): two launches, one
                     copy back -- the opt-in counterpart of `planograms.finalize_via_ransac` (the tail rule of DESIGN.md 4b)
  reclassify_batch   the re-classification of a window's expected-but-undetected positions (csrc/reclass.hip at both ends of one crop /
                     embed / match pass): one more wait -- the opt-in counterpart of the per-image loop of `PlanogramComparator._finish`
  finalize_result    a record of `finalize_batch` as the tuple `finalize_via_ransac` returns
  to_networkx        a device graph as the DiGraph the host functions expect (node order 0..n-1, adjacency in stamp order)
  nbr_table, matched_of_pairs, matched_nodes    what the step pictures draw: a host graph's neighbour table, and the matched nodes of a
                     host matching and of a `DeviceMatching` (the latter on the device, without a wait)
  prepare            caches a planogram's device graph in its dict, as `expected['graph']` caches the host graph
  DeviceActuals      a window's detections as `BatchedPipeline.run(actuals=True)` left them on the device (csrc/actuals.hip): the actual
                     side of `build_graphs`, `match_on_device` and `finalize_batch` without a copy to the host (the detections rule of
                     DESIGN.md 4b)

A graph is three [n][8] tables -- per node and direction slot (planograms.CARDINALS) the neighbour, the edge weight and an insertion
stamp -- plus the labels.  networkx's adjacency order is edge insertion order and decides the order in which the common subgraph
grows; the stamps carry it: a node's adjacency is its filled slots by ascending stamp.

The device rule.  `build_graph` takes its distances from `torch.cdist`, which for more than 25 points goes through a
matrix product and is neither exact nor reproducible, and orders each row with torch's default sort, whose order at equal distances
is unspecified.  The device uses d = sqrt(dx*dx + dy*dy) in fp32, every operation rounded on its own, walks each row in ascending
(d, j) -- lower index first at equal distance -- skips pairs at d = 0, and takes the threshold from the caller, who computes it with
`build_graph`'s own expression.  Everything else is `build_graph`'s greedy.  Where the host's distances are exact and its rows
tie-free, the device graph is the host graph.

Graphs of more than MAX_NODES nodes are refused here, and so is, with matcher='tonioni', a pair of more than
TONIONI_MAX_HYPOTHESES hypotheses; the comparator sends such an image through the host path.
"""
from collections import Counter, namedtuple
from types import SimpleNamespace

import networkx as nx
import torch

from . import torch_ops_homography, torch_ops_planogram, torch_ops_tonioni  # noqa: F401  (register torch.ops.cvpce_amd.planogram_* / homography_* / tonioni_*)
from .planograms import CARDINALS
from . import staging
from .torch_ops_planogram import MAX_NODES
from .torch_ops_tonioni import MAX_HYPOTHESES as TONIONI_MAX_HYPOTHESES       # the most hypotheses of a pair the Tonioni matcher takes

CACHE_KEY = 'device_graph'
BOXES_KEY = 'device_boxes'        # a planogram dict's boxes on the device (`expected_boxes_on_device`)
IDS_KEY = 'device_label_ids'      # a planogram dict's expected labels in the classifier's id space (`expected_label_ids`)
RANSAC_HYPOTHESES = 2048          # per image, all evaluated (the host's adaptive loop stops at 2000 at the latest)
STATUS = ('ok', 'none', 'invalid')


class Graph:
    """One graph in table form: `labels` (list, one per node) and the [n][8] tensors `nbr` (int32, -1 = empty), `weight` (float32)
    and `stamp` (int32), on any device.  `_parent`: (packed nbr, weight, stamp of the launch that built it, first row) or None."""
    __slots__ = ('labels', 'nbr', 'weight', 'stamp', '_parent')

    def __init__(self, labels, nbr, weight, stamp, parent=None):
        self.labels, self.nbr, self.weight, self.stamp, self._parent = list(labels), nbr, weight, stamp, parent

    def __len__(self):
        return len(self.labels)


class DeviceActuals:
    """The detections of a window where `actuals_pack` left them.  On the device: `boxes` [sum2][4] f32 -- every image's kept
    (non-degenerate, confident) boxes back to back in slot order --, `row` and `label` [sum2] int32 (each box's nearest gallery row and
    that row's id in the classifier's id space), `thresh` [B] f32 (`graph_threshold` of each image's kept boxes; unwritten for an
    image that keeps nothing), `status` [B] int32 (0, or what `actuals_pack` found wrong) and `off2` [B+1] int32, the row offsets.
    On the host: `n2`, the list of the images' box counts, and `thresh_size`, the fraction the thresholds were computed with."""
    __slots__ = ('boxes', 'row', 'label', 'thresh', 'status', 'off2', 'n2', 'thresh_size')

    def __init__(self, boxes, row, label, thresh, status, off2, n2, thresh_size):
        self.boxes, self.row, self.label, self.thresh, self.status, self.off2 = boxes, row, label, thresh, status, off2
        self.n2, self.thresh_size = list(n2), thresh_size

    def __len__(self):
        return len(self.n2)

    def to_host(self, i, annotations):
        """-> (boxes (n, 4) on the host, the n label strings) of image i: what `detect_and_classify_batch` hands to the comparator.
        (Two blocking copies: for an image that takes the host path.)"""
        o = sum(self.n2[:i])
        rows = self.row[o:o + self.n2[i]].cpu().tolist()
        return self.boxes[o:o + self.n2[i]].cpu(), [annotations[r] for r in rows]

    def select(self, images):
        """-> the pack of the images `images` (ascending indices), gathered on the device; all of them: the pack itself"""
        images = list(images)
        if images == list(range(len(self.n2))):
            return self
        off = staging.offsets(self.n2)
        return self.concat([DeviceActuals(self.boxes[off[i]:off[i + 1]], self.row[off[i]:off[i + 1]], self.label[off[i]:off[i + 1]],
                                          self.thresh[i:i + 1], self.status[i:i + 1], None, [self.n2[i]], self.thresh_size) for i in images])

    @staticmethod
    def concat(packs):
        """The packs of several size groups (or images) as one, joined on the device; only the new offsets are uploaded."""
        packs = list(packs)
        if len(packs) == 1 and packs[0].off2 is not None:
            return packs[0]
        if not packs or any(p.thresh_size != packs[0].thresh_size for p in packs):
            raise ValueError('at least one pack, all made with one thresh_size')
        n2 = [n for p in packs for n in p.n2]
        cat = lambda name: torch.cat([getattr(p, name) for p in packs])
        off2 = staging.upload(torch.tensor(staging.offsets(n2), dtype=torch.int32), packs[0].boxes.device)
        return DeviceActuals(cat('boxes'), cat('row'), cat('label'), cat('thresh'), cat('status'), off2, n2, packs[0].thresh_size)


def graph_threshold(boxes, thresh_size):
    """`thresh_size * span` with build_graph's own torch expression (planograms.py:42-43) -> 0-dim tensor of the boxes' dtype."""
    span = (torch.amax(boxes[:, 2]) - torch.amin(boxes[:, 0]) + torch.amax(boxes[:, 3]) - torch.amin(boxes[:, 1])) / 2
    return thresh_size * span


def _upload_tables(device, **tables):
    """Small int32 tables (lists) in ONE upload -> their views on the device by name; they lie in the order given."""
    small = staging.upload(torch.tensor([v for table in tables.values() for v in table], dtype=torch.int32), device)
    views, at = {}, 0
    for name, table in tables.items():
        views[name] = small[at:at + len(table)]
        at += len(table)
    return SimpleNamespace(**views)


def build_graphs(items, thresh_size=0.5, device=None):
    """items: list of (boxes (n,4) xyxy, labels list of n) -> list of `Graph` on the device, built by one launch.  1 <= n <= MAX_NODES.
    Device work only: nothing is copied back.  items may be a `DeviceActuals` instead: its boxes, offsets and thresholds are read
    where they lie, nothing is uploaded, and the graphs' `labels` are placeholders (the ids are `DeviceActuals.label`)."""
    if isinstance(items, DeviceActuals):
        return _build_actual_graphs(items, thresh_size)
    if not items:
        return []
    device = torch.device('cuda', torch.cuda.current_device()) if device is None else device
    sizes = [len(labels) for _, labels in items]
    for (boxes, _), n in zip(items, sizes):
        if boxes.dim() != 2 or boxes.shape[0] != n or boxes.shape[1] != 4:
            raise ValueError('one label per box, boxes (n, 4)')
        if not 1 <= n <= MAX_NODES:
            raise ValueError(f'a device graph has between 1 and {MAX_NODES} nodes, got {n}')
    host = [boxes.detach().to(device='cpu', dtype=torch.float32) for boxes, _ in items]
    thresh = torch.stack([graph_threshold(b, thresh_size) for b in host]).to(torch.float32)
    off = staging.offsets(sizes)
    boxes = staging.upload(torch.cat(host).contiguous(), device)
    offsets = staging.upload(torch.tensor(off, dtype=torch.int32), device)
    thresh = staging.upload(thresh, device)
    nbr = torch.empty((off[-1], 8), dtype=torch.int32, device=device)
    weight = torch.empty((off[-1], 8), dtype=torch.float32, device=device)
    stamp = torch.empty((off[-1], 8), dtype=torch.int32, device=device)
    torch.ops.cvpce_amd.planogram_graphs(boxes, offsets, thresh, min(sizes), max(sizes), nbr, weight, stamp)
    parent = (nbr, weight, stamp)
    return [Graph(labels, nbr[o:o + n], weight[o:o + n], stamp[o:o + n], parent + (o,)) for (_, labels), o, n in zip(items, off, sizes)]


def _build_actual_graphs(actuals, thresh_size):
    sizes = actuals.n2
    if actuals.thresh_size != thresh_size:
        raise ValueError(f'the detections carry thresholds for thresh_size {actuals.thresh_size}, not {thresh_size}')
    if not sizes or not 1 <= min(sizes) or max(sizes) > MAX_NODES:
        raise ValueError(f'a device graph has between 1 and {MAX_NODES} nodes, got {sizes}')
    device, total = actuals.boxes.device, sum(sizes)
    nbr = torch.empty((total, 8), dtype=torch.int32, device=device)
    weight = torch.empty((total, 8), dtype=torch.float32, device=device)
    stamp = torch.empty((total, 8), dtype=torch.int32, device=device)
    torch.ops.cvpce_amd.planogram_graphs(actuals.boxes, actuals.off2, actuals.thresh, min(sizes), max(sizes), nbr, weight, stamp)
    parent = (nbr, weight, stamp)
    return [Graph([None] * n, nbr[o:o + n], weight[o:o + n], stamp[o:o + n], parent + (o,)) for o, n in zip(staging.offsets(sizes), sizes)]


def _packed(graphs, device):
    """-> (nbr, stamp) of the graphs packed back to back.  Graphs that are consecutive slices of one launch's tables are not copied."""
    first = graphs[0]._parent
    if first is not None and first[0].device == device:
        row, same = first[3], True
        for g in graphs:
            same = same and g._parent is not None and g._parent[0] is first[0] and g._parent[3] == row
            row += len(g)
        if same:
            return first[0][first[3]:row], first[2][first[3]:row]
    return (torch.cat([g.nbr.to(device) for g in graphs]).contiguous(), torch.cat([g.stamp.to(device) for g in graphs]).contiguous())


def min_agree_for(min_score):
    """The smallest agree count whose hypothesis score -(agree / 8) is NOT above min_score (9 if there is none): Python's own
    arithmetic, so the device's integer test is `large_common_subgraph`'s float test."""
    return next((a for a in range(len(CARDINALS) + 1) if not -(a / len(CARDINALS)) > min_score), len(CARDINALS) + 1)


def _launch_record(name):
    """The arguments of the op `name` as a record type: one field per argument, under the op's own names and in its order (read off
    its schema), so a record is filled by keyword, read by name and launched as a whole -- `launch()` -- whatever the order is."""
    op = getattr(torch.ops.cvpce_amd, name)
    record = namedtuple(name, [a.name for a in op.default._schema.arguments])
    record.launch = lambda self: op(*self)
    return record


MATCHERS = ('large', 'tonioni')


def check_matcher(matcher):
    if matcher not in MATCHERS:
        raise ValueError(f'matcher is one of {MATCHERS}, got {matcher!r}')
    return matcher


def score8_limit(min_score):
    """The largest integer t for which the score t / 8 is NOT above min_score, by Python's own arithmetic (as `min_agree_for`): the
    Tonioni kernels' integer test on score8 = -agree - 8 * bumps is `tonioni_mcs`'s float test."""
    t = int(8 * min_score // 1)
    while not (t + 1) / 8 > min_score:
        t += 1
    while t / 8 > min_score:
        t -= 1
    return max(min(t, 2 ** 31 - 1), -2 ** 31)


def hypothesis_count(labels1, labels2):
    """The number of equal-label node pairs of two label lists: the hypotheses of the pair."""
    c1, c2 = Counter(labels1), Counter(labels2)
    return sum(c * c2[l] for l, c in c1.items() if l in c2)


MatchLaunch = _launch_record('planogram_match')
TonioniRun = _launch_record('tonioni_run')
TonioniSelect = _launch_record('tonioni_select')


class TonioniLaunch:
    """The launches of the Tonioni matcher as one: `run` (a `TonioniRun`: the hypotheses and every start's run) and `select` (a
    `TonioniSelect`: the choice and the adopted run's pairs), with the fields `match_on_device` reads off a `MatchLaunch`.
    `workspace` holds, as int32 words, the hypotheses [hypotheses], (M, F) per start [hypotheses][2] and the pairs' counts [P]."""
    __slots__ = ('run', 'select', 'label1', 'off1', 'label2', 'off2', 'out_off', 'pairs', 'count', 'workspace', 'hyp_off')

    def __init__(self, run, select, hyp_off):
        self.run, self.select, self.hyp_off = run, select, hyp_off
        self.label1, self.off1, self.label2, self.off2 = run.label1, run.off1, run.label2, run.off2
        self.out_off, self.pairs, self.count, self.workspace = select.out_off, select.pairs, select.count, run.workspace

    def launch(self):
        self.run.launch()
        self.select.launch()

    def per_start(self, p):
        """-> (M, F) of pair p's starts as an (H, 2) int32 device tensor (H: the host's count or bound of the pair)"""
        total = self.hyp_off[-1]
        return self.workspace[total:3 * total].view(-1, 2)[self.hyp_off[p]:self.hyp_off[p + 1]]
RansacLaunch = _launch_record('homography_ransac')
FinishLaunch = _launch_record('homography_finish')          # (its outputs are `TailLayout.views` of the tail's blob)


def _prepare_match(expected, actual, min_score, stop_at_fraction, actuals=None, expected_ids=None, matcher='large'):
    """Everything `planogram_match` needs, uploaded -> (`MatchLaunch`, its output tensor = pairs then counts, row offsets).
    matcher='tonioni': everything `tonioni_run` and `tonioni_select` need instead -> (`TonioniLaunch`, ...): the same tables, one
    score8 limit per pair as params, and the Tonioni workspace; stop_at_fraction is not read.
    actuals (a `DeviceActuals`, with expected_ids = `expected_label_ids`' (ids, largest multiplicity) per planogram): the actual side's
    ids and offsets are the pack's own, the expected ids come from the classifier's id space, and the hypothesis workspace is sized by
    the host's bound n2 x (largest multiplicity of an expected label) -- the kernel counts the hypotheses itself."""
    device = actual[0].nbr.device
    if device.type != 'cuda':
        raise ValueError('common_subgraphs runs on device graphs (build_graphs)')
    for g in list(expected) + list(actual):
        if not 1 <= len(g) <= MAX_NODES:
            raise ValueError(f'a device graph has between 1 and {MAX_NODES} nodes, got {len(g)}')
    n1, n2 = [len(g) for g in expected], [len(g) for g in actual]
    off1, off2 = staging.offsets(n1), staging.offsets(n2)
    hyps, params = [], []
    if actuals is None:
        ids = {}
        lab1 = [ids.setdefault(l, len(ids)) for g in expected for l in g.labels]
        lab2 = [ids.setdefault(l, len(ids)) for g in actual for l in g.labels]
    else:
        if n2 != actuals.n2 or [len(e[0]) for e in expected_ids] != n1:
            raise ValueError('the graphs of the detections, one id vector per expected graph')
        lab1, lab2 = [v for e in expected_ids for v in e[0]], []
    for p, (a, b) in enumerate(zip(n1, n2)):
        if actuals is None:
            c1, c2 = Counter(lab1[off1[p]:off1[p + 1]]), Counter(lab2[off2[p]:off2[p + 1]])
            hyps.append(sum(c * c2[l] for l, c in c1.items() if l in c2))
        else:
            hyps.append(b * expected_ids[p][1])
        params += [min_agree_for(min_score), int(min(a, b) * stop_at_fraction)] if matcher == 'large' else [score8_limit(min_score)]
    hyp_off, out_off = staging.offsets(hyps), staging.offsets([min(a, b) for a, b in zip(n1, n2)])
    if hyp_off[-1] >= 2 ** 31:
        raise ValueError('too many equal-label node pairs for one launch: split the batch')
    if matcher != 'large' and max(hyps) > TONIONI_MAX_HYPOTHESES:
        raise ValueError(f'the Tonioni matcher takes at most {TONIONI_MAX_HYPOTHESES} hypotheses per pair, got {max(hyps)}')
    small = _upload_tables(device, label1=lab1, label2=lab2, off1=off1, off2=off2 if actuals is None else [], params=params,
                           hyp_off=hyp_off, out_off=out_off)
    label2, dev_off2 = (small.label2, small.off2) if actuals is None else (actuals.label, actuals.off2)
    nbr1, stamp1 = _packed(expected, device)
    nbr2, stamp2 = _packed(actual, device)
    words = max(hyp_off[-1], 1) if matcher == 'large' else max(torch_ops_tonioni.workspace_words(hyp_off[-1], len(n1)), 1)
    workspace = torch.empty(words, dtype=torch.int32, device=device)
    out = torch.empty(out_off[-1] * 2 + len(n1), dtype=torch.int32, device=device)      # the pairs, then the counts: one copy back
    pairs, count = out[:out_off[-1] * 2].view(-1, 2), out[out_off[-1] * 2:]
    if matcher != 'large':
        common = dict(nbr1=nbr1, off1=small.off1, nbr2=nbr2, off2=dev_off2, params=small.params, hyp_off=small.hyp_off, max_n1=max(n1),
                      max_n2=max(n2), max_hyp=max(hyps), hypotheses=hyp_off[-1], workspace=workspace)
        run = TonioniRun(label1=small.label1, label2=label2, **common)
        return TonioniLaunch(run, TonioniSelect(out_off=small.out_off, pairs=pairs, count=count, **common), hyp_off), out, out_off
    match = MatchLaunch(nbr1=nbr1, stamp1=stamp1, label1=small.label1, off1=small.off1, nbr2=nbr2, stamp2=stamp2, label2=label2, off2=dev_off2,
                        params=small.params, hyp_off=small.hyp_off, out_off=small.out_off, max_n1=max(n1), max_n2=max(n2),
                        hypotheses=hyp_off[-1], workspace=workspace, pairs=pairs, count=count)
    return match, out, out_off


def common_subgraphs(expected, actual, min_score=-0.2, stop_at_fraction=1 / 2, matcher='large'):
    """`planograms.large_common_subgraph(g1, g2)` for every (g1, g2) of zip(expected, actual) -- lists of `Graph` -- in one launch
    and one device-to-host copy -> list of sets of (expected node, actual node).  A set is filled in the order its pairs grew, as
    the host's is (the order a set is built in decides the order it is iterated in).
    matcher='tonioni': `planograms.tonioni_mcs(g1, g2)` instead, in the same copy and wait; stop_at_fraction has no meaning for that
    search and is ignored."""
    if len(expected) != len(actual):
        raise ValueError('one actual graph per expected graph')
    if not expected:
        return []
    matching = match_on_device(expected, actual, min_score, stop_at_fraction, matcher=matcher)
    out, out_off = matching.out, matching.rows
    host = torch.empty(out.shape, dtype=torch.int32).pin_memory()
    host.copy_(out, non_blocking=True)
    torch.cuda.current_stream(out.device).synchronize()
    host = host.tolist()
    res = []
    for p in range(len(expected)):
        c, o = host[out_off[-1] * 2 + p], out_off[p] * 2
        grown = set()
        for k in range(c):
            grown.add((host[o + 2 * k], host[o + 2 * k + 1]))
        res.append(grown)
    return res


class DeviceMatching:
    """The matchings of a batch as the match kernel left them on the device: `pairs` [rows][2], `count` [P], `out_off` [P+1] (int32,
    views of `out` = pairs then counts), the label-id tables `label1` / `label2` with their offsets `off1` / `off2`, and on the host
    the node counts `n1` / `n2` and the row offsets `rows`.  `launch`: the `MatchLaunch` or `TonioniLaunch` that made it."""
    __slots__ = ('pairs', 'count', 'out_off', 'out', 'label1', 'off1', 'label2', 'off2', 'n1', 'n2', 'rows', 'launch')


def match_on_device(expected, actual, min_score=-0.2, stop_at_fraction=1 / 2, actuals=None, expected_ids=None, matcher='large'):
    """The launch of `common_subgraphs` alone -> `DeviceMatching`; nothing is copied back and nothing is waited for.
    actuals / expected_ids: the actual side is a `DeviceActuals` (`actual` = its graphs), see `_prepare_match`.
    matcher='tonioni': the launches of the Tonioni matcher instead, the same `DeviceMatching` (stop_at_fraction is ignored); with a
    `DeviceActuals` the launch is sized by the host's bound and the workgroups beyond a pair's real hypothesis count exit."""
    if len(expected) != len(actual) or not expected:
        raise ValueError('one actual graph per expected graph, at least one pair')
    match, out, out_off = _prepare_match(expected, actual, min_score, stop_at_fraction, actuals, expected_ids, check_matcher(matcher))
    match.launch()
    m = DeviceMatching()
    m.launch = match
    m.label1, m.off1, m.label2, m.off2 = match.label1, match.off1, match.label2, match.off2
    m.out_off, m.pairs, m.count = match.out_off, match.pairs, match.count
    m.out, m.rows, m.n1, m.n2 = out, out_off, [len(g) for g in expected], [len(g) for g in actual]
    return m


TailViews = namedtuple('TailViews', 'pos hmat status winner winner_count final_count size matched_expected matched_actual '
                                    'outcome occupant occupant_iou occupant_row stray', defaults=(None,) * 5)


class TailLayout:
    """Where the outputs of a window's tail lie in their ONE allocation, so that one copy brings them back: positions (f32), H (f64),
    then the int32 fields status, winner, winner count, final count, matching size, matched_expected, matched_actual and -- with
    `extra`, for the compliance report -- outcome, occupant, occupant IoU (f32), occupant row and stray.  The byte offsets are here
    and nowhere else: `views` is applied to the device blob for the launches and to its pinned copy for the records."""
    __slots__ = ('b', 'sum1', 'sum2', 'extra', 'at_h', 'at_i', 'at_m', 'nbytes')

    def __init__(self, b, sum1, sum2, extra=False):
        self.b, self.sum1, self.sum2, self.extra = b, sum1, sum2, bool(extra)
        self.at_h = 16 * sum1                           # bytes: H behind the positions
        self.at_i = self.at_h + 72 * b                  # bytes: the int32 fields behind H
        self.at_m = 5 * b                               # int32 words: the per-box fields behind the five per-image ones
        self.nbytes = self.at_i + 4 * (self.at_m + sum1 + sum2 + (4 * sum1 + sum2 if self.extra else 0))

    def views(self, blob):
        """blob: a uint8 tensor of `nbytes`, on any device -> `TailViews`"""
        b, sum1, sum2, m = self.b, self.sum1, self.sum2, self.at_m
        pos, hmat = blob[:self.at_h].view(torch.float32).view(sum1, 4), blob[self.at_h:self.at_i].view(torch.float64)
        i32 = blob[self.at_i:].view(torch.int32)
        per_image = [i32[k * b:(k + 1) * b] for k in range(5)]
        per_box = [i32[m:m + sum1], i32[m + sum1:m + sum1 + sum2]]
        if not self.extra:
            return TailViews(pos, hmat, *per_image, *per_box)
        r = m + sum1 + sum2
        rows = [i32[r + k * sum1:r + (k + 1) * sum1] for k in range(4)]
        return TailViews(pos, hmat, *per_image, *per_box, rows[0], rows[1], rows[2].view(torch.float32), rows[3], i32[r + 4 * sum1:])


def _prepare_tail(matching, expected_boxes, actual_boxes, reproj_thresholds, iou_threshold, seed, hypotheses, report=False):
    """Everything the two tail launches need, uploaded -> (`RansacLaunch`, `FinishLaunch`, the output blob, its `TailLayout`, the
    layout's views of the blob).  report: the blob also holds the compliance report's rows."""
    b = len(matching.n1)
    if not (b == len(expected_boxes) == len(actual_boxes) == len(reproj_thresholds)) or not b:
        raise ValueError('one entry per image, at least one image')
    if not 1 <= hypotheses <= torch_ops_homography.MAX_HYPOTHESES:
        raise ValueError(f'between 1 and {torch_ops_homography.MAX_HYPOTHESES} hypotheses, got {hypotheses}')
    device = matching.pairs.device
    n1, n2 = matching.n1, matching.n2
    on_device = isinstance(actual_boxes, DeviceActuals)
    if on_device and actual_boxes.n2 != n2:
        raise ValueError('the detections that were matched')
    for boxes, n in zip(list(expected_boxes) + ([] if on_device else list(actual_boxes)), n1 + n2):
        if boxes.dim() != 2 or boxes.shape[0] != n or boxes.shape[1] != 4:
            raise ValueError('the boxes of the graphs that were matched, (n, 4) each')
    sum1, sum2 = sum(n1), sum(n2)

    def packed(sets):
        """box sets back to back on the device: sets that lie there already (`expected_boxes_on_device`) are joined there"""
        if all(bx.device == device and bx.dtype == torch.float32 for bx in sets):
            return sets[0].contiguous() if len(sets) == 1 else torch.cat(sets)
        return staging.upload(torch.cat([bx.detach().to(device='cpu', dtype=torch.float32) for bx in sets]).contiguous(), device)

    if on_device:
        boxes1, boxes2 = packed(list(expected_boxes)), actual_boxes.boxes
    elif any(bx.device == device for bx in expected_boxes):
        boxes1, boxes2 = packed(list(expected_boxes)), packed(list(actual_boxes))
    else:                                         # (host boxes on both sides: one upload)
        boxes = packed(list(expected_boxes) + list(actual_boxes))
        boxes1, boxes2 = boxes[:sum1], boxes[sum1:]
    params = staging.upload(torch.tensor([[float(t), float(iou_threshold)] for t in reproj_thresholds], dtype=torch.float64), device)
    workspace = torch.empty(max(torch_ops_homography.workspace_bytes(b, hypotheses), 8) // 4, dtype=torch.int32, device=device)
    layout = TailLayout(b, sum1, sum2, extra=report)
    blob = torch.empty(layout.nbytes, dtype=torch.uint8, device=device)
    out = layout.views(blob)
    common = dict(boxes1=boxes1, off1=matching.off1, boxes2=boxes2, off2=matching.off2, pairs=matching.pairs, count=matching.count,
                  out_off=matching.out_off, params=params, max_pairs=max(1, max(min(a, c) for a, c in zip(n1, n2))), seed=seed,
                  hypotheses=hypotheses, workspace=workspace)
    finish = FinishLaunch(label1=matching.label1, label2=matching.label2, max_n1=max(n1), max_n2=max(n2), status=out.status, H=out.hmat,
                          winner=out.winner, winner_count=out.winner_count, final_count=out.final_count,
                          matched_expected=out.matched_expected, matched_actual=out.matched_actual, expected_positions=out.pos, **common)
    return RansacLaunch(**common), finish, blob, layout, out


class ReclassPlan:
    """What `reclass_plan` left on the device for a window, and the tail outputs the verdict kernel reads beside it: `boxes`
    [B][cap][4] f32, `expected_index` [B][cap] and `count` [B] int32 (slots at and beyond an image's count are unwritten), the views
    `status`, `matched_expected` and `off1` of the tail's tensors, and on the host `counts` (a list, brought back in the tail's own
    synchronisation), the box counts `n1` and `cap` = max n1.  `outcome`: where `report_positions` left the window's outcomes on the
    device (`finalize_batch(..., report=...)`), else None."""
    __slots__ = ('boxes', 'expected_index', 'count', 'status', 'matched_expected', 'off1', 'counts', 'n1', 'cap', 'outcome')


def _image_table(image_table, b, device):
    if len(image_table) != b:
        raise ValueError('one (h, w, enabled) row per image')
    return staging.upload(torch.tensor([[int(h), int(w), int(bool(on))] for h, w, on in image_table], dtype=torch.int32), device)


def _launch_plan(matching, finish, table):
    """`reclass_plan` behind `homography_finish` on the same stream, and its counts on their way to pinned memory -> (ReclassPlan
    without `counts`, the pinned tensor the counts land in once the stream has been waited for).  table: `_image_table`'s."""
    from . import torch_ops_reclass  # noqa: F401  (registers torch.ops.cvpce_amd.reclass_*)
    b = len(matching.n1)
    device = finish.status.device
    plan = ReclassPlan()
    plan.n1, plan.cap, plan.outcome = list(matching.n1), max(matching.n1), None
    plan.status, plan.matched_expected, plan.off1 = finish.status, finish.matched_expected, finish.off1
    plan.boxes = torch.empty((b, plan.cap, 4), dtype=torch.float32, device=device)
    slots = torch.empty(b * plan.cap + b, dtype=torch.int32, device=device)
    plan.expected_index, plan.count = slots[:b * plan.cap].view(b, plan.cap), slots[b * plan.cap:]
    torch.ops.cvpce_amd.reclass_plan(finish.status, finish.matched_expected, finish.expected_positions, finish.off1, table, plan.boxes,
                                     plan.expected_index, plan.count)
    host = torch.empty(b, dtype=torch.int32).pin_memory()
    host.copy_(plan.count, non_blocking=True)
    return plan, host


def reclassify_batch(plan, images, classifier, expected_label_ids, report=False):
    """The window's second trip through the crop / embed / match kernels in one pass (the re-classification rule of DESIGN.md 4b):
    every image's planned positions are cropped straight to the embedder's bf16 input (`production.roi_crops`: boxes and counts are
    read on the device), compacted with the host's counts, embedded by ONE schedule and matched by ONE distance GEMM;
    `reclass_verdict` compares label ids and one pinned copy brings back the per-image found counts -- the only wait of this pass.
    plan: the `ReclassPlan` of `finalize_batch(..., reclass=...)` with at least one position; images: the window's images (either
    form; read only where the image's count is > 0); expected_label_ids: one list of ids per image (`Classifier.expected_label_ids`).
    -> list of found counts, -1 for an image without a homography.
    report (the report rule of DESIGN.md 4b; a plan of `finalize_batch(..., report=...)`): the matcher also emits its distances,
    `report_reclass` runs behind the verdict on a copy of the plan's outcomes, and the same pinned copy brings back the window's final
    outcomes, seen rows and seen distances -> (found counts, outcome (sumN1,) int32, seen_row (sumN1,) int32, seen_distance (sumN1,)
    float32), host tensors; the rows of an image without a homography hold nothing."""
    from . import ops, production
    b, cap, counts = len(plan.n1), plan.cap, plan.counts
    device = plan.count.device
    total, sum1 = sum(counts), sum(plan.n1)
    if not total or len(images) != b or [len(ids) for ids in expected_label_ids] != plan.n1:
        raise ValueError('a plan with positions, one image and one id vector per image of the plan')
    crops, ext, const_in, partial = production.roi_crops(
        classifier.encoder, device, [ops.input_image(img, device) if c else None for img, c in zip(images, counts)], plan.boxes, plan.count)
    # one upload for the small tables: every slot's row in the compacted crops (-1 beyond the count), the compaction itself, the ids
    rows, sel, at = [], [], 0
    for i, c in enumerate(counts):
        rows += list(range(at, at + c)) + [-1] * (cap - c)
        sel += range(i * cap, i * cap + c)
        at += c
    small = _upload_tables(device, slot_row=rows, sel=sel, ids=[v for ids in expected_label_ids for v in ids])
    slot_row, sel, ids = small.slot_row.view(b, cap), small.sel, small.ids
    if total != b * cap:                        # (the embedder only runs over the valid crops, as BatchedPipeline._select has it)
        crops = crops.index_select(0, sel)
        ext = ext.index_select(0, sel) if ext is not None else None
    eng = classifier.encoder.engine()
    emb = eng.embed_packed(crops, ext=ext, const_in=const_in, partial=partial) if ext is not None else eng.embed_packed(crops)
    if report:
        return _verdict_and_report(plan, classifier, emb, slot_row, ids)
    indices = classifier.match(emb).contiguous()
    out = torch.empty(sum1 + b, dtype=torch.int32, device=device)
    torch.ops.cvpce_amd.reclass_verdict(plan.expected_index, plan.count, slot_row, indices, classifier.gallery_label_id, ids,
                                        plan.matched_expected, plan.off1, plan.status, out[:sum1], out[sum1:])
    host = torch.empty(b, dtype=torch.int32).pin_memory()
    host.copy_(out[sum1:], non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    return host.tolist()


class VerdictLayout:
    """The int32 words of `_verdict_and_report`'s one buffer: found counts [b], outcome, seen_row, seen_distance (f32) [sum1 each] --
    the first `back` words, which the pinned copy brings back -- then found [sum1], which stays on the device."""
    __slots__ = ('b', 'sum1', 'back', 'words')

    def __init__(self, b, sum1):
        self.b, self.sum1, self.back, self.words = b, sum1, b + 3 * sum1, b + 4 * sum1

    def views(self, buf):
        """buf: an int32 tensor of `words`, or of the first `back` of them (`found` is empty then), on any device"""
        b, sum1 = self.b, self.sum1
        return SimpleNamespace(found_count=buf[:b], outcome=buf[b:b + sum1], seen_row=buf[b + sum1:b + 2 * sum1],
                               seen_distance=buf[b + 2 * sum1:self.back].view(torch.float32), found=buf[self.back:])


def _verdict_and_report(plan, classifier, emb, slot_row, ids):
    """The end of `reclassify_batch` with the report on: match with distances, `reclass_verdict`, `report_reclass`, ONE pinned copy of
    {found counts, outcomes, seen rows, seen distances} and the pass's only wait."""
    from . import torch_ops_report  # noqa: F401  (registers torch.ops.cvpce_amd.report_*)
    b, sum1, device = len(plan.n1), sum(plan.n1), plan.count.device
    if plan.outcome is None:
        raise ValueError('a plan of finalize_batch(..., report=...)')
    indices, distances = classifier.match(emb, return_distance=True)
    indices, distances = indices.contiguous(), distances.contiguous()
    layout = VerdictLayout(b, sum1)
    buf = torch.empty(layout.words, dtype=torch.int32, device=device)
    out = layout.views(buf)
    out.outcome.copy_(plan.outcome)
    torch.ops.cvpce_amd.reclass_verdict(plan.expected_index, plan.count, slot_row, indices, classifier.gallery_label_id, ids,
                                        plan.matched_expected, plan.off1, plan.status, out.found, out.found_count)
    torch.ops.cvpce_amd.report_reclass(plan.expected_index, plan.count, slot_row, indices, distances, classifier.gallery_label_id, ids,
                                       plan.off1, plan.status, out.outcome, out.seen_row, out.seen_distance)
    host = torch.empty(layout.back, dtype=torch.int32).pin_memory()
    host.copy_(buf[:layout.back], non_blocking=True)
    torch.cuda.current_stream(device).synchronize()
    back = layout.views(host)
    return back.found_count.tolist(), back.outcome, back.seen_row, back.seen_distance


def finalize_batch(expected, actual, matching, expected_boxes, actual_boxes, reproj_thresholds, iou_threshold=0.5, seed=0,
                   hypotheses=RANSAC_HYPOTHESES, reclass=None, report=None):
    """`planograms.finalize_via_ransac` for every image of a batch under the tail rule: two launches on the matchings
    as they lie on the device (`match_on_device`) and ONE pinned copy back.  expected / actual: the lists of `Graph` the matching was
    made from; expected_boxes / actual_boxes: their (n, 4) boxes; reproj_thresholds: one per image, in pixels.  Expected boxes that lie
    on the device (`expected_boxes_on_device`) are not uploaded again; actual_boxes may be the `DeviceActuals` the matching was made
    from: its boxes are read where they lie and its `status` comes back in the same wait (non-zero: RuntimeError).
    -> one record per image: {'status': 'ok' | 'none' | 'invalid', 'matched_expected', 'matched_actual' (bool), 'expected_positions'
    (float32 (n1, 4)), 'homography' (3 x 3 float64, None unless ok), 'inliers' (of the refit), 'points', 'matching' (its size),
    'winner', 'winner_inliers'}.
    reclass (optional): one (image height, image width, enabled) per image -- `reclass_plan` is launched behind the tail and its counts
    come back in the same synchronisation -> (records, `ReclassPlan`) for `reclassify_batch`.
    report (optional; the report rule of DESIGN.md 4b): such a table too (with `reclass`: the same one) -- `report_positions` is
    launched behind the tail (and the plan) and its rows come back in the same copy: every record gains 'outcome' (int32 (n1,), PENDING
    where the position is to be re-classified), 'occupant', 'occupant_row' (int32 (n1,)), 'occupant_iou' (float32 (n1,)) and 'stray'
    (bool (n2,)); meaningful for an 'ok' record only.  The detections' gallery rows are read from a `DeviceActuals`."""
    if not len(expected) == len(actual) == len(matching.n1) or [len(g) for g in expected] != matching.n1 or [len(g) for g in actual] != matching.n2:
        raise ValueError('the graphs the matching was made from')
    b, n1, n2 = len(expected), matching.n1, matching.n2
    if reclass is not None and report is not None and list(report) != list(reclass):
        raise ValueError('the report reads the image table the plan reads')
    ransac, finish, blob, layout, out = _prepare_tail(matching, expected_boxes, actual_boxes, reproj_thresholds, iou_threshold, seed, hypotheses,
                                                      report=report is not None)
    ransac.launch()
    finish.launch()
    table = _image_table(reclass if reclass is not None else report, b, blob.device) if (reclass is not None or report is not None) else None
    plan, plan_counts = _launch_plan(matching, finish, table) if reclass is not None else (None, None)
    if report is not None:
        from . import torch_ops_report  # noqa: F401  (registers torch.ops.cvpce_amd.report_*)
        torch.ops.cvpce_amd.report_positions(finish.status, finish.matched_expected, finish.matched_actual, finish.expected_positions, finish.boxes2,
                                             finish.off1, finish.off2, table, actual_boxes.row if isinstance(actual_boxes, DeviceActuals) else None,
                                             float(iou_threshold), out.outcome, out.occupant, out.occupant_iou, out.occupant_row, out.stray)
        if plan is not None:
            plan.outcome = out.outcome
    out.size.copy_(matching.count)                                 # (the matching's size travels in the same copy)
    back = torch.empty(blob.shape, dtype=torch.uint8).pin_memory()
    back.copy_(blob, non_blocking=True)
    pack_status = None
    if isinstance(actual_boxes, DeviceActuals):                   # (what `actuals_pack` reported comes back in the same wait)
        pack_status = torch.empty(b, dtype=torch.int32).pin_memory()
        pack_status.copy_(actual_boxes.status, non_blocking=True)
    torch.cuda.current_stream(blob.device).synchronize()
    if pack_status is not None and any(pack_status.tolist()):
        raise RuntimeError(f'actuals_pack: status {pack_status.tolist()} (1: the kept count is not the offsets\', 2: a gallery row outside the gallery)')
    if plan is not None:
        plan.counts = plan_counts.tolist()
    host = layout.views(back)
    status, winner, winner_count, final_count, size = (t.tolist() for t in (host.status, host.winner, host.winner_count, host.final_count, host.size))
    me, ma, hmat = host.matched_expected != 0, host.matched_actual != 0, host.hmat.view(b, 3, 3)
    off1, off2 = staging.offsets(n1), staging.offsets(n2)
    records = []
    for p in range(b):
        e, a, m = slice(off1[p], off1[p + 1]), slice(off2[p], off2[p + 1]), size[p]
        rec = {'status': STATUS[status[p]], 'matched_expected': me[e].clone(), 'matched_actual': ma[a].clone(),
               'expected_positions': host.pos[e].clone(), 'homography': hmat[p].clone() if status[p] == torch_ops_homography.OK else None,
               'inliers': final_count[p], 'points': 5 if m == 1 else 3 * m, 'matching': m, 'winner': winner[p], 'winner_inliers': winner_count[p]}
        if report is not None:
            rec.update(outcome=host.outcome[e].clone(), occupant=host.occupant[e].clone(), occupant_iou=host.occupant_iou[e].clone(),
                       occupant_row=host.occupant_row[e].clone(), stray=host.stray[a] != 0)
        records.append(rec)
    return records if plan is None else (records, plan)


def finalize_result(record, expected_labels, return_matched_actual=False, report_accuracy=False, return_expected_positions=False):
    """A record of `finalize_batch` as the tuple `planograms.finalize_via_ransac` returns for the same flags (all None without a
    homography).  An 'invalid' record -- a matching that is not one of its graphs -- is an error."""
    if record['status'] == 'invalid':
        raise RuntimeError('finalize_batch: the matching does not belong to the graphs')
    if report_accuracy:
        print(f"Homography accuracy: {record['inliers'] / max(record['points'], 1)}")
    if record['status'] != 'ok':
        return (None,) * 5 if return_matched_actual else (None,) * 4          # (the host's own lengths)
    matched_expected, positions = record['matched_expected'], record['expected_positions']
    missing_expected = torch.where(~matched_expected)[0]
    out = (matched_expected,) + ((record['matched_actual'],) if return_matched_actual else ()) + ((positions,) if return_expected_positions else ())
    return out + (missing_expected, positions[missing_expected], [expected_labels[i] for i in missing_expected.tolist()])


def to_networkx(graph):
    """-> the DiGraph `planograms.build_graph` would hand to the host functions: nodes 0..n-1 with `label`, edges with `dir` and
    `weight`, every node's adjacency in stamp order.  (One copy to the host for a device graph.)"""
    nbr, weight, stamp = graph.nbr.cpu(), graph.weight.cpu(), graph.stamp.cpu()
    g = nx.DiGraph()
    g.add_nodes_from((i, {'label': l}) for i, l in enumerate(graph.labels))
    filled = (nbr >= 0).nonzero().tolist()
    for i, s in sorted(filled, key=lambda e: int(stamp[e[0], e[1]])):
        g.add_edge(i, int(nbr[i, s]), dir=CARDINALS[s], weight=weight[i, s])
    return g


def nbr_table(g):
    """`to_networkx` backwards, the neighbours alone: a host DiGraph of `planograms.build_graph` (nodes 0..n-1, at most one edge per node
    and direction) -> its `nbr` [n][8] int32 table on the host, -1 = empty: what the step pictures draw (`rendering.graph_strokes`)."""
    table = torch.full((g.number_of_nodes(), len(CARDINALS)), -1, dtype=torch.int32)
    for i, j, d in g.edges(data='dir'):
        table[i, CARDINALS.index(d)] = j
    return table


def matched_of_pairs(pairs, n1, n2):
    """a matching as the host has it -- (expected node, actual node) pairs -> (matched expected nodes (n1,), matched actual nodes (n2,)),
    bool, on the host"""
    me, ma = torch.zeros(n1, dtype=torch.bool), torch.zeros(n2, dtype=torch.bool)
    for a, b in pairs:
        me[a], ma[b] = True, True
    return me, ma


def matched_nodes(matching, p):
    """`matched_of_pairs` for pair p of a `DeviceMatching`, on the device and without a wait: the rows of `pairs` beyond the pair's
    count hold -1 and mark nothing."""
    rows = matching.pairs[matching.rows[p]:matching.rows[p + 1]].to(torch.int64)
    out = []
    for col, n in ((0, matching.n1[p]), (1, matching.n2[p])):
        node = rows[:, col]
        marks = torch.zeros(n + 1, dtype=torch.bool, device=rows.device)                   # (slot n: the rows that name no node)
        marks.index_fill_(0, torch.where((node >= 0) & (node < n), node, torch.full_like(node, n)), True)
        out.append(marks[:n])
    return tuple(out)


def prepare(expected, thresh_size=0.5, device=None):
    """Builds the device graph of a planogram dict ({'boxes', 'labels', ...}) once and keeps it in the dict under CACHE_KEY (with the
    threshold it was built for) -> the `Graph`."""
    cached = expected.get(CACHE_KEY)
    if cached is None or cached[0] != thresh_size:
        cached = expected[CACHE_KEY] = (thresh_size, build_graphs([(expected['boxes'], expected['labels'])], thresh_size, device)[0])
    return cached[1]


def cached(expected, thresh_size):
    c = expected.get(CACHE_KEY) if isinstance(expected, dict) else None
    return c[1] if c is not None and c[0] == thresh_size else None


def expected_boxes_on_device(expected, device):
    """A planogram's boxes as the tail kernels read them -- float32 (n, 4) on `device` -- uploaded once and kept in the planogram's
    dict under BOXES_KEY beside the cached graph (with the host tensor they were made from: other boxes, another upload)."""
    boxes = expected['boxes']
    c = expected.get(BOXES_KEY) if isinstance(expected, dict) else None
    if c is None or c[0] is not boxes or c[1].device != device:
        c = (boxes, staging.upload(boxes.detach().to(device='cpu', dtype=torch.float32).contiguous(), device))
        if isinstance(expected, dict):
            expected[BOXES_KEY] = c
    return c[1]


def expected_label_ids(planograms, classifier):
    """The expected labels of a window as ids the match and claim kernels can compare with `DeviceActuals.label`: a label some gallery
    item has gets its id of `classifier.label_ids`; a label no gallery item has gets len(label_ids) + r, r = its rank among such
    labels in the window in order of appearance -- non-negative (the match kernel masks ids with INT_MAX), and equal id <=> equal
    label across the window.  -> one (ids, largest multiplicity of a label) per planogram, or None where there is no id space or a
    label cannot be hashed.  What does not depend on the window is cached in the planogram's dict under IDS_KEY with the classifier's
    index generation, as `PlanogramComparator.LABEL_IDS_KEY` is."""
    space, generation = getattr(classifier, 'label_ids', None), getattr(classifier, 'index_generation', None)
    if space is None or generation is None:
        return None
    ranks, out = {}, []
    for plano in planograms:
        labels = plano['labels']
        c = plano.get(IDS_KEY) if isinstance(plano, dict) else None
        if c is None or c[0] != generation or len(c[1]) != len(labels):
            try:
                ids = [space.get(l, -1) for l in labels]
                c = (generation, ids, [i for i, v in enumerate(ids) if v < 0], max(Counter(labels).values(), default=0))
            except TypeError:
                return None
            if isinstance(plano, dict):
                plano[IDS_KEY] = c
        ids = c[1]
        if c[2]:
            ids = list(ids)
            for i in c[2]:
                ids[i] = len(space) + ranks.setdefault(labels[i], len(ranks))
        out.append((ids, c[3]))
    return out
