"""The stroke rule on the host (no GPU): tests/stroke_cases.py, the model csrc/strokes.hip is held to, is pinned against the rule read
pixel by pixel and against a float64 distance; the stroke lists of a hand-made graph are the edge list `to_networkx` gives; the
folder gallery and the JSON planogram of `misc pipeline-demo` read what the test writes; the binding of
include/ext/cvpce_amd_strokes.h agrees with its header."""
import ctypes
import json
import math

import numpy as np
import pytest
import torch

import abi
import stroke_cases as sc

HEADER = 'ext/cvpce_amd_strokes.h'
RED, BLUE = 0x0000FF, 0xFF0000


def _mask(hw, ends, radius):
    """the pixels one stroke covers, by painting it on a black canvas"""
    canvas = np.zeros(hw + (3,), dtype=np.uint8)
    sc.paint(canvas, np.array([ends], dtype=np.float32), np.array([0xFFFFFF], dtype=np.int32), np.array([radius], dtype=np.int32))
    return canvas[:, :, 0] == 255


def _brute(hw, ends, radius):
    """the rule pixel by pixel over the whole canvas, Python integers"""
    st = sc.integers(ends, radius)
    m = np.zeros(hw, dtype=bool)
    if st is not None:
        for y in range(hw[0]):
            for x in range(hw[1]):
                m[y, x] = sc.covers(st, x, y)
    return m


def test_the_window_of_the_model_is_the_rule_on_the_whole_canvas():
    rng = np.random.RandomState(0)
    for ends, _, radius in sc.special_strokes(17, 65):
        assert np.array_equal(_mask((17, 65), ends, radius), _brute((17, 65), ends, radius)), (ends, radius)
    for _ in range(60):
        ends = rng.uniform(-20, 60, 4)
        radius = int(rng.choice([1, 2, 3, 6, 17, 64]))
        assert np.array_equal(_mask((30, 40), ends, radius), _brute((30, 40), ends, radius)), (ends, radius)


def test_a_zero_length_stroke_is_exactly_the_disc():
    for cx, cy, r in ((10.5, 8.5, 1), (10.5, 8.5, 2), (10.0, 8.0, 5), (10.25, 8.75, 9), (3.0, 2.0, 64)):
        ax, ay = math.floor(2 * cx), math.floor(2 * cy)
        yy, xx = np.mgrid[:24, :32]
        want = (2 * xx + 1 - ax) ** 2 + (2 * yy + 1 - ay) ** 2 <= r * r
        assert np.array_equal(_mask((24, 32), (cx, cy, cx, cy), r), want), (cx, cy, r)
    # radius 2 about a pixel centre: the pixel and its four neighbours
    m = _mask((3, 5), (2.5, 1.5, 2.5, 1.5), 2)
    assert m.sum() == 5 and m[1, 1:4].all() and m[0, 2] and m[2, 2]


def test_a_stroke_is_symmetric_in_its_ends():
    rng = np.random.RandomState(1)
    for _ in range(100):
        e = rng.uniform(-10, 50, 4)
        r = int(rng.choice([1, 2, 3, 6, 20]))
        assert np.array_equal(_mask((32, 40), e, r), _mask((32, 40), (e[2], e[3], e[0], e[1]), r)), (e, r)


def test_a_horizontal_stroke_paints_the_expected_rows():
    # through pixel centres (y = 5.5): radius t covers the rows whose centres lie within t half pixels: t = 1 the row itself, t = 2 and 3
    # three rows, t = 4 five
    for t, rows in ((1, [5]), (2, [4, 5, 6]), (3, [4, 5, 6]), (4, [3, 4, 5, 6, 7])):
        m = _mask((12, 30), (4.5, 5.5, 20.5, 5.5), t)
        assert sorted(set(np.argwhere(m)[:, 0].tolist())) == rows, t
        assert m[5, 4:21].all() and not m[5, :2].any() and not m[5, 23:].any()       # (the caps of radius 4 reach two pixels past the ends)
    # on a pixel border (y = 5): radius t covers the t rows nearest to it
    for t, rows in ((1, [4, 5]), (2, [4, 5]), (3, [3, 4, 5, 6])):
        m = _mask((12, 30), (4.5, 5.0, 20.5, 5.0), t)
        assert sorted(set(np.argwhere(m)[:, 0].tolist())) == rows, t
    # a radius-1 diagonal hits every column it crosses
    m = _mask((40, 60), (2.3, 1.7, 55.1, 33.9), 1)
    assert m[:, 3:55].any(axis=0).all()


def test_the_later_stroke_wins():
    ends = np.array([[2, 5, 20, 5], [10, 0, 10, 12]], dtype=np.float32)
    radius = np.array([3, 3], dtype=np.int32)
    a = sc.paint(np.zeros((12, 24, 3), dtype=np.uint8), ends, np.array([RED, BLUE], dtype=np.int32), radius)
    b = sc.paint(np.zeros((12, 24, 3), dtype=np.uint8), ends[::-1], np.array([BLUE, RED], dtype=np.int32), radius[::-1])
    assert a[5, 10].tolist() == [0, 0, 255] and b[5, 10].tolist() == [255, 0, 0]              # the crossing: the last of the list
    assert a[5, 3].tolist() == b[5, 3].tolist() == [255, 0, 0] and a[1, 10].tolist() == b[1, 10].tolist() == [0, 0, 255]
    assert np.array_equal((a != 0).any(axis=2), (b != 0).any(axis=2))


def test_skipped_strokes_paint_nothing_and_the_radius_is_clamped():
    nan, inf = float('nan'), float('inf')
    for ends in ((nan, 1, 5, 5), (1, nan, 5, 5), (1, 1, inf, 5), (1, 1, 5, -inf), (-inf, -inf, inf, inf)):
        assert not _mask((10, 10), ends, 3).any()
    for radius in (0, -1, -2 ** 31):
        assert not _mask((10, 10), (1, 1, 8, 8), radius).any()
    for radius in (65, 1000, 2 ** 31 - 1):
        assert np.array_equal(_mask((80, 90), (40, 40, 50, 42), radius), _mask((80, 90), (40, 40, 50, 42), 64))
    assert not np.array_equal(_mask((80, 90), (40, 40, 50, 42), 63), _mask((80, 90), (40, 40, 50, 42), 64))
    # ends at +-1e9 are the ends at the clamp
    assert np.array_equal(_mask((10, 50), (-1e9, 5.5, 1e9, 5.5), 1), _mask((10, 50), (-32768, 5.5, 32767, 5.5), 1))
    assert _mask((10, 50), (-1e9, 5.5, 1e9, 5.5), 1)[5].all()
    # nothing but covered pixels is touched
    canvas = np.full((9, 9, 3), 0x5A, dtype=np.uint8)
    sc.paint(canvas, np.array([[4.5, 4.5, 4.5, 4.5]], dtype=np.float32), np.array([0x030201], dtype=np.int32), np.array([1], dtype=np.int32))
    assert canvas[4, 4].tolist() == [1, 2, 3] and (np.delete(canvas.reshape(-1, 3), 4 * 9 + 4, axis=0) == 0x5A).all()


def test_the_model_agrees_with_a_float64_distance_away_from_the_radius():
    rng = np.random.RandomState(2)
    yy, xx = np.mgrid[:48, :64]
    px, py = 2.0 * xx + 1, 2.0 * yy + 1
    for _ in range(300):
        e = rng.uniform(-15, 75, 4).astype(np.float32)
        if rng.rand() < 0.1:
            e[2:] = e[:2]
        r = int(rng.choice([1, 2, 3, 6, 11, 40, 64]))
        ax, ay, bx, by, _ = sc.integers(e, r)
        dx, dy = float(bx - ax), float(by - ay)
        l2 = dx * dx + dy * dy
        t = np.clip(((px - ax) * dx + (py - ay) * dy) / l2, 0, 1) if l2 else np.zeros_like(px)
        dist = np.hypot(px - (ax + t * dx), py - (ay + t * dy))
        sure = np.abs(dist - r) > 1e-7
        got = _mask((48, 64), e, r)
        assert np.array_equal(got[sure], (dist <= r)[sure]), (e, r)


# ---- the stroke lists ---------------------------------------------------------------------------------------------------------------
def _hand_graph():
    """4 nodes in a square: 0 - 1 on top, 2 - 3 below, the verticals 0 - 2 and 1 - 3, and the diagonal 0 - 3 one way only"""
    from cvpce_amd import planograms_device as pd
    from cvpce_amd.planograms import CARDINALS
    slot = CARDINALS.index
    nbr = torch.full((4, 8), -1, dtype=torch.int32)
    for i, d, j in ((0, 'E', 1), (1, 'W', 0), (2, 'E', 3), (3, 'W', 2), (0, 'S', 2), (2, 'N', 0), (1, 'S', 3), (3, 'N', 1), (0, 'SE', 3)):
        nbr[i, slot(d)] = j
    stamp = torch.arange(32, dtype=torch.int32).reshape(4, 8)
    graph = pd.Graph(['a', 'b', 'c', 'd'], nbr, torch.ones(4, 8), stamp)
    boxes = torch.tensor([[10.0, 10, 31, 30], [50, 10, 70, 31], [10, 50, 30, 70], [50, 50, 71, 70.5]])
    return graph, boxes


def _segments(strokes):
    """the strokes that paint: ({(ax, ay, bx, by, colour, radius) of the edges}, [the same of the discs])"""
    rows = [tuple(e) + (c, r) for e, c, r in zip(strokes.ends.tolist(), strokes.colour.tolist(), strokes.radius.tolist()) if r > 0]
    return {r for r in rows if r[:2] != r[2:4]}, [r for r in rows if r[:2] == r[2:4]]


def test_graph_strokes_are_the_edges_and_nodes_of_the_networkx_graph():
    from cvpce_amd import planograms_device as pd, rendering as rd
    graph, boxes = _hand_graph()
    g = pd.to_networkx(graph)
    assert g.number_of_edges() == 9
    centre = [((b[0] + b[2]) / 2, (b[1] + b[3]) / 2) for b in boxes.tolist()]
    strokes = rd.graph_strokes(graph, boxes)
    assert len(strokes) == 9 * 4 and strokes.ends.dtype == torch.float32 and strokes.colour.dtype == strokes.radius.dtype == torch.int32
    assert tuple(strokes.ends.shape) == (36, 4) and strokes.ends.is_contiguous()
    edges, discs = _segments(strokes)
    assert edges == {centre[i] + centre[j] + (rd.GRAPH_EDGE_COLOUR, rd.GRAPH_EDGE_RADIUS) for i, j in g.edges()}
    assert discs == [c + c + (rd.GRAPH_NODE_COLOUR, rd.GRAPH_NODE_RADIUS) for c in centre]
    assert int((strokes.radius[:32] > 0).sum()) == 9 and (strokes.radius[32:] > 0).all()         # the edge slots first, then the nodes
    assert (strokes.ends[:32][strokes.radius[:32] == 0] == 0).all()                              # an empty slot: zero ends, radius 0
    # the table of the networkx graph is the graph's table: the host routes draw what the device routes draw
    assert torch.equal(pd.nbr_table(g), graph.nbr)
    same = rd.graph_strokes(pd.nbr_table(g), boxes)
    assert all(torch.equal(getattr(same, n), getattr(strokes, n)) for n in rd.Strokes.__slots__)
    # the subgraph of the matched nodes 0, 1, 3 (`ge.subgraph(nodes)`)
    matched = torch.tensor([True, True, False, True])
    sub = g.subgraph([0, 1, 3])
    edges, discs = _segments(rd.matched_strokes(graph, boxes, matched))
    assert edges == {centre[i] + centre[j] + (rd.GRAPH_EDGE_COLOUR, rd.GRAPH_EDGE_RADIUS) for i, j in sub.edges()} and len(edges) == 5
    assert discs == [centre[i] * 2 + (rd.GRAPH_NODE_COLOUR, rd.GRAPH_NODE_RADIUS) for i in (0, 1, 3)]
    assert len(rd.matched_strokes(graph, boxes, matched)) == 36
    # from the whole graph's list: the same strokes paint
    derived = rd.matched_strokes(graph, boxes, matched, whole=strokes)
    assert _segments(derived) == (edges, discs) and len(derived) == 36 and derived.radius.dtype == torch.int32
    assert torch.equal(derived.radius > 0, rd.matched_strokes(graph, boxes, matched).radius > 0)
    with pytest.raises(ValueError):
        rd.matched_strokes(graph, boxes, matched, whole=rd.Strokes.cat([strokes, strokes]))
    nothing = rd.matched_strokes(graph, boxes, torch.zeros(4, dtype=torch.bool))
    assert len(nothing) == 36 and not (nothing.radius > 0).any()
    # a neighbour outside the graph is an empty slot; another style; the wrong number of boxes
    bad = graph.nbr.clone()
    bad[2, 1] = 4
    assert int((rd.graph_strokes(bad, boxes).radius[:32] > 0).sum()) == 9
    styled = rd.graph_strokes(graph, boxes, edge_colour=5, node_colour=6, edge_radius=1, node_radius=3)
    assert sorted(set(styled.colour.tolist())) == [5, 6] and sorted(set(styled.radius.tolist())) == [0, 1, 3]
    with pytest.raises(ValueError):
        rd.graph_strokes(graph, boxes[:3])
    pairs = {(0, 2), (1, 0), (3, 1)}
    me, ma = pd.matched_of_pairs(pairs, 4, 3)
    assert me.tolist() == [True, True, False, True] and ma.tolist() == [True, True, True]
    cat = rd.Strokes.cat([strokes, styled])
    assert len(cat) == 72 and torch.equal(cat.ends[36:], styled.ends)


def test_the_expected_side_goes_through_the_expected_items_mapping():
    from cvpce_amd import rendering as rd
    boxes = torch.tensor([[100.0, 40, 140, 100], [150, 40, 190, 100], [100, 110, 140, 170]])
    hw = rd.expected_canvas_hw(boxes, 320)
    on_canvas = rd.expected_boxes_on_canvas(boxes, hw)
    assert torch.equal(on_canvas, rd.expected_items(boxes, torch.tensor([0, 1, 2]), hw).box)
    assert float(on_canvas.min()) == 0.0 and float(on_canvas[:, 2].max()) <= 320 and float(on_canvas[:, 3].max()) <= hw[0]
    pics = rd.StepPictures(*range(9))
    assert rd.StepPictures.NAMES[-3:] == rd.CompliancePictures.NAMES and pics.detections == 0 and pics.expected == 8
    with pytest.raises(ValueError):
        rd.StepPictures(1, 2, 3)


# ---- the folder gallery and the JSON planogram of `misc pipeline-demo` -----------------------------------------------------------------
def test_simple_folder_set_reads_a_folder_of_labelled_photos(tmp_path):
    from PIL import Image
    from cvpce_amd import datautils
    rng = np.random.RandomState(3)
    rgb = rng.randint(0, 256, (7, 5, 3)).astype(np.uint8)
    rgba = rng.randint(0, 256, (4, 6, 4)).astype(np.uint8)
    rgba[:, :, 3] = 255
    rgba[1, 2, 3] = rgba[3, 5, 3] = 0                              # two transparent pixels
    rgba[0, 0, 3] = 7                                              # nearly transparent is not transparent
    grey = rng.randint(0, 256, (3, 3)).astype(np.uint8)
    Image.fromarray(rgb, 'RGB').save(tmp_path / 'zeta.png')
    Image.fromarray(rgba, 'RGBA').save(tmp_path / 'alpha.v2.png')
    Image.fromarray(grey, 'L').save(tmp_path / 'Mid.PNG.png')
    Image.fromarray(rgb, 'RGB').save(tmp_path / 'beta.jpeg', quality=95)
    (tmp_path / 'notes.txt').write_text('no image')
    (tmp_path / 'folder.png').mkdir()
    data = datautils.SimpleFolderSet(str(tmp_path), train=False)
    assert data.classes == ['Mid.PNG', 'alpha.v2', 'beta', 'zeta'] and len(data) == 4              # sorted; the label is the file stem
    assert [data.index_for_ann(c) for c in ('zeta', 'alpha.v2')] == [3, 1]
    with pytest.raises(ValueError):
        data.index_for_ann('gamma')
    img, again, c, c2 = data[3]
    assert img is again and c == c2 == 'zeta' and img.dtype == torch.float32 and tuple(img.shape) == (3, 7, 5)
    assert torch.equal(img, torch.from_numpy(rgb).permute(2, 0, 1).to(torch.float32) / 255.0)
    img = data[1][0]
    want = torch.from_numpy(rgba[:, :, :3].copy()).permute(2, 0, 1).to(torch.float32) / 255.0
    want[:, 1, 2] = want[:, 3, 5] = 1.0                            # transparent -> white, the alpha plane dropped
    assert tuple(img.shape) == (3, 4, 6) and torch.equal(img, want)
    assert tuple(data[0][0].shape) == (3, 3, 3) and torch.equal(data[0][0][0], data[0][0][2])      # a grey file: three equal planes
    assert tuple(data[2][0].shape) == (3, 7, 5)
    only_png = datautils.SimpleFolderSet(str(tmp_path), train=False, types=('.png',))
    assert only_png.classes == ['Mid.PNG', 'alpha.v2', 'zeta']
    assert datautils.SimpleFolderSet(str(tmp_path)).train is True                                  # the default resizes (on the GPU)


def test_the_planogram_json_reader(tmp_path):
    from cvpce_amd import datautils
    path = tmp_path / 'plano.json'
    path.write_text(json.dumps([{'label': 'class1', 'box': [0, 0, 5, 5]}, {'label': 'class2', 'box': [5, 0, 10.5, 5]}]))
    plano = datautils.read_planogram_json(str(path))
    assert plano['labels'] == ['class1', 'class2'] and plano['boxes'].dtype == torch.float32
    assert plano['boxes'].tolist() == [[0, 0, 5, 5], [5, 0, 10.5, 5]]
    path.write_text('[]')
    empty = datautils.read_planogram_json(str(path))
    assert empty['labels'] == [] and tuple(empty['boxes'].shape) == (0, 4)
    for bad in ({'label': 'a', 'box': [0, 0, 1, 1]}, [{'label': 'a'}], [{'label': 'a', 'box': [0, 0, 1]}]):
        path.write_text(json.dumps(bad))
        with pytest.raises(ValueError):
            datautils.read_planogram_json(str(path))


def test_the_cli_has_the_two_commands():
    from click.testing import CliRunner
    from cvpce_amd.cli import cli, _DeviceDetectionsCommand, PIPELINE_DEMO_GRAPH_THRESHOLD
    assert isinstance(cli.commands['plot-planogram-eval'], _DeviceDetectionsCommand)
    assert isinstance(cli.commands['misc'].commands['pipeline-demo'], _DeviceDetectionsCommand) and PIPELINE_DEMO_GRAPH_THRESHOLD == 0.7
    text = CliRunner().invoke(cli, ['plot-planogram-eval', '--help']).output
    for option in ('--img-dir', '--test-imgs', '--test-annotations', '--planos', '--datatype', '--load-classifier-index', '--plano-idx', '--out',
                   '--device-graphs', '--device-detections'):
        assert option in text, option
    text = CliRunner().invoke(cli, ['misc', 'pipeline-demo', '--help']).output
    assert 'GLN_STATE DIHE_STATE DATASET_FOLDER' in text and 'IMAGE_FILE PLANO_FILE' in text and '--out' in text
    assert '--scale-gallery / --no-scale-gallery' in text and '[0,' in text and '[-1, 1]' in text and '--device-tail' in text
    missing = CliRunner().invoke(cli, ['misc', 'pipeline-demo', 'a', 'b', 'c', 'd', 'e'])
    assert missing.exit_code == 2


# ---- the binding of include/ext/cvpce_amd_strokes.h ---------------------------------------------------------------------------------
def test_header_table_ops_and_constants_agree():
    import re
    from cvpce_amd import _lib, torch_ops_strokes, torch_ops_render
    assert list(_lib.PICTURE_EXTENSION_HEADERS) == [HEADER] and HEADER not in _lib.HEADERS and HEADER not in _lib.EXTENSION_HEADERS
    table, symbols = _lib.PICTURE_EXTENSION_HEADERS[HEADER], abi.header_symbols(HEADER)
    assert sorted(table) == symbols == ['cvpce_strokes_draw']
    exported = ctypes.CDLL(_lib.LIB_PATH)
    declared = abi.declarations(HEADER)
    assert sorted(declared) == symbols, 'a declaration the parser cannot read'
    for fn, (c_ret, c_args) in declared.items():
        assert hasattr(exported, fn)
        restype, argtypes = table[fn]
        assert getattr(_lib.lib, fn).restype == restype and getattr(_lib.lib, fn).argtypes == argtypes, f'{fn}: the table is not bound'
        assert abi.ctypes_kind(restype) == c_ret and [abi.ctypes_kind(t) for t in argtypes] == c_args, fn
    # its names are its own: no other header's family word, and `strokes` in no other header's names
    assert torch_ops_strokes.NAMES == ['strokes_draw']
    for name in symbols + torch_ops_strokes.NAMES:
        assert 'strokes' in name and not [w for w in abi.FAMILY_WORDS.values() if w in name] and 'tonioni' not in name, name
    others = [s for h in abi.OP_MODULES for s in abi.header_symbols(h)] + [s for t in _lib.EXTENSION_HEADERS.values() for s in t]
    assert not [s for s in others if 'strokes' in s]
    assert torch._C._dispatch_has_kernel_for_dispatch_key('cvpce_amd::strokes_draw', 'CUDA')
    assert not torch._C._dispatch_has_kernel_for_dispatch_key('cvpce_amd::strokes_draw', 'CPU')
    text = open(abi.INCLUDE + '/' + HEADER).read()
    define = lambda name: int(re.search(rf'#define CVPCE_STROKES_{name} (\d+)', text).group(1))
    assert (define('TILE_W'), define('TILE_H')) == (torch_ops_strokes.TILE_W, torch_ops_strokes.TILE_H) == (sc.TILE_W, sc.TILE_H) == \
        (torch_ops_render.TILE_W, torch_ops_render.TILE_H)
    assert define('MAX_RADIUS') == torch_ops_strokes.MAX_RADIUS == sc.MAX_RADIUS == 64 and define('CHUNK') == sc.CHUNK == define('THREADS')
    assert define('TABLE_COLS') == torch_ops_strokes.TABLE_COLS == sc.COLS and define('MAX_SIDE') == torch_ops_strokes.MAX_SIDE == sc.MAX_SIDE
    assert torch_ops_strokes.tiles(17, 65) == sc.tiles(17, 65) == 4 and torch_ops_strokes.tiles(1, 32768) == 512


def test_the_cases_hold_what_the_kernel_test_needs():
    cs = sc.window()
    assert [c['hw'] for c in cs] == [(1, 1), (3, 5), (16, 64), (17, 65), (130, 200), (1, 32768), (32768, 1)]
    assert sorted(len(c['radius']) for c in cs) == [0, 1, 5, 255, 256, 257, 600]
    assert any((c['hw'][1] * 3) % 4 for c in cs) and {1, 2, 6, 64} <= set(np.concatenate([c['radius'] for c in cs]).tolist())
    t = sc.tables(cs, align=4)
    assert t['canvases'].shape == (7, 6) and t['total_tiles'] == sum(sc.tiles(*c['hw']) for c in cs) and all(off % 4 == 0 for off, _, _ in t['spans'])
    ends = np.concatenate([c['ends'] for c in cs])
    assert np.isnan(ends).any() and np.isinf(ends).any() and (np.abs(ends[np.isfinite(ends)]) == 1e9).any()
