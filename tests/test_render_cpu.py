"""The picture rule of DESIGN.md 4b on the host: the numpy model of tests/render_cases.py does what the rule says, the item builders
of cvpce_amd/rendering.py make the lists the pictures are described by, and the atlas's size arithmetic holds.  (The kernel against
the model: test_gpu_render.py.)"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import abi
import render_cases as rc
import report_cases as rp
from test_report_cpu import StubClassifier, _scenes, host_ops  # noqa: F401  (host_ops: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the twelve shapes of the comparison with F.interpolate: source (h, w) -> box (h, w), from 1x1 to 256x256, enlarged and reduced
SHAPES = (((1, 1), (1, 1)), ((1, 1), (40, 37)), ((2, 3), (64, 96)), ((7, 5), (256, 256)), ((16, 16), (17, 15)), ((64, 48), (256, 200)),
          ((256, 256), (1, 1)), ((256, 256), (128, 128)), ((256, 256), (100, 77)), ((255, 129), (31, 200)), ((33, 256), (256, 33)), ((256, 256), (256, 256)))


def _content(kind, h, w, seed):
    if kind == 'random':
        return np.random.RandomState(seed).randint(0, 256, (h, w, 3)).astype(np.uint8)
    yy, xx = np.mgrid[:h, :w]
    return np.repeat((((yy + xx) & 1) * 255).astype(np.uint8)[:, :, None], 3, axis=2)


def test_the_model_gives_the_source_back_at_equal_size():
    for k, (h, w) in enumerate(((1, 1), (1, 256), (256, 1), (37, 53), (256, 256))):
        s = _content('random', h, w, k)
        assert np.array_equal(rc.resample(s, h, w), s), (h, w)


def test_the_model_gives_the_rounded_box_average_at_an_exact_halving():
    for k, (h, w) in enumerate(((2, 2), (8, 6), (256, 256), (2, 256))):
        s = _content('random', h, w, 10 + k).astype(np.int64)
        want = (s[0::2, 0::2] + s[0::2, 1::2] + s[1::2, 0::2] + s[1::2, 1::2] + 2) >> 2
        assert np.array_equal(rc.resample(s.astype(np.uint8), h // 2, w // 2), want.astype(np.uint8)), (h, w)


def test_the_model_stays_within_two_and_a_half_levels_of_float64_interpolate():
    """the derived bound: each axis' fraction is cut to 8 bits (below 255/256 of a level each at full contrast), the result rounded (0.5)"""
    worst = 0.0
    for k, ((sh, sw), (bh, bw)) in enumerate(SHAPES):
        for kind in ('random', 'checkerboard'):
            s = _content(kind, sh, sw, 20 + k)
            ref = F.interpolate(torch.from_numpy(s).permute(2, 0, 1)[None].to(torch.float64), size=(bh, bw), mode='bilinear', align_corners=False)[0]
            got = torch.from_numpy(rc.resample(s, bh, bw)).permute(2, 0, 1).to(torch.float64)
            diff = float((got - ref).abs().max())
            print(f'{sh}x{sw} -> {bh}x{bw} {kind}: largest difference {diff:.3f} levels')
            worst = max(worst, diff)
            assert diff < 2.5, ((sh, sw), (bh, bw), kind, diff)
    print(f'largest difference over the twelve shapes: {worst:.3f} levels')


def _paint8(items, atlas=(), base=None, background=0):
    box, src, colour, thickness = rc._arrays(items)
    return rc.paint((8, 8), box, src, colour, thickness, list(atlas), base, background)


def test_the_model_obeys_ordering_ring_and_skip_on_hand_written_cases():
    red, green = 0x0000FF, 0x00FF00
    R, G, Z = [255, 0, 0], [0, 255, 0], [0, 0, 0]
    flat = lambda v: np.full((2, 2, 3), v, dtype=np.uint8)
    # the last item wins; nothing inside lets earlier items show through, its ring does not
    c = _paint8([((1, 1, 7, 7), 0, red, 0), ((2, 2, 6, 6), rc.SRC_NONE, green, 1)], atlas=[flat(9)])
    want = np.zeros((8, 8, 3), dtype=np.uint8)
    want[1:7, 1:7] = 9
    want[2:6, 2:6] = G
    want[3:5, 3:5] = 9
    assert np.array_equal(c, want)
    # a ring of thickness 1 around a source; a thickness of half the box is the box; thickness 0 and nothing inside paints nothing
    c = _paint8([((0, 0, 4, 4), 0, red, 1), ((4, 4, 8, 8), 0, green, 2), ((0, 4, 4, 8), rc.SRC_NONE, green, 0)], atlas=[flat(7)])
    want = np.zeros((8, 8, 3), dtype=np.uint8)
    want[0:4, 0:4] = R
    want[1:3, 1:3] = 7
    want[4:8, 4:8] = G
    assert np.array_equal(c, want)
    # fractional coordinates: floor of the near side, ceil of the far side; a box half out of the canvas is cut, not squeezed
    ramp = np.zeros((1, 4, 3), dtype=np.uint8)
    ramp[0, :, 0] = [10, 20, 30, 40]
    c = _paint8([((1.5, 0.2, 2.1, 0.9), rc.SRC_NONE, red, 1), ((6, 3, 10, 4), 0, 0, 0)], atlas=[ramp])
    want = np.zeros((8, 8, 3), dtype=np.uint8)
    want[0, 1:3] = R
    want[3, 6:8, 0] = [10, 20]
    assert np.array_equal(c, want)
    # skipped: not finite, zero and negative extents, a source the atlas does not have, the base of a canvas without one
    nan, inf = float('nan'), float('inf')
    skipped = [((nan, 0, 4, 4), 0, red, 1), ((0, 0, inf, 4), 0, red, 1), ((0, -inf, 4, 4), 0, red, 1), ((3, 0, 3, 4), 0, red, 1), ((5, 0, 2, 4), 0, red, 1),
               ((0, 0, 8, 8), 1, red, 0), ((0, 0, 8, 8), 6, red, 0), ((0, 0, 8, 8), -3, red, 0), ((0, 0, 8, 8), rc.SRC_BASE, red, 0)]
    assert np.array_equal(_paint8(skipped, atlas=[flat(5)], background=0x030201), np.full((8, 8, 3), [1, 2, 3], dtype=np.uint8))
    # the base at the canvas's size comes back unchanged; coordinates are clamped to [-32768, 32767] before the extents
    base = _content('random', 8, 8, 3)
    assert np.array_equal(_paint8([((0, 0, 8, 8), rc.SRC_BASE, 0, 0)], base=base), base)
    assert rc.extents((-1e9, -40000, 1e9, 40000)) == (-32768, -32768, 65535, 65535) and rc.extents((0.3, 0, 0.6, 1)) == (0, 0, 1, 1)


def test_the_window_holds_the_cases_it_is_named_for():
    win = rc.window()
    cs = win['canvases']
    assert [c['hw'] for c in cs][:2] == [(1, 1), (5, 7)] and {c['hw'][1] for c in cs} >= {63, 64, 65, 67}
    assert sorted(len(c['src']) for c in cs)[:6] == [0, 1, 12, 255, 256, 257] and max(len(c['src']) for c in cs) == 600
    assert any(rc.tiles(*c['hw']) >= 6 and c['hw'][0] > 2 * rc.TILE_H for c in cs)
    rows = len(win['atlas'])
    src = np.concatenate([c['src'] for c in cs])
    assert {rows, rows + 5, -3, rc.SRC_NONE, rc.SRC_BASE} <= set(src.tolist())
    assert any(c['base'] is None and rc.SRC_BASE in c['src'].tolist() for c in cs)
    assert any(c['base'] is not None and c['base'].shape[:2] == c['hw'] for c in cs) and any(c['base'] is not None and c['base'].shape[:2] != c['hw'] for c in cs)
    box = np.concatenate([c['box'] for c in cs])
    assert np.isnan(box).any() and np.isposinf(box).any() and np.isneginf(box).any()
    t = rc.tables(win)
    assert t['canvases'].shape == (len(cs), rc.COLS) and t['total_tiles'] == sum(rc.tiles(*c['hw']) for c in cs)
    # the stack: the last of 257 items on one pixel shows
    got = rc.run_model(win, only=[4])[0]
    assert got[3, 64].tolist() == [0x56, 0x34, 0x12]
    # every canvas shows more than its background: the cases are visible
    for c, img in zip(cs[1:], rc.run_model(win)[1:]):
        assert (img != rc.rgb_bytes(win['background'])).any(), c['hw']


# ---------------------------------------------------------------------------------------------------------------------
# the item builders, on CPU tensors
# ---------------------------------------------------------------------------------------------------------------------
def test_observed_and_expected_items():
    from cvpce_amd import rendering as rd
    boxes = torch.tensor([[1.0, 2, 30, 40], [5, 5, 9, 9], [0, 0, 3, 3]])
    it = rd.observed_items(boxes, torch.tensor([7, -1, 0]))
    assert torch.equal(it.box, boxes) and it.box.dtype == torch.float32
    assert it.src.tolist() == [7, -1, 0] and it.thickness.tolist() == [0, 1, 0] and it.colour.tolist() == [rd.BLACK] * 3
    assert all(t.dtype == torch.int32 for t in (it.src, it.colour, it.thickness)) and len(it) == 3
    assert len(rd.observed_items(torch.zeros(0, 4), torch.zeros(0, dtype=torch.int64))) == 0
    # the planogram mapped into its canvas: (b - origin) * scale, two fp32 operations, the aspect ratio kept
    plano = torch.tensor([[20.0, 30, 84, 126], [92, 30, 156, 126], [20, 150, 84, 246]])
    assert rd.expected_canvas_hw(plano, 300) == (-(-300 * 216 // 136), 300)
    hw = rd.expected_canvas_hw(plano, 300)
    ex = rd.expected_items(plano, torch.tensor([2, -1, 5]), hw)
    scale = torch.minimum(torch.tensor(300.0) / torch.tensor(136.0), torch.tensor(float(hw[0])) / torch.tensor(216.0))
    want = (plano - torch.tensor([20.0, 30, 20, 30])) * scale
    assert torch.equal(ex.box, want) and ex.src.tolist() == [2, -1, 5] and ex.thickness.tolist() == [0, 1, 0]
    assert float(ex.box[:, 2].max()) <= 300 and float(ex.box[:, 3].max()) <= hw[0] and float(ex.box.min()) == 0.0
    assert rd.expected_canvas_hw(torch.zeros(0, 4), 64) == (64, 64)


def test_annotation_items_follow_the_report(host_ops):  # noqa: F811
    from cvpce_amd import production, rendering as rd
    cmp = production.PlanogramComparator()
    codes = set()
    for k, (expected, actual, image, clf) in enumerate(_scenes()):
        rep = cmp.report(expected, actual, image, clf)
        assert rep.status == 'ok'
        it = rd.annotation_items(rep, actual['boxes'], thickness=4, canvas_hw=(700, 900))
        outcomes = rep.outcomes.tolist()
        codes |= set(outcomes)
        drawn = [i for code in range(5) if code != rd.OUT_OF_VIEW for i, c in enumerate(outcomes) if c == code]
        n_stray = len(rep.stray)
        assert len(it) == 1 + n_stray + len(drawn), k
        assert it.src.tolist() == [rd.R.SRC_BASE] + [rd.R.SRC_NONE] * (len(it) - 1) and it.box[0].tolist() == [0, 0, 900, 700]
        assert it.thickness.tolist() == [0] + [4] * (len(it) - 1)
        assert torch.equal(it.box[1:1 + n_stray], actual['boxes'][rep.stray]) and it.colour[1:1 + n_stray].tolist() == [rd.STRAY_COLOUR] * n_stray
        assert torch.equal(it.box[1 + n_stray:], rep.expected_positions[drawn])
        assert it.colour[1 + n_stray:].tolist() == [rd.OUTCOME_COLOURS[rep.OUTCOMES[outcomes[i]]] for i in drawn]
    assert codes == {rp.DETECTED, rp.RECOVERED, rp.MISSING, rp.OUT_OF_VIEW, rp.UNCHECKED}
    assert set(rd.OUTCOME_COLOURS) == set(production.ComplianceReport.OUTCOMES) and len(set(rd.OUTCOME_COLOURS.values()) | {rd.STRAY_COLOUR}) == 6
    # a status that is not 'ok': the base alone
    expected, actual, (h, w) = rp.comparator_scene(0)
    none = {'boxes': torch.zeros(0, 4), 'labels': []}
    other = dict(actual, labels=['nothing_the_planogram_has'] * len(actual['labels']))
    for a, status in ((none, 'no_detections'), (other, 'no_matching')):
        rep = cmp.report(expected, a, torch.zeros(3, h, w), StubClassifier())
        assert rep.status == status
        it = rd.annotation_items(rep, a['boxes'], canvas_hw=(h, w))
        assert len(it) == 1 and it.src.tolist() == [rd.R.SRC_BASE] and it.box[0].tolist() == [0, 0, w, h]
    with pytest.raises(ValueError):
        rd.annotation_items(rep, a['boxes'])


def test_an_unknown_label_becomes_an_empty_rectangle():
    from cvpce_amd import rendering as rd
    rows = rd.label_rows(['b', 'a', 'b', 'c'])
    assert rows == {'b': 0, 'a': 1, 'c': 3}                       # the first gallery row per annotation
    got = rd.rows_of_labels(['a', 'nothing_the_gallery_has', 'c', 'b'], rows)
    assert got.tolist() == [1, -1, 3, 0] and got.dtype == torch.int32
    it = rd.observed_items(torch.tensor([[0.0, 0, 4, 4]] * 4), got)
    assert it.src.tolist() == [1, -1, 3, 0] and it.thickness.tolist() == [0, 1, 0, 0]


# ---------------------------------------------------------------------------------------------------------------------
# the atlas's arithmetic
# ---------------------------------------------------------------------------------------------------------------------
def test_reduced_sizes():
    from cvpce_amd import rendering as rd
    table = {(256, 256, 128): (128, 128), (256, 100, 128): (128, 50), (100, 256, 128): (50, 128), (128, 128, 128): (128, 128), (1, 1, 128): (1, 1),
             (129, 1, 128): (128, 1), (256, 1, 128): (128, 1), (255, 3, 128): (128, 2), (200, 150, 64): (64, 48), (256, 256, None): (256, 256),
             (256, 255, 1): (1, 1), (257, 128, 128): (128, 64), (300, 7, 128): (128, 3)}
    for (h, w, m), want in table.items():
        assert rd.reduced_hw(h, w, m) == want, (h, w, m)
        got = rd.reduced_hw(h, w, m)
        assert m is None or max(got) <= max(m, 1) and min(got) >= 1


def test_float_quantisation():
    from cvpce_amd import rendering as rd
    # a byte read as b / 255 * 2 - 1 (the gallery's float form) comes back as b; out-of-range values are clamped
    b = torch.arange(256, dtype=torch.float32)
    img = (b / 255 * 2 - 1).reshape(1, 16, 16).expand(3, 16, 16)
    assert torch.equal(rd.gallery_float_bytes(img)[:, :, 0].reshape(-1), torch.arange(256).to(torch.uint8))
    x = torch.tensor([-3.0, -1.0, -0.999, 0.0, 0.5, 1.0, 7.0]).reshape(1, 1, 7).expand(3, 1, 7)
    want = [max(0, min(255, int(np.floor((np.float32(np.float32(v * np.float32(0.5)) + np.float32(0.5))) * np.float32(255) + np.float32(0.5))))) for v in x[0, 0].tolist()]
    assert rd.gallery_float_bytes(x)[0, :, 1].tolist() == want and want[0] == 0 and want[-1] == 255 and want[3] == 128
    planes = (b / 255).reshape(1, 16, 16).expand(3, 16, 16)
    assert torch.equal(rd.float_image_bytes(planes)[:, :, 2].reshape(-1), torch.arange(256).to(torch.uint8))
    assert rd.float_image_bytes(torch.tensor([-1.0, 2.0, 0.5]).reshape(1, 1, 3).expand(3, 1, 3))[0, :, 0].tolist() == [0, 255, 128]
    assert rd.float_image_bytes(planes).shape == (16, 16, 3)


def test_an_oversize_atlas_is_refused_by_the_size_arithmetic():
    from cvpce_amd import rendering as rd
    rows, total = rd.atlas_layout([(2, 3), (1, 1), (256, 256)])
    assert rows == [(0, 2, 3), (18, 1, 1), (21, 256, 256)] and total == 21 + 196608
    n = (2 ** 31 - 1) // 196608                       # 10 922 images of 256 x 256 fit
    assert rd.atlas_layout([(256, 256)] * n)[1] == n * 196608
    with pytest.raises(ValueError, match='int32'):
        rd.atlas_layout([(256, 256)] * (n + 1))
    assert 3200 * 128 * 128 * 3 <= 157.3e6 and 3200 * 256 * 256 * 3 <= 629.2e6          # the figures of the docstring


# ---------------------------------------------------------------------------------------------------------------------
# the header, the binding and the op
# ---------------------------------------------------------------------------------------------------------------------
def test_render_header_is_exported_and_mirrored():
    """(exported, bound, compared argument by argument and disjoint from the other headers: test_abi_mirror_cpu.py)"""
    from cvpce_amd import torch_ops_render as R
    text = open(os.path.join(abi.INCLUDE, 'cvpce_amd_render.h')).read()
    assert list(abi.declarations('cvpce_amd_render.h')) == ['cvpce_render_canvases']
    defines = dict(re.findall(r'#define\s+(CVPCE_RENDER_\w+)\s+\(?(-?\d+)\)?\s', text))
    assert (int(defines['CVPCE_RENDER_TILE_W']), int(defines['CVPCE_RENDER_TILE_H'])) == (R.TILE_W, R.TILE_H) == (rc.TILE_W, rc.TILE_H)
    assert int(defines['CVPCE_RENDER_MAX_SIDE']) == R.MAX_SIDE == rc.MAX_SIDE and int(defines['CVPCE_RENDER_TABLE_COLS']) == R.TABLE_COLS == rc.COLS
    assert (int(defines['CVPCE_RENDER_SRC_NONE']), int(defines['CVPCE_RENDER_SRC_BASE'])) == (R.SRC_NONE, R.SRC_BASE) == (rc.SRC_NONE, rc.SRC_BASE)
    assert int(defines['CVPCE_RENDER_CHUNK']) == rc.CHUNK and R.tiles(17, 65) == 4 == rc.tiles(17, 65)


def test_the_render_op_has_its_own_name_and_is_gpu_only():
    from cvpce_amd import torch_ops_render  # noqa: F401  (registers the op; name and keys: test_abi_mirror_cpu.py)
    z = lambda *s, dt=torch.int32: torch.zeros(*s, dtype=dt)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.cvpce_amd.render_canvases(z(1, 10, dt=torch.int64), 1, None, z(0, 4, dt=torch.float32), z(0), z(0), z(0), z(0, dt=torch.uint8), z(0, 3),
                                            0, z(3, dt=torch.uint8))


def test_the_entry_point_rejects_bad_arguments_on_the_host():
    """negative sizes, null pointers with non-zero counts: CVPCE_ERR_ARG before any launch (no GPU is touched)"""
    from cvpce_amd._lib import lib
    P, N = ctypes.c_void_p(4096), ctypes.c_void_p(0)          # (never dereferenced: every call below is refused or has nothing to do)
    good = dict(canvases=P, C=1, total_tiles=1, out=P, out_bytes=3, base=N, base_bytes=0, box=P, src=P, colour=P, thickness=P, n_items=1, atlas=P,
                atlas_bytes=3, atlas_rows=P, rows=1, background=0, stream=N)
    call = lambda **kw: lib.cvpce_render_canvases(*dict(good, **kw).values())
    assert call(C=0) == 0 and call(total_tiles=0) == 0                                    # nothing to do
    for bad in (dict(C=-1), dict(total_tiles=-1), dict(total_tiles=2 ** 31), dict(out_bytes=-1), dict(base_bytes=-1), dict(n_items=-1), dict(atlas_bytes=-1),
                dict(rows=-1), dict(canvases=N), dict(canvases=ctypes.c_void_p(4100)), dict(out=N), dict(base_bytes=5), dict(box=N), dict(src=N),
                dict(colour=N), dict(thickness=N), dict(box=ctypes.c_void_p(4104)), dict(atlas=N), dict(atlas_rows=N)):
        assert call(**bad) == 1, bad


def test_the_evaluator_and_the_cli_have_the_picture_entry_points():
    from cvpce_amd import production
    for name in ('pictures', 'pictures_batch', 'pictures_iter'):
        assert callable(getattr(production.PlanogramEvaluator, name))
    from click.testing import CliRunner
    from cvpce_amd.cli import cli, _RenderCommand, _ReportCommand
    assert issubclass(_RenderCommand, _ReportCommand) and isinstance(cli.commands['eval-planograms'], _RenderCommand)
    text = CliRunner().invoke(cli, ['rebuild-scene', '--help']).output
    for option in ('--img-dir', '--test-imgs', '--test-annotations', '--planograms', '--datatype', '--load-classifier-index', '--plano-idx', '--out',
                   'GLN_STATE', 'DIHE_STATE'):
        assert option in text, option
    assert '--render DIR' in CliRunner().invoke(cli, ['eval-planograms', '--help']).output
    dirs = [a for o in ('--img-dir', '--test-imgs', '--test-annotations', '--planograms') for a in (o, ROOT)]
    missing = CliRunner().invoke(cli, ['rebuild-scene', *dirs, __file__, __file__])
    assert missing.exit_code == 2 and '--out' in missing.output                  # required: there is no window to show
    assert CliRunner().invoke(cli, ['eval-planograms', '--render']).exit_code == 2
