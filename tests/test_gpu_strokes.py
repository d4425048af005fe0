"""The step pictures' strokes on the GPU: csrc/strokes.hip equals the plain restatement of the stroke rule (tests/stroke_cases.py, pinned
on the host in test_strokes_cpu.py) byte for byte, writes only the bytes of covered pixels and nothing outside the canvases;
`SceneRenderer.render(..., strokes=...)` is one launch more and no wait."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import footprint
import stroke_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IN = ('canvases', 'ends', 'colour', 'radius')
PREFILL = 0x5A


def _counter():
    spec = importlib.util.spec_from_file_location('bench_planogram_compare', os.path.join(ROOT, 'tools', 'bench_planogram_compare.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Atlas:
    def __init__(self, images, device):
        from cvpce_amd import rendering as rd
        rows, _ = rd.atlas_layout([im.shape[:2] for im in images])
        self.data = torch.from_numpy(np.concatenate([im.reshape(-1) for im in images])).to(device)
        self.rows = torch.tensor(rows, dtype=torch.int32).to(device)


def _before(t, seed=None):
    """the output buffer before the launch: the prefill pattern, or random bytes (a written byte then differs from the model's with
    probability 255 / 256 wherever the kernel paints what it should not)"""
    if seed is None:
        return np.full(t['out_bytes'], PREFILL, dtype=np.uint8)
    return np.random.RandomState(seed).randint(0, 256, t['out_bytes']).astype(np.uint8)


def _launch(cuda, t, before):
    from cvpce_amd import torch_ops_strokes  # noqa: F401
    d = {k: torch.from_numpy(t[k]).to(cuda) for k in IN}
    out = torch.from_numpy(before).to(cuda)
    torch.ops.cvpce_amd.strokes_draw(d['canvases'], t['total_tiles'], d['ends'], d['colour'], d['radius'], out)
    return out.cpu().numpy()


def _assert_same(got, want, t, what):
    for c, (off, h, w) in enumerate(t['spans']):
        a, b = got[off:off + h * w * 3].reshape(h, w, 3), want[off:off + h * w * 3].reshape(h, w, 3)
        bad = (a != b).any(axis=2)
        assert not bad.any(), (what, c, (h, w), int(bad.sum()), np.argwhere(bad)[:4].tolist(), a[bad][:4].tolist(), b[bad][:4].tolist())
    assert np.array_equal(got, want), (what, 'a byte between the canvases was written')


@pytest.fixture(scope='module')
def window():
    """the canvases and, per alignment, the launch's tables with the model's output over a random buffer -- computed once, never changed"""
    cs = sc.window()
    runs = {}
    for align in (1, 4):
        t = sc.tables(cs, align=align)
        before = _before(t, seed=40 + align)
        runs[align] = (t, before, sc.run_model(cs, t, before))
    return cs, runs


def test_the_kernel_equals_the_model_byte_for_byte(cuda, window):
    cs, runs = window
    for align, (t, before, want) in runs.items():     # back to back (rows at odd addresses: byte stores) and at dword offsets
        assert (want != before).any()
        _assert_same(_launch(cuda, t, before), want, t, f'align {align}')
    # something of every canvas with strokes was painted, and most of the large canvases was not
    t, before, want = runs[4]
    for c, (off, h, w) in enumerate(t['spans']):
        changed = (want[off:off + h * w * 3] != before[off:off + h * w * 3]).reshape(h, w, 3).any(axis=2)
        assert changed.any() == (len(cs[c]['radius']) > 0), c
    assert not (want[t['spans'][4][0]:][:130 * 200 * 3] != before[t['spans'][4][0]:][:130 * 200 * 3]).all()


def test_overlapping_strokes_in_both_list_orders(cuda):
    """two crossing strokes and the same two in the other order, a chunk apart as well: the last of the list wins"""
    a, b = ((3.0, 8.0, 60.0, 8.0), 0x0000FF, 4), ((30.0, 0.0, 30.0, 16.0), 0xFF0000, 4)
    filler = [((200.0, 200.0, 210.0, 200.0), 0x00FF00, 2)] * 300                              # (outside the canvas: crosses the chunk boundary)
    for name, strokes, top in (('a b', [a, b], 0xFF0000), ('b a', [b, a], 0x0000FF), ('a ... b', [a] + filler + [b], 0xFF0000),
                               ('b ... a', [b] + filler + [a], 0x0000FF)):
        cs = [dict(hw=(16, 64), ends=np.array([s[0] for s in strokes], dtype=np.float32), colour=np.array([s[1] for s in strokes], dtype=np.int32),
                   radius=np.array([s[2] for s in strokes], dtype=np.int32))]
        t = sc.tables(cs)
        before = _before(t)
        got = _launch(cuda, t, before)
        _assert_same(got, sc.run_model(cs, t, before), t, name)
        assert got.reshape(16, 64, 3)[8, 30].tolist() == sc.rgb_bytes(top).tolist(), name


def test_a_canvas_launched_alone_gives_the_bytes_it_gives_inside_the_window(cuda, window):
    cs, runs = window
    t_all, _, want_all = runs[4]
    for c in range(len(cs)):
        t = sc.tables(cs, only=[c], align=4)
        off, h, w = t_all['spans'][c]
        before = runs[4][1][off:off + h * w * 3].copy()                  # the bytes it had inside the window
        got = _launch(cuda, t, before)
        assert np.array_equal(got, want_all[off:off + h * w * 3]), f'canvas {c} alone'


def test_footprint_of_the_entry_point(cuda, window):
    """the output arena is prefilled: every byte of a covered pixel is written, no other byte of the canvases, none between them and none
    of the guard bands; the strokes and the table sit between guard bands whose fill never reaches a pixel"""
    from cvpce_amd import torch_ops_strokes  # noqa: F401
    cs, _ = window
    t = sc.tables(cs, align=4)
    before = _before(t)
    model = sc.run_model(cs, t, before)
    ins = {k: footprint.put(torch.from_numpy(t[k]), cuda) for k in IN}
    out = footprint.out((t['out_bytes'],), torch.uint8, cuda)
    run = lambda: torch.ops.cvpce_amd.strokes_draw(ins['canvases'][0], t['total_tiles'], ins['ends'][0], ins['colour'][0], ins['radius'][0], out[0])
    # a covered pixel whose colour byte IS the prefill pattern cannot be told from an unwritten one: `may` is every byte of a covered
    # pixel, `must` those the model changes; the comparison below covers the rest
    may = np.zeros(t['out_bytes'], dtype=bool)
    for c, (off, h, w) in zip(cs, t['spans']):
        hit = np.zeros((h, w), dtype=bool)
        for k in range(len(c['radius'])):
            win = sc.covered((h, w), c['ends'][k], c['radius'][k])
            if win is not None:
                hit[win[0]:win[0] + win[2].shape[0], win[1]:win[1] + win[2].shape[1]] |= win[2]
        may[off:off + h * w * 3] = np.repeat(hit.reshape(-1), 3)
    must = model != before
    assert must.any() and not may.all() and not (must & ~may).any()
    res = footprint.check(run, list(ins.values()), [out], written=[(torch.from_numpy(must), torch.from_numpy(may))])
    assert np.array_equal(res[0].cpu().numpy(), model)


def test_strokes_are_one_launch_more_and_no_wait(cuda, window):
    from cvpce_amd import rendering as rd
    cs, runs = window
    pick = [1, 2, 3, 4]                                               # (3 x 5, one tile, one pixel over, 130 x 200)
    image = np.random.RandomState(8).randint(0, 256, (8, 8, 3)).astype(np.uint8)
    renderer = rd.SceneRenderer(_Atlas([image], cuda))
    hws = [cs[c]['hw'] for c in pick]
    whole = [rd._items(torch.tensor([[0.0, 0, w, h]]), 0, 0, 0).to(cuda) for h, w in hws]                # the atlas image over the whole canvas
    strokes = [rd.Strokes(*(torch.from_numpy(cs[c][k]).to(cuda) for k in ('ends', 'colour', 'radius'))) for c in pick]
    strokes[0] = None                                                 # a canvas without strokes keeps the compositor's bytes
    renderer.render(whole, hws, strokes=strokes)                      # (allocator)
    plain = [v.cpu().numpy() for v in renderer.render(whole, hws)]
    torch.cuda.synchronize()
    counts = []
    for kw in (dict(), dict(strokes=strokes), dict(strokes=[None] * 4)):
        with _counter().WindowCounter() as n:
            views = renderer.render(whole, hws, **kw)
        counts.append((n.kernels, n.waits))
    print(f'render: {counts[0]}; with strokes: {counts[1]}; with empty stroke lists: {counts[2]} (launches, waits)')
    assert counts == [(1, 0), (2, 0), (1, 0)]
    views = renderer.render(whole, hws, strokes=strokes)
    assert len({v.untyped_storage().data_ptr() for v in views}) == 1                      # views of one flat buffer, drawn on in place
    assert np.array_equal(views[0].cpu().numpy(), plain[0])
    for v, base, c in list(zip(views, plain, pick))[1:]:
        want = sc.paint(base.copy(), cs[c]['ends'], cs[c]['colour'], cs[c]['radius'])
        assert np.array_equal(v.cpu().numpy(), want) and not np.array_equal(want, base), c
    with pytest.raises(ValueError):
        renderer.render(whole, hws, strokes=strokes[:2])


def test_the_op_refuses_bad_calls_before_any_launch(cuda, window):
    from cvpce_amd import torch_ops_strokes  # noqa: F401
    cs, _ = window
    t = sc.tables(cs, only=[2, 3], align=4)
    d = {k: torch.from_numpy(t[k]).to(cuda) for k in IN}
    out = torch.full((t['out_bytes'],), PREFILL, dtype=torch.uint8, device=cuda)
    order = ('canvases', 'total_tiles', 'ends', 'colour', 'radius', 'out')
    good = dict(d, total_tiles=t['total_tiles'], out=out)
    call = lambda **kw: torch.ops.cvpce_amd.strokes_draw(*[dict(good, **kw)[k] for k in order])
    call()
    torch.cuda.synchronize()
    snap = out.clone()
    for bad in (dict(canvases=d['canvases'].to(torch.int32)), dict(canvases=d['canvases'][:, :5].contiguous()), dict(canvases=d['canvases'].reshape(-1)),
                dict(ends=d['ends'].double()), dict(ends=d['ends'][:-1]), dict(ends=d['ends'].t().contiguous().t()), dict(ends=d['ends'].reshape(-1)),
                dict(colour=d['colour'].to(torch.int64)), dict(colour=d['colour'][:-1]), dict(radius=d['radius'][:-1]), dict(radius=d['radius'].float()),
                dict(out=out.view(-1, 3)), dict(out=out.to(torch.int32)), dict(total_tiles=-1), dict(total_tiles=2 ** 31)):
        with pytest.raises(RuntimeError, match='cvpce_strokes_draw'):
            call(**bad)
    torch.cuda.synchronize()
    assert torch.equal(out, snap)
    # a table that points outside the buffer draws nothing; so does a launch without strokes or canvases
    table = d['canvases'].clone()
    table[:, 1] += t['out_bytes']
    call(canvases=table)
    call(ends=d['ends'][:0], colour=d['colour'][:0], radius=d['radius'][:0])
    call(canvases=d['canvases'][:0], total_tiles=0)
    torch.cuda.synchronize()
    assert torch.equal(out, snap)
