"""The typed work-list schedule on the host: `ops.SkipMode` / `ops.SkipLayer` against the C header's struct, the `ops.WorkLists`
accessors against the packed layout of include/cvpce_amd.h written out by hand, and `MACVGGEngine.skip_plan`'s cache key."""
import torch


def test_skip_mode_and_layer_are_the_headers():
    from cvpce_amd import _lib, ops
    assert [int(m) for m in ops.SkipMode] == [0, 1, 2, 3, 4, 5]
    assert [m.has_strips for m in ops.SkipMode] == [False, False, False, True, False, True]
    assert [m.has_thin for m in ops.SkipMode] == [False] * 5 + [True]
    assert list(ops.SkipLayer._fields) == [name for name, _ in _lib.SkipLayer._fields_]
    l = ops.skip_layer(32, 32, 16, 16, 7, 64, 64, 6, ops.SkipMode.ROWS4_STRIPS)
    assert list(l) == [32, 32, 16, 16, 7, 64, 64, 6, 3] and all(type(v) is int for v in l) and l[-1] == 3
    h, w, th, tw, out_ops, ih, iw, in_ops, skip = l
    assert l.mode is ops.SkipMode.ROWS4_STRIPS and l._replace(skip=5).mode.has_thin and (l.in_H, l.skip) == (ih, skip)


def _same_view(a, b):
    return a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride() and torch.equal(a, b)


def test_worklists_accessors_follow_the_packed_layout():
    from cvpce_amd import ops
    L, stride = 4, 10
    M = ops.SkipMode
    # with thin lists: lists (3 L, stride), counts (4 L,)
    lists, counts = torch.arange(3 * L * stride).reshape(3 * L, stride), torch.arange(4 * L, dtype=torch.int32)
    wl = ops.WorkLists(lists, counts, torch.arange(L * 3 * 2).reshape(L, 3, 2))
    assert wl.n_layers == L
    for j in range(L):
        for got, row, slot in ((wl.main(j), j, j), (wl.strips(j), L + j, 2 * L + j), (wl.thin(j), 2 * L + j, 3 * L + j)):
            assert _same_view(got[0], lists[row]) and _same_view(got[1], counts[slot:slot + 1]), (j, row, slot)
        assert _same_view(wl.units(j), counts[L + j:L + j + 1]) and _same_view(wl.computed_of(j), wl.computed[j])
    for mode in M:
        assert (wl.strips(1, mode) is not None) == (mode in (M.ROWS4_STRIPS, M.ROWS2_STRIPS_THIN))
        assert (wl.thin(1, mode) is not None) == (mode is M.ROWS2_STRIPS_THIN)
    assert _same_view(wl.strips(1, M.ROWS4_STRIPS)[0], lists[L + 1]) and _same_view(wl.thin(1, M.ROWS2_STRIPS_THIN)[1], counts[3 * L + 1:3 * L + 2])
    # without: lists (2 L, stride), counts (3 L,)
    lists, counts = lists[:2 * L], counts[:3 * L]
    wl = ops.WorkLists(lists, counts, None)
    assert wl.n_layers == L and wl.computed is None
    for j in range(L):
        for got, row, slot in ((wl.main(j), j, j), (wl.strips(j), L + j, 2 * L + j)):
            assert _same_view(got[0], lists[row]) and _same_view(got[1], counts[slot:slot + 1]), (j, row, slot)
        assert _same_view(wl.units(j), counts[L + j:L + j + 1])
        assert wl.thin(j) is None and wl.thin(j, M.ROWS2_STRIPS_THIN) is None and wl.strips(j, M.ROWS2) is None
    lists_, counts_, computed_ = wl                              # (still the three tensors `embed_worklists` filled)
    assert lists_ is lists and counts_ is counts and computed_ is None


def test_skip_plan_follows_every_switch_it_reads():
    """`skip_plan` caches under every switch it reads: with `ops.USE_FUSED_MAC` flipped on a live engine there is no work-list schedule
    (a stand-alone descriptor), and flipped back there is one again."""
    from cvpce_amd import ops, synthetic
    from cvpce_amd.models import classification as C
    eng = C.MACVGGEngine(synthetic.synthetic_macvgg(seed=1), torch.device('cpu'))
    sched = eng.skip_plan(256)
    assert isinstance(sched, C.SkipSchedule) and sched._fields == ('steps', 'layers', 'pool_mask') and eng.will_skip(256)
    old, ops.USE_FUSED_MAC = ops.USE_FUSED_MAC, False
    try:
        assert eng.skip_plan(256) is None and not eng.will_skip(256)
    finally:
        ops.USE_FUSED_MAC = old
    assert eng.skip_plan(256) is sched
    # the typed steps: five fields for the stem too, the MAC descriptor offset and the early / late split derived here
    steps, layers, pool_mask = sched
    assert all(len(st[:5]) == 5 and st._fields[:5] == ('kind', 'pc', 'pool', 'mac', 'store') for st in steps) and steps[0][:5] == ('stem', None, True, False, True)
    assert [st.mac_off for st in steps if st.mac] == [0, 512] and sched.early == 3
    assert all(isinstance(l, ops.SkipLayer) for l in layers)
