"""CPU-side checks of the device detections path (no compute on a GPU): the numpy restatement of the detections rule
(tests/actuals_cases.py) equals `production._nondegenerate` plus `planograms_device.graph_threshold` bit for bit on the shared case
set; the case set has the properties the GPU tests rely on; the expected side's label ids; the kernels' header, signature table and
torch ops stay apart from every other table and refuse CPU tensors; the switches."""
import ctypes

import numpy as np
import pytest
import torch

import abi
import actuals_cases as ac


def _classifier(monkeypatch, annotations):
    """a Classifier over an index that is never used as one: the device gallery's two ops are stood in for, the id space is real"""
    from cvpce_amd import production
    monkeypatch.setattr(production.ops, 'pad_features', lambda x: x)
    monkeypatch.setattr(production.ops, 'row_norms', lambda g: None)
    return production.Classifier.from_embedding(None, torch.zeros(len(annotations), 4), annotations, device=torch.device('cpu'),
                                                emb_device=torch.device('cpu'))


# ---------------------------------------------------------------------------------------------------------------------
# the model against the host's own lines
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('k', ac.KS)
@pytest.mark.parametrize('thresh_size', ac.THRESH_SIZES)
def test_the_model_is_the_host_path_bit_for_bit(monkeypatch, k, thresh_size):
    from cvpce_amd import planograms_device as pd, production
    clf = _classifier(monkeypatch, ac.ANNOTATIONS)
    ids, gallery_ids = ac.label_ids()
    assert clf.label_ids == ids and clf.gallery_label_id.tolist() == gallery_ids.tolist()
    indices = ac.make_indices(k)
    assert ac.model_count(ac.BOXES, ac.COUNT).tolist() == ac.KEPT.tolist()
    out_boxes, out_row, out_label, thresh, status, rows, tw = ac.model_pack(ac.BOXES, ac.COUNT, indices, gallery_ids, ac.OFF2, thresh_size)
    assert status.tolist() == [0] * ac.B and rows.all() and len(rows) == int(ac.KEPT.sum())
    for i, c in enumerate(ac.COUNTS):
        # what `detect_and_classify_batch` does with the same result: the prefix, the filter, one lookup per detection
        b, ix = torch.from_numpy(ac.BOXES[i, :c]), torch.from_numpy(indices[i, :c, 0])
        if c:
            ok = production._nondegenerate(b)
            assert ok.tolist() == ac.kept_mask(ac.BOXES[i, :c]).tolist()
            b, ix = b[ok], ix[ok]
        labels = [clf.annotations[r] for r in ix.tolist()]
        o0, o1 = int(ac.OFF2[i]), int(ac.OFF2[i + 1])
        assert o1 - o0 == len(b) == int(ac.KEPT[i])
        assert torch.equal(torch.from_numpy(out_boxes[o0:o1]).view(torch.int32), b.view(torch.int32))
        assert out_row[o0:o1].tolist() == ix.tolist()
        assert out_label[o0:o1].tolist() == [clf.label_ids[l] for l in labels]
        assert [clf.annotations[r] for r in out_row[o0:o1]] == labels
        assert bool(tw[i]) == (len(b) > 0)
        if len(b):
            want = pd.graph_threshold(b, thresh_size)
            assert want.dtype == torch.float32
            assert torch.from_numpy(thresh[i:i + 1]).view(torch.int32).item() == want.reshape(1).view(torch.int32).item(), (i, thresh[i], want)


def test_the_case_set_has_the_stated_properties():
    assert ac.BOXES.shape == (8, 300, 4) and ac.BOXES.dtype == np.float32 and ac.COUNT.tolist() == [0, 1, 63, 64, 65, 256, 257, 300]
    assert ac.KEPT[ac.ALL_DEGENERATE] == 0 and ac.COUNTS[ac.ALL_DEGENERATE] > 0
    for i, c in enumerate(ac.COUNTS):
        assert np.isnan(ac.BOXES[i, c:]).all() and np.isfinite(ac.BOXES[i, :c]).all()
        for k in ac.KS:
            idx = ac.make_indices(k)
            assert (idx[i, c:] == -1).all() and (idx[i, :c] >= 0).all() and (idx[i, :c] < ac.G).all() and idx.shape == (8, 300, k)
        keep = ac.kept_mask(ac.BOXES[i, :c])
        assert (keep == ~ac.PLANTED[i, :c]).all()                              # every planted degenerate box is one, and no other
        if c >= 64 and i != ac.ALL_DEGENERATE:
            # degenerate boxes at irregular positions: in both halves of the first wave, and the gaps between them differ
            gaps = set(np.diff(np.nonzero(~keep)[0]).tolist())
            assert len(gaps) >= 3 and (~keep[:32]).any() and (~keep[32:64]).any() and keep[:64].any()
            for name, slot in ac.SPECIAL_SLOTS.items():
                box, kept = ac.SPECIAL[name]
                assert ac.BOXES[i, slot].tolist() == np.array(box, dtype=np.float32).tolist() and bool(keep[slot]) == kept, name
    one = np.array([ac.SPECIAL['width_one'][0]], dtype=np.float32)
    assert int(one[0, 2]) - int(one[0, 0]) == 1 and float(one[0, 2] - one[0, 0]) < 1
    zero = np.array([ac.SPECIAL['around_zero'][0]], dtype=np.float32)
    assert int(zero[0, 0]) == 0 == int(zero[0, 2]) and np.floor(zero[0, 0]) == -1             # truncation, not floor
    for t in ac.THRESH_SIZES:
        assert ac.order_sensitive_images(t)


def test_stale_offsets_and_rows_outside_the_gallery_are_reported_by_the_model():
    _, gallery_ids = ac.label_ids()
    indices = ac.make_indices(1)
    stale = ac.OFF2.copy()
    stale[4:] -= 3                                                             # image 3 is given three rows too few
    out = ac.model_pack(ac.BOXES, ac.COUNT, indices, gallery_ids, stale, 0.5)
    assert out[4].tolist() == [0, 0, 0, 1, 0, 0, 0, 0] and int(out[5].sum()) == int(ac.KEPT.sum()) - 3
    first = int(np.nonzero(ac.kept_mask(ac.BOXES[5, :256]))[0][0])
    indices[5, first, 0] = ac.G
    out = ac.model_pack(ac.BOXES, ac.COUNT, indices, gallery_ids, ac.OFF2, 0.5)
    assert out[4].tolist() == [0, 0, 0, 0, 0, 2, 0, 0] and out[1][ac.OFF2[5]] == -1 and out[2][ac.OFF2[5]] == 0


# ---------------------------------------------------------------------------------------------------------------------
# the expected side's label ids
# ---------------------------------------------------------------------------------------------------------------------
def test_expected_ids_are_equal_exactly_where_the_labels_are(monkeypatch):
    from cvpce_amd import planograms_device as pd
    clf = _classifier(monkeypatch, ['b', 'a', 'b', ('c', 1), 'a'])
    planos = [{'labels': ['a', 'zzz', ('c', 1), 'b', 'yyy', 'zzz']}, {'labels': ['yyy', 'a', 'a', 'a', 'www']}, {'labels': ['b']}]
    out = pd.expected_label_ids(planos, clf)
    ids = [v for e, _ in out for v in e]
    labels = [l for p in planos for l in p['labels']]
    assert len(ids) == len(labels) and all(isinstance(v, int) and v >= 0 for v in ids)
    for i, a in enumerate(labels):
        for j, b in enumerate(labels):
            assert (ids[i] == ids[j]) == (a == b), (a, b)
    # a label some gallery item has carries the classifier's id, every other one lies beyond the id space, ranked as it appears
    assert all((v == clf.label_ids[l]) if l in clf.label_ids else v >= len(clf.label_ids) for v, l in zip(ids, labels))
    assert [ids[labels.index(l)] - len(clf.label_ids) for l in ('zzz', 'yyy', 'www')] == [0, 1, 2]
    assert [m for _, m in out] == [2, 3, 1]                                    # the largest multiplicity of a label, per planogram
    # cached with the index generation; another window ranks the outside labels anew
    assert all(p[pd.IDS_KEY][0] == clf.index_generation for p in planos)
    again = pd.expected_label_ids(planos[1:], clf)
    assert again[0][0] == [3, 1, 1, 1, 4] and planos[1][pd.IDS_KEY][1] == [-1, 1, 1, 1, -1]
    clf.set_index(clf.embedding, ['yyy', 'a'])
    assert pd.expected_label_ids(planos[1:2], clf)[0][0] == [0, 1, 1, 1, 2] and planos[1][pd.IDS_KEY][0] == clf.index_generation
    assert pd.expected_label_ids([{'labels': ['a', ['unhashable']]}], clf) is None
    assert pd.expected_label_ids(planos, _classifier(monkeypatch, ['a', ['unhashable']])) is None


# ---------------------------------------------------------------------------------------------------------------------
# boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_actuals_header_is_exported_and_mirrored():
    """(exported, bound and disjoint from the other headers: test_abi_mirror_cpu.py)"""
    assert abi.header_symbols('cvpce_amd_actuals.h') == ['cvpce_actuals_count', 'cvpce_actuals_pack']


def test_actuals_ops_have_their_own_names_and_are_gpu_only():
    from cvpce_amd import torch_ops_actuals  # noqa: F401  (registers the ops; names and keys: test_abi_mirror_cpu.py)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.actuals_count(torch.zeros(1, 2, 4), i32(1), i32(1))
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.actuals_pack(torch.zeros(1, 2, 4), i32(1), torch.zeros(1, 2, 1, dtype=torch.int64), i32(4), i32(2), 0.5,
                                         torch.zeros(2, 4), i32(2), i32(2), torch.zeros(1), i32(1))


def test_entry_points_reject_bad_arguments_on_the_host():
    """sizes out of range, null and misaligned pointers: status 1, nothing launched; B = 0: status 0, nothing launched"""
    from cvpce_amd._lib import lib
    z, a = ctypes.c_void_p(0), ctypes.c_void_p(256)          # (never dereferenced: every call below returns before a launch)

    def count(b=1, per=4, **ptr):
        p = {n: ptr.get(n, a) for n in ('boxes', 'count', 'kept')}
        return lib.cvpce_actuals_count(p['boxes'], p['count'], b, per, p['kept'], z)

    def pack(b=1, per=4, k=1, g=4, sum2=4, **ptr):
        p = {n: ptr.get(n, a) for n in ('boxes', 'count', 'indices', 'gallery_label_id', 'off2', 'out_boxes', 'out_row', 'out_label', 'thresh', 'status')}
        return lib.cvpce_actuals_pack(p['boxes'], p['count'], p['indices'], k, p['gallery_label_id'], g, p['off2'], 0.5, b, per, sum2,
                                      p['out_boxes'], p['out_row'], p['out_label'], p['thresh'], p['status'], z)

    for call, names in ((count, ('boxes', 'count', 'kept')),
                        (pack, ('boxes', 'count', 'indices', 'gallery_label_id', 'off2', 'out_boxes', 'out_row', 'out_label', 'thresh', 'status'))):
        assert call(b=-1) == 1 and call(b=65536) == 1 and call(per=0) == 1 and call(boxes=ctypes.c_void_p(264)) == 1
        for n in names:
            assert call(**{n: z}) == 1, n
        assert call(b=0) == 0 and call(b=0, boxes=z, count=z) == 0
    assert pack(k=0) == 1 and pack(g=-1) == 1 and pack(sum2=-1) == 1 and pack(indices=ctypes.c_void_p(260)) == 1 and pack(out_boxes=ctypes.c_void_p(264)) == 1


# ---------------------------------------------------------------------------------------------------------------------
# the switches
# ---------------------------------------------------------------------------------------------------------------------
def test_the_evaluator_switch_is_off_by_default_and_needs_the_device_tail():
    from cvpce_amd import production
    cmp = production.PlanogramComparator
    ev = production.PlanogramEvaluator(None, None, cmp())
    assert ev.device_detections is False and ev.detections_host_routed == 0
    for bad in (cmp(), cmp(device_graphs=True), object()):
        with pytest.raises(ValueError, match='device_detections needs a comparator with device_graphs and device_tail'):
            production.PlanogramEvaluator(None, None, bad, device_detections=True)
    for good in (cmp(device_graphs=True, device_tail=True), cmp(device_graphs=True, device_tail=True, device_reclass=True)):
        assert production.PlanogramEvaluator(None, None, good, device_detections=True).device_detections is True
    import inspect
    assert inspect.signature(production.BatchedPipeline.run).parameters['actuals'].default is False


def test_the_cli_has_the_switch():
    from click.testing import CliRunner
    from cvpce_amd.cli import cli
    cmd = cli.commands['eval-planograms']
    assert not any('device' in p.name for p in cmd.params)
    text = ''.join(CliRunner().invoke(cli, ['eval-planograms', '--help']).output.split())
    assert '--device-detections/--no-device-detections' in text and text.count('[default:off]') >= 4
    alone = CliRunner().invoke(cli, ['eval-planograms', '--device-graphs', '--device-detections', 'a', 'b'])
    assert alone.exit_code == 2 and '--device-detections needs --device-tail' in alone.output
    off = CliRunner().invoke(cli, ['eval-planograms', '--device-graphs', '--device-tail', '--device-detections', '--no-device-tail', 'a', 'b'])
    assert off.exit_code == 2 and '--device-detections needs --device-tail' in off.output
    for more in ((), ('--device-reclass',)):                                  # (gets as far as the missing files)
        on = CliRunner().invoke(cli, ['eval-planograms', '--device-graphs', '--device-tail', *more, '--device-detections', 'a', 'b'])
        assert on.exit_code == 2 and 'needs --device' not in on.output
    none = CliRunner().invoke(cli, ['eval-planograms', '--device-detections', '--no-device-detections', 'a', 'b'])
    assert none.exit_code == 2 and 'needs --device' not in none.output
