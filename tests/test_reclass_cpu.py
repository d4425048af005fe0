"""CPU-side checks of the comparator's device re-classification (no compute on a GPU): the numpy restatement of the rule
(tests/reclass_cases.py) equals `PlanogramComparator._finish`'s own torch lines on random and edge inputs; the kernels' header,
signature table and torch ops stay apart from every other table and refuse CPU tensors; the switches and the label-id space."""
import ctypes

import numpy as np
import pytest
import torch

import abi
import reclass_cases as rc

SIZES = ((480, 640), (333, 517), (1, 1), (7, 1000), (2161, 3847))          # (h, w): not multiples of anything


def _bits(t):
    return torch.as_tensor(np.ascontiguousarray(t)).view(torch.int32)


# ---------------------------------------------------------------------------------------------------------------------
# the model against _finish's lines
# ---------------------------------------------------------------------------------------------------------------------
def test_edge_positions_are_what_they_are_named():
    for h, w in SIZES[:2]:
        pos, want = rc.edge_positions(h, w)
        got_pos, got = rc.finish_clamp_and_validity(pos, h, w)
        assert got.tolist() == want
        assert sum(want) >= 5 and len(want) - sum(want) >= 10
        # a width of exactly 1.0 after the clamp is invalid, nextafter(1, 2) is valid, a NaN stays a NaN and is invalid
        assert float(got_pos[3, 2] - got_pos[3, 0]) == 1.0 and not got[3]
        assert float(got_pos[5, 2] - got_pos[5, 0]) == float(np.nextafter(np.float32(1), np.float32(2))) and got[5]
        assert torch.isnan(got_pos[8, 0]) and torch.isnan(got_pos[12]).all() and not got[8:13].any()
        assert got_pos[0].tolist() == [0.0, 0.0, 0.0, 0.0] and got_pos[14].tolist() == [0.0, 0.0, float(w), float(h)]


def test_model_clamp_and_validity_equal_the_lines_of_finish():
    seen_valid = seen_invalid = 0
    for k, (h, w) in enumerate(SIZES):
        pos = torch.cat((rc.edge_positions(h, w)[0], rc.random_positions(600, h, w, 40 + k)))
        want_pos, want_valid = rc.finish_clamp_and_validity(pos, h, w)
        got_pos, got_valid = rc.clamp_and_validity(pos.numpy(), h, w)
        assert torch.equal(_bits(got_pos), want_pos.view(torch.int32)), (h, w)          # bit for bit: NaN payloads and -0 included
        assert got_valid.tolist() == want_valid.tolist(), (h, w)
        seen_valid += int(want_valid.sum())
        seen_invalid += int((~want_valid).sum())
    assert seen_valid >= 500 and seen_invalid >= 500


def test_model_plan_equals_finish_image_by_image():
    images = [rc.plan_image(n1, kind, h, w, 7 * n1 + k)
              for k, (n1, kind, (h, w)) in enumerate(((1, 'all_missing', SIZES[0]), (65, 'edges', SIZES[1]), (257, 'mixed', SIZES[0]),
                                                      (64, 'none_missing', SIZES[1]), (200, 'mixed', SIZES[4])))]
    images.append(rc.plan_image(30, 'all_missing', 480, 640, 5, status=rc.NONE))
    images.append(rc.plan_image(30, 'all_missing', 480, 640, 6, enabled=0))
    t, cap = rc.plan_tables(images)
    boxes, index, count, written = rc.model_plan(t['status'].numpy(), t['matched_expected'].numpy(), t['expected_positions'].numpy(),
                                                 t['off1'].tolist(), t['image'].tolist(), cap)
    assert cap == 257 and count[3] == 0 and count[5] == 0 and count[6] == 0 and count[0] + count[1] + count[2] + count[4] > 100
    for p, im in enumerate(images[:5]):
        missing = torch.where(im['matched'] == 0)[0]                                    # (finalize_result's missing_expected)
        pos, valid = rc.finish_clamp_and_validity(im['positions'][missing], im['h'], im['w'])
        assert count[p] == int(valid.sum()) and written[p].tolist() == [s < count[p] for s in range(cap)]
        assert index[p, :count[p]].tolist() == missing[valid].tolist()
        assert torch.equal(_bits(boxes[p, :count[p]]), pos[valid].view(torch.int32))


def test_model_verdict_equals_the_loop_of_finish():
    g = torch.Generator().manual_seed(3)
    gallery = [f'sku{i % 6}' for i in range(24)]
    ids = {}
    gallery_id = [ids.setdefault(a, len(ids)) for a in gallery]
    n1 = 90
    labels = [('other' if i % 7 == 0 else f'sku{i % 6}') for i in range(n1)]
    matched = (torch.rand(n1, generator=g) < 0.4)
    positions = rc.random_positions(n1, 480, 640, 11)
    missing = torch.where(~matched)[0]
    pos, valid = rc.finish_clamp_and_validity(positions[missing], 480, 640)
    nearest = torch.randint(0, 24, (int(valid.sum()), 3), generator=g)
    classified = [[gallery[j] for j in row] for row in nearest.tolist()]
    want_found, want = rc.finish_compare(matched, missing, [labels[i] for i in missing.tolist()], valid, classified)
    _, index, count, _ = rc.model_plan([rc.OK], matched.to(torch.int32).numpy(), positions.numpy(), [0, n1], [[480, 640, 1]], n1)
    slot_row = np.full((1, n1), -1, dtype=np.int32)
    slot_row[0, :count[0]] = np.arange(count[0])
    found, found_count, written = rc.model_verdict(index, count, slot_row, nearest.numpy(), gallery_id, [ids.get(l, -1) for l in labels],
                                                   matched.to(torch.int32).numpy(), [0, n1], [rc.OK], n1)
    assert written.all() and torch.equal(torch.from_numpy(found != 0), want_found)
    assert int(want_found.sum()) > int(matched.sum()) and not want_found.all()          # both outcomes occur
    verdict = torch.tensor(int(found_count[0])) / n1
    assert verdict.dtype == want.dtype == torch.float32 and float(verdict) == float(want) and verdict.shape == want.shape


# ---------------------------------------------------------------------------------------------------------------------
# boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_reclass_header_is_exported_and_mirrored():
    """(exported, bound and disjoint from the other headers: test_abi_mirror_cpu.py)"""
    assert abi.header_symbols('cvpce_amd_reclass.h') == ['cvpce_reclass_plan', 'cvpce_reclass_verdict']


def test_reclass_ops_have_their_own_names_and_are_gpu_only():
    from cvpce_amd import torch_ops_reclass  # noqa: F401  (registers the ops; names and keys: test_abi_mirror_cpu.py)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.reclass_plan(i32(1), i32(2), torch.zeros(2, 4), i32(2), i32(1, 3), torch.zeros(1, 2, 4), i32(1, 2), i32(1))
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.reclass_verdict(i32(1, 2), i32(1), i32(1, 2), torch.zeros(2, 1, dtype=torch.int64), i32(4), i32(2), i32(2), i32(2), i32(1),
                                            i32(2), i32(1))


def test_entry_points_reject_bad_arguments_on_the_host():
    """counts and cap out of range, null and misaligned pointers: status 1, nothing launched"""
    from cvpce_amd._lib import lib
    z, a = ctypes.c_void_p(0), ctypes.c_void_p(256)          # (never dereferenced: every call below returns before a launch)
    plan_names = ('status', 'matched_expected', 'expected_positions', 'off1', 'image')
    plan_outs = ('boxes', 'expected_index', 'count')
    verdict_names = ('expected_index', 'count', 'slot_row', 'indices', 'gallery_label_id', 'expected_label_id', 'matched_expected', 'off1', 'status')
    verdict_outs = ('found', 'found_count')

    def plan(b=1, s1=4, cap=4, **ptr):
        p = {n: ptr.get(n, a) for n in plan_names + plan_outs}
        return lib.cvpce_reclass_plan(*[p[n] for n in plan_names], b, s1, cap, *[p[n] for n in plan_outs], z)

    def verdict(b=1, s1=4, cap=4, m=4, k=1, g=4, **ptr):
        p = {n: ptr.get(n, a) for n in verdict_names + verdict_outs}
        return lib.cvpce_reclass_verdict(*[p[n] for n in verdict_names], b, s1, cap, m, k, g, *[p[n] for n in verdict_outs], z)

    for call, names in ((plan, plan_names + plan_outs), (verdict, verdict_names + verdict_outs)):
        assert call(b=-1) == 1 and call(b=65536) == 1 and call(s1=-1) == 1 and call(cap=0) == 1 and call(cap=1025) == 1
        for n in names:
            assert call(**{n: z}) == 1, n
        assert call(b=0) == 0 and call(b=0, status=z, off1=z) == 0                       # B = 0: nothing to do
    assert plan(expected_positions=ctypes.c_void_p(260)) == 1 and plan(boxes=ctypes.c_void_p(264)) == 1
    assert verdict(m=-1) == 1 and verdict(k=0) == 1 and verdict(g=-1) == 1 and verdict(indices=ctypes.c_void_p(260)) == 1


# ---------------------------------------------------------------------------------------------------------------------
# the switches
# ---------------------------------------------------------------------------------------------------------------------
def test_defaults_are_unchanged_and_the_constructor_refuses_the_switch_alone():
    from cvpce_amd import production
    cmp = production.PlanogramComparator()
    assert cmp.device_graphs is False and cmp.device_tail is False and cmp.device_reclass is False and cmp.reclass_host_routed == 0
    assert production.PlanogramComparator(device_graphs=True, device_tail=True).device_reclass is False
    with pytest.raises(ValueError, match='device_reclass needs device_tail'):
        production.PlanogramComparator(device_reclass=True)
    with pytest.raises(ValueError, match='device_reclass needs device_tail'):
        production.PlanogramComparator(device_graphs=True, device_reclass=True)
    assert production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True).device_reclass is True


def test_the_cli_has_the_switch():
    from click.testing import CliRunner
    from cvpce_amd.cli import cli
    cmd = cli.commands['eval-planograms']
    assert not any('device' in p.name for p in cmd.params)
    text = ''.join(CliRunner().invoke(cli, ['eval-planograms', '--help']).output.split())
    assert '--device-reclass/--no-device-reclass' in text and text.count('[default:off]') >= 3
    assert '--device-tail/--no-device-tail' in text and '--device-graphs/--no-device-graphs' in text
    alone = CliRunner().invoke(cli, ['eval-planograms', '--device-graphs', '--device-reclass', 'a', 'b'])
    assert alone.exit_code == 2 and '--device-reclass needs --device-tail' in alone.output
    off = CliRunner().invoke(cli, ['eval-planograms', '--device-graphs', '--device-tail', '--device-reclass', '--no-device-tail', 'a', 'b'])
    assert off.exit_code == 2 and '--device-reclass needs --device-tail' in off.output
    all_three = CliRunner().invoke(cli, ['eval-planograms', '--device-graphs', '--device-tail', '--device-reclass', 'a', 'b'])      # (gets as far as the missing files)
    assert all_three.exit_code == 2 and 'needs --device' not in all_three.output
    none = CliRunner().invoke(cli, ['eval-planograms', '--device-reclass', '--no-device-reclass', 'a', 'b'])
    assert none.exit_code == 2 and 'needs --device' not in none.output


# ---------------------------------------------------------------------------------------------------------------------
# label ids
# ---------------------------------------------------------------------------------------------------------------------
def _classifier(monkeypatch, annotations):
    """a Classifier over an index that is never used as one: the device gallery's two ops are stood in for, the id space is real"""
    from cvpce_amd import production
    monkeypatch.setattr(production.ops, 'pad_features', lambda x: x)
    monkeypatch.setattr(production.ops, 'row_norms', lambda g: None)
    return production.Classifier.from_embedding(None, torch.zeros(len(annotations), 4), annotations, device=torch.device('cpu'),
                                                emb_device=torch.device('cpu'))


def test_label_ids_share_one_space_and_an_unknown_label_is_minus_one(monkeypatch):
    clf = _classifier(monkeypatch, ['b', 'a', 'b', ('c', 1), 'a'])
    assert clf.gallery_label_id.dtype == torch.int32 and clf.gallery_label_id.tolist() == [0, 1, 0, 2, 1]
    assert clf.expected_label_ids(['a', 'zzz', ('c', 1), 'b', None]) == [1, -1, 2, 0, -1]
    assert -1 not in clf.gallery_label_id.tolist()
    assert clf.expected_label_ids(['a', ['unhashable']]) is None
    bad = _classifier(monkeypatch, ['a', ['unhashable']])
    assert bad.label_ids is None and bad.gallery_label_id is None and bad.expected_label_ids(['a']) is None


def test_set_index_invalidates_a_cached_id_vector(monkeypatch):
    from cvpce_amd import production
    clf = _classifier(monkeypatch, ['a', 'b'])
    other = _classifier(monkeypatch, ['b', 'a'])
    assert clf.index_generation != other.index_generation
    cmp = production.PlanogramComparator(device_graphs=True, device_tail=True, device_reclass=True)
    plano = {'boxes': torch.zeros(3, 4), 'labels': ['b', 'c', 'a']}
    assert cmp._window_label_ids([plano], clf) == [[1, -1, 0]]
    key = production.PlanogramComparator.LABEL_IDS_KEY
    first = plano[key]
    assert first == (clf.index_generation, [1, -1, 0])
    assert cmp._window_label_ids([plano], clf)[0] is first[1] and plano[key] is first            # cached
    assert cmp._window_label_ids([plano], other) == [[0, -1, 1]]                                 # another classifier: another generation
    clf.set_index(torch.zeros(3, 4), ['c', 'a', 'b'])
    assert clf.index_generation not in (first[0], other.index_generation)
    assert cmp._window_label_ids([plano], clf) == [[2, 0, 1]] and plano[key] == (clf.index_generation, [2, 0, 1])
    assert cmp.reclass_host_routed == 0
    assert cmp._window_label_ids([plano, {'boxes': torch.zeros(1, 4), 'labels': [['unhashable']]}], clf) is None and cmp.reclass_host_routed == 1
    assert cmp._window_label_ids([plano], None) == [None]
