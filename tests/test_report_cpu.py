"""CPU-side checks of the comparator's compliance report (no compute on a GPU): the numpy restatement of the report rule
(tests/report_cases.py) equals the host path of `PlanogramComparator.report` on seeded scenes with a stub classifier; the report's
compliance is `compare`'s value on every status branch; the kernels' header, signature table and torch ops stay apart from every
other table and refuse CPU tensors; the command line has the option."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import abi
import reclass_cases as rc
import report_cases as rp

GALLERY = 24


class StubClassifier:
    """Stands in for `production.Classifier` without an encoder: the nearest gallery row of a position is a function of the position's
    own numbers, so `classify` (the route of `compare`) and `classify_positions` (the route of `report`) agree as the real ones do."""
    device = torch.device('cpu')

    def __init__(self):
        from cvpce_amd import synthetic
        self.annotations = [synthetic.PLANOGRAM_LABELS[i % len(synthetic.PLANOGRAM_LABELS)] for i in range(GALLERY)]
        self.calls = 0

    @staticmethod
    def rows(boxes):
        return [int(abs(x0) * 3 + abs(y0)) % GALLERY for x0, y0, _, _ in boxes.tolist()]

    @staticmethod
    def distances(boxes):
        return ((boxes[:, 0].abs() % 7) / 16 + 0.03125).to(torch.float32)

    def classify(self, crops):                   # (the stand-in for ops.crop_resize below hands the positions through)
        return [[self.annotations[r]] for r in self.rows(crops)]

    def classify_positions(self, image, boxes):
        self.calls += 1
        return self.rows(boxes), self.distances(boxes)


@pytest.fixture
def host_ops(monkeypatch):
    """`_finish` crops on the device before it classifies: here the 'crops' are the clamped positions themselves"""
    from cvpce_amd import production
    monkeypatch.setattr(production.ops, 'input_image', lambda image, device: image)
    monkeypatch.setattr(production.ops, 'crop_resize', lambda img, boxes, size, mode=0: boxes)


def _scenes():
    """(expected, actual, image, classifier) of the seeded scenes: whole shelves, a shelf cut at the image's edge, no classifier"""
    clf = StubClassifier()
    out = []
    for k, kw in enumerate((dict(), dict(cut=640.0), dict(scale=1.3), dict(cut=600.0, strays=False))):
        e, a, (h, w) = rp.comparator_scene(k, **kw)
        out.append((e, a, torch.zeros(3, h, w), clf))
    e, a, (h, w) = rp.comparator_scene(4)
    out.append((e, a, torch.zeros(3, h, w), None))                # no classifier: nothing is checked
    e, a, (h, w) = rp.comparator_scene(5)
    out.append((e, a, None, clf))                                 # no image either
    return out


def _model_report(expected, actual, image, clf, cmp):
    """the numpy model on the host tail's own tensors -> (outcome, seen_row, seen_distance, occupant, occupant_iou, stray, positions)"""
    from cvpce_amd import datautils, planograms
    m = planograms.large_common_subgraph(planograms.build_graph(expected['boxes'], expected['labels'], cmp.graph_threshold),
                                         planograms.build_graph(actual['boxes'], actual['labels'], cmp.graph_threshold))
    me, ma, pos, _, _, _ = planograms.finalize_via_ransac(m, expected['boxes'], actual['boxes'], expected['labels'], actual['labels'],
                                                          reproj_threshold=cmp._reproj_threshold(image), return_matched_actual=True,
                                                          return_expected_positions=True)
    n1, n2 = len(me), len(ma)
    on = clf is not None and image is not None
    table = [list(datautils.image_hw(image)) + [1] if on else [0, 0, 0]]
    first = rp.model_positions([rp.OK], me.to(torch.int32).numpy(), ma.to(torch.int32).numpy(), pos.numpy(), actual['boxes'].numpy(), [0, n1],
                               [0, n2], table)
    assert first['rows1'].all() and first['rows2'].all()
    _, index, count, _ = rc.model_plan([rp.OK], me.to(torch.int32).numpy(), pos.numpy(), [0, n1], table, n1)
    assert int(count[0]) == int((first['outcome'] == rp.PENDING).sum())
    c = int(count[0])
    clamped = rc.clamp_and_validity(pos.numpy(), *table[0][:2])[0][index[0, :c]] if c else np.zeros((0, 4), dtype=np.float32)
    rows = clf.rows(torch.from_numpy(clamped)) if c else []
    dist = clf.distances(torch.from_numpy(clamped)).numpy().reshape(-1, 1) if c else np.zeros((0, 1), dtype=np.float32)
    ids = {}
    gallery_id = [ids.setdefault(a, len(ids)) for a in clf.annotations] if clf is not None else []
    slot_row = np.full((1, n1), -1, dtype=np.int32)
    slot_row[0, :c] = np.arange(c)
    outcome, seen_row, seen_distance, written = rp.model_reclass(index, count, slot_row, np.array(rows, dtype=np.int64).reshape(-1, 1), dist, gallery_id,
                                                                 [ids.get(l, -1) for l in expected['labels']], [0, n1], [rp.OK], n1, first['outcome'])
    assert written.all()
    return outcome, seen_row, seen_distance, first['occupant'], first['occupant_iou'], first['stray'], pos


def test_the_model_equals_the_host_report_on_seeded_scenes(host_ops):
    from cvpce_amd import production
    cmp = production.PlanogramComparator()
    codes, occupants, strays, substituted = set(), 0, 0, 0
    for k, (expected, actual, image, clf) in enumerate(_scenes()):
        rep = cmp.report(expected, actual, image, clf)
        assert rep.status == 'ok', k
        outcome, seen_row, seen_distance, occupant, occupant_iou, stray, pos = _model_report(expected, actual, image, clf, cmp)
        assert rep.outcomes.dtype == torch.int8 and rep.outcomes.tolist() == outcome.tolist(), k
        assert torch.equal(rep.expected_positions, pos)
        assert rep.seen_labels == [clf.annotations[r] if r >= 0 else None for r in seen_row.tolist()], k
        assert torch.equal(rep.seen_distance.view(torch.int32), torch.from_numpy(seen_distance).view(torch.int32)), k
        assert rep.occupant.dtype == torch.int32 and rep.occupant.tolist() == occupant.tolist(), k
        assert torch.equal(rep.occupant_iou.view(torch.int32), torch.from_numpy(occupant_iou).view(torch.int32)), k      # bit for bit
        assert rep.occupant_labels == [actual['labels'][j] if j >= 0 else None for j in occupant.tolist()], k
        assert rep.stray.tolist() == np.nonzero(stray)[0].tolist(), k
        # the verdict is the share of positions that hold their product
        n1 = len(expected['labels'])
        assert float((rep.outcomes <= 1).sum() / n1) == float(rep.compliance)
        assert rep.missing() == [i for i, c in enumerate(outcome.tolist()) if c >= 2]
        assert rep.substituted() == [i for i in rep.missing() if occupant[i] >= 0]
        assert rp.PENDING not in outcome.tolist()
        codes |= set(outcome.tolist())
        occupants += int((occupant >= 0).sum())
        strays += int(stray.sum())
        substituted += len(rep.substituted())
    # a test that never sees a code proves nothing about it
    assert codes == {rp.DETECTED, rp.RECOVERED, rp.MISSING, rp.OUT_OF_VIEW, rp.UNCHECKED}, codes
    assert occupants >= 4 and strays >= 4 and substituted >= 2


def _same_verdict(got, want):
    assert type(got) is type(want) and float(got) == float(want), (got, want)
    if torch.is_tensor(want):
        assert got.dtype == want.dtype and got.shape == want.shape


def test_compliance_is_what_compare_returns_on_every_branch(host_ops, monkeypatch):
    from cvpce_amd import planograms, production
    cmp = production.PlanogramComparator()
    seen = set()
    for expected, actual, image, clf in _scenes():
        rep = cmp.report(expected, actual, image, clf)
        _same_verdict(rep.compliance, cmp.compare(expected, actual, image, clf))
        assert torch.is_tensor(rep.compliance) and rep.compliance.dtype == torch.float32
        seen.add(rep.status)
    expected, actual, (h, w) = rp.comparator_scene(0)
    image, clf = torch.zeros(3, h, w), StubClassifier()
    none = {'boxes': torch.zeros(0, 4), 'labels': []}
    for e, a, want in ((expected, none, 0), (none, none, 1)):                              # no detections: 0, or 1 for an empty planogram
        rep = cmp.report(e, a, image, clf)
        _same_verdict(rep.compliance, cmp.compare(e, a, image, clf))
        assert rep.compliance == want and rep.status == 'no_detections'
        seen.add(rep.status)
    other = dict(actual, labels=['nothing_the_planogram_has'] * len(actual['labels']))      # no common label: an empty matching
    rep = cmp.report(expected, other, image, clf)
    _same_verdict(rep.compliance, cmp.compare(expected, other, image, clf))
    assert rep.compliance == 0 and rep.status == 'no_matching'
    seen.add(rep.status)
    # no homography: the share of the matching (production.py:98-99)
    monkeypatch.setattr(planograms, 'find_homography', lambda p1, p2, *a, **kw: (None, torch.zeros(len(p1), dtype=torch.bool)))
    rep = cmp.report(expected, actual, image, clf)
    _same_verdict(rep.compliance, cmp.compare(expected, actual, image, clf))
    assert rep.status == 'no_homography' and isinstance(rep.compliance, float) and 0 < rep.compliance <= 1
    seen.add(rep.status)
    assert seen == {'ok', 'no_detections', 'no_matching', 'no_homography'}
    for name in production.ComplianceReport.FIELDS:
        assert getattr(rep, name) is None
    assert rep.missing() == [] and rep.substituted() == []
    assert json.loads(json.dumps(rep.to_dict())) == rep.to_dict()


def test_to_dict_round_trips_through_json(host_ops):
    from cvpce_amd import production
    cmp = production.PlanogramComparator()
    expected, actual, image, clf = _scenes()[1]
    rep = cmp.report(expected, actual, image, clf)
    d = rep.to_dict()
    assert json.loads(json.dumps(d)) == d
    assert d['status'] == 'ok' and d['compliance'] == float(rep.compliance) and d['outcomes'] == rep.outcomes.tolist()
    assert d['missing'] == rep.missing() and d['substituted'] == rep.substituted() and d['stray'] == rep.stray.tolist()
    assert len(d['expected_positions']) == len(expected['labels']) and all(len(r) == 4 for r in d['expected_positions'])
    assert d['seen_labels'] == rep.seen_labels and d['occupant_labels'] == rep.occupant_labels
    assert set(d) == {'compliance', 'status', 'missing', 'substituted'} | set(production.ComplianceReport.FIELDS)
    # a value that is not finite has no JSON form: it goes as null
    rep.seen_distance = rep.seen_distance.clone()
    rep.seen_distance[0] = float('nan')
    assert rep.to_dict()['seen_distance'][0] is None and json.loads(json.dumps(rep.to_dict()))['seen_distance'][0] is None


def test_the_host_restatement_keeps_the_rule_at_its_edges():
    """`planograms.report_positions` against the numpy model on the kernels' own edge scenes (a tie, the threshold itself, shared
    occupants, zero areas); NaN boxes are left out: torch.max keeps a NaN where fmaxf drops it, and no host tail produces one"""
    from cvpce_amd import planograms
    for im in rp.small_images():
        if im['status'] != rp.OK:
            continue
        ok2 = ~torch.isnan(im['boxes']).any(dim=1)
        ok1 = ~torch.isnan(im['positions']).any(dim=1)
        one = dict(im, positions=im['positions'][ok1], matched=im['matched'][ok1], boxes=im['boxes'][ok2], claimed=im['claimed'][ok2])
        want = rp.run_model_positions(rp.report_tables([one], with_rows=False))
        hw = (im['h'], im['w']) if im['enabled'] else None
        outcome, occupant, occupant_iou, stray = planograms.report_positions(one['matched'] != 0, one['claimed'] != 0, one['positions'], one['boxes'], hw)
        assert outcome.tolist() == want['outcome'].tolist() and occupant.tolist() == want['occupant'].tolist()
        assert torch.equal(occupant_iou.view(torch.int32), torch.from_numpy(want['occupant_iou']).view(torch.int32))
        assert stray.to(torch.int32).tolist() == want['stray'].tolist()


def test_the_edge_scenes_hold_what_they_are_named_for():
    im = rp.report_image(30, 12, 'edges', 480, 640, 109)
    t = rp.report_tables([im])
    m = rp.run_model_positions(t)
    e, j = 30 - rp.SPECIAL_POSITIONS, 12 - rp.SPECIAL_DETECTIONS
    assert m['occupant'][e] == j and m['occupant_iou'][e] == np.float32(0.5)                # exactly at the threshold
    assert m['stray'][j + 1] == 1                                                          # just below it
    assert m['occupant'][e + 1] == m['occupant'][e + 2] == j + 2                            # two positions, one occupant
    assert m['occupant'][e + 3] == j + 3 and m['stray'][j + 4] == 1 and torch.equal(im['boxes'][j + 3], im['boxes'][j + 4])      # a tie: the lower index
    assert m['occupant'][e + 4] == -1 and m['occupant_iou'][e + 4] == -1 and m['outcome'][e + 4] == rp.OUT_OF_VIEW               # 0 / 0 is no overlap
    assert m['stray'][j + 5] == m['stray'][j + 6] == m['stray'][j + 7] == 1                 # NaN and zero-area detections sit nowhere
    assert m['occupant'][e + 5] == j + 9 and m['stray'][j + 8] == 0 and t['matched_actual'][j + 8] == 1                          # a claimed detection is no occupant
    assert m['occupant_row'][e] == t['actual_row'][j]
    assert {rp.PENDING, rp.OUT_OF_VIEW} <= set(m['outcome'].tolist())
    # the window of the GPU test: every code the first kernel writes, on both sides of every size
    w = rp.run_model_positions(rp.report_tables(rp.window_images()))
    assert set(w['outcome'][w['rows1']].tolist()) == {rp.DETECTED, rp.OUT_OF_VIEW, rp.UNCHECKED, rp.PENDING}
    assert int((w['occupant'][w['rows1']] >= 0).sum()) > 100 and int(w['stray'][w['rows2']].sum()) > 100
    assert int((~w['rows1']).sum()) == 80 and int((~w['rows2']).sum()) == 80
    # and the second kernel's: positions recovered, missing, named by no slot, by two slots, by a row or index out of range
    small = rp.small_images()
    first = rp.run_model_positions(rp.report_tables(small))
    host, cap = rp.reclass_case(small, first['outcome'], 3)
    outcome, seen_row, seen_distance, written = rp.run_model_reclass(host, cap)
    codes = outcome[written].tolist()
    assert rp.PENDING not in codes and codes.count(rp.RECOVERED) > 10 and codes.count(rp.MISSING) > 10
    pending = (first['outcome'] == rp.PENDING) & written
    assert int((seen_row[pending] < 0).sum()) >= 4 and int((seen_row[written & ~pending] >= 0).sum()) == 0
    assert int((~written).sum()) == 80 and (first['outcome'][~pending] == outcome[~pending]).all()


# ---------------------------------------------------------------------------------------------------------------------
# boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_report_header_is_exported_and_mirrored():
    """(exported, bound and disjoint from the other headers: test_abi_mirror_cpu.py)"""
    assert abi.header_symbols('cvpce_amd_report.h') == ['cvpce_report_positions', 'cvpce_report_reclass']
    from cvpce_amd import planograms, torch_ops_report
    codes = ('DETECTED', 'RECOVERED', 'MISSING', 'OUT_OF_VIEW', 'UNCHECKED', 'PENDING')
    text = open(os.path.join(abi.INCLUDE, 'cvpce_amd_report.h')).read()
    for value, name in enumerate(codes):
        assert f'#define CVPCE_REPORT_{name} {value} ' in text
        assert getattr(torch_ops_report, name) == getattr(planograms, name) == getattr(rp, name) == value


def test_report_ops_have_their_own_names_and_are_gpu_only():
    from cvpce_amd import torch_ops_report  # noqa: F401  (registers the ops; names and keys: test_abi_mirror_cpu.py)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    for rows in (None, i32(3)):
        with pytest.raises(NotImplementedError, match='CPU'):
            torch.ops.cvpce_amd.report_positions(i32(1), i32(2), i32(3), torch.zeros(2, 4), torch.zeros(3, 4), i32(2), i32(2), i32(1, 3), rows, 0.5,
                                                 i32(2), i32(2), torch.zeros(2), i32(2), i32(3))
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.report_reclass(i32(1, 2), i32(1), i32(1, 2), torch.zeros(2, 1, dtype=torch.int64), torch.zeros(2, 1), i32(4), i32(2), i32(2),
                                           i32(1), i32(2), i32(2), torch.zeros(2))


def test_entry_points_reject_bad_arguments_on_the_host():
    """counts and cap out of range, null and misaligned pointers: status 1, nothing launched"""
    from cvpce_amd._lib import lib
    z, a = ctypes.c_void_p(0), ctypes.c_void_p(256)          # (never dereferenced: every call below returns before a launch)
    pos_names = ('status', 'matched_expected', 'matched_actual', 'expected_positions', 'actual_boxes', 'off1', 'off2', 'image', 'actual_row')
    pos_outs = ('outcome', 'occupant', 'occupant_iou', 'occupant_row', 'stray')
    re_names = ('expected_index', 'count', 'slot_row', 'indices', 'distances', 'gallery_label_id', 'expected_label_id', 'off1', 'status')
    re_outs = ('outcome', 'seen_row', 'seen_distance')

    def positions(b=1, s1=4, s2=4, **ptr):
        p = {n: ptr.get(n, a) for n in pos_names + pos_outs}
        return lib.cvpce_report_positions(*[p[n] for n in pos_names], 0.5, b, s1, s2, *[p[n] for n in pos_outs], z)

    def reclass(b=1, s1=4, cap=4, m=4, k=1, g=4, **ptr):
        p = {n: ptr.get(n, a) for n in re_names + re_outs}
        return lib.cvpce_report_reclass(*[p[n] for n in re_names], b, s1, cap, m, k, g, *[p[n] for n in re_outs], z)

    for call, names in ((positions, pos_names + pos_outs), (reclass, re_names + re_outs)):
        assert call(b=-1) == 1 and call(b=65536) == 1 and call(s1=-1) == 1
        for n in names:
            if n != 'actual_row':                                                          # (optional)
                assert call(**{n: z}) == 1, n
        assert call(b=0) == 0 and call(b=0, status=z, off1=z) == 0                       # B = 0: nothing to do
    assert positions(s2=-1) == 1 and positions(expected_positions=ctypes.c_void_p(260)) == 1 and positions(actual_boxes=ctypes.c_void_p(264)) == 1
    assert reclass(cap=0) == 1 and reclass(cap=1025) == 1 and reclass(m=-1) == 1 and reclass(k=0) == 1 and reclass(g=-1) == 1
    assert reclass(indices=ctypes.c_void_p(260)) == 1


# ---------------------------------------------------------------------------------------------------------------------
# the interface
# ---------------------------------------------------------------------------------------------------------------------
def test_match_takes_the_distance_keyword_and_passes_it_on(monkeypatch):
    from test_reclass_cpu import _classifier
    from cvpce_amd import production
    clf = _classifier(monkeypatch, ['a', 'b'])
    seen = []
    monkeypatch.setattr(production.ops, 'match_topk', lambda q, g, k, g_norms=None, return_distance=False: seen.append(return_distance) or 'result')
    assert clf.match(torch.zeros(1, 4)) == 'result' and clf.match(torch.zeros(1, 4), return_distance=True) == 'result'
    assert seen == [False, True]


def test_the_evaluator_has_the_three_entry_points():
    from cvpce_amd import production
    for name in ('report', 'report_batch', 'report_iter'):
        assert callable(getattr(production.PlanogramEvaluator, name))
    for name in ('report', 'report_batch'):
        assert callable(getattr(production.PlanogramComparator, name))


def test_the_cli_has_the_option(tmp_path):
    from click.testing import CliRunner
    from cvpce_amd.cli import cli
    cmd = cli.commands['eval-planograms']
    assert not any('report' in p.name for p in cmd.params)                                  # (the declared options stay the reference's)
    text = ''.join(CliRunner().invoke(cli, ['eval-planograms', '--help']).output.split())
    assert '--reportFILE' in text and '[default:none]' in text and '--device-reclass/--no-device-reclass' in text
    for args in (['--report', str(tmp_path / 'r.jsonl')], [f'--report={tmp_path / "r.jsonl"}'], []):
        r = CliRunner().invoke(cli, ['eval-planograms', *args, 'a', 'b'])                   # (gets as far as the missing files)
        assert r.exit_code == 2 and 'No such option' not in r.output and "'a'" in r.output, r.output
    last = CliRunner().invoke(cli, ['eval-planograms', 'a', 'b', '--report'])
    assert last.exit_code == 2 and '--report needs a file name' in last.output
    assert not (tmp_path / 'r.jsonl').exists()
