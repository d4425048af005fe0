"""CPU-side checks of the device metrics (no compute on a GPU): the evaluation kernels' own header, signature table and torch
op stay apart from the pinned inference ABI, and the host half of `DetectionMetrics` -- everything after the device-to-host
copy -- reproduces `metrics.calculate_metrics` exactly when fed the flags of a plain-torch restatement of the closed form."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

import abi
import device_metrics_cases as cases          # tests/device_metrics_cases.py
from cvpce_amd import metrics

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_eval_header_is_exported_and_mirrored():
    """(exported, bound and disjoint from the other headers: test_abi_mirror_cpu.py)"""
    assert 'cvpce_eval_match_detections' in abi.header_symbols('cvpce_amd_eval.h')


def test_eval_op_is_gpu_only():
    from cvpce_amd import torch_ops_eval  # noqa: F401  (registers the op)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.eval_match_detections(torch.zeros(2, 4), i32(2), i32(2), None, torch.zeros(1, 4), i32(2), None,
                                                  torch.tensor([0.5]), 1, i32(1, 1), torch.zeros(1, 2, dtype=torch.uint8))


def test_entry_point_rejects_bad_arguments_on_the_host():
    """K > 16, negative sizes and one class array without the other are refused before anything is launched."""
    from cvpce_amd._lib import lib
    z = ctypes.c_void_p(0)
    a = ctypes.c_void_p(256)          # (never dereferenced: every call below fails its argument check first)
    call = lambda n, sp, st, mt, k, pc=z, tc=z: lib.cvpce_eval_match_detections(a, a, a, pc, a, a, tc, a, n, sp, st, mt, k, a, a, z)
    assert call(1, 4, 4, 4, 17) == 1 and call(1, 4, 4, 4, 0) == 1
    assert call(-1, 4, 4, 4, 1) == 1 and call(1, -4, 4, 4, 1) == 1 and call(1, 4, -4, 4, 1) == 1 and call(1, 4, 4, -1, 1) == 1
    assert call(1, 4, 4, 4, 1, pc=a) == 1 and call(1, 4, 4, 4, 1, tc=a) == 1
    assert call(0, 0, 0, 0, 1) == 0 and call(3, 10, 0, 0, 16) == 0          # nothing to match: no launch, no error


def test_metrics_module_imports_without_the_library(tmp_path):
    """The metric worker processes import cvpce_amd.metrics alone: it must not pull in the library (device_metrics does)."""
    import shutil
    dst = tmp_path / 'cvpce_amd'
    shutil.copytree(os.path.join(ROOT, 'cvpce_amd'), dst, ignore=shutil.ignore_patterns('*.so', 'build', '__pycache__'))
    r = subprocess.run([sys.executable, '-c', 'import sys, cvpce_amd.metrics; assert "cvpce_amd._lib" not in sys.modules'],
                       cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([sys.executable, '-c', 'import cvpce_amd.device_metrics'], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode != 0 and 'HipLibraryMissing' in r.stderr
    r = subprocess.run([sys.executable, '-c', 'import sys, cvpce_amd.metrics; assert "cvpce_amd._lib" not in sys.modules'],
                       cwd=ROOT, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _units(targets, predictions, confidences, thresholds):
    out = []
    for t, p, c in zip(targets, predictions, confidences):
        flags, _, conf, _ = cases.closed_form(t, p, c, thresholds)
        out.append((flags, conf, len(t)))
    return out


@pytest.mark.parametrize('thresholds', cases.THRESHOLD_SETS, ids=('t50', 'coco', 't70_95'))
def test_closed_form_flags_equal_check_matches(golden_dir, thresholds):
    for name, targets, predictions, confidences in cases.known_answer_cases(golden_dir) + cases.golden_cases(golden_dir):
        for t, p, c in zip(targets, predictions, confidences):
            flags, first, conf, order = cases.closed_form(t, p, c, thresholds)
            want, want_conf, _ = metrics._process_one(t, p, c, thresholds)
            assert torch.equal(conf, want_conf), name
            for k, thr in enumerate(thresholds):
                assert torch.equal(flags[k].float(), want[thr]['true_positives']), (name, float(thr))
                assert flags[k].sum() == len(first[k][first[k] >= 0].unique())


@pytest.mark.parametrize('thresholds', cases.THRESHOLD_SETS, ids=('t50', 'coco', 't70_95'))
def test_host_half_reproduces_calculate_metrics(golden_dir, thresholds):
    from cvpce_amd.device_metrics import DetectionMetrics
    for name, targets, predictions, confidences in cases.known_answer_cases(golden_dir) + cases.golden_cases(golden_dir):
        got = DetectionMetrics(thresholds).calculate_from_flags(_units(targets, predictions, confidences, thresholds))
        want = metrics.calculate_metrics(targets, predictions, confidences, thresholds)
        cases.assert_results_equal(got, want, thresholds)


def test_host_half_per_class_grouping_equals_the_harness_grouping():
    """`per_class_from_records` against the grouping written out in detection_eval.evaluate_detections (restated here on host
    tensors): (image, class) units, class -1 pooled only, classes present on one side only."""
    from cvpce_amd.device_metrics import DetectionMetrics
    g = torch.Generator().manual_seed(3)
    thresholds, n_cls = (0.5, 0.75), 5
    records, all_t, all_p, all_c = [], [], [], []
    per = {c: ([], [], []) for c in range(n_cls)}
    for i in range(6):
        n_t, n_p = (0, 7) if i == 4 else (9, 0) if i == 5 else (12, 40)
        xy = torch.rand(n_t, 2, generator=g) * 50
        t = torch.cat([xy, xy + 5 + torch.rand(n_t, 2, generator=g) * 10], 1)
        tl = torch.randint(-1, n_cls, (n_t,), generator=g)
        src = torch.randint(0, max(n_t, 1), (n_p,), generator=g)
        p = (t[src] if n_t else torch.rand(n_p, 4, generator=g) * 10 + torch.tensor([0, 0, 20, 20.])) + torch.randn(n_p, 4, generator=g)
        pl = torch.where(torch.rand(n_p, generator=g) < 0.7, tl[src] if n_t else torch.zeros(n_p, dtype=torch.long),
                         torch.randint(-1, n_cls, (n_p,), generator=g))
        if i == 0:
            pl[pl == 2] = 3                      # class 2 only among the targets of image 0
        s = torch.rand(n_p, generator=g)
        assert len(s.unique()) == n_p
        flags, _, conf, order = cases.closed_form(t, p, s, thresholds, tl, pl)
        records.append({'tp': flags, 'conf': conf, 'pcls': pl[order].int(), 'pcls_given': pl.int(), 'tcls': tl.int()})
        for c in {int(x) for x in pl} | {int(x) for x in tl}:
            b, sc, tb = p[pl == c], s[pl == c], t[tl == c]
            all_p.append(b); all_c.append(sc); all_t.append(tb)
            if c != -1:
                per[c][0].append(tb); per[c][1].append(b); per[c][2].append(sc)
    strip = lambda res: {thr: {k: v for k, v in itm.items() if k != 'raw'} for thr, itm in res.items()}
    want_per = {c: strip(metrics.calculate_metrics(*per[c], thresholds)) for c in range(n_cls) if per[c][0] or per[c][1]}
    want_all = strip(metrics.calculate_metrics(all_t, all_p, all_c, thresholds))
    got_per, got_all = DetectionMetrics(thresholds).per_class_from_records(records, n_cls)
    assert sorted(got_per) == sorted(want_per) and len(got_per) >= 4
    for c in want_per:
        cases.assert_results_equal(got_per[c], want_per[c], thresholds)
    cases.assert_results_equal(got_all, want_all, thresholds)


def test_threshold_count_is_checked():
    from cvpce_amd.device_metrics import DetectionMetrics
    with pytest.raises(ValueError):
        DetectionMetrics(())
    with pytest.raises(ValueError):
        DetectionMetrics([0.5 + 0.01 * i for i in range(17)])


def test_cli_switch_is_parsed_and_documented_without_joining_the_reference_options():
    """`gln eval` and `eval-product-detection` take --device-metrics / --no-device-metrics (default off) and say in --help that
    --metric-workers is ignored with it; the declared options stay the reference's (tests/test_datasets_cpu.py pins them)."""
    import click
    from click.testing import CliRunner
    from cvpce_amd.cli import cli, _DeviceMetricsCommand
    for path in (('gln', 'eval'), ('eval-product-detection',)):
        cmd = cli
        for name in path:
            cmd = cmd.commands[name]
        assert isinstance(cmd, _DeviceMetricsCommand)
        assert not any('device' in p.name for p in cmd.params)
        text = ''.join(CliRunner().invoke(cli, list(path) + ['--help']).output.split())
        assert '--device-metrics/--no-device-metrics' in text and '--metric-workersisignored' in text
    seen = []

    @click.command(cls=_DeviceMetricsCommand)
    @click.option('--n', type=int, default=1)
    @click.argument('name')
    def probe(n, name):
        from cvpce_amd.cli import _device_metrics_switch
        seen.append((n, name, _device_metrics_switch()))

    for args, want in ((['x'], (1, 'x', False)), (['--device-metrics', 'x'], (1, 'x', True)), (['--n', '3', 'x', '--device-metrics'], (3, 'x', True)),
                       (['--device-metrics', '--no-device-metrics', 'x'], (1, 'x', False)), (['--', '--device-metrics'], (1, '--device-metrics', False))):
        r = CliRunner().invoke(probe, args)
        assert r.exit_code == 0 and seen[-1] == want, (args, r.output)
    assert CliRunner().invoke(probe, ['--device-metric', 'x']).exit_code == 2          # anything else is still an unknown option
