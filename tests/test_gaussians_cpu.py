"""The Gaussian-map scoring rule on the host: the numpy fp32 model of tests/gaussian_cases.py against what the reference's own
`generate_gaussians` and `gaussian_loss` produced (tests/golden/gaussian_targets.pt), the conditions the golden inputs must meet, and the
plumbing of the new stage (header, ctypes table, op names, descriptors, the CLI switch).  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

import abi
import gaussian_cases as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def golden():
    return torch.load(os.path.join(ROOT, 'tests', 'golden', 'gaussian_targets.pt'), weights_only=False)


def _case_args(c):
    return dict(w=c['w'], h=c['h'], boxes=c['boxes'], size_reduction=c['size_reduction'], method=c['method'], join=c['join'], tanh=c['tanh'])


def test_golden_covers_the_cases(golden):
    assert list(golden['targets']) == [n for n, _ in gc.target_cases()]
    pairs = {(c['method'], c['join']) for c in golden['targets'].values()}
    assert pairs == {(m, j) for m in gc.METHODS for j in gc.JOINS} - {('kant_method', 'addition')}
    assert {c['size_reduction'] for c in golden['targets'].values()} == {1, 2}
    assert any(c['tanh'] and c['method'] == 'simple_and_scaled' for c in golden['targets'].values())
    assert list(golden['losses']['cases']) == list(gc.LOSS_PARAMS)
    for name, c in gc.target_cases():
        assert golden['targets'][name]['boxes'] == c['boxes']
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'gaussian_targets.pt')) < (1 << 20)


def test_golden_inputs_meet_their_conditions(golden):
    """No multivariate_normal or kant box with zero reduced extent or an empty clip (the reference raises there); negative odd
    coordinates, overlaps and edge crossings are present; wholly outside boxes only with simple_and_scaled."""
    for name, c in golden['targets'].items():
        r, ws, hs = c['size_reduction'], c['w'] // c['size_reduction'], c['h'] // c['size_reduction']
        empty = 0
        for x1, y1, x2, y2 in ([v // r for v in b] for b in c['boxes']):
            if x1 == x2 or y1 == y2 or max(x1, 0) >= min(x2, ws) or max(y1, 0) >= min(y2, hs):
                empty += 1
        assert (empty > 0) == (c['method'] == 'simple_and_scaled'), name
        flat = [v for b in c['boxes'] for v in b]
        assert any(v < 0 and v % 2 for v in flat) and any(b[2] > c['w'] for b in c['boxes']) and any(b[3] > c['h'] for b in c['boxes'])


def test_model_equals_the_reference_targets(golden):
    """T_ref: the largest absolute difference (relative to max(1, |value|) under `addition`) between the host model and the
    reference, over every golden case.  It bounds the tolerance of the GPU tests and does not involve the kernel."""
    worst = 0.0
    for name, c in golden['targets'].items():
        got, _ = gc.render(**_case_args(c))
        want = c['expected'].numpy()
        assert got.shape == want.shape, name
        d = np.abs(got - want)
        if c['join'] == 'addition':
            d = d / np.maximum(1, np.abs(want))
        worst = max(worst, float(d.max()))
        if c['tanh']:
            assert float(want.min()) == -1.0
    print(f'T_ref = {worst:.3e}')
    assert worst <= gc.T_REF


def test_background_is_exact(golden):
    for name, c in golden['targets'].items():
        got, covered = gc.render(**_case_args(c))
        want = c['expected'].numpy()
        assert np.array_equal(got[~covered], want[~covered]), name
        assert (~covered).any() and covered.any()


def _loss_case(golden, name):
    L = golden['losses']
    c = L['cases'][name]
    maps = [m.numpy() * (0 if c['zero_maps'] else 1) for m in L['maps']]
    pred = L['predictions'][c['prediction']].numpy()
    target = np.zeros_like(pred)
    for n, (m, s) in enumerate(zip(maps, L['sizes'])):
        target[n, 0, :s[0] // 2, :s[1] // 2] = gc.resize(m.astype(np.float32), s[0] // 2, s[1] // 2)
    return pred, target, c


def test_loss_inputs_keep_clear_of_the_thresholds(golden):
    """No target value within 100 x the target tolerance of a threshold (exact background zeros apart): the masks, and with them
    pos_count and neg_count_used, are then the same on every implementation within that tolerance."""
    gap = 100 * gc.TARGET_TOL
    for name in gc.LOSS_PARAMS:
        _, target, _ = _loss_case(golden, name)
        live = target[target != 0]
        if live.size:
            assert float(np.abs(live - np.float32(0.1)).min()) > gap and float(np.abs(live).min()) > gap, name


def test_model_equals_the_reference_losses(golden):
    seen = {}
    for name in gc.LOSS_PARAMS:
        pred, target, c = _loss_case(golden, name)
        got = gc.loss(pred, target, **c['params'])
        want = float(c['expected'])
        assert abs(got['loss'] - want) <= gc.loss_tolerance(want), (name, got, want)
        seen[name] = got
    nneg = seen['fewer_negatives_than_n']['neg_count_used']
    assert seen['more_negatives_than_n']['neg_count_used'] < nneg                   # nneg > n
    assert nneg < 100000                                                            # nneg < n
    assert seen['no_positives']['pos_count'] == 0 and seen['no_positives']['neg_count_used'] == 1000
    assert seen['ties_at_tau']['tau_ties'] > seen['ties_at_tau']['neg_count_used']  # the cut falls inside a run of equal values


def test_header_table_and_op_names():
    """(exported, bound, compared argument by argument, the op names: test_abi_mirror_cpu.py)"""
    from cvpce_amd import _lib, torch_ops_gaussians as G
    header = 'cvpce_amd_gaussians.h'
    text = open(os.path.join(abi.INCLUDE, header)).read()
    assert list(abi.declarations(header)) == list(_lib.HEADERS[header]) == ['cvpce_gauss_kant_table', 'cvpce_gauss_targets',
                                                                            'cvpce_gauss_loss_workspace_bytes', 'cvpce_gauss_loss']
    for macro, value in (('CVPCE_GAUSS_TILE', G.TILE), ('CVPCE_GAUSS_LIST', G.LIST), ('CVPCE_GAUSS_GEOM', G.GEOM)):
        assert int(re.search(rf'#define {macro} (\d+)', text).group(1)) == value
    assert G.METHODS == gc.METHODS and G.JOINS == gc.JOINS
    make = open(os.path.join(ROOT, 'cvpce_amd', 'csrc', 'Makefile')).read()
    assert 'gaussians.hip' in make and 'cvpce_amd_gaussians.h' in make and 'FLAGS_gaussians := -ffp-contract=off' in make
    # host-only size query: refused shapes give 0
    assert G.loss_workspace_bytes(0, 4, 4) == 0 and G.loss_workspace_bytes(1, 1 << 16, 1 << 15) == 0
    assert G.loss_workspace_bytes(2, 48, 64) == 4 * (2 * 1024 + 4 + 2 * 2 * 2)


def test_descriptors_and_argument_errors():
    from cvpce_amd import datautils as d
    m = d.generate_via_multivariate_normal()
    assert (m.name, m.params, m.table) == ('multivariate_normal', gc.DEFAULT_PARAMS['multivariate_normal'], None)
    k = d.generate_via_kant_method()
    assert (k.name, k.table) == ('kant_method', gc.DEFAULT_PARAMS['kant_method'])
    s = d.generate_via_simple_and_scaled()
    assert (s.name, s.params) == ('simple_and_scaled', gc.DEFAULT_PARAMS['simple_and_scaled'])
    assert (d.join_via_max.name, d.join_via_addition.name, d.join_via_replacement.name) == ('max', 'addition', 'replacement')
    with pytest.raises(TypeError, match='variance_scale'):
        d.generate_via_multivariate_normal(1, lambda a: (a / 2) ** 2)
    with pytest.raises(TypeError, match='sigma_divisor'):
        d.generate_via_simple_and_scaled(sigma_func=lambda c: c / 6)
    with pytest.raises(TypeError, match='INTEGER'):
        d.generate_gaussians(32, 32, torch.tensor([[1.0, 2.0, 8.0, 9.0]]))
    with pytest.raises(TypeError):
        d.generate_gaussians(32, 32, torch.tensor([[1, 2, 8, 9]]), generate_method=lambda *a: None)


def test_model_geometry_is_the_transform_s():
    from cvpce_amd.models import proposals
    assert proposals.padded_hw(800, 1066) == (800, 1088) and proposals.padded_hw(1, 33) == (32, 64)
    imgs = [torch.zeros(3, 384, 512), torch.zeros(3, 300, 840)]
    sizes, rs, padded = proposals.GLNEngine.batch_geometry(imgs)
    assert padded == proposals.padded_hw(max(r[0] for r in rs), max(r[1] for r in rs)) == (800, 1344)


def test_cli_switch_is_declared_beside_the_reference_s_options(tmp_path):
    from click.testing import CliRunner
    from cvpce_amd.cli import cli, eval as gln_eval
    assert not any('gaussian' in (o.name or '') for o in gln_eval.params)            # the reference's option set is untouched
    out = CliRunner().invoke(cli, ['gln', 'eval', '--help']).output
    beyond = out[out.index("Options beyond the reference's"):]
    assert '--device-metrics / --no-device-metrics' in beyond and '--gaussian-loss / --no-gaussian-loss' in beyond
    assert '--gaussian-outlier-threshold' in beyond
    (tmp_path / 'imgs').mkdir()
    (tmp_path / 'ann.csv').write_text('')
    (tmp_path / 'state.tar').write_text('')
    r = CliRunner().invoke(cli, ['gln', 'eval', '--gaussian-loss', '--device-metrics', '--dataset', 'gp180', '--imgs', str(tmp_path / 'imgs'),
                                 '--annotations', str(tmp_path / 'ann.csv'), '--gaussian-outlier-threshold', '2.5', str(tmp_path / 'state.tar')])
    assert r.exit_code == 2 and '--gaussian-loss needs --dataset sku110k' in r.output
