"""`gln eval --gaussian-loss` end to end on a tiny on-disk SKU-110K-like set (the kind test_gpu_cli.py builds): files -> reader -> detector
-> Gaussian targets and losses on the GPU -> the printed lines."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def world(cuda, tmp_path_factory):
    from PIL import Image
    from cvpce_amd import synthetic
    root = tmp_path_factory.mktemp('gauss_cli')
    to_img = lambda t: Image.fromarray((t.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy())
    det = synthetic.synthetic_gln(seed=0, detections_per_img=60)
    torch.save({'model_state_dict': det.state_dict()}, root / 'gln.tar')
    (root / 'sku').mkdir()
    rows = []
    for k in range(3):
        to_img(synthetic.shelf_image(30 + k, 384, 512)).save(root / 'sku' / f'test_{k}.png')
        rows += [f'test_{k}.png,{20 + 60 * b},{30 + 11 * k},{70 + 60 * b},{120 + 40 * k},object,512,384' for b in range(4 + k)]
    (root / 'sku' / 'annotations.csv').write_text('\n'.join(rows) + '\n')
    return root


def _invoke(args):
    from click.testing import CliRunner
    from cvpce_amd.cli import cli
    return CliRunner().invoke(cli, [str(a) for a in args])


def _common(world):
    return ['--imgs', world / 'sku', '--annotations', world / 'sku' / 'annotations.csv', '-t', '0.5', '--no-plots', '--metric-workers', '0']


def test_gln_eval_prints_the_gaussian_loss(world):
    from cvpce_amd import datautils, device_gaussians, proposals_eval
    plain = _invoke(['gln', 'eval', '--dataset', 'sku110k', *_common(world), world / 'gln.tar'])
    assert plain.exit_code == 0, plain.output
    assert 'Gaussian loss' not in plain.output
    # (a threshold of 0 makes every image above the mean an outlier: the lines are exercised on three images)
    scored = _invoke(['gln', 'eval', '--gaussian-loss', '--gaussian-outlier-threshold', '0', '--dataset', 'sku110k', *_common(world), world / 'gln.tar'])
    assert scored.exit_code == 0, scored.output
    lines = scored.output.splitlines()
    keep = lambda out: [l for l in out.splitlines() if l.startswith(('0.5:\t', '--> AP', '--> AR300'))]
    assert len(keep(plain.output)) == 3 and keep(scored.output) == keep(plain.output)
    at = next(i for i, l in enumerate(lines) if l.startswith('--> Gaussian loss'))
    assert lines[at - 1].startswith('--> AR300')                                  # after the reference's lines
    mean, std = (float(v) for v in re.match(r'--> Gaussian loss (\S+) \(std (\S+)\)', lines[at]).groups())
    data = datautils.SKU110KDataset(str(world / 'sku'), str(world / 'sku' / 'annotations.csv'), image_format='uint8')
    direct = proposals_eval.evaluate_gln(str(world / 'gln.tar'), data, thresholds=[0.5], num_metric_processes=0, trim_module_prefix=False,
                                         gaussian_score=lambda model: device_gaussians.GaussianScore(model, outlier_threshold=0))['gaussians']
    # (two runs of the detector in one process, as test_gpu_cli.py compares them: 1e-6)
    assert abs(mean - direct['mean']) <= 1e-6 * abs(direct['mean']) and abs(std - direct['std']) <= 1e-6 and tuple(direct['loss'].shape) == (3,)
    outliers = [re.match(r'Outlier at index (\d+): (\S+)\t(\S+)', l).groups() for l in lines[at + 1:]]
    assert [(int(i), n) for i, n, _ in outliers] == [(i, f'test_{i}.png') for i in direct['outliers']]
    assert all(abs(float(v) - float(direct['loss'][int(i)])) <= 1e-6 * float(v) for i, _, v in outliers)
    assert 0 < len(outliers) < 3


def test_gaussian_loss_needs_integer_boxes(world):
    r = _invoke(['gln', 'eval', '--gaussian-loss', '--dataset', 'gp180', *_common(world), world / 'gln.tar'])
    assert r.exit_code != 0 and '--gaussian-loss needs --dataset sku110k' in r.output
