"""`gln seek-sku110k-outliers` end to end on a tiny on-disk SKU-110K-like set (the kind test_gpu_gaussians_cli.py builds): files -> reader
-> detector -> the three losses on the GPU -> the reference's lines, with one copy back."""
import re

import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def world(cuda, tmp_path_factory):
    from PIL import Image
    from cvpce_amd import synthetic
    root = tmp_path_factory.mktemp('headloss_cli')
    to_img = lambda t: Image.fromarray((t.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy())
    det = synthetic.synthetic_gln(seed=0, detections_per_img=60)
    torch.save({'model_state_dict': det.state_dict()}, root / 'gln.tar')
    (root / 'sku').mkdir()
    rows = []
    for k in range(4):
        to_img(synthetic.shelf_image(40 + k, 192, 256)).save(root / 'sku' / f'test_{k}.png')
        rows += [f'test_{k}.png,{10 + 30 * b},{15 + 6 * k},{35 + 30 * b},{60 + 20 * k},object,256,192' for b in range(3 + k)]
    (root / 'sku' / 'annotations.csv').write_text('\n'.join(rows) + '\n')
    return root


def _invoke(args):
    from click.testing import CliRunner
    from cvpce_amd.cli import cli
    return CliRunner().invoke(cli, [str(a) for a in args])


def test_seek_outliers_prints_the_three_losses(world, monkeypatch):
    from cvpce_amd import datautils, device_gaussians, device_headloss, proposals_eval
    seen = []
    together = device_headloss.compute_together
    monkeypatch.setattr(device_headloss, 'compute_together', lambda h, g: (seen.append((h, g)), together(h, g))[1])
    # (a threshold of 0 makes every image above a mean an outlier: the lines are exercised on four images)
    r = _invoke(['gln', 'seek-sku110k-outliers', '--imgs', world / 'sku', '--annotations', world / 'sku' / 'annotations.csv',
                 '--outlier-threshold', '0', '--dataloader-workers', '0', world / 'gln.tar'])
    assert r.exit_code == 0, r.output
    (head, gauss), = seen
    assert head.host_copies == 1 and gauss.host_copies == 0 and head.images == gauss.images == 4      # one copy back
    lines = r.output.splitlines()
    at = lines.index('-' * 10)
    assert lines[0] == '0...' and lines[at + 3] == '-' * 10
    means = [float(v) for v in re.match(r'Mean loss:\t(\S+)\t(\S+)\t(\S+)$', lines[at + 1]).groups()]
    stds = [float(v) for v in re.match(r'Std loss:\t(\S+)\t(\S+)\t(\S+)$', lines[at + 2]).groups()]
    # by hand: the same data through HeadScore and GaussianScore, one image per batch
    data = datautils.SKU110KDataset(str(world / 'sku'), str(world / 'sku' / 'annotations.csv'), image_format='uint8')
    model = proposals_eval.load_gln(str(world / 'gln.tar'), False)
    hs, gs = device_headloss.HeadScore(model, outlier_threshold=0), device_gaussians.GaussianScore(model, outlier_threshold=0)
    model.keep_head_outputs(True)
    with torch.no_grad():
        for img, t in data:
            res = model([img.cuda()])
            hs.update(model.head_outputs(), [t], [datautils.image_hw(img)])
            gs.update(res, [t['boxes']], [datautils.image_hw(img)])
    direct = dict(hs.compute(), gaussian=gs.compute())
    names = ('classification', 'bbox_regression', 'gaussian')
    assert int(direct['counts'][:, 0].min()) > 0                                    # every image has foreground anchors
    # (two runs of the detector in one process, as test_gpu_cli.py compares them: 1e-6)
    for k, name in enumerate(names):
        assert tuple(direct[name]['loss'].shape) == (4,)
        assert abs(means[k] - direct[name]['mean']) <= 1e-6 * abs(direct[name]['mean']), name
        assert abs(stds[k] - direct[name]['std']) <= 1e-6 * abs(direct[name]['std']) + 1e-9, name
    want = sorted(set().union(*(direct[n]['outliers'] for n in names)))
    found = [(i, re.match(r'Outlier at index (\d+): (\S+)$', l)) for i, l in enumerate(lines[at + 4:], at + 4)]
    found = [(i, int(m.group(1)), m.group(2)) for i, m in found if m]
    assert [(i, n) for _, i, n in found] == [(i, f'test_{i}.png') for i in want] and 0 < len(want) <= 4
    for line, i, _ in found:
        values = [float(v) for v in lines[line + 1].split('\t')[1:]]
        assert len(values) == 3 and all(abs(v - float(direct[n]['loss'][i])) <= 1e-6 * abs(v) for v, n in zip(values, names))
    assert 'No outliers' not in r.output
    # an absurd threshold: no outliers, the reference's farewell
    calm = _invoke(['gln', 'seek-sku110k-outliers', '--imgs', world / 'sku', '--annotations', world / 'sku' / 'annotations.csv',
                    '--outlier-threshold', '100', '--batch-size', '2', '--dataloader-workers', '0', world / 'gln.tar'])
    assert calm.exit_code == 0, calm.output
    assert calm.output.splitlines()[-1] == 'No outliers! Have a nice day!' and 'Outlier at index' not in calm.output
