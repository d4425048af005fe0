"""`plot-planogram-eval --out PREFIX` on the tiny on-disk dataset of test_gpu_cli.py and `misc pipeline-demo` over a folder of product
photos and a JSON planogram the test writes: the nine step pictures as PNG files, and the compliance printed."""
import json
import re

import pytest
import torch

from test_gpu_cli import _run, world  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

NAMES = ('detections', 'positions', 'expected_graph', 'observed_graph', 'expected_matched', 'observed_matched', 'annotated', 'observed', 'expected')


def _pictures(prefix):
    import numpy as np
    from PIL import Image
    out = {}
    for n in NAMES:
        with Image.open(f'{prefix}_{n}.png') as im:
            assert im.mode == 'RGB'
            out[n] = np.asarray(im).copy()
    return out


def test_plot_planogram_eval_writes_the_step_pictures_and_prints_the_compliance(world):  # noqa: F811
    import numpy as np
    common = ['--img-dir', world / 'Training', '--test-imgs', world / 'Testing', '--test-annotations', world / 'ann']
    states = [world / 'gln.tar', world / 'dihe.tar']
    verbose = _run(['eval-planograms', *common, '--planograms', world / 'plano', '--verbose', *states])
    lines = [l for l in verbose.splitlines() if l.startswith('Detected accuracy')]
    assert len(lines) == 2
    # image 1 on the host route; then with device switches and without --plano-idx: an image drawn at random, as in the reference
    for switches, index in (((), ('--plano-idx', '1')), (('--device-graphs', '--device-tail'), ())):
        prefix = world / 'out' / ('steps' + '_device' * bool(switches))
        out = _run(['plot-planogram-eval', *switches, *common, '--planos', world / 'plano', *index, '--out', prefix, *states])
        printed = [l for l in out.splitlines() if l.startswith('Detected accuracy')]
        assert len(printed) == 1 and (printed == [lines[1]] if index else printed[0] in lines)         # what `eval-planograms --verbose` prints for it
        assert [l for l in out.splitlines() if l.endswith('.png')] == [f'{prefix}_{n}.png' for n in NAMES]
        pics = _pictures(prefix)
        for n in ('detections', 'positions', 'annotated', 'observed', 'observed_graph', 'observed_matched'):
            assert pics[n].shape == (300, 840, 3), n                                                   # the photo's size
        assert pics['expected'].shape == pics['expected_graph'].shape == pics['expected_matched'].shape and pics['expected'].shape[1] == 840
        assert not np.array_equal(pics['detections'], pics['annotated'])


def test_pipeline_demo_over_a_folder_and_a_json_planogram(world, tmp_path):  # noqa: F811
    from PIL import Image
    from cvpce_amd import synthetic
    folder = tmp_path / 'products'
    folder.mkdir()
    gal = (synthetic.gallery_images(6, seed=5) + 1) / 2
    to_img = lambda t: Image.fromarray((t.clamp(0, 1) * 255).round().to(torch.uint8).permute(1, 2, 0).numpy())
    for i in range(6):
        to_img(gal[i]).save(folder / f'product{i}.png')
    # a shelf of three of the products, as test_gpu_cli.py builds its test images, and its planogram at half the scale
    picks = (3, 1, 4)
    shelf = torch.full((3, 300, 840), 0.3)
    plano = []
    for j, i in enumerate(picks):
        x = 10 + j * 270
        shelf[:, 20:276, x:x + 256] = gal[i]
        plano.append({'label': f'product{i}', 'box': [x / 2, 10, (x + 256) / 2, 138]})
    to_img(shelf).save(tmp_path / 'shelf.png')
    (tmp_path / 'plano.json').write_text(json.dumps(plano))
    args = [world / 'gln.tar', world / 'dihe.tar', folder, tmp_path / 'shelf.png', tmp_path / 'plano.json']
    seen = []
    for switches, tag in (((), 'plain'), (('--scale-gallery', '--device-graphs', '--device-tail', '--device-detections'), 'scaled_device')):
        prefix = tmp_path / tag
        out = _run(['misc', 'pipeline-demo', *switches, '--out', prefix, *args])
        assert [l for l in out.splitlines() if l.endswith('.png')] == [f'{prefix}_{n}.png' for n in NAMES]
        m = re.search(r'^Compliance: ([0-9.]+) \((\w+)\)$', out, flags=re.M)
        assert m is not None and 0.0 <= float(m.group(1)) <= 1.0
        seen.append((float(m.group(1)), m.group(2)))
        pics = _pictures(prefix)
        assert pics['detections'].shape == pics['observed_graph'].shape == (300, 840, 3) and pics['expected_graph'].shape[1] == 840
        # the expected planogram is rebuilt from the folder's photos (the [0, 1] floats of `train=False`): products on white, none of
        # them black as a photo read in the wrong range would come out
        assert (pics['expected'] != 255).any() and (pics['expected'] != 0).any()
        if m.group(2) in ('ok', 'no_homography'):                       # a matching: the graphs are drawn over the rebuilt planograms
            assert (pics['observed_graph'] != pics['observed']).any() and (pics['expected_graph'] != pics['expected']).any()
            assert (pics['expected_matched'] != pics['expected']).any()
    print(seen)
    assert all(status in ('ok', 'no_detections', 'no_matching', 'no_homography') for _, status in seen)
