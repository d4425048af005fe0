"""`rebuild-scene --out PREFIX` and `eval-planograms --render DIR` end to end on the tiny on-disk dataset of test_gpu_cli.py: the three
compliance pictures as PNG files beside what the commands print anyway."""
import re

import pytest

from test_gpu_cli import _run, world  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

NAMES = ('annotated', 'observed', 'expected')


def _args(world):  # noqa: F811
    return ['--img-dir', world / 'Training', '--test-imgs', world / 'Testing', '--test-annotations', world / 'ann', '--planograms', world / 'plano']


def _sizes(prefix):
    from PIL import Image
    out = {}
    for n in NAMES:
        with Image.open(f'{prefix}_{n}.png') as im:
            assert im.mode == 'RGB'
            out[n] = im.size
    return out


def test_rebuild_scene_writes_three_pictures_and_prints_the_compliance(world):  # noqa: F811
    states = [world / 'gln.tar', world / 'dihe.tar']
    verbose = _run(['eval-planograms', *_args(world), '--verbose', *states])
    lines = [l for l in verbose.splitlines() if l.startswith('Detected accuracy')]
    assert len(lines) == 2
    prefix = world / 'out' / 'scene'
    out = _run(['rebuild-scene', *_args(world), '--out', prefix, *states])
    printed = [l for l in out.splitlines() if l.startswith('Detected accuracy')]
    assert printed == [lines[0]] and len(re.findall(r'Detected accuracy: ([0-9.]+)', out)) == 1      # what `eval-planograms --verbose` prints for image 0
    assert [l for l in out.splitlines() if l.endswith('.png')] == [f'{prefix}_{n}.png' for n in NAMES]
    sizes = _sizes(prefix)
    assert sizes['annotated'] == (840, 300) == sizes['observed']             # (PIL: width, height) the photo's size
    assert sizes['expected'][0] == 840 and 1 <= sizes['expected'][1] <= 32768  # the photo's width, the planogram's aspect ratio


def test_eval_planograms_render_writes_three_files_per_image(world):  # noqa: F811
    args = [*_args(world), '--verbose', world / 'gln.tar', world / 'dihe.tar']
    plain = _run(['eval-planograms', *args])
    directory = world / 'out' / 'pictures'
    out = _run(['eval-planograms', '--render', directory, *args])
    assert out == plain                                                           # the same summary, line for line
    assert sorted(p.name for p in directory.iterdir()) == sorted(f'{i}_{n}.png' for i in (0, 1) for n in NAMES)
    for i in (0, 1):
        assert _sizes(directory / str(i))['annotated'] == (840, 300)
