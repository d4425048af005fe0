"""`eval-planograms --report FILE` end to end on the tiny on-disk dataset of test_gpu_cli.py: one JSON line per image beside the
summary the command always prints, and without the option the same summary and no file."""
import json
import re

import pytest

from test_gpu_cli import _run, world  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu


def test_eval_planograms_writes_one_json_line_per_image(world):  # noqa: F811
    args = ['--img-dir', world / 'Training', '--test-imgs', world / 'Testing', '--test-annotations', world / 'ann', '--planograms', world / 'plano',
            '--verbose', world / 'gln.tar', world / 'dihe.tar']
    plain = _run(['eval-planograms', *args])
    path = world / 'out' / 'report.jsonl'
    for switches in ((), ('--device-graphs', '--device-tail', '--device-reclass')):
        out = _run(['eval-planograms', *switches, '--report', path, *args])
        if not switches:
            assert out == plain                                                            # the same summary, line for line
        lines = [json.loads(l) for l in path.read_text().splitlines()]
        assert [l['image'] for l in lines] == [0, 1]
        printed = [float(v) for v in re.findall(r'Detected accuracy: ([0-9.]+)', out)]
        assert len(printed) == 2 and all(abs(l['compliance'] - v) < 5e-4 for l, v in zip(lines, printed))
        for l in lines:
            assert l['status'] in ('ok', 'no_detections', 'no_matching', 'no_homography')
            if l['status'] == 'ok':
                assert len(l['outcomes']) == 3 == len(l['expected_positions']) and set(l['outcomes']) <= {0, 1, 2, 3}
                assert sum(c <= 1 for c in l['outcomes']) / 3 == pytest.approx(l['compliance'])
                assert l['missing'] == [i for i, c in enumerate(l['outcomes']) if c >= 2]
            else:
                assert l['outcomes'] is None and l['missing'] == []
