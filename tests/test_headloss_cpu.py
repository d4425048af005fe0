"""The head-loss rule of DESIGN.md 4d on the host: the conditions the cases of tests/headloss_cases.py must meet (so that a changed case
cannot quietly stop exercising a branch), the fp32 model by hand on two boxes and one level, T_ref, and the surface of the new stage
(header, ctypes table, op name, validation errors, the CLI command, the evaluation keyword).  No GPU."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import abi
import headloss_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cases_exercise_their_branches():
    for name in ('seven_boxes_k1', 'seven_boxes_k3'):
        _, r32, _ = hc.reference(name)
        assert r32[0]['counts'] == (154, 211, 20) and r32[0]['matched'].shape == (3069,)    # foreground, between, restored from below 0.5
    _, ties, _ = hc.reference('ties')
    m = ties[0]['matched']
    assert ties[0]['counts'][:2] == (36, 56)
    assert (m == 0).sum() > 0 and (m == 2).sum() > 0 and not (m == 1).any()                 # the duplicate pair: always the lower index
    _, empty, _ = hc.reference('no_boxes')
    assert (empty[0]['matched'] == -1).all() and empty[0]['counts'] == (0, 0, 0)
    assert empty[0]['bbox_regression'] == 0.0 and empty[0]['classification'] > 0
    case, chunked, _ = hc.reference('chunk_plus_one')
    assert len(case['images'][0]['boxes']) == hc.CHUNK + 1 and chunked[0]['matched'].shape == (2907,)
    assert hc.strides(case['padded'], case['grids'])[3:] == [(48, 53), (96, 80)]           # per axis, not powers of two
    fg, between, restored = chunked[0]['counts']
    assert fg > 0 and between > 0 and restored > 0 and 2907 - fg - between > 0
    m = chunked[0]['matched']
    assert (m == hc.CHUNK).any() and (m[m >= 0] < hc.CHUNK).any()                           # both chunks are matched, the last index too
    case, batch, _ = hc.reference('batch')
    assert [len(i['boxes']) for i in case['images']] == [7, 0, 3]
    assert all(i['original'] != i['transformed'] for i in case['images'])                   # scale factors that are not 1
    assert batch[0]['counts'][0] > 0 and batch[1]['counts'] == (0, 0, 0) and batch[2]['counts'][0] > 0
    assert not (batch[2]['matched'] == 1).any() and (batch[2]['matched'] == 0).any()        # the duplicates survive the scaling
    assert list(hc.cases()) == list(hc.CASE_NAMES)


def test_model_by_hand():
    """One level, one cell: 9 anchors centred on (0, 0), two boxes.  Box 0 is the 1:1 anchor of size 32 itself; box 1 overlaps no
    anchor by 0.4 and is met best by the largest 1:2 anchor, which lies between the thresholds with box 0 and is restored."""
    anc = hc.anchors((8, 8), [(1, 1)])
    assert anc.shape == (9, 4) and anc[3].tolist() == [-16, -16, 16, 16]
    boxes = np.array([[-16, -16, 16, 16], [10, -35, 60, 35]], hc.F32)
    iou = hc.iou_matrix(anc, boxes)
    assert iou[3, 0] == 1.0
    # anchor 0 is [-23, -11, 23, 11]: with box 0, inter 32 * 22, union 46 * 22 + 32 * 32 - 32 * 22
    assert iou[0, 0] == np.float32(704.0) / np.float32(1012.0 + 1024.0 - 704.0)
    best1 = int(iou[:, 1].argmax())
    assert best1 == 2 and 0 < iou[2, 1] < 0.4 <= iou[2, 0] < 0.5                            # anchor [-35, -18, 35, 18]
    m, restored = hc.match(anc, boxes)
    assert m[3] == 0 and not restored[3]
    assert restored[2] and m[2] == 0                                                        # its OWN best box, not box 1 (the quirk)
    assert restored.sum() == 1 and m.tolist() == [0, 0, 0, 0, 0, -2, 0, 0, -2]
    logits = np.zeros((9, 2), hc.F32)
    regs = np.zeros((9, 4), hc.F32)
    res = hc.model(anc, boxes, [1, 0], logits, regs, hc.F64)
    assert res['counts'] == (7, 2, 1)
    fg, used = 7, 9 - 2
    # every logit 0: p = 0.5, ce = ln 2, (1 - p_t)^2 = 0.25; alpha 0.25 on the fg positives, 0.75 on every other class
    want = (fg * 0.25 + (2 * used - fg) * 0.75) * np.log(2.0) * 0.25 / fg
    assert abs(res['classification'] - want) <= 1e-12 * want
    # anchor 3 meets box 0 exactly: its encoding is 0; with zero regressions the L1 sum is that of the other foreground anchors' encodings
    only = hc.model(anc[3:4], boxes[:1], [1], logits[:1], regs[:1], hc.F64)
    assert only['bbox_regression'] == 0.0 and only['counts'] == (1, 0, 0)
    shifted = hc.model(anc[3:4], boxes[:1] + np.array([8, 0, 8, 0], hc.F32), [1], logits[:1], regs[:1], hc.F64)
    assert shifted['counts'][0] == 1 and shifted['bbox_regression'] == 0.25                 # IoU 0.6; (gcx - cx) / w = 8 / 32


def test_t_ref():
    """T_ref: the largest relative distance of the fp32 model from the float64 model over the cases."""
    worst = 0.0
    for name in hc.CASE_NAMES:
        _, r32, r64 = hc.reference(name)
        for a, b in zip(r32, r64):
            assert (a['matched'] == b['matched']).all() and a['counts'] == b['counts']
            for key in ('classification', 'bbox_regression'):
                if b[key]:
                    worst = max(worst, abs(a[key] - b[key]) / abs(b[key]))
    print(f'T_ref measured {worst:.3e}, recorded {hc.T_REF:.3e}')
    assert 1e-9 < worst <= hc.T_REF <= 1.000001 * worst                               # the measured value itself, not a rounder one
    assert hc.LOSS_RTOL == 8 * hc.T_REF


def test_header_table_and_op_names():
    """(exported, bound, compared argument by argument, the op name: test_abi_mirror_cpu.py)"""
    from cvpce_amd import _lib, torch_ops_headloss as H
    header = 'cvpce_amd_headloss.h'
    text = open(os.path.join(abi.INCLUDE, header)).read()
    assert list(abi.declarations(header)) == list(_lib.HEADERS[header]) == ['cvpce_headloss_workspace_bytes', 'cvpce_headloss']
    for macro, value in (('CVPCE_HEADLOSS_CHUNK', H.CHUNK), ('CVPCE_HEADLOSS_THREADS', H.THREADS), ('CVPCE_HEADLOSS_MAX_LEVELS', H.MAX_LEVELS)):
        assert int(re.search(rf'#define {macro} (\d+)', text).group(1)) == value
    assert H.CHUNK == hc.CHUNK
    make = open(os.path.join(ROOT, 'cvpce_amd', 'csrc', 'Makefile')).read()
    assert 'headloss.hip' in make and 'cvpce_amd_headloss.h' in make and 'anchors.h' in make and 'FLAGS_headloss := -ffp-contract=off' in make
    # the anchor expression is shared with the decode, not restated
    for src in ('detect.hip', 'headloss.hip'):
        assert 'grid_anchor(' in open(os.path.join(ROOT, 'cvpce_amd', 'csrc', src)).read()
    # host-only size query: refused shapes give 0
    grids = hc.GRIDS_128
    gh, gw = [g[0] for g in grids], [g[1] for g in grids]
    assert H.workspace_bytes(gh, gw, 9, 0, 0) == 0 and H.workspace_bytes([0], [4], 9, 1, 0) == 0 and H.workspace_bytes(gh, gw, 9, 1, -1) == 0
    assert H.workspace_bytes([16] * 9, [16] * 9, 9, 1, 0) == 0 and H.workspace_bytes([4096], [4096], 9, 16, 0) == 0
    tiles = -(-3069 // 256)
    assert H.workspace_bytes(gh, gw, 9, 2, 7) == 4 * (8 + 2 * (2 * 3069 + 2) + 2 * tiles * 5)


def test_targets_are_validated_before_anything_is_queued():
    from cvpce_amd import device_headloss as dh
    ok = {'boxes': torch.tensor([[1.0, 2.0, 8.0, 9.0]]), 'labels': torch.tensor([0])}
    dh.check_targets([ok, {'boxes': torch.zeros((0, 4)), 'labels': torch.zeros(0, dtype=torch.long)}], 1)
    with pytest.raises(ValueError, match='positive height and width'):
        dh.check_targets([ok, dict(ok, boxes=torch.tensor([[1.0, 2.0, 1.0, 9.0]]))], 1)
    with pytest.raises(ValueError, match='positive height and width'):
        dh.check_targets([dict(ok, boxes=torch.tensor([[1.0, 9.0, 8.0, 2.0]]))], 1)
    with pytest.raises(ValueError, match='positive height and width'):
        dh.check_targets([dict(ok, boxes=torch.tensor([[1.0, 2.0, float('nan'), 9.0]]))], 1)
    with pytest.raises(ValueError, match=r'labels lie in \[0, 1\)'):
        dh.check_targets([dict(ok, labels=torch.tensor([1]))], 1)
    with pytest.raises(ValueError, match=r'labels lie in'):
        dh.check_targets([dict(ok, labels=torch.tensor([-1]))], 3)
    with pytest.raises(ValueError, match='1 boxes and 2 labels'):
        dh.check_targets([dict(ok, labels=torch.tensor([0, 0]))], 1)
    with pytest.raises(ValueError, match='labels are integers'):
        dh.check_targets([dict(ok, labels=torch.tensor([0.0]))], 1)
    with pytest.raises(ValueError, match=r'\(T,4\)'):
        dh.check_targets([dict(ok, boxes=torch.zeros((2, 3)), labels=torch.zeros(1, dtype=torch.long))], 1)
    s = dh.scale_factors([(125, 128)], [(100, 90)])
    assert s.dtype == torch.float32 and s.tolist() == [[1.25, float(np.float32(128) / np.float32(90))]]
    assert (dh.LAUNCHES_PER_BATCH, dh.UPLOADS_PER_BATCH, dh.HOST_WAITS_PER_BATCH) == (5, 4, 0)


def test_head_score_on_nothing_returns_empties():
    from cvpce_amd import device_headloss as dh
    score = dh.HeadScore(model=None)
    res = score.compute()
    assert set(res) == {'classification', 'bbox_regression', 'counts'} and tuple(res['counts'].shape) == (0, 3)
    for key in ('classification', 'bbox_regression'):
        assert res[key]['loss'].numel() == 0 and res[key]['outliers'] == [] and res[key]['mean'] != res[key]['mean']
    assert score.host_copies == 0 and score.images == 0
    score.update({'cls': [], 'reg': [], 'padded': (32, 32), 'sizes': []}, [], [])           # an empty batch queues nothing
    assert score.images == 0
    with pytest.raises(RuntimeError, match='keep_head_outputs'):
        score.update(None, [], [])


def test_surface():
    from click.testing import CliRunner
    from cvpce_amd import proposals_eval
    from cvpce_amd.cli import cli, seek_sku110k_outliers
    from cvpce_amd.models import proposals
    opts = {o.name: o for o in seek_sku110k_outliers.params}
    assert list(opts) == ['imgs', 'annotations', 'outlier_threshold', 'trim_module_prefix', 'batch_size', 'dataloader_workers', 'state_file']
    assert opts['outlier_threshold'].default == 3 and opts['batch_size'].default == 1 and opts['trim_module_prefix'].default is False
    out = CliRunner().invoke(cli, ['gln', 'seek-sku110k-outliers', '--help']).output
    for flag in ('--imgs', '--annotations', '--outlier-threshold', '--trim-module-prefix / --no-trim-module-prefix', '--batch-size',
                 '--dataloader-workers', 'STATE_FILE'):
        assert flag in out, flag
    for fn in (proposals_eval.evaluate_gln_sync, proposals_eval.evaluate_gln_async, proposals_eval.evaluate_gln):
        p = inspect.signature(fn).parameters
        assert p['head_score'].default is None and list(p).index('head_score') == list(p).index('gaussian_score') + 1
    model = proposals.gln(pretrained_backbone=False)
    assert model._keep_head_outputs is False and model.head_outputs() is None
    assert model.keep_head_outputs(True) is model and model._keep_head_outputs is True
    model.train()
    with pytest.raises(NotImplementedError):
        model([torch.zeros(3, 32, 32)], [{'boxes': torch.zeros((0, 4)), 'labels': torch.zeros(0, dtype=torch.long)}])
    model.eval()
    with pytest.raises(ValueError, match='positive height and width'):                      # before the device is even looked at
        model.losses([torch.zeros(3, 32, 32)], [{'boxes': torch.tensor([[4.0, 4.0, 4.0, 9.0]]), 'labels': torch.tensor([0])}])
    with pytest.raises(RuntimeError, match='HIP'):
        model.losses([torch.zeros(3, 32, 32)], [{'boxes': torch.tensor([[4.0, 4.0, 8.0, 9.0]]), 'labels': torch.tensor([0])}])
