"""CPU-side checks of the classification harness's device comparison (no compute on a GPU): the torch model of the kernel
(tests/classeval_cases.py) equals the reference's string loop, `ClassificationTally`'s host reduction gives the loop's counts from
the model's records, the kernel's header, signature table and torch op stay apart from every other table, and `dihe eval` has the
switch."""
import ctypes
import os
import types

import pytest
import torch

import abi
import classeval_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KNN = (1, 2, 4, 9)          # 9 > K = 4


def _case(seed):
    targets, indices, predictions = cc.label_case(seed)
    ids, gallery_id = cc.label_space(cc.GALLERY)
    want = torch.tensor([ids.get(t, -1) for t in targets], dtype=torch.int32)
    return targets, indices, predictions, ids, gallery_id, want


# ---------------------------------------------------------------------------------------------------------------------
# the model against the reference's loop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', (0, 1, 2))
def test_model_equals_the_string_loop(seed):
    targets, indices, predictions, ids, gallery_id, want = _case(seed)
    k = indices.shape[1]
    records = cc.model_rank(indices, gallery_id, want)
    label_of = {i: a for a, i in ids.items()}
    # the cases hold what they are meant to hold
    assert len(set(cc.GALLERY)) < len(cc.GALLERY) and gallery_id.tolist().count(ids['a']) == 3
    assert cc.NOWHERE in targets and cc.NOWHERE not in cc.GALLERY and int((want < 0).sum()) >= 5
    assert {0, 1, k - 1, k} <= set(records[:, 0].tolist())
    assert max(KNN) > k
    shared_first = [r for r, (t, got) in enumerate(zip(targets, predictions)) if got.count(t) >= 2]
    assert shared_first, 'no row holds two neighbours of the wanted label'
    for r in shared_first:
        assert int(records[r, 0]) == predictions[r].index(targets[r])                      # the smaller rank
    for (rank, nearest), a1, a2 in zip(records.tolist(), targets, predictions):
        for knn in KNN:
            assert (a1 in a2[:knn]) == (rank < min(knn, k)), (a1, a2, knn, rank)
        assert (a1 != a2[0]) == (rank != 0)
        assert label_of[nearest] == a2[0]


def test_model_ignores_indices_outside_the_gallery():
    gallery_id = torch.tensor([3, 4, 3], dtype=torch.int32)
    indices = torch.tensor([[3, 0, 2], [-1, 1, 1], [2, 3, -1], [0, 1, 2]], dtype=torch.int64)
    want = torch.tensor([3, 4, 4, -1], dtype=torch.int32)
    assert cc.model_rank(indices, gallery_id, want).tolist() == [[1, -1], [1, -1], [3, 3], [3, 3]]


# ---------------------------------------------------------------------------------------------------------------------
# the tally's host reduction
# ---------------------------------------------------------------------------------------------------------------------
def _tally(ids, k=KNN):
    from cvpce_amd.device_classification import ClassificationTally
    return ClassificationTally(types.SimpleNamespace(label_ids=ids, encoder=None, k=max(k)), k)


def test_the_tallys_reduction_gives_the_loops_counts():
    tally = None
    all_targets, all_predictions = [], []
    for seed in (0, 1, 2):
        targets, indices, predictions, ids, gallery_id, want = _case(seed)
        tally = tally or _tally(ids)
        tally.reduce(targets, cc.model_rank(indices, gallery_id, want).tolist(), indices.shape[1])        # one window each
        all_targets += targets
        all_predictions += predictions
    want = cc.string_loop(all_targets, all_predictions, KNN)
    got = tally.result()
    assert got == want
    assert 0 < want['accuracy'][1] < want['accuracy'][2] < want['accuracy'][4] == want['accuracy'][9] < 1
    assert want['missed'] and any(len(v) > 1 for v in want['confusion'].values())


def test_the_report_is_the_references():
    from cvpce_amd import device_classification
    targets, indices, predictions, ids, gallery_id, want = _case(0)
    res = cc.string_loop(targets, predictions, KNN)
    lines = device_classification.report(res)
    # classification_eval.py:50-55, restated
    total_per_ann, missed, misclassification = res['per_ann'], res['missed'], res['confusion']
    expect = [f'Total annotations: {res["total"]}, Correctly guessed: {res["correct"]}, Accuracy: {res["accuracy"]}']
    most_missed = sorted(((v / total_per_ann[k], v, k) for k, v in missed.items()), reverse=True)[:10]
    expect.append(f'Most missed: {", ".join(f"{a} ({n}, {p * 100} %)" for p, n, a in most_missed)}')
    for _, n, k in most_missed[:3]:
        common_misclassifications = sorted(((v / n, v, k) for k, v in misclassification[k].items()), reverse=True)[:3]
        expect.append(f'{k}: Commonly mistaken for {", ".join(f"{a} ({n}, {p * 100} %)" for p, n, a in common_misclassifications)}')
    assert lines == expect and len(lines) == 5


# ---------------------------------------------------------------------------------------------------------------------
# boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_classeval_header_is_exported_and_mirrored():
    """(exported, bound and disjoint from the other headers: test_abi_mirror_cpu.py)"""
    assert abi.header_symbols('cvpce_amd_classeval.h') == ['cvpce_classeval_rank']


def test_the_pinned_header_and_names_are_unchanged():
    # the inference header does not know the new entry, not even in a comment (its symbols, table and op names: test_abi_mirror_cpu.py)
    assert 'classeval' not in open(os.path.join(abi.INCLUDE, 'cvpce_amd.h')).read()


def test_classeval_op_has_its_own_name_and_is_gpu_only():
    from cvpce_amd import torch_ops_classeval  # noqa: F401  (registers the op; name and keys: test_abi_mirror_cpu.py)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.classeval_rank(torch.zeros(2, 3, dtype=torch.int64), torch.zeros(4, dtype=torch.int32), torch.zeros(2, dtype=torch.int32),
                                           torch.zeros(2, 2, dtype=torch.int32))


def test_the_entry_point_rejects_bad_arguments_on_the_host():
    """sizes out of range, null and misaligned pointers: status 1, nothing launched; Q = 0: status 0, nothing launched"""
    from cvpce_amd._lib import lib
    z, a = ctypes.c_void_p(0), ctypes.c_void_p(256)          # (never dereferenced: every call below returns before a launch)
    names = ('indices', 'gallery_label_id', 'want', 'records')

    def rank(q=4, k=3, g=5, **ptr):
        p = {n: ptr.get(n, a) for n in names}
        return lib.cvpce_classeval_rank(p['indices'], p['gallery_label_id'], p['want'], q, k, g, p['records'], z)

    assert rank(k=0) == 1 and rank(k=-1) == 1 and rank(q=-1) == 1 and rank(g=0) == 1 and rank(g=-3) == 1
    for n in names:
        assert rank(**{n: z}) == 1, n
    assert rank(indices=ctypes.c_void_p(260)) == 1 and rank(records=ctypes.c_void_p(260)) == 1
    assert rank(q=0) == 0 and rank(q=0, indices=z, want=z, records=z) == 0
    assert rank(q=0, k=0) == 1 and rank(q=0, g=0) == 1


# ---------------------------------------------------------------------------------------------------------------------
# the switch
# ---------------------------------------------------------------------------------------------------------------------
DIHE_EVAL_OPTIONS = {'model': 'vgg16', 'resnet_layers': (2, 3), 'batch_norm': False, 'batch_size': 8, 'dataloader_workers': 8,
                     'enc_weights': None, 'only': 'none', 'knn': (1,), 'img_dir': None, 'test_imgs': None, 'annotations': None}


def test_eval_dihe_takes_the_switch_and_defaults_to_off():
    import inspect
    from cvpce_amd import classification_eval
    p = inspect.signature(classification_eval.eval_dihe).parameters
    assert p['device_eval'].default is False and p['window'].default == 8


def test_the_cli_has_the_switch_under_its_own_heading():
    import click
    from click.testing import CliRunner
    from cvpce_amd.cli import cli
    cmd = cli.commands['dihe'].commands['eval']
    got = {p.name: p.default for p in cmd.params if isinstance(p, click.Option)}
    assert set(got) == set(DIHE_EVAL_OPTIONS) and not [p for p in cmd.params if isinstance(p, click.Argument)]
    for name, v in DIHE_EVAL_OPTIONS.items():
        if v is not None:
            assert (tuple(got[name]) if isinstance(v, tuple) else got[name]) == v, name
    out = CliRunner().invoke(cli, ['dihe', 'eval', '--help']).output
    heading = out.index("Options beyond the reference's")
    assert out.index('--knn') < heading < out.index('--device-eval / --no-device-eval')
    assert '[default:off]' in ''.join(out[heading:].split())
    # the other commands do not grow the switch
    assert '--device-eval' not in CliRunner().invoke(cli, ['dihe', 'prebuild-index', '--help']).output
    assert '--device-eval' not in CliRunner().invoke(cli, ['eval-planograms', '--help']).output


@pytest.mark.parametrize('args, want', ((['--device-eval'], True), ([], False), (['--device-eval', '--no-device-eval'], False),
                                         (['--no-device-eval', '--device-eval'], True)))
def test_the_switch_reaches_eval_dihe(monkeypatch, tmp_path, args, want):
    from click.testing import CliRunner
    from cvpce_amd import cli as cli_module, classification_eval
    seen = {}

    def fake_eval_dihe(encoder, sampleset, testset, batch_size, num_workers=0, k=(1,), verbose=False, **kw):
        seen.update(kw, k=tuple(k), batch_size=batch_size, num_workers=num_workers)
        return {knn: 0.5 for knn in k}

    class Encoder:
        def cuda(self):
            return self

        def load_state_dict(self, state):
            seen['state'] = state

        def eval(self):
            return self

        def requires_grad_(self, flag):
            return self

    monkeypatch.setattr(classification_eval, 'eval_dihe', fake_eval_dihe)
    monkeypatch.setattr(cli_module.classification, 'macvgg_embedder', lambda **kw: Encoder())
    monkeypatch.setattr(cli_module.datautils, 'GroceryProductsDataset', lambda *a, **kw: 'samples')
    monkeypatch.setattr(cli_module.datautils, 'GroceryProductsTestSet', lambda *a, **kw: 'tests')
    for d in ('train', 'test', 'ann'):
        (tmp_path / d).mkdir()
    torch.save({'model_state_dict': {'w': torch.zeros(1)}}, tmp_path / 'enc.tar')
    r = CliRunner().invoke(cli_module.cli, ['dihe', 'eval', '--img-dir', str(tmp_path / 'train'), '--test-imgs', str(tmp_path / 'test'),
                                            '--annotations', str(tmp_path / 'ann'), '--enc-weights', str(tmp_path / 'enc.tar'), '--knn', '1',
                                            '--knn', '3'] + args, catch_exceptions=False)
    assert r.exit_code == 0, r.output
    assert seen['device_eval'] is want and seen['k'] == (1, 3) and '--> accuracy {1: 0.5, 3: 0.5}' in r.output
    assert seen.get('window', 8) == cli_module.EVAL_WINDOW


def test_the_new_sources_are_what_the_makefile_builds():
    mk = open(os.path.join(ROOT, 'cvpce_amd', 'csrc', 'Makefile')).read()
    assert ' classeval.hip' in mk and 'include/cvpce_amd_classeval.h' in mk
