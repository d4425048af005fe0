"""The Tonioni matcher on the host (no compute on a GPU): `planograms.tonioni_mcs` against the reference's recorded results
(tests/golden/tonioni.pt), `tonioni_cases.model_tonioni` -- the device algorithm restated -- against the host pair by pair, what the
fixture must contain, the comparator's `matcher` switch on the host route, and the binding of include/ext/cvpce_amd_tonioni.h,
checked as tests/test_abi_mirror_cpu.py checks the headers of include/."""
import ctypes

import pytest
import torch

import abi
import tonioni_cases as tc
from planogram_device_cases import golden_cases
from cvpce_amd import planograms

HEADER = 'ext/cvpce_amd_tonioni.h'


@pytest.fixture(scope='module')
def solved(golden_dir):
    """every fixture case with its host graphs, the host's pairs in growth order and the model's answers, computed once"""
    out = []
    for c in tc.golden(golden_dir):
        g1, g2 = planograms.build_graph(c['boxes1'], c['labels1']), planograms.build_graph(c['boxes2'], c['labels2'])
        t1, t2 = tc.tables_of_host(g1), tc.tables_of_host(g2)
        model = tc.model_tonioni(t1, c['labels1'], t2, c['labels2'], c['min_score'])
        unbounded = tc.model_tonioni(t1, c['labels1'], t2, c['labels2'], c['min_score'], use_bound=False)
        out.append(dict(c, g1=g1, g2=g2, host=planograms.tonioni_pairs(g1, g2, min_score=c['min_score']), model=model, unbounded=unbounded))
    return out


def test_fixture_is_the_generator_s(golden_dir):
    gold = tc.golden(golden_dir)
    assert [c['name'] for c in gold] == [c['name'] for c in tc.cases()]
    for c, d in zip(gold, tc.cases()):
        assert torch.equal(c['boxes1'], d['boxes1']) and torch.equal(c['boxes2'], d['boxes2'])
        assert c['labels1'] == d['labels1'] and c['labels2'] == d['labels2'] and c['min_score'] == d['min_score']


def test_host_matches_reference(solved):
    for c in solved:
        found = planograms.tonioni_mcs(c['g1'], c['g2'], min_score=c['min_score'])
        assert isinstance(found, set) and sorted(found) == c['tonioni'], c['name']
        assert found == set(c['host']) and len(found) == len(c['host'])
        assert len(planograms.build_hypotheses(c['g1'], c['g2'])) == c['hypotheses'], c['name']
        assert len(planograms.large_common_subgraph(c['g1'], c['g2'], min_score=c['min_score'])) == c['large'], c['name']


def test_set_is_filled_in_growth_order(solved):
    for c in solved:
        grown = set()
        for pair in c['host']:
            grown.add(pair)
        assert list(planograms.tonioni_mcs(c['g1'], c['g2'], min_score=c['min_score'])) == list(grown), c['name']


def test_model_equals_host_pair_by_pair(solved):
    for c in solved:
        pairs, mf, start, _ = c['model']
        assert pairs == c['host'], c['name']
        assert len(mf) == c['hypotheses'] and (start >= 0) == bool(pairs)
        if pairs:
            assert mf[start][1] == len(pairs)


def test_per_start_form_is_the_lazy_search(solved):
    """the scan over complete runs adopts what the search that gives runs up adopts (the argument of DESIGN.md 4b)"""
    for c in solved[:12]:
        hyp = planograms.build_hypotheses(c['g1'], c['g2'])
        steps = lambda a, b, c=c: planograms._compatible_steps(c['g1'], c['g2'], a, b, 'dir')
        mf = c['model'][1]
        for i in range(len(hyp)):
            taken, low = planograms.tonioni_run(hyp[i:], steps, c['min_score'])
            assert (low, len(taken)) == mf[i], (c['name'], i)


def test_fixture_conditions(solved):
    by_name = {c['name']: c for c in solved}
    changed = [c['name'] for c in solved if set(c['unbounded'][0]) != set(c['model'][0])]
    larger = [c['name'] for c in solved if len(c['tonioni']) > c['large']]
    stopped = [c['name'] for c in solved if c['model'][3]]
    print(f'{len(changed)} cases change without the bound, {len(larger)} are larger than large_common_subgraph, {len(stopped)} end on min_score')
    assert len(changed) >= 5, 'ignoring the bound must change at least 5 results'
    assert len(larger) >= 5
    assert by_name['no_equal_labels']['hypotheses'] == 0 and by_name['no_equal_labels']['tonioni'] == []
    assert len(by_name['one_node']['labels1']) == len(by_name['one_node']['labels2']) == 1 and by_name['one_node']['hypotheses'] == 1
    assert stopped, 'a run that ends on the min_score stop with hypotheses left'
    assert any(c['min_score'] == -0.5 and c['tonioni'] for c in solved)


def test_score8_limit_is_the_float_test():
    from cvpce_amd import planograms_device as pd
    for min_score in (-0.2, -0.5, -0.125, 0.0, -1.0, -3.3, 0.4, -0.1250001):
        t = pd.score8_limit(min_score)
        assert t == tc.score8_limit(min_score)
        assert not t / 8 > min_score and (t + 1) / 8 > min_score


def _scene(i):
    b1, l1, b2, l2 = tc.window_scene(i)
    return {'boxes': b1, 'labels': l1}, {'boxes': b2, 'labels': l2}


def test_comparator_host_route():
    from cvpce_amd import production
    comparator = production.PlanogramComparator(matcher='tonioni')
    for i in range(4):
        expected, actual = _scene(i)
        ge, ga = planograms.build_graph(expected['boxes'], expected['labels']), planograms.build_graph(actual['boxes'], actual['labels'])
        matching = planograms.tonioni_mcs(ge, ga)
        want = comparator._finish(matching, expected, actual, None, None)
        got = comparator.compare(expected, actual)
        assert float(got) == float(want)
        report = comparator.report(expected, actual)
        assert float(report.compliance) == float(want)
    assert comparator.host_routed == 0


def test_unknown_matcher_raises():
    from cvpce_amd import production, planograms_device as pd
    with pytest.raises(ValueError):
        production.PlanogramComparator(matcher='largest')
    with pytest.raises(ValueError):
        pd.check_matcher('Tonioni')
    assert production.PlanogramComparator().matcher == 'large'


def test_default_comparator_is_unchanged(golden_dir):
    from cvpce_amd import production
    default, explicit = production.PlanogramComparator(), production.PlanogramComparator(matcher='large')
    for c in golden_cases(golden_dir):
        expected = {'boxes': c['expected_boxes'], 'labels': c['expected_labels']}
        actual = {'boxes': c['actual_boxes'], 'labels': c['actual_labels']}
        ge, ga = planograms.build_graph(expected['boxes'], expected['labels'], 0.5), planograms.build_graph(actual['boxes'], actual['labels'], 0.5)
        matching = planograms.large_common_subgraph(ge, ga)
        assert sorted(matching) == c['matching']
        want = default._finish(matching, expected, actual, None, None)
        assert float(default.compare(expected, actual)) == float(explicit.compare(expected, actual)) == float(want)


def test_cli_switch():
    from click.testing import CliRunner
    from cvpce_amd.cli import cli, _MatcherCommand, _RenderCommand
    assert issubclass(_MatcherCommand, _RenderCommand) and isinstance(cli.commands['eval-planograms'], _MatcherCommand)
    text = CliRunner().invoke(cli, ['eval-planograms', '--help']).output
    assert '--matcher [large|tonioni]' in text and '[default: large]' in text
    bad = CliRunner().invoke(cli, ['eval-planograms', '--matcher', 'best', 'a', 'b'])
    assert bad.exit_code == 2 and '--matcher is one of large, tonioni' in bad.output


# ---- the binding of include/ext/cvpce_amd_tonioni.h ------------------------------------------------------------------------------
def test_header_table_and_library_agree():
    from cvpce_amd import _lib
    assert list(_lib.EXTENSION_HEADERS) == [HEADER] and HEADER not in _lib.HEADERS
    table, symbols = _lib.EXTENSION_HEADERS[HEADER], abi.header_symbols(HEADER)
    assert sorted(table) == symbols == ['cvpce_tonioni_run', 'cvpce_tonioni_select', 'cvpce_tonioni_workspace_bytes']
    exported = ctypes.CDLL(_lib.LIB_PATH)
    for fn in symbols:
        assert hasattr(exported, fn), f'{fn} declared in include/{HEADER} but not exported'
        assert getattr(_lib.lib, fn).restype == table[fn][0] and getattr(_lib.lib, fn).argtypes == table[fn][1], f'{fn}: the table is not bound'


def test_declarations_and_ctypes_agree_in_count_and_kind():
    from cvpce_amd import _lib
    table, declared = _lib.EXTENSION_HEADERS[HEADER], abi.declarations(HEADER)
    assert sorted(declared) == abi.header_symbols(HEADER), 'a declaration the parser cannot read'
    for fn, (c_ret, c_args) in declared.items():
        restype, argtypes = table[fn]
        assert len(argtypes) == len(c_args), f'{fn}: {len(c_args)} arguments declared, {len(argtypes)} in the table'
        assert abi.ctypes_kind(restype) == c_ret, f'{fn}: returns {c_ret}, the table says {abi.ctypes_kind(restype)}'
        for i, (t, kind) in enumerate(zip(argtypes, c_args)):
            assert abi.ctypes_kind(t) == kind, f'{fn}: argument {i} is declared {kind}, the table says {abi.ctypes_kind(t)}'


def test_symbols_and_ops_are_the_header_s_own():
    from cvpce_amd import _lib, torch_ops_tonioni
    symbols = set(abi.header_symbols(HEADER))
    for header, table in _lib.HEADERS.items():
        assert not symbols & set(table) and not symbols & set(abi.header_symbols(header)), header
    words = set(abi.FAMILY_WORDS.values())
    assert torch_ops_tonioni.NAMES == ['tonioni_run', 'tonioni_select']
    for name in list(symbols) + torch_ops_tonioni.NAMES:
        assert 'tonioni' in name and not [w for w in words if w in name], name
    for header in abi.FEATURES:                                         # ... and no other header's names carry this one's word
        assert not [s for s in abi.header_symbols(header) if 'tonioni' in s] and not [n for n in abi.op_module(header).NAMES if 'tonioni' in n]
    # an op stands for every entry point that launches; the workspace size is host-only
    assert sorted('cvpce_' + n for n in torch_ops_tonioni.NAMES) == sorted(s for s in symbols if not s.endswith('_bytes'))
    for name in torch_ops_tonioni.NAMES:
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'cvpce_amd::{name}', 'CUDA'), name
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'cvpce_amd::{name}', 'CPU'), name


def test_limit_is_mirrored_once():
    import re
    from cvpce_amd import planograms_device as pd, torch_ops_tonioni
    text = open(abi.INCLUDE + '/' + HEADER).read()
    assert int(re.search(r'#define CVPCE_TONIONI_MAX_HYPOTHESES (\d+)', text).group(1)) == torch_ops_tonioni.MAX_HYPOTHESES == pd.TONIONI_MAX_HYPOTHESES
    assert 'folds it into include/' in text
