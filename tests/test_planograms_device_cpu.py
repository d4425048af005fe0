"""CPU-side checks of the device planogram comparator (no compute on a GPU): the kernels' own header, signature table and torch
ops stay apart from the pinned inference ABI and refuse bad arguments on the host; the plain restatement of the device rule
(tests/planogram_device_cases.py) is pinned against the stock host functions wherever the two are comparable."""
import ctypes
import os

import pytest
import torch

import abi
import planogram_device_cases as cases          # tests/planogram_device_cases.py
from cvpce_amd import planograms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIE_FREE_SIZES = (1, 2, 3, 7, 26, 64, 65)


def test_planogram_header_is_exported_and_mirrored():
    """(exported, bound and disjoint from the other headers: test_abi_mirror_cpu.py)"""
    syms = abi.header_symbols('cvpce_amd_planogram.h')
    assert 'cvpce_planogram_graphs' in syms and 'cvpce_planogram_match' in syms


def test_planogram_ops_are_gpu_only():
    from cvpce_amd import torch_ops_planogram  # noqa: F401  (registers the ops)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.planogram_graphs(torch.zeros(2, 4), i32(2), torch.zeros(1), 2, 2, i32(2, 8), torch.zeros(2, 8), i32(2, 8))
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.planogram_match(i32(2, 8), i32(2, 8), i32(2), i32(2), i32(2, 8), i32(2, 8), i32(2), i32(2), i32(1, 2), i32(2), i32(2),
                                            2, 2, 4, i32(4), i32(2, 2), i32(1))


def test_entry_points_reject_bad_arguments_on_the_host():
    """A graph of 0 or 1025 nodes, negative sizes and null pointers are refused before anything is launched; an empty batch is no error."""
    from cvpce_amd._lib import lib
    z = ctypes.c_void_p(0)
    a = ctypes.c_void_p(256)          # (never dereferenced: every call below returns before a launch)
    graphs = lambda b, sum_n, lo, hi, boxes=a, off=a, thr=a, nbr=a, w=a, st=a: lib.cvpce_planogram_graphs(boxes, off, thr, b, sum_n, lo, hi, nbr, w, st, z)
    assert graphs(1, 0, 0, 0) == 1 and graphs(2, 5, 0, 5) == 1                      # n = 0
    assert graphs(1, 1025, 1025, 1025) == 1 and graphs(2, 1026, 1, 1025) == 1       # n = 1025
    assert graphs(-1, 4, 4, 4) == 1 and graphs(1, -4, 4, 4) == 1 and graphs(1, 4, -4, 4) == 1 and graphs(1, 4, 4, -4) == 1
    assert graphs(1, 4, 5, 4) == 1 and graphs(2, 4, 4, 4) == 1 and graphs(1, 9, 4, 4) == 1      # bounds that cannot hold
    for k in ('boxes', 'off', 'thr', 'nbr', 'w', 'st'):
        assert graphs(1, 4, 4, 4, **{k: z}) == 1, k
    assert graphs(1, 4, 4, 4, boxes=ctypes.c_void_p(260)) == 1                       # misaligned boxes
    assert graphs(0, 0, 0, 0) == 0 and graphs(0, 0, 1, 1024, boxes=z, off=z) == 0   # B = 0

    def match(p=1, s1=4, s2=4, m1=4, m2=4, so=4, sh=16, ws=a, wsb=64, **null):
        ptr = {k: a for k in ('nbr1', 'stamp1', 'label1', 'off1', 'nbr2', 'stamp2', 'label2', 'off2', 'params', 'hyp_off', 'out_off', 'pairs', 'count')}
        ptr.update(null)
        return lib.cvpce_planogram_match(ptr['nbr1'], ptr['stamp1'], ptr['label1'], ptr['off1'], ptr['nbr2'], ptr['stamp2'], ptr['label2'], ptr['off2'],
                                         ptr['params'], ptr['hyp_off'], ptr['out_off'], p, s1, s2, m1, m2, so, sh, ws, wsb, ptr['pairs'], ptr['count'], z)
    assert match(m1=0) == 1 and match(m2=0) == 1 and match(m1=1025) == 1 and match(m2=1025) == 1
    assert match(p=-1) == 1 and match(s1=-4) == 1 and match(s2=-4) == 1 and match(so=-1) == 1 and match(sh=-1) == 1 and match(sh=2 ** 31) == 1
    for k in ('nbr1', 'stamp1', 'label1', 'off1', 'nbr2', 'stamp2', 'label2', 'off2', 'params', 'hyp_off', 'out_off', 'pairs', 'count'):
        assert match(**{k: z}) == 1, k
    assert match(ws=z) == 1 and match(wsb=63) == 1                                   # no workspace, a short one
    assert match(p=0) == 0 and match(p=0, m1=0, m2=0, ws=z, wsb=0, sh=0, off1=z) == 0
    assert lib.cvpce_planogram_match_workspace_bytes(16) == 64 and lib.cvpce_planogram_match_workspace_bytes(-1) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the rule model against the stock host functions
# ---------------------------------------------------------------------------------------------------------------------
def _structure(adj):
    return [[(nb, d) for nb, d, _ in row] for row in adj]


def test_generator_and_seeds():
    for n, seed in cases.TIE_FREE_SEEDS.items():
        boxes, labels = cases.scene(n, seed)
        assert boxes.shape == (n, 4) and len(labels) == n and set(labels) <= set(cases.NAMES)
        assert torch.equal(boxes, boxes.round()) and bool((boxes[:, :2] >= 0).all()) and bool((boxes[:, :2] < 2000).all())
        wh = boxes[:, 2:] - boxes[:, :2]
        assert bool((wh >= 40).all()) and bool((wh < 120).all()) and bool((wh % 2 == 0).all())
        assert cases.is_tie_free(boxes) and cases.first_tie_free_seed(n) == seed
    assert not cases.is_tie_free(cases.grid(4, 6, 0)[0])                                      # exact ties
    assert not cases.is_tie_free(torch.tensor([[0., 0, 10, 10], [100, 0, 110, 10], [0, 100, 10, 110]]).repeat(2, 1)[:4])   # a shared centre
    on_boundary = torch.tensor([[0., 0, 2, 2], [10000, 4142, 10002, 4144], [3000, 9000, 3002, 9002]])   # atan(.4142) is 1.6e-6 rad from pi/8
    assert not cases.is_tie_free(on_boundary) and cases.is_tie_free(on_boundary, margin=1e-6)


@pytest.mark.parametrize('n', TIE_FREE_SIZES)
def test_model_equals_stock_build_graph_on_tie_free_scenes(n):
    """adjacency lists with direction, order and bitwise weights (cases.assert_same_as_stock: bitwise wherever this machine's
    torch.sqrt, which the host's distances go through, returns the correctly rounded root)"""
    boxes, labels = cases.scene(n, cases.TIE_FREE_SEEDS[n])
    host = planograms.build_graph(boxes, labels, 0.5)
    cases.assert_same_as_stock(cases.adjacency_of_tables(*cases.model_graph(boxes, 0.5)), cases.adjacency_of_host(host), boxes)
    if n > 3:
        assert host.number_of_edges() > 0


def test_model_at_25_points_equals_stock_structure_and_weights_to_2_ulps():
    """up to 25 points torch.cdist takes its direct path, within 1 ulp of sqrt(dx*dx + dy*dy) but not equal"""
    boxes, labels = cases.scene(25, cases.TIE_FREE_SEEDS[25])
    host = cases.adjacency_of_host(planograms.build_graph(boxes, labels, 0.5))
    model = cases.adjacency_of_tables(*cases.model_graph(boxes, 0.5))
    assert _structure(model) == _structure(host) and sum(len(r) for r in host) > 0
    for hr, mr in zip(host, model):
        for (_, _, hw), (_, _, mw) in zip(hr, mr):
            ulp = float(torch.nextafter(torch.tensor(hw, dtype=torch.float32), torch.tensor(float('inf'))) - hw)
            assert abs(hw - mw) <= 2 * ulp


def test_model_on_the_golden_cases(golden_dir):
    """equal edge sets everywhere; equal adjacency order on the four jittered (tie-free) detection graphs"""
    edges = lambda adj: sorted((i, nb, d) for i, row in enumerate(adj) for nb, d, _ in row)
    for c in cases.golden_cases(golden_dir):
        for side in ('expected', 'actual'):
            boxes, labels = c[f'{side}_boxes'], c[f'{side}_labels']
            host = cases.adjacency_of_host(planograms.build_graph(boxes, labels, 0.5))
            model = cases.adjacency_of_tables(*cases.model_graph(boxes, 0.5))
            assert edges(model) == edges(host)
            assert edges(model) == [(a, b, d) for a, b, d, _ in c[f'{side}_edges']]
            if side == 'actual':
                assert _structure(model) == _structure(host)


def test_exact_root_is_the_correctly_rounded_one():
    g = torch.Generator().manual_seed(1)
    x = torch.cat((torch.randint(0, 2 ** 24, (20000,), generator=g).float(), torch.rand(20000, generator=g) * 1e6, torch.tensor([0.0, 1.0, 2.0, 238554.0, 697.0])))
    want = torch.tensor([__import__('math').sqrt(v) for v in x.tolist()], dtype=torch.float64).float()     # libm's double root, rounded once more: exact for fp32 inputs
    assert torch.equal(cases.exact_root(x).view(torch.int32), want.view(torch.int32))
    assert cases.exact_root(torch.tensor([238554.0])).view(torch.int32).item() == 1140078015


def test_model_tie_rule_and_shared_centres():
    """lower index first at equal distance; a pair at d = 0 is skipped; empty slots are (-1, 0, -1)"""
    boxes = torch.tensor([[100., 100, 120, 120], [200, 100, 220, 120], [0, 100, 20, 120], [100, 100, 120, 120], [100, 0, 120, 20]])
    nbr, weight, stamp = cases.model_graph(boxes, 10.0)
    assert nbr[0].tolist() == [1, -1, -1, -1, 2, -1, 4, -1]           # E, W, S(-y) at distance 100: node 3 shares the centre and is skipped
    assert stamp[0].tolist() == [0, -1, -1, -1, 2, -1, 4, -1]         # candidates 1, 2, 4 tie at d = 100: taken in index order
    assert nbr[3].tolist() == [-1] * 8 or nbr[3, 0] != 0              # node 3 never links to node 0
    assert not bool(((nbr == 3) & (torch.arange(5)[:, None] == 0)).any())
    empty = nbr < 0
    assert bool((weight[empty] == 0).all()) and bool((stamp[empty] == -1).all())
    filled = stamp[~empty]
    assert sorted(filled.tolist()) == list(range(len(filled)))          # stamps of a graph without unlinking: 0 .. 2E-1


def _device_graph(boxes, labels, thresh_size=0.5):
    from cvpce_amd import planograms_device as pd
    return pd.Graph(labels, *cases.model_graph(boxes, thresh_size))


def _pairs():
    out = []
    for n in (2, 3, 7, 26, 64, 65):
        eb, el = cases.scene(n, cases.TIE_FREE_SEEDS[n])
        out.append((f'scene{n}', eb, el, *cases.detections_of(eb, el, 7 + n)))
    for rows, cols in ((4, 6), (8, 25)):
        eb, el = cases.grid(rows, cols, 3)
        out.append((f'grid{rows}x{cols}', eb, el, *cases.detections_of(eb, el, 11)))
    eb, el = cases.repeated_blocks(5)
    out.append(('blocks', eb, el, *cases.detections_of(eb, el, 5, drop=0.2)))
    out.append(('blocks_self', eb, el, eb, el))
    return out


@pytest.mark.parametrize('case', _pairs(), ids=lambda c: c[0])
def test_round_trip_through_networkx(case):
    """`to_networkx` of the model's tables, fed to the host large_common_subgraph, equals the plain restatement of the match rule
    over the tables -- as a set and in the order the host's set is iterated."""
    from cvpce_amd import planograms_device as pd
    _, eb, el, ab, al = case
    ge, ga = _device_graph(eb, el), _device_graph(ab, al)
    n1, n2 = pd.to_networkx(ge), pd.to_networkx(ga)
    assert list(n1.nodes) == list(range(len(el))) and [n1.nodes[i]['label'] for i in n1] == el
    assert cases.adjacency_of_host(n1) == cases.adjacency_of_tables(ge.nbr, ge.weight, ge.stamp)
    for kw in ({}, {'min_score': -0.5, 'stop_at_fraction': 0.9}, {'min_score': 0.0, 'stop_at_fraction': 1.0}):
        want = planograms.large_common_subgraph(n1, n2, **kw)
        got = cases.model_match((ge.nbr, ge.weight, ge.stamp), el, (ga.nbr, ga.weight, ga.stamp), al, **kw)
        assert len(got) == len(set(got)) and set(got) == want
        rebuilt = set()
        for pair in got:
            rebuilt.add(pair)
        assert list(rebuilt) == list(want)                              # (what finalize_via_ransac's zip(*solution) walks)


def test_min_agree_is_the_float_test():
    from cvpce_amd import planograms_device as pd
    assert pd.min_agree_for(-0.2) == 2
    for min_score in (-1.5, -1.0, -0.99, -0.5, -0.25, -0.2, -0.125, -0.01, 0.0, 0.3):
        k = pd.min_agree_for(min_score)
        assert all((-(a / 8) > min_score) == (a < k) for a in range(9))


def test_comparator_defaults_are_unchanged_and_the_cli_has_the_switch():
    from click.testing import CliRunner
    from cvpce_amd import production
    from cvpce_amd.cli import cli
    cmp = production.PlanogramComparator()
    assert cmp.graph_threshold == 0.5 and cmp.device_graphs is False and cmp.host_routed == 0
    cmd = cli.commands['eval-planograms']
    assert not any('device' in p.name for p in cmd.params)
    text = ''.join(CliRunner().invoke(cli, ['eval-planograms', '--help']).output.split())
    assert '--device-graphs/--no-device-graphs' in text and '[default:off]' in text
    # with the switch off the comparator is the host path: a golden case keeps its value, compare_batch is the plain loop
    c = cases.golden_cases(os.path.join(ROOT, 'tests', 'golden'))[1]
    e = {'boxes': c['expected_boxes'], 'labels': c['expected_labels']}
    a = {'boxes': c['actual_boxes'], 'labels': c['actual_labels']}
    assert float(cmp.compare(e, a)) == float(cmp.compare_batch([e], [a])[0]) == pytest.approx(23 / 24)
