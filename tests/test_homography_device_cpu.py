"""CPU-side checks of the comparator's device tail (no compute on a GPU): the kernels' header, signature table and torch ops stay
apart from every pinned table and refuse bad arguments on the host; the plain restatement of the tail rule
(tests/homography_device_cases.py) is pinned against `planograms._dlt` and `planograms.finalize_via_ransac` wherever the two are
comparable."""
import ctypes

import numpy as np
import pytest
import torch

import abi
import homography_device_cases as hc
import planogram_device_cases as cases
from cvpce_amd import metrics, planograms

# the model's refit against planograms._dlt on the same correspondences, as the largest distance between the projected corners:
# 1.43e-11 px is the largest value measured over the cases of test_refit_is_the_minimiser_of_dlt (scene of 26 boxes, jittered)
REFIT_MEASURED_PX = 1.43e-11
REFIT_TOLERANCE_PX = 16 * REFIT_MEASURED_PX
# the model's positions against finalize_via_ransac's where both refit the same inliers: fp32 positions of up to 3600 px, both sides
# rounded from homographies that agree to 1e-11 px, the host's through a matrix-vector product, the rule's through its own
# expression: 7.4e-4 px (3 ulp at 3600 px) is the largest measured over the cases of test_whole_model_against_the_host_tail
POSITIONS_MEASURED_PX = 7.4e-4
POSITIONS_TOLERANCE_PX = 16 * POSITIONS_MEASURED_PX


# ---------------------------------------------------------------------------------------------------------------------
# boundary
# ---------------------------------------------------------------------------------------------------------------------
def test_homography_header_is_exported_and_mirrored():
    """(exported, bound and disjoint from the other headers: test_abi_mirror_cpu.py)"""
    syms = abi.header_symbols('cvpce_amd_homography.h')
    assert syms == ['cvpce_homography_finish', 'cvpce_homography_ransac', 'cvpce_homography_workspace_bytes']


def test_homography_ops_are_gpu_only():
    from cvpce_amd import torch_ops_homography  # noqa: F401  (registers the ops)
    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32)
    f64 = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.homography_ransac(torch.zeros(2, 4), i32(2), torch.zeros(2, 4), i32(2), i32(2, 2), i32(1), i32(2), f64(1, 2), 2, 0, 16, i32(2))
    with pytest.raises(NotImplementedError, match='CPU'):
        torch.ops.cvpce_amd.homography_finish(torch.zeros(2, 4), i32(2), i32(2), torch.zeros(2, 4), i32(2), i32(2), i32(2, 2), i32(1), i32(2), f64(1, 2),
                                              2, 2, 2, 0, 16, i32(2), i32(1), f64(9), i32(1), i32(1), i32(1), i32(2), i32(2), torch.zeros(2, 4))


def test_entry_points_reject_bad_arguments_on_the_host():
    """counts out of range, 0 and 65 537 hypotheses, 1025 pairs, a workspace one byte short, null pointers: status 1, nothing launched"""
    from cvpce_amd._lib import lib
    z = ctypes.c_void_p(0)
    a = ctypes.c_void_p(256)          # (never dereferenced: every call below returns before a launch)
    names = ('boxes1', 'off1', 'boxes2', 'off2', 'pairs', 'count', 'out_off', 'params')
    outs = ('status', 'H', 'winner', 'winner_count', 'final_count', 'matched_expected', 'matched_actual', 'expected_positions')

    def ransac(b=1, s1=4, s2=4, so=4, mp=4, k=16, ws=a, wsb=8, **ptr):
        p = {n: ptr.get(n, a) for n in names}
        return lib.cvpce_homography_ransac(*[p[n] for n in names], b, s1, s2, so, mp, 0, k, ws, wsb, z)

    def finish(b=1, s1=4, s2=4, so=4, m1=4, m2=4, mp=4, k=16, ws=a, wsb=8, **ptr):
        p = {n: ptr.get(n, a) for n in names + ('label1', 'label2') + outs}
        return lib.cvpce_homography_finish(p['boxes1'], p['label1'], p['off1'], p['boxes2'], p['label2'], p['off2'], p['pairs'], p['count'], p['out_off'],
                                           p['params'], b, s1, s2, so, m1, m2, mp, 0, k, ws, wsb, *[p[n] for n in outs], z)
    for call in (ransac, finish):
        assert call(b=-1) == 1 and call(s1=-4) == 1 and call(s2=-4) == 1 and call(so=-1) == 1                    # counts out of range
        assert call(k=0) == 1 and call(k=65537) == 1 and call(k=-1) == 1                                          # hypotheses
        assert call(mp=0) == 1 and call(mp=1025) == 1                                                             # pairs
        assert call(wsb=7) == 1 and call(ws=z) == 1 and call(k=257, wsb=15) == 1 and call(b=3, k=65536, wsb=3 * 256 * 8 - 1) == 1
        for n in names:
            assert call(**{n: z}) == 1, n
        assert call(boxes1=ctypes.c_void_p(260)) == 1 and call(boxes2=ctypes.c_void_p(264)) == 1                 # misaligned boxes
        assert call(b=0) == 0 and call(b=0, ws=z, wsb=0, off1=z, count=z) == 0                                     # B = 0: nothing to do
    assert finish(m1=0) == 1 and finish(m1=1025) == 1 and finish(m2=0) == 1 and finish(m2=1025) == 1
    for n in ('label1', 'label2') + outs:
        assert finish(**{n: z}) == 1, n
    # all pointers null, as the header allows a caller to probe: still status 1, nothing launched
    assert lib.cvpce_homography_ransac(*[z] * 8, 1, 4, 4, 4, 4, 0, 16, z, 8, z) == 1
    assert lib.cvpce_homography_finish(*[z] * 10, 1, 4, 4, 4, 4, 4, 4, 0, 16, z, 8, *[z] * 8, z) == 1
    ws = lib.cvpce_homography_workspace_bytes
    assert ws(1, 1) == 8 and ws(1, 256) == 8 and ws(1, 257) == 16 and ws(8, 2048) == 8 * 8 * 8 and ws(3, 65536) == 3 * 256 * 8
    assert ws(0, 16) == 0 and ws(-1, 16) == 0 and ws(1, 0) == 0 and ws(1, 65537) == 0


# ---------------------------------------------------------------------------------------------------------------------
# the rule model against the host functions
# ---------------------------------------------------------------------------------------------------------------------
def _through(h, pts):
    x, y = pts[:, 0], pts[:, 1]
    w = h[2, 0] * x + h[2, 1] * y + h[2, 2]
    return np.stack(((h[0, 0] * x + h[0, 1] * y + h[0, 2]) / w, (h[1, 0] * x + h[1, 1] * y + h[1, 2]) / w), axis=1)


def _refit_cases():
    out = []
    for n in (3, 7, 26, 65, 200, 1024):
        for jitter in (0.0, 3.0):
            b1, _ = cases.scene(n, 0)
            g = torch.Generator().manual_seed(n)
            b2 = b1 * 1.7 + torch.tensor([30.0, 12.0, 30.0, 12.0]) + (torch.rand(n, 4, generator=g) * 2 - 1) * jitter
            src, dst = hc.points_of([(i, i) for i in range(n)], b1.numpy(), b2.numpy())
            corners = np.concatenate((b1.numpy()[:, :2], b1.numpy()[:, 2:])).astype(np.float64)
            out.append((f'scene{n}_jitter{jitter:g}', src, dst, corners))
    g = torch.Generator().manual_seed(3)                                      # the perspective case of tests/test_planograms_cpu.py, 300 points, 1 px noise
    src = (torch.rand(300, 2, generator=g, dtype=torch.float64) * 800).float()
    dst = torch.tensor(_through(hc.H_TRUE, src.double().numpy())) + torch.randn(300, 2, generator=g, dtype=torch.float64) * 1.0
    out.append(('perspective300', src.numpy(), dst.float().numpy(), src.double().numpy()))
    return out


def test_refit_is_the_minimiser_of_dlt():
    """the 45-entry normal matrix and its Jacobi eigenvector against the SVD of planograms._dlt, as projected corner positions"""
    assert REFIT_TOLERANCE_PX <= 1e-6          # a condition, not a measurement: beyond it the algorithm is not _dlt's minimiser
    worst = 0.0
    for name, src, dst, corners in _refit_cases():
        h, ok = hc.refit(src, dst, np.ones(len(src), dtype=bool))
        host = planograms._dlt(torch.tensor(src).double(), torch.tensor(dst).double())
        assert ok and host is not None and h[2, 2] == 1.0, name
        d = float(np.abs(_through(h, corners) - _through(host.numpy(), corners)).max())
        print(f'{name}: {d:.3g} px')
        worst = max(worst, d)
        assert d <= REFIT_TOLERANCE_PX, (name, d)
    print(f'largest: {worst:.3g} px')


def _overlapping_scenes():
    out = []
    for k, (rows, cols) in enumerate(((4, 5), (4, 6), (5, 6), (5, 8), (6, 8), (6, 10), (7, 10), (8, 10), (8, 12), (9, 14), (10, 16), (8, 25))):
        # under 64 x 96 boxes the neighbours overlap at IoU 0.23, under 80 x 120 at 0.33: above the threshold, so a box claims its
        # neighbours' detections as well
        b1, l1 = cases.grid(rows, cols, k, pitch=(40, 60), size=(80, 120) if k % 2 else (64, 96))
        l1 = [cases.NAMES[cases.NAMES.index(l) % 3] for l in l1]
        g = torch.Generator().manual_seed(50 + k)
        b2 = b1 * 1.7 + torch.tensor([30.0, 12.0, 30.0, 12.0]) + (torch.rand(len(l1), 4, generator=g) * 2 - 1) * 3
        keep = [i for i in range(len(l1)) if i % 7 != k % 7]                  # some expected boxes have no detection of their own
        out.append((b1, l1, b2[keep].contiguous(), [l1[i] for i in keep], {(i, j) for j, i in enumerate(keep)}))
    return out


def test_claim_rule_equals_the_host_loop():
    """given the host's own expected positions, the sort-free claim gives finalize_via_ransac's two masks exactly"""
    scenes = _overlapping_scenes()
    assert len(scenes) >= 12 and {len(s[1]) for s in scenes} >= {20, 200}
    more_detections = 0
    for b1, l1, b2, l2, matching in scenes:
        me, ma, pos, *_ = planograms.finalize_via_ransac(matching, b1, b2, l1, l2, reproj_threshold=10, iou_threshold=0.3,
                                                         return_matched_actual=True, return_expected_positions=True)
        assert me is not None
        id1, id2 = hc.label_ids(l1, l2)
        got_e, got_a = hc.claim(pos.numpy(), b2.numpy(), id1, id2, 0.3)
        assert torch.equal(torch.from_numpy(got_e), me) and torch.equal(torch.from_numpy(got_a), ma)
        assert torch.equal(torch.from_numpy(hc.iou_matrix(pos.numpy(), b2.numpy())).view(torch.int32), metrics.box_iou(pos, b2).view(torch.int32))
        more_detections += int(ma.sum()) > int(me.sum())
    assert more_detections >= 1


def _whole_cases(golden_dir):
    c = cases.golden_cases(golden_dir)[1]
    out = [('golden1', c['expected_boxes'], c['expected_labels'], c['actual_boxes'], c['actual_labels'])]
    for n in (7, 26, 65, 200):
        eb, el = cases.scene(n, 0)
        out.append((f'scene{n}', eb, el, *cases.detections_of(eb, el, 7 + n)))
    return out


def _host_refit_mask(src, dst, reproj_threshold, max_iters=2000, confidence=0.995, seed=0):
    """The inlier mask planograms.find_homography refits over -- its loop replayed with its own helpers, because it returns the mask
    under the refit homography only -> (mask the refit runs over, mask under the refit)."""
    src, dst = src.to(torch.float64), dst.to(torch.float64)
    n = len(src)
    gen = torch.Generator().manual_seed(seed)
    best_mask, best_count, iters, it = None, 0, max_iters, 0
    while it < iters:
        it += 1
        pick = torch.randperm(n, generator=gen)[:4]
        h = planograms._dlt(src[pick], dst[pick])
        if h is None:
            continue
        mask = planograms._reproj_err(h, src, dst) < reproj_threshold
        count = int(mask.sum())
        if count > best_count:
            best_mask, best_count = mask, count
            w = count / n
            if w >= 1.0:
                break
            denom = torch.log1p(torch.tensor(-(w ** 4)))
            iters = min(max_iters, int(torch.ceil(torch.log(torch.tensor(1 - confidence)) / denom).item()) + 1)
    return best_mask, planograms._reproj_err(planograms._dlt(src[best_mask], dst[best_mask]), src, dst) < reproj_threshold


def test_whole_model_against_the_host_tail(golden_dir):
    """Where the model refits the points the host refits (equal masks before the refit, and equal masks after it), the two tails
    differ by rounding alone: equal matched boxes, positions within rounding.  (Equal masks under the refit homography alone do not
    say that: scene65's are equal while the host's sample leaves three points out of its refit, and the positions differ by 1.6 px.)"""
    comparable, worst = 0, 0.0
    for name, eb, el, ab, al in _whole_cases(golden_dir):
        matching = planograms.large_common_subgraph(planograms.build_graph(eb, el, 0.5), planograms.build_graph(ab, al, 0.5))
        pairs = list(matching)                                                # (the order finalize_via_ransac's zip(*solution) walks)
        assert len(pairs) >= 2, name
        me, ma, pos, *_ = planograms.finalize_via_ransac(matching, eb, ab, el, al, reproj_threshold=10, return_matched_actual=True,
                                                         return_expected_positions=True)
        nodes1, nodes2 = (list(x) for x in zip(*pairs))
        p1, p2 = planograms._three_points(eb[nodes1]), planograms._three_points(ab[nodes2])
        _, host_mask = planograms.find_homography(p1, p2, 10)
        host_refit_mask, replayed = _host_refit_mask(p1, p2, 10)
        assert torch.equal(replayed, host_mask), name
        same = torch.tensor([[x == y for y in al] for x in el])
        assert float((metrics.box_iou(pos, ab)[same] - 0.5).abs().min()) >= 1e-4, f'{name}: an IoU within 1e-4 of the threshold'
        got = hc.model_tail(eb, el, ab, al, pairs, 10.0, 0.5, 0, 2048)
        assert got['status'] == hc.OK and got['winner_count'] >= 4, name
        if name == 'golden1':
            assert int(got['matched_expected'].sum()) == 23 and len(el) == 24
        print(f"{name}: {len(pairs)} pairs, refit over {int(got['winner_mask'].sum())} (model) / {int(host_refit_mask.sum())} (host) of {len(p1)} points")
        if not (torch.equal(torch.from_numpy(got['final_mask']), host_mask) and torch.equal(torch.from_numpy(got['winner_mask']), host_refit_mask)):
            continue
        comparable += 1
        assert torch.equal(torch.from_numpy(got['matched_expected']), me) and torch.equal(torch.from_numpy(got['matched_actual']), ma), name
        d = float((torch.from_numpy(got['expected_positions']) - pos).abs().max())
        print(f'{name}: positions within {d:.3g} px of the host\'s (largest coordinate {float(pos.abs().max()):.0f})')
        worst = max(worst, d)
        assert d <= POSITIONS_TOLERANCE_PX, (name, d)
    print(f'largest: {worst:.3g} px')
    assert comparable >= 3


def test_winner_rule():
    """highest inlier count, lowest hypothesis at equal counts; 20 % permuted pairs end up outside the winner's mask"""
    c = hc.tail_case(40, 'permuted')
    m, n = 40, 120
    bad = sorted(k + j * m for k in c['wrong'] for j in range(3))
    assert len(c['wrong']) == 8
    src, dst = hc.points_of(c['pairs'], c['b1'].numpy(), c['b2'].numpy())
    seed = next(s for s in range(64) if set(hc.sample(s, [0], n)[0].tolist()) & set(bad))      # hypothesis 0 draws a permuted point
    got = hc.model_tail(c['b1'], c['l1'], c['b2'], c['l2'], c['pairs'], 10.0, 0.5, seed, 512)
    assert got['status'] == hc.OK and got['winner'] != 0
    assert np.nonzero(~got['winner_mask'])[0].tolist() == bad and got['winner_count'] == n - len(bad)
    # the winner is the FIRST hypothesis with the largest count
    na, nb = hc.normalise(src)[0], hc.normalise(dst)[0]
    h, ok = hc.minimal(hc.sample(seed, np.arange(512), n), src, dst, na, nb)
    counts = np.where(ok, (hc.errors(h, src, dst) < 10.0).sum(axis=1), 0)
    assert counts.max() == got['winner_count'] and got['winner'] == int(np.nonzero(counts == counts.max())[0][0])
    assert int((counts == counts.max()).sum()) > 1, 'the case was meant to have equal counts'
    # one hypothesis: it is hypothesis 0, or there is no homography
    for s in range(6):
        one = hc.model_tail(c['b1'], c['l1'], c['b2'], c['l2'], c['pairs'], 10.0, 0.5, s, 1)
        assert one['winner'] == 0 and one['status'] in (hc.OK, hc.NONE)
        assert (one['status'] == hc.OK) == (counts_of_first(s, src, dst, n) >= 4)


def counts_of_first(seed, src, dst, n):
    h, ok = hc.minimal(hc.sample(seed, [0], n), src, dst, hc.normalise(src)[0], hc.normalise(dst)[0])
    return int(np.where(ok, (hc.errors(h, src, dst) < 10.0).sum(axis=1), 0)[0])


def test_sampler_draws_four_distinct_indices_from_a_stateless_hash():
    for n in (4, 5, 6, 66, 3072):
        s = hc.sample(7, np.arange(4096), n)
        assert s.min() >= 0 and s.max() < n
        assert all(len(set(row)) == 4 for row in s.tolist())
        assert np.array_equal(s[100:200], hc.sample(7, np.arange(100, 200), n))          # (seed, t, n) alone decide a sample
        if n >= 66:
            assert len(np.unique(s)) == min(n, len(np.unique(s))) and len(np.unique(s)) > n // 2
    assert int(hc.hash32(0, [0], 0)[0]) == _fmix(0x9E3779B9) and int(hc.hash32(5, [3], 2)[0]) == _fmix((5 + 0x9E3779B9 * 15) & 0xFFFFFFFF)


def _fmix(x):
    x ^= x >> 16
    x = (x * 0x85EBCA6B) & 0xFFFFFFFF
    x ^= x >> 13
    x = (x * 0xC2B2AE35) & 0xFFFFFFFF
    return x ^ (x >> 16)


def test_status_rules_of_the_model():
    c = hc.tail_case(5, 'clean')
    args = (c['b1'], c['l1'], c['b2'], c['l2'])
    assert hc.model_tail(*args, [], hypotheses=16)['status'] == hc.NONE
    assert hc.model_tail(*args, [(len(c['l1']), 0)], hypotheses=16)['status'] == hc.INVALID
    assert hc.model_tail(*args, [(0, -1)], hypotheses=16)['status'] == hc.INVALID
    one = hc.model_tail(*args, c['pairs'][:1], hypotheses=64)
    assert one['status'] == hc.OK and len(one['points'][0]) == 5                        # m = 1: the other two corners are appended
    same = c['b1'][:1].repeat(len(c['l1']), 1)
    assert hc.model_tail(same, c['l1'], same, c['l2'], c['pairs'], hypotheses=16)['status'] == hc.NONE
    nan = c['b2'].clone()
    nan[0, 0] = float('nan')
    assert hc.model_tail(c['b1'], c['l1'], nan, c['l2'], c['pairs'], hypotheses=16)['status'] == hc.NONE


# ---------------------------------------------------------------------------------------------------------------------
def test_defaults_are_unchanged_and_the_cli_has_the_switch():
    from click.testing import CliRunner
    from cvpce_amd import production
    from cvpce_amd.cli import cli
    cmp = production.PlanogramComparator()
    assert cmp.device_graphs is False and cmp.device_tail is False
    assert production.PlanogramComparator(device_graphs=True).device_tail is False
    with pytest.raises(ValueError):
        production.PlanogramComparator(device_tail=True)
    assert production.PlanogramComparator(device_graphs=True, device_tail=True).device_tail is True
    cmd = cli.commands['eval-planograms']
    assert not any('device' in p.name for p in cmd.params)
    text = ''.join(CliRunner().invoke(cli, ['eval-planograms', '--help']).output.split())
    assert '--device-tail/--no-device-tail' in text and text.count('[default:off]') >= 2 and '--device-graphs/--no-device-graphs' in text
    alone = CliRunner().invoke(cli, ['eval-planograms', '--device-tail', 'a', 'b'])
    assert alone.exit_code == 2 and '--device-tail needs --device-graphs' in alone.output
    both = CliRunner().invoke(cli, ['eval-planograms', '--device-graphs', '--device-tail', 'a', 'b'])          # (gets as far as the missing files)
    assert both.exit_code == 2 and 'needs --device-graphs' not in both.output
    from cvpce_amd import planograms_device as pd
    assert pd.RANSAC_HYPOTHESES == 2048
