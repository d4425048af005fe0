"""Host-side checks of the matcher's launch plan (csrc/match.hip match_plan through include/cvpce_amd.h cvpce_match_plan): the path, the
core and tile, the grid and the LDS bytes of every launch equal tests/match_plan.py, the restatement of the decision as it stood inside
cvpce_match_topk before the plan existed -- a transcription slip in the cost model would otherwise show only as a slower launch."""
import ctypes
import os
import re

import pytest

import match_plan as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH_SHAPES = [(200, 10000, 512), (200, 10000, 1024), (400, 10000, 1024), (800, 10000, 1024), (1600, 10000, 512), (1600, 10000, 1024),
                (1600, 3200, 1024), (1600, 1000, 1024), (3200, 10000, 1024)]            # the defaults of tools/dev/bench_match.py
SHAPES = BENCH_SHAPES + [(5, 40, 64), (333, 1357, 256), (130, 129, 512), (37, 3200, 1024), (768, 10000, 64), (200, 100, 64)]
FORCED = [(core, nq, mg) for core in (0, 1, 2) for nq in (0, 2, 3, 4, 5) for mg in (0, 1, 2) if not (mg == 1 and nq == 5)]


def query(qn, gn, d, k, f32):
    from cvpce_amd._lib import lib
    out = (ctypes.c_longlong * len(mp.FIELDS))()
    rc = lib.cvpce_match_plan(qn, gn, d, k, int(f32), out)
    return rc, dict(zip(mp.FIELDS, out))


@pytest.fixture
def set_core():
    from cvpce_amd._lib import lib
    try:
        yield lib.cvpce_match_set_core
    finally:
        assert lib.cvpce_match_set_core(0, 0, 0) == 0


def test_bench_shapes_are_the_tools_defaults():
    text = open(os.path.join(ROOT, 'tools', 'dev', 'bench_match.py')).read()
    assert [tuple(int(v) for v in m) for m in re.findall(r'\((\d{3,}), (\d{3,}), (\d{3,})\)', text)] == BENCH_SHAPES


@pytest.mark.parametrize('qn,gn,d', SHAPES)
def test_plan_equals_the_restated_decision(set_core, qn, gn, d):
    from cvpce_amd._lib import lib
    for forced in FORCED:
        assert set_core(*forced) == 0
        for f32 in (False, True):
            for k in (1, 4, 16, 17, gn):
                want = mp.plan(qn, gn, d, k, f32, forced)
                rc, got = query(qn, gn, d, k, f32)
                assert want is not None and rc == 0, (forced, f32, k)
                assert got == want, (forced, f32, k)
                assert lib.cvpce_match_workspace_bytes(qn, gn, k) == want['workspace']
    assert set_core(2, 5, 1) == 1 and set_core(3, 0, 0) == 1 and set_core(0, 6, 0) == 1 and set_core(0, 0, 3) == 1


def test_lds_totals(set_core):
    """The dynamic LDS of every GEMM instance, as the launcher's literals stated it before the layouts were written once."""
    assert set_core(1, 0, 0) == 0
    lds = lambda qn, gn, d, k, f32: query(qn, gn, d, k, f32)[1]
    for k in (1, 17):                                             # select and store
        assert lds(768, 10000, 64, k, True)['lds'] == 131072 and lds(200, 10000, 512, k, True)['tq'] == 128
    p = lds(768, 10000, 64, 1, False)
    assert (p['tq'], p['lds'], p['threads']) == (128, 68096, 256)
    p = lds(768, 10000, 64, 17, False)
    assert (p['path'], p['tq'], p['lds']) == (2, 128, 66560)
    for k in (1, 17):
        p = lds(200, 10000, 512, k, False)
        assert (p['tq'], p['lds']) == (64, 49152)
    for nq in (2, 3, 4, 5):
        for mg in (1, 2):
            if mg == 1 and nq == 5:
                continue
            assert set_core(2, nq, mg) == 0
            p = lds(1600, 10000, 1024, 1, False)
            assert (p['path'], p['nq'], p['mg'], p['threads']) == (1, nq, mg, 512)
            assert p['lds'] == 2 * (128 * mg + 64 * nq) * 128


def test_anchors_of_the_rounds_rule(set_core):
    assert set_core(1, 0, 0) == 0
    # 768 x 10 000: 79 x 6 = 474 tiles of 128 queries are ONE round of 512 slots (cost 1.0); 79 x 12 = 948 tiles of 64 queries are two
    # rounds of 768 slots at 0.6 each (1.2)
    for d in (64, 512, 1024):
        p = query(768, 10000, d, 1, False)[1]
        assert (p['path'], p['tq'], p['tiles_g'], p['tiles_q']) == (0, 128, 79, 6)
    # 200 x 10 000: 158 tiles of 128 or 316 of 64, one round either way: 0.6 < 1.0
    p = query(200, 10000, 512, 1, False)[1]
    assert (p['path'], p['tq'], p['tiles_g'], p['tiles_q']) == (0, 64, 79, 4)


def test_rejected_arguments_stay_rejected():
    assert query(200, 1000, 100, 1, False)[0] == 1 and query(200, 1000, 0, 1, False)[0] == 1        # D % 64 != 0
    assert query(200, 1000, 64, 1001, False)[0] == 1 and query(200, 1000, 64, 0, False)[0] == 1     # k > Gn, k < 1
    # rows x D past 2^32 bytes (the buffer descriptors take 32-bit offsets), rows rounded up to whole tiles
    assert query(5, 2 ** 21, 1024, 1, False)[0] == 1 and query(5, 2 ** 21 - 128, 1024, 1, False)[0] == 1
    assert query(5, 2 ** 21 - 129, 1024, 1, False)[0] == 0 and query(5, 2 ** 20, 1024, 1, True)[0] == 1
    assert query(2 ** 21, 5000, 1024, 1, False)[0] == 1
    for args in ((200, 1000, 100, 1, False), (5, 2 ** 21, 1024, 17, True), (2 ** 21, 5000, 1024, 1, False)):
        assert mp.plan(*args) is None
    # the wider query tiles of the LDS-DMA core reach 2^32 sooner than the 128-row check
    qn = 2 ** 21 - 200
    assert mp.plan(qn, 5000, 1024, 1, False) is None and query(qn, 5000, 1024, 1, False)[0] == 1
    assert query(0, 1000, 64, 1, False)[0] == 0                   # no queries: accepted, nothing to launch
