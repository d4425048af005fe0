"""Host-side checks of the launch plan of the detector's post-processing (csrc/detect.hip detect_plan through include/cvpce_amd.h
cvpce_detect_plan): the capacity, chunked or one-kernel decode and why, the chunk list, the dynamic LDS of nms_sort, the NMS phases, the
number of launches and the workspace layout equal tests/detect_plan.py, the restatement of the decision as it stood inside
cvpce_detect_postprocess, launch_postprocess and cvpce_detect_workspace_bytes before the plan existed."""
import ctypes

import pytest

import detect_plan as dp

DEFAULT = [(100, 104), (50, 52), (25, 26), (13, 13), (7, 7)]          # 800 x 832 padded; LARGE of test_gpu_detector_options.py
SMALL = [(64, 80), (32, 40), (16, 20), (8, 10), (4, 5)]
SWITCHES = ('CVPCE_DECODE_ONE_KERNEL', 'CVPCE_NMS_ONE_PHASE')


query = dp.query


def agreed(grids, n, a, k, topk, dpi):
    """the plan, after comparing it field for field with the restated decision"""
    from cvpce_amd._lib import lib
    want = dp.plan(grids, n, a, k, topk, dpi)
    rc, got = query(grids, n, a, k, topk, dpi)
    assert want is not None and rc == 0, (grids, n, a, k, topk, dpi)
    assert got == want, (grids, n, a, k, topk, dpi)
    assert got['workspace'] == lib.cvpce_detect_workspace_bytes(n, len(grids), topk)
    offs = [got['off_' + p] for p in dp.PARTS]
    assert offs[0] == 0 and offs == sorted(offs) and all(o % 256 == 0 for o in offs)
    sizes = [s for _, s in dp.carve(n, len(grids), topk, got['cap'])]
    assert all(o + s <= nxt for o, s, nxt in zip(offs, sizes, offs[1:]))
    assert offs[-1] + (sizes[-1] + 255) // 256 * 256 <= got['workspace']
    return got


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)


def test_field_count_is_the_headers():
    import os
    import re
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, 'include', 'cvpce_amd.h')).read()
    assert int(re.search(r'#define CVPCE_DETECT_PLAN_FIELDS (\d+)', text).group(1)) == len(dp.FIELDS)


@pytest.mark.parametrize('n', [1, 2, 8])
def test_default_geometry(n):
    for dpi, limit, launches in ((1000, 0, 5), (200, 1600, 7), (150, 1216, 7), (100, 1024, 7)):
        p = agreed(DEFAULT, n, 9, 1, 1000, dpi)
        assert (p['cap'], p['chunked'], p['why']) == (1024, 1, dp.CHUNKED)
        assert [p[f'chunk_first{l}'] for l in range(6)] == [0, 12, 15, 16, 17, 18] and p['chunks'] == 18
        assert (p['Tmax'], p['words'], p['sort_lds']) == (5056, 79, 5 * 1024 * 4)
        assert (p['limit'], p['launches']) == (limit, launches)
    # K = 3: P3 has 280 800 logits = 35 chunks, more than the 32 runs one merge workgroup holds
    p = agreed(DEFAULT, n, 9, 3, 1000, 1000)
    assert (p['chunked'], p['why'], p['launches']) == (0, dp.MERGE_LIMIT, 4)
    assert p['chunk_first1'] == 32                                            # (the level's runs are capped, as the chunk list always was)
    assert agreed(DEFAULT, n, 9, 3, 1000, 300)['launches'] == 6


def test_wide_capacity():
    p = agreed(SMALL, 2, 9, 1, 1500, 3000)
    assert (p['cap'], p['chunked'], p['chunk_first1'], p['sort_lds']) == (4096, 1, 6, 5 * 1500 * 4)
    p = agreed(SMALL, 2, 9, 2, 4096, 3000)                                    # P3 12 chunks, one merge workgroup holds 8 runs of 4096
    assert (p['cap'], p['chunked'], p['why'], p['chunk_first1']) == (4096, 0, dp.MERGE_LIMIT, 8)
    p = agreed(DEFAULT, 2, 9, 1, 4096, 3000)
    assert (p['cap'], p['sort_lds'], p['Tmax'], p['words']) == (4096, 81920, 20480, 320) and p['sort_lds'] > 64 * 1024
    assert agreed(DEFAULT, 2, 9, 1, 1024, 3000)['sort_lds'] == 20480
    assert agreed(DEFAULT, 2, 9, 1, 1025, 3000)['cap'] == 4096 and agreed(DEFAULT, 2, 9, 3, 2048, 2500)['cap'] == 4096
    assert agreed(SMALL, 2, 9, 1, 4096, 1000)['limit'] == 8000                # the two-phase case of the wide parity test


def test_workspace_room_fallback():
    # one level of 110 x 110 x 9 = 108 900 logits: 14 chunks fit one merge workgroup (32) but not the level's 12 runs of workspace
    p = agreed([(110, 110)], 1, 9, 1, 1000, 300)
    assert (p['chunks'], p['chunked'], p['why'], p['launches']) == (14, 0, dp.WORKSPACE_ROOM, 4)
    p = agreed([(100, 100)], 1, 9, 1, 1000, 300)
    assert (p['chunks'], p['chunked'], p['why'], p['launches']) == (11, 1, dp.CHUNKED, 5)


def test_smallest_call():
    p = agreed([(1, 1)], 1, 1, 1, 1, 1)
    assert (p['cap'], p['chunked'], p['chunks'], p['Tmax'], p['words'], p['sort_lds'], p['limit'], p['launches']) == (1024, 1, 1, 64, 1, 4096, 0, 5)
    assert p['workspace'] == 104744                                           # test_default_capacity_workspace_is_unchanged's (1, 1, 1)


def test_more_shapes_agree():
    for grids in (DEFAULT, SMALL, DEFAULT[:1], SMALL[2:], [(167, 167)] * 3, [(3, 5)] * 8):
        for n in (1, 3):
            for a, k in ((9, 1), (9, 2), (1, 1), (3, 7)):
                for topk in (1, 63, 1000, 1024, 1025, 2500, 4096):
                    for dpi in (1, 100, 300, 1000, 2560, 8192):
                        if len(grids) * topk <= (8192 if topk <= 1024 else 20480):
                            agreed(grids, n, a, k, topk, dpi)


def test_switches_are_read_on_every_call(monkeypatch):
    assert agreed(DEFAULT, 2, 9, 1, 1000, 200)['launches'] == 7
    monkeypatch.setenv('CVPCE_DECODE_ONE_KERNEL', '1')
    p = agreed(DEFAULT, 2, 9, 1, 1000, 200)
    assert (p['chunked'], p['why'], p['limit'], p['launches']) == (0, dp.SWITCH, 1600, 6)
    assert agreed(DEFAULT, 2, 9, 3, 1000, 200)['why'] == dp.MERGE_LIMIT      # (the switch is not the reason where there was no choice)
    monkeypatch.setenv('CVPCE_NMS_ONE_PHASE', '1')
    p = agreed(DEFAULT, 2, 9, 1, 1000, 200)
    assert (p['chunked'], p['limit'], p['launches']) == (0, 0, 4)
    monkeypatch.delenv('CVPCE_DECODE_ONE_KERNEL')
    p = agreed(DEFAULT, 2, 9, 1, 1000, 200)
    assert (p['chunked'], p['limit'], p['launches']) == (1, 0, 5)
    monkeypatch.delenv('CVPCE_NMS_ONE_PHASE')
    assert agreed(DEFAULT, 2, 9, 1, 1000, 200)['launches'] == 7


def test_rejected_arguments_stay_rejected():
    from cvpce_amd._lib import lib
    bad = [([], 1, 9, 1, 1000, 300), ([(4, 4)] * 9, 1, 9, 1, 100, 300),                       # L = 0, L = 9
           (DEFAULT, 1, 9, 1, 0, 300), (DEFAULT, 1, 9, 1, 4097, 300),                          # topk 0, 4097
           ([(4, 4)] * 8, 1, 9, 1, 2561, 300), ([(4, 4)] * 6, 1, 9, 1, 4096, 300),             # L * topk = 20 488, 24 576 > 20 480
           (DEFAULT, 1, 9, 1, 1000, 8193), (DEFAULT, 1, 9, 1, 4096, 20481), (DEFAULT, 1, 9, 1, 1000, 0),
           (DEFAULT, 1, 0, 1, 1000, 300), (DEFAULT, 1, 9, 0, 1000, 300),                       # A = 0, K = 0
           ([(100, 104), (0, 52)], 1, 9, 1, 1000, 300), ([(100, 104), (50, 0)], 1, 9, 1, 1000, 300),
           ([(40000, 40000)], 1, 9, 1, 1000, 300)]                                            # n > 2^31 - 1 logits in a level
    for args in bad:
        assert dp.plan(*args) is None and query(*args)[0] == 1, args
    assert query(DEFAULT, 1, 9, 1, 1000, 8192)[0] == 0 and query(DEFAULT, 1, 9, 1, 4096, 20480)[0] == 0
    assert query([(4, 4)] * 8, 1, 9, 1, 1024, 300)[0] == 0 and query([(4, 4)] * 5, 1, 9, 1, 4096, 300)[0] == 0
    # eight levels at topk 1025 are 8 200 candidates at the wide capacity (room for 20 480): accepted, as they always were
    assert agreed([(4, 4)] * 8, 1, 9, 1, 1025, 300)['cap'] == 4096 and query([(4, 4)] * 8, 1, 9, 1, 2560, 300)[0] == 0
    out = (ctypes.c_longlong * len(dp.FIELDS))()
    g = (ctypes.c_int * 1)(4)
    assert lib.cvpce_detect_plan(None, g, 1, 1, 9, 1, 10, 5, out) == 1 and lib.cvpce_detect_plan(g, None, 1, 1, 9, 1, 10, 5, out) == 1
    assert lib.cvpce_detect_plan(g, g, 1, 1, 9, 1, 10, 5, None) == 1
    assert query(DEFAULT, 0, 9, 1, 1000, 300)[0] == 0                         # no images: accepted, nothing to launch
