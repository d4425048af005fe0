"""What the 3x3 halo entry points accept and refuse, replayed on the host against the committed table tests/halo_host_cases.json
(tests/halo_host_cases.py: the cases, the recorder, why the return code is the whole decision where there is no GPU).  The table was
written from the library that preceded csrc/halo_common.h; it changes only with a change that means to change a decision."""
import json

import pytest

from halo_host_cases import ENTRIES, TABLE, cases, gpu_visible, run

# The decisions that differ from the table on purpose: a work-list launch of the wide-tile kernel (Cout <= 128, 32-pixel tiles) took
# W up to 8160 = 255 tiles, but an entry holds the crop's extent on that tensor in 12 bits (csrc/worklist.h): W > 4095 is refused now.
TIGHTENED = {'halo_list: W 4096 cout 128': 1, 'halo_list: W 8160 cout 128': 1}


@pytest.fixture(scope='module')
def codes():
    if gpu_visible():
        pytest.skip('a GPU is visible: an accepted case would launch a kernel on dummy pointers')
    from cvpce_amd._lib import lib
    return run(lib)


@pytest.fixture(scope='module')
def table():
    with open(TABLE) as f:
        return json.load(f)


def test_every_decision_matches_the_table(codes, table):
    assert sorted(codes) == sorted(table)
    assert all(table[name] == 2 for name in TIGHTENED)           # accepted before
    want = dict(table, **TIGHTENED)
    wrong = {name: (code, want[name]) for name, code in codes.items() if code != want[name]}
    assert not wrong


def test_table_covers_every_entry_point_and_both_sides(table):
    assert len(table) == len(cases()) > 500
    for fn in ENTRIES:
        short = fn[len('cvpce_conv3x3_'):] + ': '
        got = {code for name, code in table.items() if name.startswith(short)}
        assert got == {0, 1, 2}, fn                               # N <= 0, refused, accepted
    # a boundary's two sides differ where the entry point can reach it
    for under, at in (('halo: chunks 2^30 under', 'halo: chunks 2^30 at'), ('halo_wide: chunks 2^29 under', 'halo_wide: chunks 2^29 at'),
                      ('halo_list: N 65535 cout 256', 'halo_list: N 65536 cout 256'), ('halo_list: W 4080 cout 256', 'halo_list: W 4081 cout 256'),
                      ('halo_list: H 4080 cout 128', 'halo_list: H 4081 cout 128'), ('halo_list: W 8160 cout 128', 'halo_list: W 8161 cout 128'),
                      ('halo_thin_out: Cout 128', 'halo_thin_out: Cout 129'), ('halo_thin_out: in bytes under cout 9', 'halo_thin_out: in bytes at cout 9'),
                      ('halo_mac: mac cout 136', 'halo_mac: mac cout 128'), ('halo_strips: Cout 136', 'halo_strips: Cout 128')):
        assert (table[under], table[at]) == (2, 1), (under, at)
