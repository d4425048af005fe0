"""The host decisions of cvpce_conv3x3_halo_strips2 (the thin-strip companion of cvpce_conv3x3_halo_list): dummy pointers, return codes
only, as tests/halo_host_cases.py does for the eleven entry points of its table.  The new entry point takes the operands of
cvpce_conv3x3_halo_strips and decides every case as that one does."""

import pytest

import abi
import halo_host_cases as hc

FN, TWIN = 'cvpce_conv3x3_halo_strips2', 'cvpce_conv3x3_halo_strips'


def _cases():
    out = {}
    for label, over in hc.variations():
        if not set(over) <= set(hc._LIST):
            continue
        a = dict(hc.BASE, **over)
        if a['K_pad'] is None:
            a['K_pad'] = 9 * a['Cin']
        if a['Cout_pad'] is None:
            a['Cout_pad'] = (a['Cout'] + 255) // 256 * 256
        out[label] = tuple(a[p] for p in hc._LIST)
    return out


@pytest.fixture(scope='module')
def lib():
    if hc.gpu_visible():
        pytest.skip('a GPU is visible: an accepted case would launch a kernel on dummy pointers')
    from cvpce_amd._lib import lib
    return lib


def test_thin_strips_decide_as_strips(lib):
    cases = _cases()
    assert len(cases) > 80
    codes = {label: int(getattr(lib, FN)(*args)) for label, args in cases.items()}
    twin = {label: int(getattr(lib, TWIN)(*args)) for label, args in cases.items()}
    assert codes == twin
    assert set(codes.values()) == {0, 1, 2}                      # N <= 0, refused, accepted


def test_thin_strips_boundaries(lib):
    codes = {label: int(getattr(lib, FN)(*args)) for label, args in _cases().items()}
    assert codes['base'] == 2 and codes['N 0'] == 0 and codes['N -1'] == 0
    assert (codes['Cout 136'], codes['Cout 128']) == (2, 1)      # strips need the 16 x 16-tile kernel: Cout > 128
    assert codes['null list'] == 1 and codes['null count'] == 1 and codes['no mac no out'] == 1
    assert (codes['mac'], codes['mac no out'], codes['mac no relu'], codes['mac off over']) == (2, 2, 1, 1)
    assert (codes['pool'], codes['pool odd H']) == (2, 1)
    assert (codes['N 65535 cout 256'], codes['N 65536 cout 256']) == (2, 1)
    assert (codes['W 4080 cout 256'], codes['W 4081 cout 256']) == (2, 1)


def test_lists_header_table_and_op_agree():
    """include/cvpce_amd_lists.h is a header of its own beside the inference header: its one entry point is exported, has its own ctypes
    table and its own torch op (GPU only), and none of them overlaps the inference header's"""
    from cvpce_amd import _lib
    assert abi.header_symbols('cvpce_amd_lists.h') == [FN]
    assert _lib.HEADERS['cvpce_amd_lists.h'][FN] == _lib.SIGNATURES[TWIN]
