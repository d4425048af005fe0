"""Which kernel every conv gets, and what every profiled wrapper of cvpce_amd/ops.py files with a ConvProfile, checked on the host
against the committed table tests/conv_routes.json (tests/conv_routes.py: the recorder that stands in for the custom ops, the
cases, `--write`).  The table was written from the ops.py that preceded the routing function and the launch timer; it changes only
with a change that means to change a route or a record."""
import pytest

from conv_routes import OPS_CONV2D, RECORD_NAMES_CONV2D, Event, load_table, replay


@pytest.fixture(scope='module')
def table():
    from cvpce_amd import ops
    return load_table(ops)


def test_routes_and_records_match_the_table(table):
    from cvpce_amd import ops
    got = replay(ops, profile=True)
    assert list(got) == list(table)
    for group in table:
        assert list(got[group]) == list(table[group]), group
        for key, want in table[group].items():
            assert got[group][key] == want, (group, key)
    assert Event.made > 0


def test_launch_path_makes_no_event_without_a_profile(table):
    """PROFILE None: the same op calls, and not one event made over all cases."""
    from cvpce_amd import ops
    got = replay(ops, profile=False)
    assert Event.made == 0
    for group in table:
        for key, want in table[group].items():
            assert got[group][key] == want[:1], (group, key)


def test_table_covers_every_route(table):
    base = [case for group in ('conv2d bf16', 'conv2d fp16') for case in table[group].values()]
    assert len(base) == 578
    conv2d = [case for group, cases in table.items() if group.startswith('conv2d') for case in cases.values()]
    assert all(len(calls) == 1 and len(records) == 1 for calls, records, _, _ in conv2d)
    assert {calls[0][0] for calls, _, _, _ in base} == OPS_CONV2D
    assert {records[0][0] for _, records, _, _ in base} == RECORD_NAMES_CONV2D
    assert {records[0][0] for _, records, _, _ in conv2d} == RECORD_NAMES_CONV2D | {'conv3x3_halo2_kernel[detector]'}
    assert any(calls[0][0] == 'conv2d_splitk' and calls[0][-1] == 4 for calls, _, _, _ in base)


@pytest.mark.parametrize('entry', ['cvpce_conv2d_nhwc_bf16', 'cvpce_conv2d_nhwc_f16'])
def test_force_generic_is_zero_or_one(entry):
    """`force_generic` selects no kernel variants any more: the entry points refuse every value but 0 and 1, behind the N <= 0 return
    that comes before every check.  Dummy pointers and the return-code convention of tests/halo_host_cases.py (0: N <= 0; 1: refused;
    2: accepted, failed at the launch for want of a device), so only where no GPU is visible."""
    from halo_host_cases import P, gpu_visible
    if gpu_visible():
        pytest.skip('a GPU is visible: an accepted case would launch a kernel on dummy pointers')
    from cvpce_amd._lib import lib

    def call(n, force_generic):
        # in, wgt, bias, res, out, N, H, W, Cin, Cout, KH, KW, stride, pad, Ho, Wo, K_pad, Cout_pad, act, out_f32, in_up_shift,
        # res_mode, Hr, Wr, fuse_pool2, force_generic, stream: a 64 -> 64 3x3 layer on 16 x 16 maps
        return int(getattr(lib, entry)(P, P, P, 0, P, n, 16, 16, 64, 64, 3, 3, 1, 1, 16, 16, 576, 256, 1, 0, 0, 0, 0, 0, 0, force_generic, 0))

    assert [call(2, fg) for fg in (2, 3, -1)] == [1, 1, 1]
    assert call(0, 2) == 0
    assert [call(2, fg) for fg in (0, 1)] == [2, 2]              # the same call is refused for nothing else
