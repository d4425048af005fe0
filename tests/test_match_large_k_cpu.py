"""Host-side checks of the matcher's workspace query (include/cvpce_amd.h cvpce_match_workspace_bytes): k > 16 takes the large-k
path, whose workspace is a distance block processed in query chunks under a fixed budget; k <= 16 keeps the fused path's size."""
import pytest

BUDGET = 256 << 20


@pytest.mark.parametrize('qn,gn,k', [(20000, 100000, 100), (1600, 10000, 10000), (1500, 100000, 17), (3, 40000, 40000),
                                     (1, 17, 17), (5000, 3000, 3000)])
def test_large_k_workspace_stays_within_the_budget(qn, gn, k):
    from cvpce_amd._lib import lib
    ws = lib.cvpce_match_workspace_bytes(qn, gn, k)
    assert ws <= BUDGET + 4096
    # at least one query's distance row and its k survivor keys
    gpad = (gn + 127) // 128 * 128
    assert ws >= gpad * 4 + k * 8


@pytest.mark.parametrize('qn,gn,k', [(200, 10000, 1), (1600, 10000, 16), (37, 3200, 4), (333, 1357, 16), (1, 16, 16), (20000, 100000, 16)])
def test_small_k_workspace_is_unchanged(qn, gn, k):
    from cvpce_amd._lib import lib
    tiles_g = (gn + 127) // 128
    assert lib.cvpce_match_workspace_bytes(qn, gn, k) == qn * tiles_g * k * 8 + 512
