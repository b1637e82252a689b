"""The "win_lds_hits" option at the C boundary, without a device (as tests/test_abi_icp_f32_filter_cpu.py): -1 / 0 / 1 get
as far as the context (a null one here), anything else is refused by name."""
import pytest

from conftest import pkg


@pytest.mark.parametrize("value", [-1, 0, 1])
def test_set_option_accepts_the_three_settings(value):
    abi = pkg("_abi")
    L = abi.lib()
    assert L.slam_set_option(None, b"win_lds_hits", float(value)) == abi.ERR_INVALID
    assert b"null context" in L.slam_last_error()


@pytest.mark.parametrize("value", [-2, 2, 0.5, float("nan")])
def test_set_option_refuses_other_values(value):
    abi = pkg("_abi")
    L = abi.lib()
    assert L.slam_set_option(None, b"win_lds_hits", float(value)) == abi.ERR_INVALID
    assert b"win_lds_hits is -1, 0 or 1" in L.slam_last_error()
