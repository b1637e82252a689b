"""The "icp_one_wave" option at the C boundary, without a device: slam_set_option checks an option's name and value
before it touches the context, so -1 / 0 / 1 get as far as the context (a null one here) and anything else is refused by
name - as for every other option."""
import pytest

from conftest import pkg


@pytest.mark.parametrize("value", [-1, 0, 1])
def test_set_option_accepts_the_three_settings(value):
    abi = pkg("_abi")
    L = abi.lib()
    assert L.slam_set_option(None, b"icp_one_wave", float(value)) == abi.ERR_INVALID
    assert b"null context" in L.slam_last_error()


@pytest.mark.parametrize("value", [-2, 2, 0.5, 3, float("nan")])
def test_set_option_refuses_other_values(value):
    abi = pkg("_abi")
    L = abi.lib()
    assert L.slam_set_option(None, b"icp_one_wave", float(value)) == abi.ERR_INVALID
    assert b"icp_one_wave is -1, 0 or 1" in L.slam_last_error()



def test_every_option_is_checked_before_the_context():
    abi = pkg("_abi")
    L = abi.lib()
    for name, bad, words in ((b"grid_split", 2.0, b"grid_split is -1, 0 or 1"), (b"icp_qpt", 4.0, b"icp_qpt in [0, 3]"),
                             (b"icp_team", -1.0, b"icp_team is 0 or 1"), (b"no_such_option", 0.0, b"unknown option no_such_option")):
        assert L.slam_set_option(None, name, bad) == abi.ERR_INVALID
        assert words in L.slam_last_error()
