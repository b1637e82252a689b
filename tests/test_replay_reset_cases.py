"""The table of tests/replay_reset_cases.py held to the edges it is there for, without a GPU: the sizes are the library's
own (slam_plan_icp for the launch, slam_plan_query "grid_state_bytes" for the words to clear), so a change of a block size,
of the batch rule or of the grid's layout moves the cases with it - or fails here, where a case no longer sits on its edge."""
import pytest

import icp_shapes
import replay_reset_cases as K

# block of (form, kind): what the scan matcher launches for 360 beams.  The preferred queries per lane hold from 65 pairs
# on, so on the 64 x 64 map only the one-trip cases of icp_qpt 2 and 3 run in those shapes (and K.preferred_cases()).
BLOCKS = {"workgroup_qpt1": [384] * 5, "workgroup_qpt2": [384] * 4 + [192], "workgroup_qpt3": [384] * 4 + [128],
          "wave_f32": [64] * 5, "wave_f64": [64] * 5}


def test_words_of_the_maps():
    """Two counter planes, each rounded up to 256 bytes, and 256 visit slots of 64 bytes."""
    up = lambda v: (v + 255) // 256 * 256                  # noqa: E731
    for G, xw, yw in ((1, 64, 64), (3, 37, 53), (1, 256, 256), (2, 200, 200), (1, 1, 1)):
        assert K.grid_state_bytes(G, xw, yw) == 2 * up(G * xw * yw * 4) + 256 * 64, (G, xw, yw)
    assert K.grid_state_bytes(1, K.XW, K.YW) == 16 * K.N16 and K.N16 == 3072
    assert K.grid_state_bytes(3, 37, 53) % 16 == 0 and K.grid_state_bytes(3, 37, 53) > 2 * 3 * 37 * 53 * 4 + 256 * 64    # padded planes


@pytest.mark.parametrize("form", sorted(K.FORMS))
def test_form_and_block_of_every_case(form):
    cs = [K.case(form, k) for k in K.KINDS]
    for c, block in zip(cs, BLOCKS[form]):
        p = K.plan(form, c.pairs)
        assert p.form == K.FORMS[form][2] and p.block == c.block == block, (c, p)
        assert c.lanes == c.pairs * c.block and c.n16 == K.N16 and c.trips == -(-c.n16 // c.lanes)
        if p.form != "Workgroup":
            assert p.block == icp_shapes.WAVE and p.qpt == icp_shapes.WAVE_QPT
        else:
            assert p.block == icp_shapes.icp_block(K.BEAMS, p.qpt)
    asked = K.FORMS[form][1].get("icp_qpt")
    if asked:
        assert K.plan(form, cs[-1].pairs).qpt == asked              # the one-trip case runs in the form's own shape


@pytest.mark.parametrize("form", sorted(K.FORMS))
def test_cases_sit_on_the_edges_of_the_loop(form):
    many, below, equal, above, one = (K.case(form, k) for k in K.KINDS)
    assert many.pairs == 1 and many.trips >= 8
    assert one.trips == 1 and one.lanes >= 4 * one.n16
    assert below.block == equal.block == above.block
    assert (below.pairs, above.pairs) == (equal.pairs - 1, equal.pairs + 1)
    assert below.lanes < K.N16 == equal.lanes < above.lanes
    assert (below.trips, equal.trips, above.trips) == (2, 1, 1)


def test_preferred_shapes_take_several_trips():
    cs = K.preferred_cases()
    assert [(c.form, K.plan(c.form, c.pairs).qpt, c.block) for c in cs] == [("workgroup_qpt2", 2, 192), ("workgroup_qpt3", 3, 128)]
    for c in cs:
        assert c.pairs > 64 and c.trips >= 3 and c.lanes < c.n16 and c.n16 * 16 == K.grid_state_bytes(1, K.PREFERRED_MAP, K.PREFERRED_MAP)


def test_several_maps_case():
    m = K.MANY
    n16 = K.grid_state_bytes(m["G"], m["xw"], m["yw"]) // 16
    pairs = m["L"] * (m["n_scan"] - 1)
    lanes = pairs * icp_shapes.plan_icp(pairs, K.BEAMS, K.BEAMS, True).block
    assert K.trips(n16, lanes) >= 2                         # the clear of the three maps takes more than one trip
    assert sorted(set(range(m["G"])) - set(m["grid_of_traj"])) == [1]
