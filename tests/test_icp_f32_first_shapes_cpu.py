"""The one-wave scan matcher's LDS with the float32 image serving the first iteration too (csrc/launch_shapes.h,
icp_wave_lds_bytes): the image takes the place the list had and the list of that form is kept in registers, so the pair's
LDS does not depend on the list.  Asked of the library through slam_plan_icp / slam_plan_query: no GPU needed."""
import pytest

import icp_shapes as sh


def test_image_in_the_lists_place_at_360_beams():
    """368 points of 16 B, 30 boxes of 32 B and 368 image points of 8 B: 9 792 B whatever the list's length, under the
    10 KiB at which 16 pairs fit a CU's LDS.  The float64 form keeps its 96 slots of 20 B."""
    points, boxes, cap = 368, 24 + 6, 96
    want = points * sh.DOUBLE2 + boxes * sh.BOX + points * 8
    assert want == 9792 <= 10 * 1024
    assert [sh.query("icp_wave_lds_bytes", 360, c, 1) for c in (0, 16, cap)] == [want] * 3
    assert sh.query("icp_wave_lds_bytes", 360, cap, 0) == want - points * 8 + cap * sh.LIST_SLOT == 8768
    p = sh.plan_icp(2, 360, 360, True, one_wave=1)
    assert (p.form, p.lds, p.team_cap, p.qpt, p.block) == ("WaveF32", want, cap, sh.WAVE_QPT, sh.WAVE)
    assert sh.plan_icp(2, 360, 360, True, one_wave=1, f32_filter=0).lds == 8768
    assert sh.plan_icp(2, 360, 360, True, one_wave=1, icp_team=1).lds == want                  # no list: the same
    assert sh.plan_icp(2, 1, 360, True, one_wave=1).lds == want                                # a list of 16: the same
    # the register list holds two rounds of 64 entries: the longest list of the shape fits
    assert max(sh.plan_icp(2, n, 360, True, one_wave=1).team_cap for n in range(1, sh.WAVE * sh.WAVE_QPT + 1)) == cap <= 2 * sh.WAVE


@pytest.mark.parametrize("guard", [0, 512])
def test_the_benchmark_launch_keeps_the_one_wave_form(guard):
    """31 968 pairs of 360 beams: the automatic rule still takes the float32 one-wave form, and goes by the shipped size -
    the debug build's guard bytes are added to the launch and do not choose the shape."""
    p = sh.plan_icp(31968, 360, 360, True, guard=guard)
    assert (p.form, p.lds, p.team_cap) == ("WaveF32", 9792 + guard, 96)
    assert sh.plan_icp(31968, 360, 360, True, f32_filter=0, guard=guard).form == "WaveF64"
    # the largest scan of the automatic form is the same with and without the guard, and fits 10 KiB without it
    forms = [sh.plan_icp(31968, 384, n, True, guard=guard).form for n in range(300, 420)]
    last = 300 + forms.index("Workgroup") - 1
    assert forms[:last - 299] == ["WaveF32"] * (last - 299) and set(forms[last - 299:]) == {"Workgroup"}
    assert sh.query("icp_wave_lds_bytes", last, 96, 1) <= 10 * 1024 < sh.query("icp_wave_lds_bytes", last + 1, 96, 1)
    assert last >= 360
