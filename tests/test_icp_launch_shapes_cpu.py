"""The scan matcher's launch decision (plan_icp, csrc/launch_shapes.h) without a GPU, as the library answers for it
(tests/icp_shapes.py: slam_plan_icp, slam_plan_query): every size at which a decision of the workgroup shapes changes is
asserted over n = 1..8192, and the rule that chooses the one-wave shape at its edges."""
import icp_shapes as sh


def test_lds_regions_at_the_sizes_worked_out_by_hand():
    """n_src = n_tar = n, a replay of a few scans, the shipped build:
      n = 1 376: 86 blocks -> 86 * 272 = 23 392, boxes padded to 88 -> 110 * 32 = 3 520; copy 1 380 * 16 = 22 080;
                 two queries per lane, 688 of them: 11 waves -> 2 * 11 * 12 * 8 + 64 = 2 176; flags 32; list 688 * 20 =
                 13 760: 64 960 <= 65 536;
      n = 1 377: 87 blocks -> 23 664 + 3 520, copy 22 096, 2 176 + 32, list 704 * 20 = 14 080: 65 568 > 65 536;
      n = 4 557: 285 blocks -> 77 520, boxes 288 -> 360 * 32 = 11 520; eight per lane: 570 -> 9 waves -> 1 792; 32: 90 864,
                 and the copy 4 561 * 16 = 72 976: 163 840 = 160 KiB exactly, no room for a list;
      n = 4 558: the copy is 16 bytes more and no longer fits."""
    assert sh.nn_lds_bytes(1376) == 23392 + 3520 and sh.icp_polar_bytes(1376) == 22080 and sh.icp_red_bytes(11) == 2176
    assert sh.launch(2, 1376, 1376, True) == sh.Shape(2, 704, 11, True, 688, 688, 64960)
    assert sh.launch(2, 1377, 1377, True) == sh.Shape(2, 704, 11, True, 704, 704, 65568)
    assert sh.nn_lds_bytes(4557) == 77520 + 11520 and sh.icp_red_bytes(9) == 1792 and sh.icp_polar_bytes(4557) == 72976
    assert sh.launch(2, 4557, 4557, True) == sh.Shape(8, 576, 9, True, 0, 2288, 160 * 1024)
    assert sh.launch(2, 4558, 4558, True) == sh.Shape(8, 576, 9, False, 0, 0, 90864)
    assert sh.launch(2, 8192, 8192, True) == sh.launch(2, 8192, 8192, False) == sh.Shape(8, 1024, 16, False, 0, 0, 162912)


def test_every_transition_of_the_sweep():
    """n = n_src = n_tar over 1..8192, for scans and for point clouds: the first n of each shape, the first n over
    64 KiB, the first n whose list is cut and the first without one, the first n without the unpadded copy - and each
    holds from there on (icp_shapes.first checks that there is ONE transition).  Nothing exceeds 160 KiB."""
    scans, clouds = sh.edges(True), sh.edges(False)
    assert scans == {"qpt2": 1025, "qpt3": 2049, "qpt4": 3073, "qpt8": 4097, "raised": 1377, "cut": 3526, "zero": 4545, "dropped": 4558}
    assert clouds == {"qpt2": 1025, "qpt3": 2049, "qpt4": 3073, "qpt8": 4097, "raised": 3217}
    for is_scan in (True, False):
        for n in range(1, sh.N_MAX + 1):
            s = sh.launch(3, n, n, is_scan)
            assert s is not None and s.lds <= 160 * 1024, (is_scan, n)
            assert s.qpt in sh.QPTS and s.block == s.waves * 64 <= 1024 and s.block * s.qpt >= n, (is_scan, n, s)
            assert s.team_cap % 16 == 0 and 0 <= s.team_cap <= s.cap_wanted, (is_scan, n, s)
            assert is_scan or (not s.polar_copy and s.team_cap == 0)
    # the list at the sizes either side of each change
    at = lambda n, **kw: sh.launch(2, n, n, True, **kw)
    assert (at(3525).team_cap, at(3525).cap_wanted) == (1776, 1776) and (at(3526).team_cap, at(3526).cap_wanted) == (1760, 1776)
    assert (at(4097).team_cap, at(4097).cap_wanted) == (800, 2064)
    assert at(4544).team_cap == 32 and at(4545).team_cap == 0 and at(4545).polar_copy and at(4557).polar_copy
    assert at(3526, icp_team=1).team_cap == 0 and at(3526, icp_team=1).polar_copy      # icp_team 1: no list, the copy stays
    # waves per pair at the first size of the wide shapes: 9 ... 16
    assert [at(n).waves for n in (3073, 4096, 4097, 8192)] == [13, 16, 9, 16]
    # a point cloud against a small target never comes near either limit
    assert sh.launch(3, 8192, 700, False).lds < 64 * 1024


def test_the_debug_builds_guard_moves_the_lds_edges_only():
    """With the 512 guard bytes of the LDS-guard build the copy is dropped 13 beams earlier (4 545: where the source's
    comment used to put it) and the shapes stay where they are."""
    g = sh.edges(True, guard=512)
    assert {k: g[k] for k in ("qpt2", "qpt3", "qpt4", "qpt8")} == {"qpt2": 1025, "qpt3": 2049, "qpt4": 3073, "qpt8": 4097}
    assert g["dropped"] == 4545 and g["dropped"] < sh.edges(True)["dropped"]
    assert all(sh.launch(3, n, n, True, guard=512).lds <= 160 * 1024 for n in range(1, sh.N_MAX + 1))


def test_every_wave_has_a_live_first_query_in_lane_0():
    """SameMatch compares every query's match with that of its wave's lane 0, first query: that query must exist in every
    wave of every shape - for each n_src, for the size-derived shape and for every preference that may replace it."""
    for n in range(1, sh.N_MAX + 1):
        for qpt in {sh.queries_per_lane(1, n)} | {sh.queries_per_lane(65, n, icp_qpt=p) for p in (1, 2, 3)}:
            live = sh.live_first_queries(n, qpt)
            assert len(live) == sh.icp_block(n, qpt) // 64 and all(live), (n, qpt)


def test_the_preference_rules_truth_table():
    """B > 64 && qpt < pref && n_src > 64 * pref, pref = icp_qpt or, left at 0, 2 (3 from 7 500 waves at two queries
    per lane).  At B = 64 it never applies; at 65 it applies from 129 points for pref 2 (and so for icp_qpt 0: 65 pairs
    are far from 7 500 waves) and from 193 for pref 3; pref 1 changes nothing, the size-derived shape has one already."""
    for n in (128, 129, 192, 193):
        for q in (0, 1, 2, 3):
            assert not sh.preferred(64, n, icp_qpt=q) and sh.queries_per_lane(64, n, icp_qpt=q) == 1, (n, q)
    want = {(128, 0): 1, (129, 0): 2, (192, 0): 2, (193, 0): 2,
            (128, 1): 1, (129, 1): 1, (192, 1): 1, (193, 1): 1,
            (128, 2): 1, (129, 2): 2, (192, 2): 2, (193, 2): 2,
            (128, 3): 1, (129, 3): 1, (192, 3): 1, (193, 3): 3}
    for (n, q), qpt in want.items():
        assert sh.queries_per_lane(65, n, icp_qpt=q) == qpt and sh.preferred(65, n, icp_qpt=q) == (qpt > 1), (n, q)
        s64, s65 = sh.launch(64, n, n, True, icp_qpt=q), sh.launch(65, n, n, True, icp_qpt=q)
        assert (s64 == s65) == (qpt == 1) and s65.block == sh.icp_block(n, qpt)
    # the automatic preference: 3 from 7 500 waves at two per lane - 2 500 pairs of 360 beams
    assert sh.preference(2499, 360) == 2 and sh.preference(2500, 360) == 3
    # a batch-invariant launch (the node replays) takes two per lane whatever B
    assert sh.queries_per_lane(1, 360, batch_invariant=True) == sh.queries_per_lane(5000, 360, batch_invariant=True) == 2
    # the preference never lowers a size-derived shape
    assert all(sh.queries_per_lane(65, n, icp_qpt=q) >= sh.queries_per_lane(1, n) for n in range(1, 8193, 7) for q in (0, 1, 2, 3))


def test_one_wave_where_a_pair_fits():
    """icp_one_wave = 1: one wave per pair exactly while n_src <= 384 (six queries a lane) and the pair's LDS is at most the
    64 KiB a kernel gets by default; else the workgroup shape, as with icp_one_wave = 0."""
    for scans in (True, False):
        at = {n: sh.plan_icp(2, 384, n, scans, one_wave=1) for n in range(1, sh.N_MAX + 1)}
        last = sh.first(lambda n: not at[n].form.startswith("Wave")) - 1
        assert 2000 < last < sh.N_MAX and at[last].lds <= sh.LDS_DEFAULT and (at[last].qpt, at[last].block) == (sh.WAVE_QPT, sh.WAVE)
        assert sh.query("icp_wave_lds_bytes", last + 1, at[last].team_cap, scans) > sh.LDS_DEFAULT
        assert at[last].lds == sh.query("icp_wave_lds_bytes", last, at[last].team_cap, scans)
        for n_tar in (1, 360, last, last + 1):
            wave = [sh.plan_icp(2, n_src, n_tar, scans, one_wave=1).form.startswith("Wave") for n_src in (1, 383, 384, 385, 1000)]
            assert wave == [n_tar <= last] * 3 + [False, False], (scans, n_tar, wave)
            off = sh.plan_icp(2, 385, n_tar, scans, one_wave=1)
            assert off == sh.plan_icp(2, 385, n_tar, scans, one_wave=0) and off.form == "Workgroup"
    assert sh.plan_icp(2, 360, 360, True, one_wave=1, guard=512).lds == sh.plan_icp(2, 360, 360, True, one_wave=1).lds + 512 == 9792 + 512


def test_one_wave_by_itself_only_in_launches_that_fill_the_chip_four_times():
    """icp_one_wave = -1: scans, B >= 16 384, n_src > 192, the preference three queries per lane, not batch-invariant, a
    pair's LDS at most 10 KiB; the guard build's 512 bytes do not change the choice."""
    auto = lambda B, n, scans=True, **kw: sh.plan_icp(B, n, n, scans, **kw).form
    assert auto(4 * sh.WAVE_ROUND - 1, 360) == "Workgroup" and auto(4 * sh.WAVE_ROUND, 360) == "WaveF32"
    assert 4 * sh.WAVE_ROUND == 16384
    assert auto(16384, 192) == "Workgroup" and auto(16384, 193) == "WaveF32"
    assert auto(16384, 360, icp_qpt=3) == "WaveF32" and auto(16384, 360, icp_qpt=2) == auto(16384, 360, icp_qpt=1) == "Workgroup"
    assert auto(16384, 360, batch_invariant=True) == "Workgroup" and auto(16384, 360, batch_invariant=True, one_wave=1) == "WaveF32"
    assert auto(16384, 360, scans=False) == "Workgroup" and auto(16384, 360, one_wave=0) == "Workgroup"
    assert sh.plan_icp(16384, 384, 360, True).form == "WaveF32" and sh.plan_icp(16384, 385, 360, True).form == "Workgroup"
    # 10 KiB: the shipped layout's size decides, with and without the guard
    for guard in (0, 512):
        forms = {n: sh.plan_icp(16384, 384, n, True, guard=guard).form for n in range(300, 500)}
        last = sh.first(lambda n: forms[n] == "Workgroup", lo=300, hi=499) - 1
        assert sh.plan_icp(16384, 384, last, True).lds <= 10 * 1024 < sh.plan_icp(16384, 384, last + 1, True, one_wave=1).lds
        assert guard == 0 or forms == keep
        keep = forms
    assert all(sh.plan_icp(B, n, n, True, guard=512).form == sh.plan_icp(B, n, n, True).form
               for B in (16383, 16384, 40000) for n in range(1, 500, 7))


def test_the_float32_filter_is_for_scans():
    """icp_f32_filter -1 / 1: the float32 form, for scans only; 0: the float64 form.  A point cloud has no beam windows."""
    form = lambda scans, f: sh.plan_icp(2, 360, 360, scans, one_wave=1, f32_filter=f).form
    assert [form(True, f) for f in (-1, 0, 1)] == ["WaveF32", "WaveF64", "WaveF32"]
    assert [form(False, f) for f in (-1, 0, 1)] == ["WaveF64"] * 3
    assert sh.plan_icp(2, 360, 360, True, one_wave=1, f32_filter=0).lds == 8768     # a list of 96; 9 792 with the image over it
