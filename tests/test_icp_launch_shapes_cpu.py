"""The scan matcher's workgroup launch decision (launch_icp_t, csrc/icp_kernels.hip) without a GPU: tests/icp_shapes.py
restates it; here its constants and deciding expressions are read back from the source text, so that an edit to the
kernel fails these tests instead of silently moving the edges the GPU tests sit on, and every size at which a decision
changes is asserted over n = 1..8192."""
import os
import re

import pytest

import icp_shapes as sh
from conftest import PKG, ROOT

CSRC = os.path.join(ROOT, PKG, "csrc")


def source_text():
    """The scan matcher's source and the header with the constants every kernel file shares (kWave)."""
    return open(os.path.join(CSRC, "icp_kernels.hip")).read() + open(os.path.join(CSRC, "slam_internal.h")).read()


def constants(text):
    """name -> value of the integer constants the launch decision rests on, as the source spells them."""
    def one(pattern):
        m = re.findall(pattern, text)
        assert len(m) == 1, (pattern, m)
        return int(m[0])
    return {"kNNBlock": one(r"constexpr int kNNBlock = (\d+);"),
            "kNNStride - kNNBlock": one(r"constexpr int kNNStride = kNNBlock \+ (\d+);"),
            "kRedStride": one(r"constexpr int kRedStride = (\d+);"),
            "kPolarTail": one(r"constexpr int kPolarTail = (\d+);"),
            "kIcpExtraLds": one(r"constexpr int kIcpExtraLds = (\d+);"),
            "kWave": one(r"constexpr int kWave = (\d+);")}


# the deciding expressions, each as the source writes it (whitespace free); sh.launch() is their restatement
EXPRESSIONS = [
    # sizes of the LDS regions
    r"return \(size_t\)nn_blocks\(n_tar\) \* kNNStride \* sizeof\(double2\) \+\s*\(size_t\)\(nn_boxes_padded\(n_tar\) \+ nn_boxes4\(n_tar\)\) \* sizeof\(Box\);",
    r"int nn_blocks\(int n_tar\) \{ return \(n_tar \+ kNNBlock - 1\) / kNNBlock; \}",
    r"int nn_boxes_padded\(int n_tar\) \{ return \(nn_blocks\(n_tar\) \+ 3\) / 4 \* 4; \}",
    r"int nn_boxes4\(int n_tar\) \{ return nn_boxes_padded\(n_tar\) / 4; \}",
    r"size_t icp_polar_bytes\(int n_tar\) \{ return \(size_t\)\(n_tar \+ kPolarTail\) \* sizeof\(double2\); \}",
    r"size_t icp_red_bytes\(int nwaves\) \{ return \(size_t\)2 \* nwaves \* \(kRedStride \+ 4\) \* sizeof\(double\) \+ 8 \* sizeof\(double\); \}",
    # the block
    r"static inline int icp_block\(int n_src, int qpt\)\s*\{\s*int per = \(n_src \+ qpt - 1\) / qpt;\s*int blk = \(\(per \+ kWave - 1\) / kWave\) \* kWave;\s*return blk < kWave \? kWave : blk;\s*\}",
    # queries per lane: by size, the preference, the shapes that exist
    r"int qpt = \(a\.n_src \+ 1023\) / 1024;",
    r"const long waves_at_two = \(long\)a\.B \* \(\(a\.n_src \+ 127\) / 128\);",
    r"int pref = a\.qpt_pref > 0 \? a\.qpt_pref : \(a\.batch_invariant \? 2 : waves_at_two >= 7500 \? 3 : 2\);",
    r"if \(\(a\.B > 64 \|\| a\.batch_invariant\) && qpt < pref && a\.n_src > 64 \* pref\) qpt = pref;",
    r"if \(qpt > 4\) qpt = 8;",
    # LDS: the base, the copy, the list, the two limits
    r"const int block = icp_block\(a\.n_src, qpt\);",
    r"const size_t lds_base = nn_lds_bytes\(a\.n_tar\) \+ icp_red_bytes\(block / kWave\) \+ kIcpExtraLds \+ kLdsGuard;",
    r"a\.polar_copy = \(a\.ranges && lds_base \+ icp_polar_bytes\(a\.n_tar\) <= 160 \* 1024\) \? 1 : 0;",
    r"size_t lds = lds_base \+ \(a\.polar_copy \? icp_polar_bytes\(a\.n_tar\) : 0\);",
    r"a\.team_cap = 0;\s*if \(a\.polar_copy && a\.team_mode == 0\) \{\s*long cap = \(\(a\.n_src \+ 1\) / 2 \+ 15\) / 16 \* 16;\s*"
    r"const long room = \(\(long\)160 \* 1024 - \(long\)lds\) / \(long\)\(sizeof\(double2\) \+ sizeof\(int\)\);\s*"
    r"cap = cap < room \? cap : room / 16 \* 16;\s*a\.team_cap = cap > 0 \? \(int\)cap : 0;\s*\}\s*"
    r"lds \+= \(size_t\)a\.team_cap \* \(sizeof\(double2\) \+ sizeof\(int\)\);\s*"
    r"if \(lds > 160 \* 1024\) return hipErrorInvalidValue;",
    r"if \(lds > 64 \* 1024\) \{\s*\\\s*hipError_t e = hipFuncSetAttribute\(reinterpret_cast<const void \*>\(&k_icp<T, Q, U>\),",
    # the five instances
    r"if \(qpt <= 1\) SLAM_ICP_CASE\(1, 4\)\s*else if \(qpt <= 2\) SLAM_ICP_CASE\(2, 4\)\s*else if \(qpt <= 3\) SLAM_ICP_CASE\(3, 4\)\s*"
    r"else if \(qpt <= 4\) SLAM_ICP_CASE\(4, 2\)\s*else if \(qpt <= 8\) SLAM_ICP_CASE\(8, 2\)",
    # what the regions hold: a Box is four doubles, the flag words behind the hand-over are kIcpExtraLds bytes
    r"struct Box \{\s*double x0, x1, y0, y1;\s*\};",
    r"unsigned \*geo = reinterpret_cast<unsigned \*>\(lead \+ 8\);",
    r"double2 \*qlist = reinterpret_cast<double2 \*>\(geo \+ 8\);",
]


def check_source(text):
    """The restatement's constants are the source's, and every expression it restates is in the source once."""
    got = constants(text)
    want = {"kNNBlock": sh.NN_BLOCK, "kNNStride - kNNBlock": sh.NN_STRIDE - sh.NN_BLOCK, "kRedStride": sh.RED_STRIDE,
            "kPolarTail": sh.POLAR_TAIL, "kIcpExtraLds": sh.EXTRA_LDS, "kWave": sh.WAVE}
    assert got == want, (got, want)
    for e in EXPRESSIONS:
        assert len(re.findall(e, text)) == 1, e
    assert sh.LDS_LIMIT == 160 * 1024 and sh.LDS_DEFAULT == 64 * 1024 and sh.FULL_CHIP_WAVES == 7500
    assert sh.EXTRA_LDS == 8 * 4 and sh.BOX == 4 * 8 and sh.LIST_SLOT == 16 + 4


def test_constants_and_expressions_are_those_of_the_source():
    check_source(source_text())


@pytest.mark.parametrize("edit", [("constexpr int kRedStride = 8;", "constexpr int kRedStride = 16;"),
                                  ("constexpr int kPolarTail = 4;", "constexpr int kPolarTail = 8;"),
                                  ("<= 160 * 1024) ? 1 : 0;", "<= 128 * 1024) ? 1 : 0;"),
                                  ("if (qpt > 4) qpt = 8;", "if (qpt > 5) qpt = 8;"),
                                  ("a.n_src > 64 * pref) qpt = pref;", "a.n_src >= 64 * pref) qpt = pref;")])
def test_an_edit_to_the_source_is_noticed(edit):
    """The check above on a copy of the source text with one constant or comparison changed: it must fail."""
    text = source_text()
    assert text.count(edit[0]) == 1
    with pytest.raises(AssertionError):
        check_source(text.replace(edit[0], edit[1]))


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
