"""Plain-Python restatement of the scan matcher's launch decision for its workgroup shapes
(launch_icp_t in csrc/icp_kernels.hip, the branch behind the one-wave shape: k_icp<T, QPT, UNROLL>,
one workgroup per pair).  Test infrastructure only: tests/test_icp_launch_shapes_cpu.py checks it
against the source text and asserts the sizes at which a decision changes; the GPU tests of
tests/test_gpu_icp_workgroup_shapes.py and tests/test_gpu_parity.py take their sizes from edges().

What the launch decides, and what launch() returns as a Shape:
  qpt         queries per lane: 1, 2, 3, 4 or 8 (by n_src, or by the preference for batches)
  block       threads per workgroup: ceil(n_src / qpt) rounded up to whole waves of 64
  waves       block / 64
  polar_copy  whether a second, unpadded copy of the target goes into LDS (scans only, while it fits)
  team_cap    slots of the first-iteration list (nn_listed): half of the queries rounded up to 16,
              as far as the LDS has room; 0 without the copy or with icp_team != 0
  cap_wanted  the list before the LDS cuts it
  lds         dynamic LDS bytes of the launch; above 64 KiB the launch raises the kernel's limit
"""
from __future__ import annotations

from collections import namedtuple

WAVE = 64
NN_BLOCK = 16                  # kNNBlock
NN_STRIDE = NN_BLOCK + 1       # kNNStride
RED_STRIDE = 8                 # kRedStride
POLAR_TAIL = 4                 # kPolarTail
EXTRA_LDS = 32                 # kIcpExtraLds
DOUBLE2, BOX, LIST_SLOT = 16, 32, 16 + 4   # sizeof(double2), sizeof(Box) (4 doubles), a list slot: double2 + int
LDS_LIMIT = 160 * 1024         # what a CU has: the launch fails above it
LDS_DEFAULT = 64 * 1024        # what a kernel gets without hipFuncSetAttribute
FULL_CHIP_WAVES = 7500         # waves at two queries per lane from which the automatic preference is 3
N_MAX = 8192                   # documented maximum of n_src and n_tar
QPTS = (1, 2, 3, 4, 8)

Shape = namedtuple("Shape", "qpt block waves polar_copy team_cap cap_wanted lds")


def nn_lds_bytes(n_tar):
    """Padded image of the target and its boxes: one per block padded to a multiple of 4, one per 4 blocks."""
    blocks = (n_tar + NN_BLOCK - 1) // NN_BLOCK
    padded = (blocks + 3) // 4 * 4
    return blocks * NN_STRIDE * DOUBLE2 + (padded + padded // 4) * BOX


def icp_red_bytes(waves):
    """Two alternating buffers of [waves][kRedStride] sums and [waves][4] collapsed-set words, and the 8 doubles a
    pair's first wave hands the others (kLead)."""
    return 2 * waves * (RED_STRIDE + 4) * 8 + 8 * 8


def icp_polar_bytes(n_tar):
    return (n_tar + POLAR_TAIL) * DOUBLE2


def icp_block(n_src, qpt):
    per = (n_src + qpt - 1) // qpt
    return max(WAVE, (per + WAVE - 1) // WAVE * WAVE)


def preference(B, n_src, icp_qpt=0, batch_invariant=False):
    if icp_qpt > 0:
        return icp_qpt
    if batch_invariant:
        return 2
    return 3 if B * ((n_src + 127) // 128) >= FULL_CHIP_WAVES else 2


def preferred(B, n_src, icp_qpt=0, batch_invariant=False):
    """Whether the preference replaces the size-derived queries per lane."""
    pref = preference(B, n_src, icp_qpt, batch_invariant)
    return (B > 64 or batch_invariant) and (n_src + 1023) // 1024 < pref and n_src > 64 * pref


def queries_per_lane(B, n_src, icp_qpt=0, batch_invariant=False):
    qpt = (n_src + 1023) // 1024
    if preferred(B, n_src, icp_qpt, batch_invariant):
        qpt = preference(B, n_src, icp_qpt, batch_invariant)
    return 8 if qpt > 4 else qpt


def launch(B, n_src, n_tar, scans, icp_qpt=0, batch_invariant=False, icp_team=0, guard=0):
    """The workgroup launch of B pairs; scans: the clouds are raw scans (a replay, particles), not point buffers.
    guard: the debug build's guard bytes (kLdsGuard), 0 in the shipped build.  None where the launch fails."""
    qpt = queries_per_lane(B, n_src, icp_qpt, batch_invariant)
    block = icp_block(n_src, qpt)
    base = nn_lds_bytes(n_tar) + icp_red_bytes(block // WAVE) + EXTRA_LDS + guard
    polar_copy = bool(scans) and base + icp_polar_bytes(n_tar) <= LDS_LIMIT
    lds = base + (icp_polar_bytes(n_tar) if polar_copy else 0)
    team_cap = cap_wanted = 0
    if polar_copy and icp_team == 0:
        cap_wanted = ((n_src + 1) // 2 + 15) // 16 * 16
        room = (LDS_LIMIT - lds) // LIST_SLOT
        team_cap = max(0, cap_wanted if cap_wanted < room else room // 16 * 16)
    lds += team_cap * LIST_SLOT
    if lds > LDS_LIMIT or qpt > 8:
        return None
    return Shape(qpt, block, block // WAVE, polar_copy, team_cap, cap_wanted, lds)


def live_first_queries(n_src, qpt):
    """Per wave of the workgroup: whether lane 0's first query exists (SameMatch reads it in every wave)."""
    return [w * WAVE < n_src for w in range(icp_block(n_src, qpt) // WAVE)]


def first(pred, lo=1, hi=N_MAX):
    """The smallest n in lo..hi with pred(n), after checking that pred holds from there on (one transition)."""
    hits = [n for n in range(lo, hi + 1) if pred(n)]
    assert hits and hits == list(range(hits[0], hi + 1)), "not a single transition"
    return hits[0]


def edges(scans, B=2, guard=0, **options):
    """The sizes n = n_src = n_tar in 1..8192 at which a decision changes, each as the FIRST n on the far side:
      qpt2, qpt3, qpt4, qpt8   first n with that many queries per lane
      raised                   first n whose launch needs more than 64 KiB
    and for scans
      cut, zero                first n whose list is shorter than wanted; first n without a list
      dropped                  first n without the unpadded copy."""
    def at(n):
        return launch(B, n, n, scans, guard=guard, **options)
    out = {"qpt%d" % q: first(lambda n, q=q: at(n).qpt >= q) for q in QPTS[1:]}
    out["raised"] = first(lambda n: at(n).lds > LDS_DEFAULT)
    if scans:
        out["dropped"] = first(lambda n: not at(n).polar_copy)
        out["cut"] = first(lambda n: at(n).team_cap < at(n).cap_wanted, hi=out["dropped"] - 1)
        out["zero"] = first(lambda n: at(n).team_cap == 0, hi=out["dropped"] - 1)
    return out
