"""The device workspaces of the two ray casts for large maps without a GPU, as the library answers for them
(slam_plan_query "wedge_ws_bytes" / "tile_ws_bytes": a = scans of the cast, b = beams, c = groups).  The library declares each
engine's pieces once (csrc/grid_kernels.hip: wedge_pieces, tile_pieces, on a Layout of csrc/workspace.h) and both sizes the
arena and places the pieces from that one list; here the list is restated from the comments of WedgeScratch and TileScratch."""
import itertools

import pytest

import icp_shapes as sh

ALIGN = 256                    # Layout::kAlign: every piece starts on a multiple of it
WEDGE_CLASSES = 16             # kWedgeClasses: 4 slope classes x steep x direction
WEDGE_PART_MIN = 512 * 4       # kWedgePartMin: rays per part of a unit (kWedgeThreads * kWedgeSlots)
TILE_WORDS = 2048 // 32        # kTileWords: a recorded walk is kTileSteps bits
RAY_REC = 32                   # sizeof(RayRec): x0, y0, dx, yend, flags, pad[3]

BEAMS = (1, 360, 8192)
SCANS = (1, 2, 17, 65535, 70000)


def groups_of(scans):
    return sorted({1, -(-scans // 16), scans})


def laid_out(pieces):
    return sum(-(-size * count // ALIGN) * ALIGN for size, count in pieces)


def wedge_pieces(rays, scans, groups):
    return [(4, rays),                                                          # ends  [rays] uint32
            (4, scans),                                                         # orgs  [scans] uint32
            (4, groups * (WEDGE_CLASSES + 1)),                                  # offs  [groups][kWedgeClasses + 1] int
            (4, groups * WEDGE_CLASSES),                                        # cost  [groups][kWedgeClasses] uint32
            (4, 1 + groups * WEDGE_CLASSES + rays // WEDGE_PART_MIN),           # order [1 + groups * kWedgeClasses + rays / kWedgePartMin] uint32
            (2, rays)]                                                          # list  [rays] unsigned short


def tile_pieces(rays, groups):
    return [(RAY_REC, rays),                                                    # recs   [rays] RayRec
            (4, rays * TILE_WORDS),                                             # bits   [rays][kTileWords] uint32
            (2, rays * TILE_WORDS),                                             # prefix [rays][kTileWords] unsigned short
            (4, groups * 4)]                                                    # gbox   [groups][4] int


@pytest.mark.parametrize("beams,scans", list(itertools.product(BEAMS, SCANS)))
def test_the_library_lays_out_the_pieces_the_structs_list(beams, scans):
    rays = scans * beams
    for groups in groups_of(scans):
        assert sh.query("wedge_ws_bytes", scans, beams, groups) == laid_out(wedge_pieces(rays, scans, groups)), (beams, scans, groups)
        assert sh.query("tile_ws_bytes", scans, beams, groups) == laid_out(tile_pieces(rays, groups)), (beams, scans, groups)


@pytest.mark.parametrize("name", ["wedge_ws_bytes", "tile_ws_bytes"])
def test_the_reservation_at_one_group_per_scan_covers_every_launch(name):
    """Non-decreasing in groups (the reservation is taken at groups = scans, the launch places the pieces at its own group
    count), and in scans at a fixed group size (a chunk of an oversize launch has fewer scans than the whole)."""
    for beams in BEAMS:
        for scans in SCANS:
            sizes = [sh.query(name, scans, beams, g) for g in groups_of(scans)]
            assert sizes == sorted(sizes) and sizes[0] > 0, (beams, scans, sizes)
        whole = [sh.query(name, s, beams, s) for s in SCANS]
        assert whole == sorted(whole), (beams, whole)


def test_the_arithmetic_is_done_in_64_bits():
    """70 000 scans of 8 192 beams: 573 440 000 rays, whose recorded walks alone are 32 + 256 + 128 bytes each."""
    rays = 70000 * 8192
    tiles = sh.query("tile_ws_bytes", 70000, 8192, 70000)
    assert tiles == laid_out(tile_pieces(rays, 70000)) and tiles > rays * 416 > 2 ** 31
    wedges = sh.query("wedge_ws_bytes", 70000, 8192, 70000)
    assert wedges == laid_out(wedge_pieces(rays, 70000, 70000)) and wedges > rays * 6 > 2 ** 31
