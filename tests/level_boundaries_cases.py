"""Id images for the level boundary tests (not collected by pytest): the planes the level region and level
component case modules lack, and the list of theirs that the boundary tests reuse.  A case is
level_regions_cases.Case: (name, message, W, H, levels to ask for).  Pixels of -1 have no region."""
import numpy as np

import level_components_cases as cc
import level_regions_cases as lc

Case = lc.Case
case = cc.case

# the padded width W + 2 crosses a wavefront (64) and a block (256) of the classify kernel
WIDTHS = (62, 63, 64, 65, 254, 255, 256, 257)
HEIGHTS = (1, 2, 3, 4, 5)


def widths():
    return [case("width_%dx%d" % (W, H), lc.boundary_ids(W, H)) for W in WIDTHS for H in HEIGHTS]


def full_cover():
    """One region covering the frame: every outer point lies outside the frame, 2W + 2H of them, none at a
    corner.  300 x 3 takes two steps of the classify kernel."""
    return [case("full_%dx%d" % (W, H), np.full((H, W), 8, np.int32)) for W, H in ((5, 4), (300, 3))]


def pixel_checker():
    """13 x 11 of one-pixel regions with id (x + 2y) mod 5: the four neighbours of a pixel have four
    different ids, none its own.  Every pixel is an inner point, and every pixel away from the frame edge
    an outer point of four groups."""
    yy, xx = np.mgrid[0:11, 0:13]
    return case("pixel_checker", ((xx + 2 * yy) % 5 + 3).astype(np.int32))


def flanked():
    """Positions with group 5 on two, three and four sides: an uncovered pixel and a pixel of group 6
    enclosed by 5 (four sides), the mouths of two U shapes (three), the inside of an L's corner and a gap
    between two bars (two).  Each is one outer point of group 5."""
    ids = np.full((9, 24), -1, np.int32)
    ids[1:4, 1:4] = 5
    ids[2, 2] = -1                  # four sides, uncovered
    ids[1:4, 5:8] = 5
    ids[2, 6] = 6                   # four sides, another group
    ids[1:4, 9:12] = 5
    ids[1, 10] = -1                 # a U open to the top: three sides
    ids[5:8, 1:4] = 5
    ids[6, 3] = 6                   # a U open to the right, filled by group 6: three sides
    ids[5:8, 6] = 5
    ids[7, 6:9] = 5                 # an L: (7, 6) has it on two sides
    ids[5:8, 11] = 5
    ids[5:8, 13] = 5                # two bars one column apart: two opposite sides
    ids[1:8, 16] = 5
    ids[4, 17:23] = 7
    ids[1:8, 23] = 5                # the frame's last column
    return case("flanked", ids)


def diagonal():
    """Two ids in one-pixel diagonal stripes over 9 x 7: the N4 components are single pixels, the N8
    components whole stripes."""
    yy, xx = np.mgrid[0:7, 0:9]
    ids = np.where((xx + yy) % 3 == 0, 2, np.where((xx + yy) % 3 == 1, 9, -1)).astype(np.int32)
    return case("diagonal", ids)


def own():
    return widths() + full_cover() + [pixel_checker(), flanked(), diagonal()]


REUSED = ("one_region_1x1", "one_region_7x1", "one_region_1x7", "one_region_9x5", "uncovered", "uncovered_frame",
          "three_levels", "region_ids", "reuse_small", "reuse_large", "rings", "interleaved", "parts",
          "fan_diagonal", "comb_up")


def all_cases():
    by_name = {c.name: c for c in cc.all_cases()}
    return own() + [by_name[n] for n in REUSED]
