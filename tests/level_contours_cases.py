"""Id images for the level contour tests (not collected by pytest): planes of the level region, component,
boundary, adjacency and colour tests, and the shapes only a contour tracer can get wrong.  A case is
level_regions_cases.Case: (name, message, W, H, levels to ask for).  Pixels of -1 have no region."""
import numpy as np

import level_adjacency_cases as ac
import level_boundaries_cases as bc
import level_colors_cases as kc
import level_components_cases as cc
import level_regions_cases as lc

Case = bc.Case
case = bc.case

LONG = (4096, 3)       # the widest full cover: collinear runs of 4096 cracks across 16 blocks of a crack kernel
COMB = (4096, 7)       # W, H of comb_8192
SPIRAL = (129, 65)


def full_cover():
    """One region covering the frame: one contour of four vertices whatever the size; its sides are runs of
    collinear cracks that cross every wavefront and block boundary of the crack kernels."""
    sizes = [(W, H) for W in bc.WIDTHS for H in bc.HEIGHTS] + [LONG]
    return [case("cover_%dx%d" % (W, H), np.full((H, W), 8, np.int32)) for W, H in sizes]


def saddle():
    """Two diagonal pixels of one region and nothing else: two contours under every connectedness, though
    they are one N8 component."""
    ids = np.full((4, 5), -1, np.int32)
    ids[1, 1] = ids[2, 2] = 6
    return case("saddle", ids)


def diagonal_hole():
    """A ring whose hole is two diagonal pixels: the hole is one contour of 8 vertices that passes the middle
    corner twice."""
    ids = np.full((6, 6), 4, np.int32)
    ids[2, 2] = ids[3, 3] = -1
    return case("diagonal_hole", ids)


def wide_hole():
    """A ring with a hole three pixels wide and two high: the crack of smallest key of the hole, the bottom
    side of the pixel above the hole's left end, has a straight predecessor."""
    ids = np.full((7, 9), 4, np.int32)
    ids[2:4, 3:6] = 9
    ids[5, 1:3] = -1
    return case("wide_hole", ids)


def nested():
    """Ring in ring in ring: region 1 around region 2 around region 1 around uncovered pixels around region 2
    around region 1, each ring one pixel wide; holes and islands nested three deep."""
    n = 13
    ids = np.full((n, n), -1, np.int32)
    for k, v in enumerate((1, 2, 1, -1, 2, 1)):
        ids[k:n - k, k:n - k] = v
    return case("nested", ids)


def comb_8192():
    """8192 one-pixel teeth on two spines (rows 1 and 5; teeth in rows 0, 2, 4 and 6 at the even columns),
    the spines joined at column 0: one region, one contour of more than 2^14 vertices."""
    W, H = COMB
    ids = np.full((H, W), -1, np.int32)
    ids[[1, 5], :] = 5
    ids[0::2, 0::2] = 5
    ids[3, 0] = 5
    return case("comb_8192", ids)


def spiral():
    """129 x 65: a one-pixel-wide rectangular spiral with one-pixel gaps between its arms, wound inwards: one
    contour that holds every crack of the frame, the longest chain a frame of this size has."""
    W, H = SPIRAL
    ids = np.full((H, W), -1, np.int32)
    def free(y, x):
        return 0 <= y < H and 0 <= x < W and ids[y, x] < 0

    y = x = 0
    ids[0, 0] = 9
    dy, dx = 0, 1
    turned = False
    while True:
        # forward while the next pixel is free and the one behind it is not an arm already
        if free(y + dy, x + dx) and (free(y + 2 * dy, x + 2 * dx) or not (0 <= y + 2 * dy < H and 0 <= x + 2 * dx < W)):
            y, x = y + dy, x + dx
            ids[y, x] = 9
            turned = False
        elif turned:
            break
        else:
            dy, dx = dx, -dy                       # turn right: (0, 1) -> (1, 0) -> (0, -1) -> (-1, 0)
            turned = True
    return case("spiral_129x65", ids)


def own():
    return full_cover() + [saddle(), diagonal_hole(), wide_hole(), nested(), comb_8192(), spiral()]


REUSED = ("one_region_1x1", "one_region_7x1", "one_region_1x7", "one_region_9x5", "uncovered", "uncovered_frame",
          "three_levels", "checker", "region_ids", "rings", "interleaved", "parts", "fan_diagonal", "comb_up",
          "serpentine")


def reuse():
    """Small and large content for one 160 x 120 handle."""
    return lc.reuse_sequence()


def all_cases():
    by_name = {c.name: c for c in cc.all_cases()}
    reused = [by_name[n] for n in REUSED]
    return (own() + reused + [bc.pixel_checker(), bc.flanked(), bc.diagonal(), ac.max_id(), ac.hole(),
                              kc.comb().case] + [case("width_%dx%d" % (W, 5), lc.boundary_ids(W, 5))
                                                 for W in (63, 64, 65, 257)])
