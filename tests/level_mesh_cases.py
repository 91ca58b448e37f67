"""Id images for the level mesh tests (not collected by pytest): the smallest planes at which a stage of the
mesh can go wrong, and planes of the contour tests.  A case is level_regions_cases.Case: (name, message, W, H,
levels to ask for).  Pixels of -1 have no region."""
import numpy as np

import level_boundaries_cases as bc
import level_components_cases as cc
import level_contours_cases as tc
import level_regions_cases as lc
import vector_cases as vc

Case = bc.Case
case = bc.case

STRIPES = (4096, 3)
VORONOI = (640, 360)


def saddle_2x2():
    """a, b, a, b around the only interior corner: a junction of four sides.  Four N4 groups, two N8 groups."""
    return case("saddle_2x2", [[0, 1], [1, 0]])


def t_junction():
    """A bar over two regions: the bar's lower border runs straight through the junction (3, 2), which ends two
    segments there all the same; both list it, a collinear end corner."""
    ids = np.full((5, 6), 1, np.int32)
    ids[2:, :3] = 2
    ids[2:, 3:] = 3
    return case("t_junction", ids)


def island(inner, outer):
    """An island in a region: the owner is whichever has the larger group index, the twin runs the other way
    round."""
    ids = np.full((5, 6), outer, np.int32)
    ids[1:3, 2:4] = inner
    return case("island_%d_in_%d" % (inner, outer), ids)


def uncovered_hole():
    ids = np.full((5, 5), 4, np.int32)
    ids[2, 2] = -1
    return case("uncovered_hole", ids)


def uncovered_edge_pixel():
    """An uncovered pixel on the frame edge: the frame segment goes round it, no junction anywhere."""
    ids = np.full((4, 5), 4, np.int32)
    ids[0, 2] = -1
    return case("uncovered_edge_pixel", ids)


def border_to_edge():
    """A border arriving at the frame edge at both ends: two junctions of three sides."""
    ids = np.full((3, 5), 1, np.int32)
    ids[:, 2:] = 2
    return case("border_to_edge", ids)


def four_at_a_corner():
    return case("four_at_a_corner", np.repeat(np.repeat(np.array([[1, 2], [4, 3]], np.int32), 2, 0), 3, 1))


def abac():
    """a, b, a, c around a corner."""
    return case("abac", np.repeat(np.repeat(np.array([[1, 2], [3, 1]], np.int32), 3, 0), 2, 1))


def diagonal_islands(second):
    """Two one-pixel islands touching diagonally inside a third region: each island's contour is one open half
    that starts and ends at the junction between them."""
    ids = np.full((6, 7), 1, np.int32)
    ids[2, 2] = 5
    ids[3, 3] = second
    return case("diagonal_islands_5_%d" % second, ids)


def stripes():
    """Two stripes: their border is one segment of 4096 cracks and 2 vertices across 16 blocks of a crack
    kernel."""
    W, H = STRIPES
    ids = np.full((H, W), 1, np.int32)
    ids[2:] = 2
    return case("stripes_4096x3", ids)


def spiral_in_a_region():
    """The contour tests' spiral with the gaps between its arms a second region: one shared open segment that
    holds nearly every crack, and the most rounds a frame of this size takes."""
    ids = np.array(lc.id_image(tc.spiral().msg, 0), np.int32)
    ids[ids < 0] = 3
    return case("spiral_in_a_region", ids)


def voronoi():
    W, H = VORONOI
    return case("voronoi_640x360", vc.l1_voronoi(7, W, H, 60))


REUSED = ("one_region_1x1", "one_region_7x1", "one_region_1x7", "uncovered", "uncovered_frame", "three_levels",
          "checker", "rings", "parts")


def small():
    """Everything but the Voronoi plane."""
    by_name = {c.name: c for c in cc.all_cases()}
    own = [saddle_2x2(), t_junction(), island(7, 2), island(2, 7), uncovered_hole(), uncovered_edge_pixel(),
           border_to_edge(), four_at_a_corner(), abac(), diagonal_islands(5), diagonal_islands(6), stripes(),
           spiral_in_a_region(), tc.comb_8192(), tc.saddle(), tc.diagonal_hole(), tc.nested(), bc.pixel_checker(),
           bc.diagonal()]
    return own + [by_name[n] for n in REUSED]


def all_cases():
    return small() + [voronoi()]
