"""Id images for the level adjacency tests (not collected by pytest): every plane of the level boundary
tests, and the ones only an adjacency graph can get wrong.  A case is level_regions_cases.Case: (name,
message, W, H, levels to ask for).  Pixels of -1 have no region."""
import numpy as np

import level_boundaries_cases as bc

Case = bc.Case
case = bc.case

MAX_ID = (1 << 31) - 1
STAR_HUB = 7
STAR_LEAVES = 300


def stars():
    """Row 0 is one hub region, row 1 holds 300 distinct one-pixel regions: a node with 300 edges, more
    than a wavefront (64) and more than a block (256) of any kernel that walks a node's edges; and its
    transpose, where every leaf is in a row of its own."""
    ids = np.empty((2, STAR_LEAVES), np.int32)
    ids[0] = STAR_HUB
    ids[1] = 100 + np.arange(STAR_LEAVES)
    return [case("star_300x2", ids), case("star_2x300", np.ascontiguousarray(ids.T))]


def diag_only():
    """A two-id one-pixel checker of 9 x 7: under N4 components every component is one pixel whose only
    neighbours of its own id are diagonal."""
    yy, xx = np.mgrid[0:7, 0:9]
    return case("diag_only", np.where((xx + yy) % 2 == 0, 4, 6).astype(np.int32))


def max_id():
    """Ids 0 and 2^31 - 1 side by side: the key's group and neighbour fields at their full 31 bits."""
    ids = np.zeros((3, 6), np.int32)
    ids[:, 3:] = MAX_ID
    ids[1, 1] = MAX_ID                                # and enclosed by the other, both ways round
    ids[1, 4] = 0
    return case("max_id", ids)


def hole():
    """Region 3 covers the frame but for an uncovered hole; region 8 lies in the hole and touches 3 along
    its top: node 3 has sides on the frame edge, next to uncovered pixels and next to another group."""
    ids = np.full((10, 12), 3, np.int32)
    ids[2:8, 3:9] = -1
    ids[2:5, 5:7] = 8
    return case("hole", ids)


def own():
    return stars() + [diag_only(), max_id(), hole()]


def all_cases():
    return bc.all_cases() + own()
