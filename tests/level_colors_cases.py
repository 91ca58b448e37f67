"""Pairs of an id image and a BGR24 frame for the level colour tests (not collected by pytest).  A case is
(name, case, F): `case` a level_regions_cases.Case (name, message, W, H, levels to ask for) that gives P at
every one of its levels, and F the H x W x 3 uint8 frame, made from a fixed seed.  The planes are those of the
level region, boundary, adjacency and overlap tests."""
import collections
import zlib

import numpy as np

import level_adjacency_cases as ac
import level_boundaries_cases as bc
import level_overlap_cases as oc
import level_regions_cases as lc

CCase = collections.namedtuple("CCase", "name case F")

MAX = oc.MAX
COMB = (256, 64)      # W, H of the comb
COMB_INTERVALS = 128 * 64


def frame(W, H, seed):
    """Uniform noise over all 256 values; the same frame for the same arguments."""
    return np.random.RandomState(seed).randint(0, 256, (H, W, 3)).astype(np.uint8)


def ccase(name, ids, F=None):
    ids = np.asarray(ids, np.int32)
    H, W = ids.shape
    return CCase(name, bc.case(name, ids), frame(W, H, zlib.crc32(name.encode())) if F is None else F)


def of(case):
    return CCase(case.name, case, frame(case.W, case.H, zlib.crc32(case.name.encode())))


def widths():
    """level_regions_cases.boundary_ids: runs that start and end on and around the multiples of 64 and 256,
    long and short ones side by side, and row 1 one run."""
    return [ccase("width_%dx%d" % (W, H), lc.boundary_ids(W, H)) for W in bc.WIDTHS for H in bc.HEIGHTS]


def checker():
    """A one-pixel checker of two ids over 64 x 8: every interval is one pixel."""
    yy, xx = np.mgrid[0:8, 0:64]
    return ccase("checker", np.where((xx + yy) % 2 == 0, 4, 6))


def stars():
    """The 300-region stars of the adjacency tests and their transposes."""
    return [of(c) for c in ac.stars()]


def comb():
    """One region on every other column of 256 x 64: 8192 one-pixel intervals in one group, which no single
    slice of the interval list holds."""
    W, H = COMB
    ids = np.full((H, W), -1, np.int32)
    ids[:, 0::2] = 5
    return ccase("comb", ids)


RUNS_WAVES = 2048     # k_color_runs gives a wavefront one interval until there are this many wavefronts,
SHARES = (1, 2, 4, 8, 16, 32, 64)      # then two, four, ... up to 64


def share_of(intervals):
    """The intervals one wavefront of k_color_runs takes for a list of that length."""
    share = 64
    while share > 1 and intervals // share < RUNS_WAVES:
        share //= 2
    return share


def mixed(share):
    """128 columns: a one-pixel checker of two ids over the left 96, then runs of 15, 16 and 1 pixels of three
    more ids (the two lengths around the one from which all lanes sum an interval together); 99 intervals per
    row, and as many rows as make k_color_runs give a wavefront `share` intervals."""
    W, per_row = 128, 99
    H = 8 if share == 1 else (RUNS_WAVES * share + per_row - 1) // per_row + 1
    yy, xx = np.mgrid[0:H, 0:W]
    ids = np.where((xx + yy) % 2 == 0, 4, 6)
    ids[:, 96:111] = 20 + yy[:, 96:111] % 2
    ids[:, 111:127] = 30
    ids[:, 127] = 20
    assert share_of(H * per_row) == share
    return ccase("mixed_share_%d" % share, ids)


def shares():
    return [mixed(s) for s in SHARES]


def hierarchies():
    """The hole (one level) and the three-level hierarchy; asked at every level."""
    return [of(ac.hole()), of(lc.three_levels())]


def max_id():
    return of(ac.max_id())


def uncovered_frame():
    return of({k.name: k for k in lc.uncovered()}["uncovered_frame"])


def halves():
    """Groups of two and of four pixels whose channel sums are odd multiples of half their area: the mean is
    an exact half and has to go up.  Group 0: bytes (0, 1), (254, 255), (7, 8); group 1: four pixels summing to
    4 * 10 + 2, 4 * 200 + 2 and 2; group 2: one pixel."""
    ids = np.array([[0, 0, 1, 1, 1, 1, 2]], np.int32)
    F = np.zeros((1, 7, 3), np.uint8)
    F[0, 0:2] = [[0, 254, 7], [1, 255, 8]]
    F[0, 2:6] = [[10, 200, 0], [10, 200, 0], [11, 201, 1], [11, 201, 1]]
    F[0, 6] = [9, 90, 255]
    return ccase("halves", ids, F)


def equal_means():
    """Two neighbours with equal means and different pixels, next to a third group: the picture shows no edge
    between the first two."""
    ids = np.zeros((6, 12), np.int32)
    ids[:, 4:8] = 1
    ids[:, 8:] = 2
    F = np.empty((6, 12, 3), np.uint8)
    F[:, 0:4] = [100, 50, 200]
    F[:, 4:8:2] = [90, 40, 190]
    F[:, 5:8:2] = [110, 60, 210]
    F[:, 8:] = [10, 20, 30]
    return ccase("equal_means", ids, F)


def small():
    """The cases small enough for the brute-force double loop."""
    return [c for c in all_cases() if c.case.W * c.case.H <= 1500]


def all_cases():
    return (widths() + [checker()] + stars() + [comb()] + hierarchies() + [max_id(), uncovered_frame(), halves(),
                                                                          equal_means()])
