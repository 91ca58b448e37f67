"""Id images for the level component tests (not collected by pytest), as SegmentationDesc messages built
with level_regions_cases.desc_from_ids.  A case is level_regions_cases.Case: (name, message, W, H, levels
to ask for).  Pixels of -1 have no region."""
import numpy as np

import level_regions_cases as lc

Case = lc.Case


def case(name, ids, maps=(), levels=(0,)):
    ids = np.asarray(ids, np.int32)
    return Case(name, lc.desc_from_ids(ids, maps), ids.shape[1], ids.shape[0], tuple(levels))


def serpentine():
    """65 x 65: the even columns are filled, the odd ones join them alternately at the top and at the
    bottom.  One component either way, of 2 113 runs, all but two rows' of one pixel, linked end to end:
    the longest chain of unions a frame of this size has."""
    ids = np.full((65, 65), -1, np.int32)
    ids[:, 0::2] = 4
    for x in range(1, 65, 2):
        ids[0 if (x // 2) % 2 else 64, x] = 4
    return case("serpentine", ids)


def spiral():
    """65 x 65: a one-pixel-wide square spiral with one-pixel gaps between its arms, wound inwards."""
    n = 65
    ids = np.full((n, n), -1, np.int32)
    y = x = 0
    ids[0, 0] = 9
    dy, dx = 0, 1
    # arms of n - 1, n - 1, n - 1, then n - 3, n - 3, n - 5, n - 5, ... pixels
    lengths = [n - 1] + [n - 1 - 2 * (k // 2) for k in range(2 * n)]
    for length in lengths:
        if length <= 0:
            break
        for _ in range(length):
            y, x = y + dy, x + dx
            ids[y, x] = 9
        dy, dx = dx, -dy                           # turn right: (0, 1) -> (1, 0) -> (0, -1) -> (-1, 0)
    return case("spiral", ids)


def comb(up):
    """64 x 9: 32 one-pixel teeth at the even columns, eight rows long, joined by one full row: the
    bottom row when the teeth point up (the labels merge in the last row) or the top row when they
    point down (they merge in the first)."""
    ids = np.full((9, 64), -1, np.int32)
    ids[:, 0::2] = 6
    ids[8 if up else 0, :] = 6
    return case("comb_up" if up else "comb_down", ids)


def fans():
    """257 x 2, one row pair.  fan_down: one run of the full width above 128 one-pixel runs of the same
    id; fan_up: the mirror image; fan_offset: the lower runs one column further right; fan_diagonal:
    one-pixel runs at the even columns above one-pixel runs at the odd columns, which touch diagonally
    only: one component under N8, 256 under N4."""
    W = 257
    out = []
    for name, top, bottom in (("fan_down", None, range(0, 256, 2)), ("fan_up", range(0, 256, 2), None),
                              ("fan_offset", None, range(1, 257, 2)),
                              ("fan_diagonal", range(0, 256, 2), range(1, 257, 2))):
        ids = np.full((2, W), -1, np.int32)
        for y, cols in ((0, top), (1, bottom)):
            if cols is None:
                ids[y, :] = 2
            else:
                ids[y, list(cols)] = 2
        out.append(case(name, ids))
    return out


def rings():
    """33 x 33: region 11 around region 12 around uncovered pixels around region 11 again."""
    ids = np.full((33, 33), 11, np.int32)
    ids[4:29, 4:29] = 12
    ids[9:24, 9:24] = -1
    ids[13:20, 13:20] = 11
    return case("rings", ids)


def interleaved():
    """24 x 18 in 2 x 3 blocks (rows x columns) of two ids laid out as a checker: the blocks of an id
    touch diagonally only.  The ids are 7 and 2^30."""
    yy, xx = np.mgrid[0:18, 0:24]
    ids = np.where(((yy // 2) + (xx // 3)) % 2 == 0, 7, 1 << 30).astype(np.int32)
    return case("interleaved", ids)


def parts():
    """40 x 12 with a hierarchy: four blobs of four ids; level 1 joins the two left ones (which touch
    at a corner only) and the two right ones (four columns apart)."""
    ids = np.full((12, 40), -1, np.int32)
    ids[1:5, 2:8] = 1
    ids[5:9, 8:14] = 2            # touches blob 1 diagonally
    ids[1:5, 22:26] = 3
    ids[1:5, 30:36] = 4
    return case("parts", ids, [{1: 50, 2: 50, 3: 60, 4: 60}], (0, 1))


def named():
    return [serpentine(), spiral(), comb(True), comb(False)] + fans() + [rings(), interleaved(), parts()]


def all_cases():
    return (lc.degenerate() + lc.boundaries() + lc.uncovered() + [lc.checker(), lc.three_levels(), lc.region_ids()]
            + lc.reuse_sequence() + named())
