"""SegmentationDesc messages for the boundary persistence tests (not collected by pytest), built from
level_regions_cases.desc_from_ids / add_hierarchy.  A case is level_regions_cases.Case: (name, message, W, H,
levels), levels being every level of the hierarchy, range(L).  Each is one of the smallest shapes at which a
kernel can still go wrong."""
import numpy as np

import level_adjacency_cases as ac
import level_boundaries_cases as bc
import level_regions_cases as lc

Case = lc.Case
LADDER_HEIGHTS = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 20)


def case(name, ids, maps=(), order=None):
    ids = np.asarray(ids, np.int32)
    maps = list(maps)
    return Case(name, lc.desc_from_ids(ids, maps, order), ids.shape[1], ids.shape[0], tuple(range(len(maps) + 1)))


def two_level_map(ids):
    """Level 1 merges the ids of the plane in threes."""
    return {int(r): 500 + int(r) // 3 for r in np.unique(ids[ids >= 0])}


def widths():
    """The tile (4 x 4 pixels a thread) and block (256 x 16 pixels) edges of the plane kernels."""
    out = []
    for W in bc.WIDTHS:
        for H in bc.HEIGHTS:
            ids = lc.boundary_ids(W, H)
            out.append(case("width_%dx%d" % (W, H), ids, [two_level_map(ids)]))
    return out


def ladder_maps(L):
    """L + 1 regions 0 .. L of level 0; neighbours k, k + 1 merge at level k + 1, the last pair never.  At level
    l the regions 0 .. l are one (named 1000 * l), k > l is still itself (1000 * l + k)."""
    def name(l, k):
        return k if l == 0 else 1000 * l + (0 if k <= l else k)
    return [{name(l, k): name(l + 1, k) for k in range(L + 1)} for l in range(L - 1)]


def ladder(L):
    """A 2-row frame of L + 1 one-column regions: pers(k, k + 1) = k + 1 for k < L - 1 and L for the last pair, so
    every value 1 .. L occurs and every end of the bisection is hit.  L = 1 is the desc without a hierarchy."""
    ids = np.tile(np.arange(L + 1, dtype=np.int32), (2, 1))
    c = case("ladder_%d" % L, ids, ladder_maps(L))
    assert len(c.msg.hierarchy) == (L if L > 1 else 0)
    return c


def ladders():
    return [ladder(L) for L in LADDER_HEIGHTS]


def narrow():
    """W = 5 and W = 7: 3 * W is no multiple of 4, every row of the picture ends in a partial tile."""
    out = []
    for W in (5, 7):
        yy, xx = np.mgrid[0:6, 0:W]
        ids = (xx // 2 + 4 * (yy // 3)).astype(np.int32)
        out.append(case("narrow_%d" % W, ids, [{int(r): 50 + int(r) % 4 for r in np.unique(ids)},
                                                {50 + k: 90 + k // 2 for k in range(4)}]))
    return out


def max_id():
    """Ids 0 and 2^31 - 1 with a parent of 2^31 - 2: the dense numbering makes them columns 0 and 1."""
    c = ac.max_id()
    ids = lc.id_image(c.msg, 0)
    return case("max_id", ids, [{0: 5, ac.MAX_ID: ac.MAX_ID - 1}, {5: 9, ac.MAX_ID - 1: 9}])


def out_of_order():
    """Regions listed in descending id order: the dense numbers are not in id order."""
    yy, xx = np.mgrid[0:7, 0:9]
    ids = (10 * (xx // 3) + yy // 2 + 1).astype(np.int32)
    present = sorted(int(r) for r in np.unique(ids))
    return case("out_of_order", ids, [{r: 100 + r // 10 for r in present}, {100: 7, 101: 7, 102: 8}],
                order=present[::-1])


def reused():
    by_name = {c.name: c for c in lc.all_cases()}
    out = []
    for n in ("three_levels", "checker", "uncovered", "uncovered_frame", "reuse_small", "reuse_large"):
        c = by_name[n]
        out.append(Case(c.name, c.msg, c.W, c.H, tuple(range(max(1, len(c.msg.hierarchy))))))
    return out


def all_cases():
    return widths() + ladders() + narrow() + [max_id(), out_of_order()] + reused()
