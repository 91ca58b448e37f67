"""SegmentationDesc messages with rasters and hierarchies for the level region tests (not collected by
pytest).  Messages are of test_proto_wire.build_schema().

A case is (name, message, W, H, levels to ask for).  Every case's regions have no two touching intervals
in one row, except touching_counter_example(), which is what it says."""
import collections

import numpy as np

import level_regions_model as lm
from test_proto_wire import build_schema

Msg = build_schema()
Case = collections.namedtuple("Case", "name msg W H levels")


def add_hierarchy(m, maps):
    """maps[l]: {id at level l: id at level l + 1}.  Writes len(maps) + 1 levels sorted by id; the top
    level's regions keep the default parent_id of -1.  CompoundRegion.size is required by the schema and
    read by nothing here: it is set to 1."""
    del m.hierarchy[:]
    for l, parents in enumerate(maps):
        level = m.hierarchy.add()
        for rid in sorted(parents):
            c = level.region.add()
            c.id, c.size, c.parent_id = rid, 1, parents[rid]
    if maps:
        level = m.hierarchy.add()
        for rid in sorted(set(maps[-1].values())):
            c = level.region.add()
            c.id, c.size = rid, 1
    return m


def desc_from_ids(ids, maps=(), order=None):
    """One Region2D per id of the image (-1: no region), its raster the maximal runs of the id; regions
    in ascending id order, or in `order`."""
    ids = np.asarray(ids, np.int32)
    H, W = ids.shape
    m = Msg()
    m.frame_width, m.frame_height = W, H
    ys, lx, rx, rid = lm.runs_of(ids)
    per = collections.defaultdict(list)
    for y, a, b, r in zip(ys.tolist(), lx.tolist(), rx.tolist(), rid.tolist()):
        per[r].append((y, a, b))
    for r in (order if order is not None else sorted(per)):
        reg = m.region.add()
        reg.id = r
        for y, a, b in per[r]:
            s = reg.raster.scan_inter.add()
            s.y, s.left_x, s.right_x = y, a, b
    return add_hierarchy(m, list(maps))


def id_image(m, level=0):
    hier = lm.rm.hierarchy_of(m)
    out = np.full((m.frame_height, m.frame_width), -1, np.int32)
    for r in m.region:
        mapped = lm.rm.get_parent_id(r.id, level, hier)
        for s in r.raster.scan_inter:
            out[s.y, s.left_x:s.right_x + 1] = mapped
    return out


# ---- the cases ------------------------------------------------------------------------------------------

def degenerate():
    out = []
    for H, W in ((1, 1), (1, 7), (7, 1), (5, 9)):
        out.append(Case("one_region_%dx%d" % (W, H), desc_from_ids(np.full((H, W), 3, np.int32)), W, H, (0,)))
    return out


BOUNDARY_WIDTHS = (63, 64, 65, 255, 256, 257, 1025)


def boundary_ids(W, H):
    """Rows whose runs start and end on and around the multiples of 64 (a wavefront) and 256 (a block):
    row 0 cuts at every such column and its two neighbours, row 1 is one run, row 2 has one-pixel
    holes at the cuts, row 3 ends runs at 64k - 1 and starts the next at 64k + 1, row 4 is made of
    one-pixel runs around the cuts with the rest uncovered."""
    ids = np.full((H, W), -1, np.int32)
    cuts = sorted({c + d for c in range(64, W + 64, 64) for d in (-1, 0, 1) if 0 < c + d < W})
    x = np.arange(W)
    which = np.searchsorted(np.asarray(cuts, np.int64), x, side="right") if cuts else np.zeros(W, np.int64)
    rows = [
        10 + which % 3,                                                  # many runs of three regions
        np.full(W, 7),                                                   # one run spans the row
        np.where(np.isin(x, cuts[1::3]), -1, 20 + (which // 3) % 2),     # holes at the cuts
        np.where(x % 64 == 0, -1, 30 + (x // 64) % 2),                   # ..., 64k - 1] and [64k + 1, ...
        np.where(np.isin(x, cuts), 40 + x % 2, -1),                      # one-pixel runs, the rest uncovered
    ]
    for y in range(H):
        ids[y] = rows[y % 5]
    return ids


def boundaries():
    return [Case("boundary_%dx%d" % (W, H), desc_from_ids(boundary_ids(W, H)), W, H, (0,))
            for W in BOUNDARY_WIDTHS for H in (1, 2, 3, 4, 5)]


def uncovered():
    W, H = 70, 6
    ids = np.full((H, W), -1, np.int32)
    ids[0, 5:] = 1                 # uncovered at the row's start
    ids[1, :30] = 1
    ids[1, 40:] = 2                # in the middle
    ids[2, :W - 9] = 2             # at the end
    # row 3 stays uncovered
    ids[4, 0] = 1
    ids[4, W - 1] = 1              # one-pixel runs at both ends of a row
    ids[5, :] = 2
    empty = Msg()
    empty.frame_width, empty.frame_height = 9, 4
    empty.region.add().id = 4      # a region without a raster
    return [Case("uncovered", desc_from_ids(ids), W, H, (0,)), Case("uncovered_frame", empty, 9, 4, (0,))]


def checker():
    """Every pixel of 96 x 64 a region of its own; level 1 has the checker's two colours."""
    W, H = 96, 64
    ids = np.arange(W * H, dtype=np.int32).reshape(H, W)
    yy, xx = np.divmod(np.arange(W * H), W)
    parents = {int(k): 100 + int((xx[k] + yy[k]) % 2) for k in range(W * H)}
    return Case("checker", desc_from_ids(ids, [parents]), W, H, (0, 1))


def three_levels():
    """64 x 48 in 8 x 8 blocks.  Level 1 groups 2 x 2 blocks; in the groups of the first block row the
    two diagonals are a region each (children that touch diagonally only), elsewhere the left and the
    right column are (children that touch vertically only), except in the last block row, where a
    group is one region (children adjacent in a row).  Level 2 has three regions.  Ids are not
    contiguous and reach 2^30 at the upper levels."""
    W, H, B = 64, 48, 8
    by, bx = np.divmod(np.arange((W // B) * (H // B)), W // B)
    block_id = {int(k): 3 + 7 * int(k) for k in range(len(by))}
    ids = np.zeros((H, W), np.int32)
    for k in block_id:
        ids[by[k] * B:(by[k] + 1) * B, bx[k] * B:(bx[k] + 1) * B] = block_id[k]
    l1, l2 = {}, {}
    for k in block_id:
        gy, gx = int(by[k]) // 2, int(bx[k]) // 2
        group = gy * 4 + gx
        if gy == 0:
            half = (int(by[k]) + int(bx[k])) % 2          # diagonals
        elif gy == 1:
            half = int(bx[k]) % 2                         # columns
        else:
            half = 0                                      # the whole group
        parent = (1 << 30) - 50 + 2 * group + half
        l1[block_id[k]] = parent
        l2[parent] = (0, 1, (1 << 30) + 7)[gy]
    return Case("three_levels", desc_from_ids(ids, [l1, l2]), W, H, (0, 1, 2))


def region_ids():
    ids = np.array([[0, 0, 1, 1, 5, 1000], [1, 0, (1 << 30) - 1, (1 << 30) - 1, (1 << 30) + 7, 0]], np.int32)
    return Case("region_ids", desc_from_ids(ids), 6, 2, (0,))


def moments():
    """3840 x 4, everything at x >= 3000, where 2 * n * n is above 2^24.  Region 1: one-pixel intervals
    at every other column of all four rows, 4 * 420 = 1680 of them (the frame has room for no more
    right of x = 3000); region 2: the columns between them in rows 0 and 1."""
    W, H = 3840, 4
    ids = np.full((H, W), -1, np.int32)
    ids[:, 3000::2] = 1
    ids[0:2, 3001::2] = 2
    m = desc_from_ids(ids)
    assert len(m.region[0].raster.scan_inter) == 1680
    return Case("moments", m, W, H, (0,))


def reuse_sequence():
    """Small, large, small content for one 160 x 120 handle."""
    W, H = 160, 120
    small = np.full((H, W), -1, np.int32)
    small[10:20, 5:101] = 9
    large = (np.arange(W * H, dtype=np.int32).reshape(H, W) // 2) * 3 + 1     # two-pixel regions
    return [Case("reuse_small", desc_from_ids(small), W, H, (0,)), Case("reuse_large", desc_from_ids(large), W, H, (0,))]


def all_cases():
    return (degenerate() + boundaries() + uncovered() + [checker(), three_levels(), region_ids(), moments()]
            + reuse_sequence())


def touching_counter_example():
    """Region 5 has the touching intervals [0, 3] and [4, 7] in row 0 and nothing else; region 6 lies
    in row 1.  Both have parent 9.  MergeRasterization copies row 0, which only one side has, as it
    is: two intervals.  The id plane shows one run [0, 7]."""
    m = Msg()
    m.frame_width, m.frame_height = 8, 2
    a = m.region.add()
    a.id = 5
    for lx, rx in ((0, 3), (4, 7)):
        s = a.raster.scan_inter.add()
        s.y, s.left_x, s.right_x = 0, lx, rx
    b = m.region.add()
    b.id = 6
    s = b.raster.scan_inter.add()
    s.y, s.left_x, s.right_x = 1, 2, 5
    return add_hierarchy(m, [{5: 9, 6: 9}])
