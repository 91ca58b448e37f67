"""Plain numpy / Python model of the regions of a hierarchy level (not collected by pytest; the level
region tests compare the product against it bit for bit).  Two definitions:

  literal   the reference, restated member by member from reading it:
              GetParentMap                      segment_util/segmentation_util.cpp:199-213
              MergeRasterization                :484-570
              MergeRasterizations               :572-590 (the fold Merge(rasters[i], prev))
              GetCompoundRegionRasterizations   :592-605
              RasterizationArea                 :644-650
              ShapeMomentsFromRasterization     :652-693, in np.float32 and np.float64 where it has
                                                float and double
  runs      the maximal runs of equal id per row of an id image, all rows at once, and the same sums

A rasterization is a list of (y, left_x, right_x).  Both return (regions, intervals): a REGION_DTYPE
array ordered by id and an (n, 4) int32 array {y, left_x, right_x, id} grouped in that order, the
layout of vsg_render_level_regions.  A region whose merged rasterization is empty is left out: it
covers no pixel (the reference would divide by its area of 0).

Messages are parsed SegmentationDesc objects of test_proto_wire.build_schema()."""
import numpy as np

import render_model as rm

REGION_DTYPE = np.dtype([
    ("id", np.int32), ("first_interval", np.int32), ("num_intervals", np.int32), ("area", np.int32),
    ("min_x", np.int32), ("min_y", np.int32), ("max_x", np.int32), ("max_y", np.int32),
    ("size", np.float32), ("mean_x", np.float32), ("mean_y", np.float32),
    ("moment_xx", np.float32), ("moment_xy", np.float32), ("moment_yy", np.float32),
])
FLOAT_FIELDS = ("size", "mean_x", "mean_y", "moment_xx", "moment_xy", "moment_yy")

F = np.float32
INT_MAX = 2 ** 31 - 1


# ---- literal ------------------------------------------------------------------------------------------

def get_parent_map(msg, level, hierarchy):
    """{parent id: [Region2D, ...]} in the desc's order (an unordered_map of vectors filled by
    push_back; the clamp of `level` is left to the caller, as the library refuses such a level)."""
    parent_map = {}
    for region in msg.region:
        parent_id = rm.get_parent_id(region.id, level, hierarchy)
        parent_map.setdefault(parent_id, []).append(region)
    return parent_map


def raster_of(region):
    return [(s.y, s.left_x, s.right_x) for s in region.raster.scan_inter]


def merge_rasterization(lhs, rhs):
    merged = []
    li, ri = 0, 0
    while li != len(lhs) or ri != len(rhs):
        lhs_y = 1 << 30 if li == len(lhs) else lhs[li][0]
        rhs_y = 1 << 30 if ri == len(rhs) else rhs[ri][0]
        if lhs_y < rhs_y:
            merged.append(lhs[li])
            li += 1
        elif rhs_y < lhs_y:
            merged.append(rhs[ri])
            ri += 1
        else:
            interval_offsets = []
            while True:
                left_cond = li != len(lhs) and lhs[li][0] == lhs_y
                right_cond = ri != len(rhs) and rhs[ri][0] == rhs_y
                if not (left_cond or right_cond):
                    break
                lhs_x = lhs[li][1] if left_cond else INT_MAX
                rhs_x = rhs[ri][1] if right_cond else INT_MAX
                if lhs_x < rhs_x:
                    interval_offsets += [lhs[li][1], lhs[li][2]]
                    li += 1
                else:
                    interval_offsets += [rhs[ri][1], rhs[ri][2]]
                    ri += 1
            k, l, sz_k = 0, 0, len(interval_offsets)
            while k < sz_k:
                if k + 2 == sz_k:
                    merged.append((lhs_y, interval_offsets[l], interval_offsets[k + 1]))
                    break
                elif interval_offsets[k + 2] - 1 == interval_offsets[k + 1]:
                    k += 2
                else:
                    merged.append((lhs_y, interval_offsets[l], interval_offsets[k + 1]))
                    k += 2
                    l = k
    return merged


def merge_rasterizations(rasters):
    if not rasters:
        return []
    prev = list(rasters[0])
    for i in range(1, len(rasters)):
        prev = merge_rasterization(rasters[i], prev)
    return prev


def rasterization_area(raster):
    area = 0
    for _, left_x, right_x in raster:
        area += right_x - left_x + 1
    return area


def shape_moments(raster):
    """(size, mean_x, mean_y, moment_xx, moment_xy, moment_yy) as np.float32."""
    mean_x = mean_y = moment_xx = moment_yy = moment_xy = area_sum = F(0)
    for y, left_x, right_x in raster:
        m = F(left_x)
        n = F(right_x)
        curr_y = F(y)
        length = n - m + F(1)
        area_sum = area_sum + length
        center_x = F(np.float64(n + m) * np.float64(0.5))
        sum_x = center_x * length
        sum_y = curr_y * length
        mean_x = mean_x + sum_x
        mean_y = mean_y + sum_y
        moment_xy = moment_xy + curr_y * sum_x
        moment_yy = moment_yy + curr_y * sum_y
        poly = -m + F(2) * m * m + n + F(2) * m * n + F(2) * n * n
        moment_xx = moment_xx + length * poly / F(6)
    for v in (length, center_x, poly, area_sum, moment_xx):
        assert type(v) is np.float32
    inv_area = F(1) / area_sum
    return (area_sum, mean_x * inv_area, mean_y * inv_area, moment_xx * inv_area, moment_xy * inv_area,
            moment_yy * inv_area)


def pack(per_region):
    """[(id, raster)] -> (regions, intervals), regions by ascending id, empty ones left out."""
    per_region = sorted((p for p in per_region if p[1]), key=lambda p: p[0])
    regions = np.zeros(len(per_region), REGION_DTYPE)
    rows = []
    for k, (rid, raster) in enumerate(per_region):
        r = regions[k]
        r["id"], r["first_interval"], r["num_intervals"] = rid, len(rows), len(raster)
        r["area"] = rasterization_area(raster)
        r["min_x"] = min(s[1] for s in raster)
        r["max_x"] = max(s[2] for s in raster)
        r["min_y"] = min(s[0] for s in raster)
        r["max_y"] = max(s[0] for s in raster)
        for name, v in zip(FLOAT_FIELDS, shape_moments(raster)):
            r[name] = v
        rows += [(y, lx, rx, rid) for y, lx, rx in raster]
    return regions, np.asarray(rows, np.int32).reshape(-1, 4)


def literal(msg, level, hierarchy, child_order=None):
    """child_order: a function that reorders the list of a parent's children (the parent map's vectors
    are in the desc's order; a permutation shows what does not depend on it)."""
    per_region = []
    for parent_id, children in get_parent_map(msg, level, hierarchy).items():
        if child_order is not None:
            children = child_order(children)
        per_region.append((parent_id, merge_rasterizations([raster_of(c) for c in children])))
    return pack(per_region)


# ---- runs ---------------------------------------------------------------------------------------------

def runs_of(ids):
    """The maximal runs of an H x W id image, -1 belonging to none: (y, left_x, right_x, id) arrays in
    row-major order."""
    ids = np.asarray(ids, np.int32)
    H, W = ids.shape
    pad = np.full((H, 1), -1, np.int64)
    wide = np.concatenate([pad, ids.astype(np.int64), pad], axis=1)
    # a border column of -1 differs from every id, so a run ends with its row
    start = (wide[:, 1:-1] != -1) & (wide[:, 1:-1] != wide[:, :-2])
    end = (wide[:, 1:-1] != -1) & (wide[:, 1:-1] != wide[:, 2:])
    ys, lx = np.nonzero(start)
    ye, rx = np.nonzero(end)
    assert np.array_equal(ys, ye) and (lx <= rx).all()
    return ys, lx, rx, ids[ys, lx]


def runs(ids):
    ys, lx, rx, rid = runs_of(ids)
    W = np.asarray(ids).shape[1]
    order = np.argsort((rid.astype(np.int64) << 32) | (ys.astype(np.int64) * W + lx), kind="stable")
    ys, lx, rx, rid = ys[order], lx[order], rx[order], rid[order]
    intervals = np.stack([ys, lx, rx, rid], axis=1).astype(np.int32).reshape(-1, 4)
    n = len(rid)
    heads = np.nonzero(np.concatenate([[True], rid[1:] != rid[:-1]]))[0] if n else np.zeros(0, np.int64)
    ends = np.concatenate([heads[1:], [n]]).astype(np.int64)
    # the per-interval terms for all intervals at once: elementwise float32, as the scalar statements
    m, nn, cy = lx.astype(F), rx.astype(F), ys.astype(F)
    length = nn - m + F(1)
    center_x = ((nn + m).astype(np.float64) * 0.5).astype(F)
    sum_x = center_x * length
    sum_y = cy * length
    t_xy = cy * sum_x
    t_yy = cy * sum_y
    poly = -m + F(2) * m * m + nn + F(2) * m * nn + F(2) * nn * nn
    t_xx = length * poly / F(6)
    for v in (length, sum_x, t_xx):
        assert v.dtype == np.float32
    regions = np.zeros(len(heads), REGION_DTYPE)
    for k, (a, b) in enumerate(zip(heads, ends)):
        r = regions[k]
        r["id"], r["first_interval"], r["num_intervals"] = rid[a], a, b - a
        r["area"] = int((rx[a:b] - lx[a:b] + 1).sum())
        r["min_x"], r["max_x"] = lx[a:b].min(), rx[a:b].max()
        r["min_y"], r["max_y"] = ys[a:b].min(), ys[a:b].max()
        # ufunc.accumulate adds one element after the other, in order (a reduce would sum pairwise)
        acc = [np.add.accumulate(t[a:b], dtype=F)[-1] for t in (length, sum_x, sum_y, t_xx, t_xy, t_yy)]
        inv_area = F(1) / acc[0]
        r["size"] = acc[0]
        for name, v in zip(FLOAT_FIELDS[1:], acc[1:]):
            r[name] = v * inv_area
    return regions, intervals


def same_bits(a, b):
    """Regions or intervals compared as raw bytes (floats as their uint32 patterns)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def reversed_moments(regions, intervals):
    """The float fields of every region with its intervals summed in reverse order."""
    out = regions.copy()
    for r in out:
        a, n = int(r["first_interval"]), int(r["num_intervals"])
        raster = [(int(y), int(lx), int(rx)) for y, lx, rx, _ in intervals[a:a + n][::-1]]
        for name, v in zip(FLOAT_FIELDS, shape_moments(raster)):
            r[name] = v
    return out
