"""Plain numpy / Python model of the connected components of a hierarchy level's regions (not collected
by pytest; the level component tests compare the product against it bit for bit).  Three definitions:

  literal   the reference's ConnectedComponents (segment_util/segmentation_util.cpp:1025-1101) restated
            loop for loop -- test_idx, last_change_idx, a disjoint-set forest, the first-appearance
            compile loop -- with ScanIntervalsNeighbored (:1009-1022), applied to the rasterization of
            every region that level_regions_model.literal returns
  sweep     a two-pointer sweep over adjacent rows of every region's runs, O(runs), from an id image
  pixels    a flood fill of the id image per id over 4- or 8-neighbourhoods; knows nothing of runs

All three return (components, intervals, labels): a COMPONENT_DTYPE array ordered by (id, component), an
(n, 4) int32 array {y, left_x, right_x, id} grouped by component in that order, and the H x W int32
image of every pixel's index in the component list (-1: none): the layout of
vsg_render_level_components.  Area, bounding box and moments of a component are those of
level_regions_model on its interval list (rasterization_area and shape_moments for literal and pixels, the
runs definition for sweep): they are not restated here.

literal takes the (regions, intervals) of level_regions_model.literal and the frame size; sweep and
pixels take an id image."""
import numpy as np

import level_regions_model as lm

N4 = 1
N8 = 2

COMPONENT_DTYPE = np.dtype([
    ("id", np.int32), ("component", np.int32), ("region_components", np.int32),
    ("first_interval", np.int32), ("num_intervals", np.int32), ("area", np.int32),
    ("min_x", np.int32), ("min_y", np.int32), ("max_x", np.int32), ("max_y", np.int32),
    ("size", np.float32), ("mean_x", np.float32), ("mean_y", np.float32),
    ("moment_xx", np.float32), ("moment_xy", np.float32), ("moment_yy", np.float32),
])


def scan_intervals_neighbored(lhs, rhs, connect):
    """lhs, rhs: (y, left_x, right_x)."""
    if connect == N8:
        return abs(lhs[0] - rhs[0]) <= 1 and max(lhs[1], rhs[1]) - min(lhs[2], rhs[2]) <= 1
    assert connect == N4
    return abs(lhs[0] - rhs[0]) <= 1 and max(lhs[1], rhs[1]) <= min(lhs[2], rhs[2])


class DisjointSets:
    """boost::disjoint_sets: union by rank, find with path compression."""

    def __init__(self):
        self.parent, self.rank = {}, {}

    def make_set(self, x):
        self.parent[x], self.rank[x] = x, 0

    def find_set(self, x):
        root = x
        while self.parent[root] != root:
            root = self.parent[root]
        while self.parent[x] != root:
            self.parent[x], x = root, self.parent[x]
        return root

    def union_set(self, a, b):
        a, b = self.find_set(a), self.find_set(b)
        if a == b:
            return
        if self.rank[a] > self.rank[b]:
            self.parent[b] = a
        else:
            self.parent[a] = b
            if self.rank[a] == self.rank[b]:
                self.rank[b] += 1


def connected_components(raster, connect):
    """ConnectedComponents: raster [(y, left_x, right_x)] -> (list of component rasters, unions made).
    The second number counts the pairs ScanIntervalsNeighbored accepted."""
    size = len(raster)
    classes = DisjointSets()
    last_change_idx = -1
    last_y = -2
    test_idx = 0
    pairs = 0
    for i in range(size):
        classes.make_set(i)
        curr_scan = raster[i]
        if curr_scan[0] != last_y:
            if last_y + 1 == curr_scan[0]:
                test_idx = last_change_idx
            else:
                test_idx = i
            last_y = curr_scan[0]
            last_change_idx = i
        for k in range(test_idx, i):
            if scan_intervals_neighbored(curr_scan, raster[k], connect):
                classes.union_set(i, k)
                pairs += 1
    # the early return for one component pushes the raster itself: the same list
    components, rep_to_component = [], {}
    for i in range(size):
        rep = classes.find_set(i)
        if rep not in rep_to_component:
            components.append([raster[i]])
            rep_to_component[rep] = components[-1]
        else:
            rep_to_component[rep].append(raster[i])
    return components, pairs


def pack(per_component, W, H):
    """[(id, component, region_components, raster)] in output order -> (components, intervals, labels)."""
    comps = np.zeros(len(per_component), COMPONENT_DTYPE)
    labels = np.full((H, W), -1, np.int32)
    rows = []
    for k, (rid, idx, count, raster) in enumerate(per_component):
        c = comps[k]
        c["id"], c["component"], c["region_components"] = rid, idx, count
        c["first_interval"], c["num_intervals"] = len(rows), len(raster)
        c["area"] = lm.rasterization_area(raster)
        c["min_x"] = min(s[1] for s in raster)
        c["max_x"] = max(s[2] for s in raster)
        c["min_y"] = min(s[0] for s in raster)
        c["max_y"] = max(s[0] for s in raster)
        for name, v in zip(lm.FLOAT_FIELDS, lm.shape_moments(raster)):
            c[name] = v
        for y, lx, rx in raster:
            rows.append((y, lx, rx, rid))
            labels[y, lx:rx + 1] = k
    return comps, np.asarray(rows, np.int32).reshape(-1, 4), labels


def literal(regions, intervals, W, H, connect, stats=None):
    """regions, intervals: what level_regions_model.literal (or .runs) returns.  stats: a dict that
    receives "runs" and "links"."""
    per_component, links = [], 0
    for r in regions:
        a, n = int(r["first_interval"]), int(r["num_intervals"])
        raster = [(int(y), int(lx), int(rx)) for y, lx, rx, _ in intervals[a:a + n]]
        comps, pairs = connected_components(raster, connect)
        links += pairs
        for idx, comp in enumerate(comps):
            per_component.append((int(r["id"]), idx, len(comps), comp))
    if stats is not None:
        stats["runs"], stats["links"] = len(intervals), links
    return pack(per_component, W, H)


def sweep(ids, connect, stats=None):
    """The runs of every id, row by row: two pointers walk the runs of rows y - 1 and y of one id;
    every neighbouring pair is united (smaller index wins), and the pointer whose run ends first moves
    on.  Fast enough for a 1080p frame."""
    ids = np.asarray(ids, np.int32)
    H, W = ids.shape
    slack = 1 if connect == N8 else 0
    ys, lx, rx, rid = lm.runs_of(ids)
    order = np.argsort((rid.astype(np.int64) << 32) | (ys.astype(np.int64) * W + lx), kind="stable")
    ys, lx, rx, rid = ys[order].tolist(), lx[order].tolist(), rx[order].tolist(), rid[order].tolist()
    n = len(rid)
    parent = list(range(n))

    def find(x):
        root = x
        while parent[root] != root:
            root = parent[root]
        while parent[x] != root:
            parent[x], x = root, parent[x]
        return root

    links = 0
    prev_a = prev_b = 0          # the previous group [prev_a, prev_b) of the same id, if it is row y - 1
    a = 0
    while a < n:
        b = a
        while b < n and rid[b] == rid[a] and ys[b] == ys[a]:
            b += 1
        if prev_b == a and prev_b > prev_a and rid[prev_a] == rid[a] and ys[prev_a] + 1 == ys[a]:
            i, j = prev_a, a
            while i < prev_b and j < b:
                if max(lx[i], lx[j]) - min(rx[i], rx[j]) <= slack:
                    links += 1
                    ri, rj = find(i), find(j)
                    if ri != rj:
                        parent[max(ri, rj)] = min(ri, rj)
                if rx[i] < rx[j]:
                    i += 1
                else:
                    j += 1
        prev_a, prev_b = a, b
        a = b
    if stats is not None:
        stats["runs"], stats["links"] = n, links
    roots = [find(k) for k in range(n)]
    # the root is the smallest index of its set: sorting by it keeps regions together, orders a region's
    # components by their first interval and, being stable, a component's intervals by list order
    by_root = sorted(range(n), key=lambda k: roots[k])
    per_component = []
    for k in by_root:
        if k == roots[k]:
            per_component.append([rid[k], 0, 0])
    first_of = {}
    for k, c in enumerate(per_component):
        first_of.setdefault(c[0], k)
    count_of = {}
    for c in per_component:
        count_of[c[0]] = count_of.get(c[0], 0) + 1
    for k, c in enumerate(per_component):
        c[1], c[2] = k - first_of[c[0]], count_of[c[0]]
    # The rest through the runs model on the image of component indices: a component's runs are the
    # maximal runs of its index (runs of one id never touch within a row), ascending index is the
    # component order and (y, left_x) the order within a component.
    labels = np.full((H, W), -1, np.int32)
    k = -1
    for i in by_root:
        if i == roots[i]:
            k += 1
        labels[ys[i], lx[i]:rx[i] + 1] = k
    regions, rows = lm.runs(labels)
    assert len(regions) == len(per_component)
    comps = np.zeros(len(regions), COMPONENT_DTYPE)
    for name in lm.REGION_DTYPE.names[1:]:
        comps[name] = regions[name]
    comps["id"] = [c[0] for c in per_component]
    comps["component"] = [c[1] for c in per_component]
    comps["region_components"] = [c[2] for c in per_component]
    rows = rows.copy()
    rows[:, 3] = comps["id"][rows[:, 3]] if len(rows) else rows[:, 3]
    return comps, rows, labels


def pixels(ids, connect):
    """Flood fill.  Components of one id are found in row-major order of their first pixel; ids are then
    taken in ascending order.  A component's intervals are the maximal runs of its pixels per row."""
    ids = np.asarray(ids, np.int32)
    H, W = ids.shape
    steps = [(-1, 0), (1, 0), (0, -1), (0, 1)]
    if connect == N8:
        steps += [(-1, -1), (-1, 1), (1, -1), (1, 1)]
    mark = np.full((H, W), -1, np.int64)
    found = []     # (id, pixels of the component)
    for y0 in range(H):
        for x0 in range(W):
            if ids[y0, x0] == -1 or mark[y0, x0] != -1:
                continue
            k, rid = len(found), int(ids[y0, x0])
            mark[y0, x0] = k
            stack, members = [(y0, x0)], []
            while stack:
                y, x = stack.pop()
                members.append((y, x))
                for dy, dx in steps:
                    v, u = y + dy, x + dx
                    if 0 <= v < H and 0 <= u < W and mark[v, u] == -1 and ids[v, u] == rid:
                        mark[v, u] = k
                        stack.append((v, u))
            found.append((rid, sorted(members)))
    # a stable sort by id keeps the row-major order of first pixels within an id
    found.sort(key=lambda f: f[0])
    per_component = []
    counts = {}
    for rid, _ in found:
        counts[rid] = counts.get(rid, 0) + 1
    seen = {}
    for rid, members in found:
        raster = []
        for y, x in members:
            if raster and raster[-1][0] == y and raster[-1][2] + 1 == x:
                raster[-1] = (y, raster[-1][1], x)
            else:
                raster.append((y, x, x))
        idx = seen.get(rid, 0)
        seen[rid] = idx + 1
        per_component.append((rid, idx, counts[rid], raster))
    return pack(per_component, W, H)


def same(a, b):
    """Two (components, intervals, labels) results compared as raw bytes."""
    return all(lm.same_bits(x, y) for x, y in zip(a, b)) and len(a) == len(b) == 3
