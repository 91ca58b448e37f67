"""Plain Python model of the traced contours of a hierarchy level (not collected by pytest; the level contour
tests compare the product against it byte for byte).  A literal tracer straight from the definition in
include/vsg_render.h: the set of cracks, the successor of each by trying the three candidates in the stated
order, then a walk along every cycle.

P is a plane of W x H, -1 where nothing covers a pixel; positions outside the frame count as -1.  Side s of
pixel (x, y): 0 top, 1 right, 2 bottom, 3 left; key = 4 * (y * W + x) + s; a side is a crack of g = P(x, y)
>= 0 when the pixel across it is not g.  Cracks run clockwise on screen around their pixel."""
import numpy as np

CONTOUR_DTYPE = np.dtype([
    ("id", np.int32), ("component", np.int32), ("group", np.int32),
    ("first_vertex", np.int32), ("num_vertices", np.int32), ("length", np.int32),
    ("min_x", np.int32), ("min_y", np.int32), ("max_x", np.int32), ("max_y", np.int32),
    ("area2", np.int64),
])

STEP = ((1, 0), (0, 1), (-1, 0), (0, -1))              # direction of travel along side s
START = ((0, 0), (1, 0), (1, 1), (0, 1))               # the corner side s starts at, relative to (x, y)
ACROSS = ((0, -1), (1, 0), (0, 1), (-1, 0))            # the pixel across side s


def cracks_of(plane):
    """The keys of all cracks, as a set."""
    plane = np.asarray(plane, np.int32)
    H, W = plane.shape
    R = np.full((H + 2, W + 2), -1, np.int64)
    R[1:-1, 1:-1] = plane
    c = R[1:-1, 1:-1]
    out = set()
    for s, (dx, dy) in enumerate(ACROSS):
        nb = R[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]
        y, x = np.nonzero((c >= 0) & (nb != c))
        out.update((4 * (y.astype(np.int64) * W + x) + s).tolist())
    return out


def trace(plane):
    """[(group, [keys of the cycle, from its smallest-key turn crack on], [vertices (x, y)])] in (group, first
    key) order."""
    plane = np.asarray(plane, np.int32)
    H, W = plane.shape
    cracks = cracks_of(plane)

    def value(x, y):
        return int(plane[y, x]) if 0 <= x < W and 0 <= y < H else -1

    def successor(key):
        p, s = divmod(key, 4)
        y, x = divmod(p, W)
        g = value(x, y)
        dx, dy = STEP[s]
        lx, ly = STEP[(s + 3) % 4]
        # right turn, straight on, left turn: the first that is a crack of g
        for qx, qy, qs in ((x, y, (s + 1) % 4), (x + dx, y + dy, s), (x + dx + lx, y + dy + ly, (s + 3) % 4)):
            if value(qx, qy) == g and 4 * (qy * W + qx) + qs in cracks:
                # it starts where this one ends
                assert (qx + START[qs][0], qy + START[qs][1]) == (x + START[s][0] + dx, y + START[s][1] + dy)
                return 4 * (qy * W + qx) + qs
        raise AssertionError("a crack without a successor")

    succ = {k: successor(k) for k in cracks}
    pred = {v: k for k, v in succ.items()}
    assert len(pred) == len(succ)                      # a permutation
    seen = set()
    out = []
    for k0 in sorted(cracks):
        if k0 in seen:
            continue
        cycle = [k0]
        seen.add(k0)
        k = succ[k0]
        while k != k0:
            cycle.append(k)
            seen.add(k)
            k = succ[k]
        turns = [k for k in cycle if pred[k] % 4 != k % 4]
        start = cycle.index(min(turns))
        cycle = cycle[start:] + cycle[:start]
        vertices = []
        for k in cycle:
            if pred[k] % 4 != k % 4:
                p, s = divmod(k, 4)
                y, x = divmod(p, W)
                vertices.append((x + START[s][0], y + START[s][1]))
        p = cycle[0] // 4
        out.append((value(p % W, p // W), cycle, vertices))
    out.sort(key=lambda c: (c[0], c[1][0]))
    return out


def contours(plane, components=None):
    """(records, vertices): a CONTOUR_DTYPE array and (n, 2) int32 {x, y}.  id = group value, component = -1
    and group = the rank of the value among the plane's, or, with the component list of level_components_model
    the plane is the label image of, that component's id and component and group = the value."""
    traced = trace(plane)
    values = sorted({g for g, _, _ in traced})
    rank = {g: k for k, g in enumerate(values)}
    records = np.zeros(len(traced), CONTOUR_DTYPE)
    points = []
    for r, (g, cycle, vertices) in zip(records, traced):
        if components is None:
            r["id"], r["component"], r["group"] = g, -1, rank[g]
        else:
            r["id"], r["component"], r["group"] = components["id"][g], components["component"][g], g
        r["first_vertex"], r["num_vertices"], r["length"] = len(points), len(vertices), len(cycle)
        xs, ys = [v[0] for v in vertices], [v[1] for v in vertices]
        r["min_x"], r["min_y"], r["max_x"], r["max_y"] = min(xs), min(ys), max(xs), max(ys)
        r["area2"] = sum(xs[i] * ys[(i + 1) % len(xs)] - xs[(i + 1) % len(xs)] * ys[i] for i in range(len(xs)))
        points += vertices
    return records, np.asarray(points, np.int32).reshape(-1, 2)


def stats_of(plane):
    """The counts of vsg_render_contour_stats."""
    records, vertices = contours(plane)
    return {"cracks": len(cracks_of(plane)), "vertices": len(vertices), "contours": len(records),
            "holes": int((records["area2"] < 0).sum()),
            "largest_contour_cracks": int(records["length"].max()) if len(records) else 0}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
