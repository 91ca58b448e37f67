"""Plain Python model of vsg_render_level_mesh_simplified (not collected by pytest; the simplification tests
compare the product against it byte for byte).  simplified() is straight from the definition in
include/vsg_render.h: the mesh of level_mesh_model, every segment expanded to its full lattice point list, the
collapse rule, then boundary_oracle.approx_poly_dp (imported, not copied).

dp_levels() is a second Douglas-Peucker written the way the device stages run it: the closed curve's sweeps,
then rounds in which every open slice between two neighbouring kept points looks for its farthest point and
keeps it when it fails the test, then the joint pass.  It returns what the recursion does not show from outside:
its depth, the sweeps' start, ties, the points the joint pass dropped.  That both give the same list, on corner
lists and on lattice lists alike, is a finding of the tests."""
import numpy as np

import boundary_oracle as bo
import level_mesh_model as mm

COUNTS = ("segments", "collapsed_segments", "vertices_in", "vertices_kept", "vertices_out", "single_vertex_closed",
          "longest_segment_vertices_in", "max_rounds")


def lattice(corners, closed):
    """Every lattice point a segment passes, from its corner list: length + 1 points when open, length when
    closed (the first is not repeated)."""
    corners = [tuple(int(v) for v in p) for p in corners]
    out = []
    n = len(corners)
    for k in range(n if closed else n - 1):
        (ax, ay), (bx, by) = corners[k], corners[(k + 1) % n]
        assert (ax == bx) != (ay == by)
        steps = abs(bx - ax) + abs(by - ay)
        sx, sy = (bx > ax) - (bx < ax), (by > ay) - (by < ay)
        out += [(ax + sx * i, ay + sy * i) for i in range(steps)]
    if not closed:
        out.append(corners[-1])
    return out


def threshold(min_segment_points):
    return max(3, int(min_segment_points)) if min_segment_points > 0 else 0


def dp_levels(src, max_error, closed):
    """(list, info) of src (tuples of ints) the way the device runs it.  info: depth (rounds that kept a point),
    start (index of the point the kept list of a closed curve begins at), ties (arg-max decisions in which a
    later point had the same distance), kept (points after the recursion), dropped (points the joint pass
    dropped), wrap_read_written (a closed list's wrapped read saw a value the pass had changed), coincide (the
    start_pt == end_pt branch)."""
    src = [tuple(p) for p in src]
    count = len(src)
    eps = float(max_error) * float(max_error)
    info = {"depth": 0, "start": 0, "ties": 0, "kept": 0, "dropped": [], "wrap_read_written": False,
            "coincide": False}
    if count == 0:
        return [], info

    def at(i):
        return src[i % count]

    pts = np.asarray(src, np.float64).reshape(-1, 2)
    ring = closed
    sweeps = 3
    if not closed and src[0] == src[-1]:
        ring, sweeps = True, 1
        info["coincide"] = True
    base, last = 0, count - 1                    # virtual index v is point (base + v) % count, v in [0, last]
    kept = None
    if ring:
        start, arg, best = 0, 0, 0.0
        for k in range(sweeps):
            # every distance of a sweep or a slice at once: the values are integers below 2^32, exact in float64
            d = pts[(start + np.arange(1, count)) % count] - pts[start]
            dist = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]
            best = float(dist.max()) if count > 1 else 0.0
            if best > 0:
                arg = 1 + int(np.argmax(dist))                 # the first of equals
                info["ties"] += int((dist == best).sum()) - 1
            if k + 1 < sweeps:
                start = (start + arg) % count
        base, last = start, count
        info["start"] = start
        if best <= eps:
            out = [at(base)] + ([] if closed else [src[0]])
        else:
            kept = {0, arg, last}
    else:
        kept = {0, last}
    if kept is not None:
        active = sorted(kept)
        active = list(zip(active[:-1], active[1:]))
        for _ in range(count + 1):               # bounded as the kernel is
            nxt = []
            for a, b in active:
                if b <= a + 1:
                    continue
                sp, ep = at(base + a), at(base + b)
                dx, dy = float(ep[0] - sp[0]), float(ep[1] - sp[1])
                d = pts[(base + np.arange(a + 1, b)) % count] - pts[(base + a) % count]
                dist = np.abs(d[:, 1] * dx - d[:, 0] * dy)
                best = float(dist.max())
                arg = a + 1 + int(np.argmax(dist))
                tie = best > 0 and int((dist == best).sum()) > 1
                if not best * best <= eps * (dx * dx + dy * dy):
                    info["ties"] += tie
                    kept.add(arg)
                    nxt += [(a, arg), (arg, b)]
            if not nxt:
                break
            info["depth"] += 1
            active = nxt
        else:
            raise AssertionError("the rounds did not end")
        out = [at(base + v) for v in sorted(kept) if v < last or not closed]
    info["kept"] = len(out)

    # the joint pass, in place as the host runs it
    d = list(out)
    cnt = len(d)
    new_count = cnt
    written = {}
    state = {"rd": cnt - 1 if closed else 0, "wrapped": False}

    def read():
        r = state["rd"]
        if state["wrapped"] and r in written and written[r] != out[r]:
            info["wrap_read_written"] = True
        v = d[r]
        r += 1
        if r >= cnt:
            r = 0
            state["wrapped"] = closed and True
        state["rd"] = r
        return v

    sp = read()
    state["wrapped"] = False                      # the first wrap of a closed list is its start, not a wrap-around
    wr = state["rd"]
    pt = read()
    i = 0 if closed else 1
    end = cnt if closed else cnt - 1
    while i < end and new_count > 2:
        ep = read()
        dx, dy = float(ep[0] - sp[0]), float(ep[1] - sp[1])
        dist = abs((pt[0] - sp[0]) * dy - (pt[1] - sp[1]) * dx)
        sip = float(pt[0] - sp[0]) * (ep[0] - pt[0]) + float(pt[1] - sp[1]) * (ep[1] - pt[1])
        if dist * dist <= 0.5 * eps * (dx * dx + dy * dy) and dx != 0 and dy != 0 and sip >= 0:
            new_count -= 1
            info["dropped"].append(pt)
            d[wr] = sp = ep
            written[wr] = ep
            wr = (wr + 1) % cnt
            pt = read()
            i += 2
            continue
        d[wr] = sp = pt
        written[wr] = pt
        wr = (wr + 1) % cnt
        pt = ep
        i += 1
    if not closed:
        d[wr] = pt
    return d[:new_count], info


def simplify_segment(corners, length, closed, max_error, min_segment_points, lattice_lists=True):
    """The new vertex list of one segment: the definition."""
    corners = tuple(tuple(int(v) for v in p) for p in corners)
    if not closed and length + 1 < threshold(min_segment_points):
        return [corners[0], corners[-1]]
    key = (corners, bool(closed), float(max_error), bool(lattice_lists))
    if key not in _MEMO:                          # the modes and levels of a case share most of their segments
        q = lattice(corners, closed) if lattice_lists else list(corners)
        assert len(q) == (length if closed else length + 1) or not lattice_lists
        _MEMO[key] = bo.approx_poly_dp(q, float(max_error), bool(closed))
    return list(_MEMO[key])


_MEMO = {}
_LEVELS = {}


def rebuild(result, lists):
    """The four lists with the segments' vertex lists replaced by `lists`."""
    segments, _, loops, refs = result
    segments = segments.copy()
    points = []
    for rec, pts in zip(segments, lists):
        rec["first_vertex"], rec["num_vertices"] = len(points), len(pts)
        points += pts
    return segments, np.asarray(points, np.int32).reshape(-1, 2), loops, refs


def corner_lists(result):
    segments, vertices = result[0], result[1]
    return [[tuple(p) for p in vertices[int(s["first_vertex"]):int(s["first_vertex"]) + int(s["num_vertices"])].tolist()]
            for s in segments]


def simplified(plane, components=None, max_error=1.0, min_segment_points=4, result=None, lattice_lists=True):
    """(segments, vertices, loops, refs) of vsg_render_level_mesh_simplified.  result: level_mesh_model.mesh of
    the same plane, where the caller has it."""
    result = result if result is not None else mm.mesh(plane, components)
    lists = [simplify_segment(c, int(s["length"]), bool(s["closed"]), max_error, min_segment_points, lattice_lists)
             for s, c in zip(result[0], corner_lists(result))]
    return rebuild(result, lists)


def stats_of(result, max_error, min_segment_points):
    """The counts of vsg_render_simplify_stats, from the level-by-level model on the corner lists."""
    out = dict.fromkeys(COUNTS, 0)
    t = threshold(min_segment_points)
    for s, c in zip(result[0], corner_lists(result)):
        out["segments"] += 1
        out["vertices_in"] += len(c)
        out["longest_segment_vertices_in"] = max(out["longest_segment_vertices_in"], len(c))
        if not s["closed"] and int(s["length"]) + 1 < t:
            out["collapsed_segments"] += 1
            out["vertices_kept"] += 2
            out["vertices_out"] += 2
            continue
        key = (tuple(c), bool(s["closed"]), float(max_error))
        if key not in _LEVELS:
            pts, info = dp_levels(c, max_error, bool(s["closed"]))
            _LEVELS[key] = (info["kept"], len(pts), info["depth"])
        kept, left, depth = _LEVELS[key]
        out["vertices_kept"] += kept
        out["vertices_out"] += left
        out["max_rounds"] = max(out["max_rounds"], depth)
        out["single_vertex_closed"] += bool(s["closed"]) and left == 1
    return out


def same_bits(a, b):
    return mm.same_bits(a, b)
