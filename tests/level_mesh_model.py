"""Plain Python model of the shared-segment mesh of a hierarchy level (not collected by pytest; the level mesh
tests compare the product against it byte for byte).  Straight from the definition in include/vsg_render.h,
and not by cutting the cycles of level_contours_model: it computes sides() at every corner, takes every
undirected pixel side between two different values once (as the crack of its owner, the side's larger value),
and walks these from junction to junction; what no junction reaches is a closed segment.  The loops are then
chained from the segments' two directions by the successor rule.  That every loop so rebuilt equals a contour
of level_contours_model is a finding of the tests, not a construction.

P is a plane of W x H, -1 where nothing covers a pixel; positions outside the frame count as -1.  Sides,
keys, directions and corners are those of level_contours_model."""
import numpy as np

SEGMENT_DTYPE = np.dtype([
    ("right", np.int32), ("left", np.int32), ("first_vertex", np.int32), ("num_vertices", np.int32),
    ("length", np.int32), ("closed", np.int32), ("start_sides", np.int32), ("end_sides", np.int32),
])
LOOP_DTYPE = np.dtype([("group", np.int32), ("first_ref", np.int32), ("num_refs", np.int32), ("length", np.int32)])

STEP = ((1, 0), (0, 1), (-1, 0), (0, -1))              # direction of travel along side s
START = ((0, 0), (1, 0), (1, 1), (0, 1))               # the corner side s starts at, relative to (x, y)
ACROSS = ((0, -1), (1, 0), (0, 1), (-1, 0))            # the pixel across side s

COUNTS = ("cracks", "segments", "closed_segments", "shared_segments", "vertices", "loops", "refs", "junctions",
          "longest_segment_cracks")


class Plane:
    def __init__(self, plane):
        self.P = np.asarray(plane, np.int32)
        self.H, self.W = self.P.shape

    def value(self, x, y):
        return int(self.P[y, x]) if 0 <= x < self.W and 0 <= y < self.H else -1

    def key(self, x, y, s):
        return 4 * (y * self.W + x) + s

    def unkey(self, k):
        p, s = divmod(k, 4)
        y, x = divmod(p, self.W)
        return x, y, s

    def is_crack(self, x, y, s):
        g = self.value(x, y)
        return g >= 0 and self.value(x + ACROSS[s][0], y + ACROSS[s][1]) != g

    def other(self, k):
        x, y, s = self.unkey(k)
        return self.value(x + ACROSS[s][0], y + ACROSS[s][1])

    def start(self, k):
        x, y, s = self.unkey(k)
        return x + START[s][0], y + START[s][1]

    def end(self, k):
        x, y, s = self.unkey(k)
        return x + START[s][0] + STEP[s][0], y + START[s][1] + STEP[s][1]

    def twin(self, k):
        """The same side seen from the pixel across it."""
        x, y, s = self.unkey(k)
        return self.key(x + ACROSS[s][0], y + ACROSS[s][1], (s + 2) % 4)

    def sides(self, cx, cy):
        v = (self.value(cx - 1, cy - 1), self.value(cx, cy - 1), self.value(cx, cy), self.value(cx - 1, cy))
        return sum(v[k] != v[(k + 1) % 4] for k in range(4))

    def successor(self, k):
        """Right turn, straight on, left turn: the first that is a crack of the same group."""
        x, y, s = self.unkey(k)
        g = self.value(x, y)
        dx, dy = STEP[s]
        lx, ly = STEP[(s + 3) % 4]
        for qx, qy, qs in ((x, y, (s + 1) % 4), (x + dx, y + dy, s), (x + dx + lx, y + dy + ly, (s + 3) % 4)):
            if self.value(qx, qy) == g and self.is_crack(qx, qy, qs):
                return self.key(qx, qy, qs)
        raise AssertionError("a crack without a successor")


def sides_plane(plane):
    """sides() at every corner: (H + 1) x (W + 1)."""
    plane = np.asarray(plane, np.int32)
    H, W = plane.shape
    R = np.full((H + 2, W + 2), -1, np.int64)
    R[1:-1, 1:-1] = plane
    a, b, c, d = R[:H + 1, :W + 1], R[:H + 1, 1:], R[1:, 1:], R[1:, :W + 1]      # clockwise from the top left
    return (a != b).astype(np.int64) + (b != c) + (c != d) + (d != a)


def junction_sides(plane):
    """{corner: sides} of every junction."""
    n = sides_plane(plane)
    assert np.isin(n, (0, 2, 3, 4)).all()
    cy, cx = np.nonzero(n >= 3)
    return {(int(x), int(y)): int(n[y, x]) for x, y in zip(cx, cy)}


def owner_cracks(plane):
    """The keys of the cracks whose other side is smaller: every undirected side between two values once."""
    plane = np.asarray(plane, np.int32)
    H, W = plane.shape
    R = np.full((H + 2, W + 2), -1, np.int64)
    R[1:-1, 1:-1] = plane
    c = R[1:-1, 1:-1]
    out = []
    for s, (dx, dy) in enumerate(ACROSS):
        y, x = np.nonzero(R[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx] < c)
        out += (4 * (y.astype(np.int64) * W + x) + s).tolist()
    return sorted(out)


def chains(plane):
    """[(keys of the owner's cracks in its direction of travel, closed)]: every undirected side once."""
    pl = Plane(plane)
    junctions = junction_sides(plane)
    owner = owner_cracks(plane)
    leaving = {}                                        # non-junction corner -> the owner crack that leaves it
    for k in owner:
        c = pl.start(k)
        if c not in junctions:
            assert c not in leaving                     # two sides meet there: one arrives, one leaves
            leaving[c] = k
    seen = set()
    out = []

    def walk(k0):
        chain = [k0]
        seen.add(k0)
        while pl.end(chain[-1]) not in junctions:
            k = leaving[pl.end(chain[-1])]
            if k == k0:
                return chain, True
            assert k not in seen
            chain.append(k)
            seen.add(k)
        return chain, False

    for k in sorted(owner):
        if pl.start(k) in junctions:
            chain, closed = walk(k)
            assert not closed
            out.append((chain, False))
    for k in sorted(owner):
        if k not in seen:
            chain, closed = walk(k)
            assert closed
            turns = [i for i in range(len(chain)) if chain[i - 1] % 4 != chain[i] % 4]
            first = min(turns, key=lambda i: chain[i])
            out.append((chain[first:] + chain[:first], True))
    assert len(seen) == len(owner)
    return out


def mesh(plane, components=None):
    """(segments, vertices, loops, refs): SEGMENT_DTYPE, (n, 2) int32 {x, y}, LOOP_DTYPE, int32.  Group index
    = the rank of the value among the plane's, or, with the component list of level_components_model the plane
    is the label image of, the value."""
    pl = Plane(plane)
    values = sorted(set(int(v) for v in np.unique(pl.P) if v >= 0))
    index = {g: (k if components is None else g) for k, g in enumerate(values)}
    index[-1] = -1
    junctions = junction_sides(plane)
    found = chains(plane)
    found.sort(key=lambda c: (index[pl.value(*pl.unkey(c[0][0])[:2])], c[0][0]))
    segments = np.zeros(len(found), SEGMENT_DTYPE)
    points = []
    halves = {}                                          # first crack -> (ref, keys in travel order)
    for s, (rec, (chain, closed)) in enumerate(zip(segments, found)):
        g, o = pl.value(*pl.unkey(chain[0])[:2]), pl.other(chain[0])
        assert all(pl.other(k) == o for k in chain) and o < g
        if closed:
            vertices = [pl.start(k) for i, k in enumerate(chain) if chain[i - 1] % 4 != k % 4]
        else:
            vertices = [pl.start(chain[0])] + [pl.start(k) for i, k in enumerate(chain)
                                               if i > 0 and chain[i - 1] % 4 != k % 4] + [pl.end(chain[-1])]
        rec["right"], rec["left"] = index[g], index[o]
        rec["first_vertex"], rec["num_vertices"], rec["length"], rec["closed"] = len(points), len(vertices), len(chain), closed
        if not closed:
            rec["start_sides"], rec["end_sides"] = junctions[pl.start(chain[0])], junctions[pl.end(chain[-1])]
        points += vertices
        halves[chain[0]] = (s, chain)
        if o >= 0:
            back = [pl.twin(k) for k in reversed(chain)]
            if closed:
                # a closed half begins at its own contour's leader
                turns = [i for i in range(len(back)) if back[i - 1] % 4 != back[i] % 4]
                first = min(turns, key=lambda i: back[i])
                back = back[first:] + back[:first]
            halves[back[0]] = (~s, back)
    # the loops: halves chained by the successor rule
    seen = set()
    cycles = []
    for k0 in sorted(halves):
        if k0 in seen:
            continue
        cycle = []
        k = k0
        while k not in seen:
            seen.add(k)
            cycle.append(k)
            k = pl.successor(halves[k][1][-1])
            assert k in halves, "a half ends where no half begins"
        assert k == k0
        keys = [c for h in cycle for c in halves[h][1]]
        leader = min(c for i, c in enumerate(keys) if keys[i - 1] % 4 != c % 4)
        at = next(i for i, h in enumerate(cycle) if leader in halves[h][1])
        cycle = cycle[at:] + cycle[:at]
        g = pl.value(*pl.unkey(leader)[:2])
        cycles.append((index[g], leader, cycle, len(keys)))
    cycles.sort(key=lambda c: c[:2])
    loops = np.zeros(len(cycles), LOOP_DTYPE)
    refs = []
    for rec, (g, _, cycle, length) in zip(loops, cycles):
        rec["group"], rec["first_ref"], rec["num_refs"], rec["length"] = g, len(refs), len(cycle), length
        refs += [halves[h][0] for h in cycle]
    return segments, np.asarray(points, np.int32).reshape(-1, 2), loops, np.asarray(refs, np.int32)


def stats_of(plane, result=None):
    """The counts of vsg_render_mesh_stats."""
    segments, vertices, loops, refs = result if result is not None else mesh(plane)
    P = np.pad(np.asarray(plane, np.int64), 1, constant_values=-1)
    c = P[1:-1, 1:-1]
    cracks = sum(int(((c >= 0) & (P[1 + dy:P.shape[0] - 1 + dy, 1 + dx:P.shape[1] - 1 + dx] != c)).sum())
                 for dx, dy in ACROSS)
    return {"cracks": cracks, "segments": len(segments), "closed_segments": int(segments["closed"].sum()),
            "shared_segments": int((segments["left"] >= 0).sum()), "vertices": len(vertices), "loops": len(loops),
            "refs": len(refs), "junctions": len(junction_sides(plane)),
            "longest_segment_cracks": int(segments["length"].max()) if len(segments) else 0}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
