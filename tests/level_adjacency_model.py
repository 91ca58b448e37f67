"""Plain numpy / Python model of the region adjacency graph of a hierarchy level (not collected by pytest;
the level adjacency tests compare the product against it byte for byte).  Two definitions:

  adjacency_literal  a loop over the pixels, their four sides and, with N8, the two diagonal pairs of every
                     2 x 2 block, that walks the definition word for word; for small planes
  adjacency          the same counts from shifted comparisons of the whole plane

The definition.  P is a plane of W x H, -1 where nothing covers a pixel; positions outside the frame are
not pixels.  A group g >= 0 is a value of P.  Every pixel of g has four sides; what lies across a side
classifies it: outside the frame -> border_frame of g; an in-frame pixel with -1 -> border_uncovered of g;
a pixel of another group b -> border_shared of g and shared_n4 of the edge g -> b; a pixel of g -> nothing.
With N8, every pair of in-frame positions {(x, y), (x+1, y+1)} or {(x+1, y), (x, y+1)} with different
non-negative values a, b adds 1 to shared_diagonal of a -> b and of b -> a.  An edge exists when
shared_n4 + shared_diagonal > 0.  One node per group by ascending group; edges grouped by node, within a
node by ascending neighbour."""
import numpy as np

NODE_DTYPE = np.dtype([("id", np.int32), ("component", np.int32), ("first_edge", np.int32),
                       ("num_edges", np.int32), ("border_frame", np.int32), ("border_uncovered", np.int32),
                       ("border_shared", np.int32)])
EDGE_DTYPE = np.dtype([("neighbour", np.int32), ("neighbour_id", np.int32), ("shared_n4", np.int32),
                       ("shared_diagonal", np.int32)])

ADJACENT_N4 = 1
ADJACENT_N8 = 2

SIDES = ((0, -1), (-1, 0), (1, 0), (0, 1))          # (dx, dy)
DIAGONALS = ((-1, -1), (1, -1), (-1, 1), (1, 1))


def _assemble(groups, frame, uncovered, pairs, components):
    """groups: ascending group values.  frame, uncovered: {group: sides}.  pairs: {(g, b): [n4, diagonal]}.
    Node k is group groups[k]; with `components` the groups are 0 .. len - 1 and index that list."""
    index = {int(g): k for k, g in enumerate(groups)}
    nodes = np.zeros(len(groups), NODE_DTYPE)
    keys = sorted(pairs)                            # by (group, other): by node, then by neighbour
    edges = np.zeros(len(keys), EDGE_DTYPE)
    for k, g in enumerate(groups):
        g = int(g)
        nodes[k]["id"] = g if components is None else components["id"][g]
        nodes[k]["component"] = -1 if components is None else components["component"][g]
        nodes[k]["border_frame"] = frame.get(g, 0)
        nodes[k]["border_uncovered"] = uncovered.get(g, 0)
    for e, (g, b) in enumerate(keys):
        n4, diag = pairs[g, b]
        edges[e] = (index[b], b if components is None else components["id"][b], n4, diag)
        node = nodes[index[g]]
        if node["num_edges"] == 0:
            node["first_edge"] = e
        node["num_edges"] += 1
        node["border_shared"] += n4
    # a node without edges starts where its predecessor's edges end
    end = 0
    for node in nodes:
        if node["num_edges"] == 0:
            node["first_edge"] = end
        end = node["first_edge"] + node["num_edges"]
    return nodes, edges


def adjacency_literal(plane, neighbourhood, components=None):
    plane = np.asarray(plane, np.int32)
    H, W = plane.shape
    frame, uncovered, pairs = {}, {}, {}
    groups = set()
    for y in range(H):
        for x in range(W):
            g = int(plane[y, x])
            if g < 0:
                continue
            groups.add(g)
            for dx, dy in SIDES:
                ax, ay = x + dx, y + dy
                if not (0 <= ax < W and 0 <= ay < H):
                    frame[g] = frame.get(g, 0) + 1
                elif plane[ay, ax] < 0:
                    uncovered[g] = uncovered.get(g, 0) + 1
                elif plane[ay, ax] != g:
                    pairs.setdefault((g, int(plane[ay, ax])), [0, 0])[0] += 1
    if neighbourhood == ADJACENT_N8:
        for y in range(H - 1):
            for x in range(W - 1):
                for (ax, ay), (bx, by) in (((x, y), (x + 1, y + 1)), ((x + 1, y), (x, y + 1))):
                    a, b = int(plane[ay, ax]), int(plane[by, bx])
                    if a >= 0 and b >= 0 and a != b:
                        pairs.setdefault((a, b), [0, 0])[1] += 1
                        pairs.setdefault((b, a), [0, 0])[1] += 1
    return _assemble(sorted(groups), frame, uncovered, pairs, components)


def adjacency(plane, neighbourhood, components=None):
    """(nodes, edges) of every group of the plane: NODE_DTYPE by ascending group and EDGE_DTYPE.  id = group
    and component = -1, or, with the component list of level_components_model the plane is the label image
    of, that component's id and component (neighbour_id likewise)."""
    plane = np.asarray(plane, np.int32)
    H, W = plane.shape
    R = np.full((H + 2, W + 2), -2, np.int64)        # -2: outside the frame
    R[1:-1, 1:-1] = np.maximum(plane, -1)
    c = R[1:-1, 1:-1]
    groups = np.unique(c[c >= 0])
    nodes = np.zeros(len(groups), NODE_DTYPE)
    if components is None:
        nodes["id"], nodes["component"] = groups, -1
        id_of = lambda g: g
    else:
        nodes["id"], nodes["component"] = components["id"][groups], components["component"][groups]
        id_of = lambda g: components["id"][g]

    def shifted(dx, dy):
        return R[1 + dy:H + 1 + dy, 1 + dx:W + 1 + dx]

    def per_group(values):
        at = np.searchsorted(groups, values)
        return np.bincount(at, minlength=len(groups))

    triples = []                                    # (group, other, kind)
    frame = np.zeros(len(groups), np.int64)
    uncovered = np.zeros(len(groups), np.int64)
    for dx, dy in SIDES:
        a = shifted(dx, dy)
        frame += per_group(c[(c >= 0) & (a == -2)])
        uncovered += per_group(c[(c >= 0) & (a == -1)])
        m = (c >= 0) & (a >= 0) & (a != c)
        triples.append(np.stack([c[m], a[m], np.zeros(m.sum(), np.int64)], axis=1))
    if neighbourhood == ADJACENT_N8:
        for dx, dy in DIAGONALS:
            a = shifted(dx, dy)
            m = (c >= 0) & (a >= 0) & (a != c)
            triples.append(np.stack([c[m], a[m], np.ones(m.sum(), np.int64)], axis=1))
    t = np.concatenate(triples).reshape(-1, 3)
    nodes["border_frame"], nodes["border_uncovered"] = frame, uncovered
    if len(t):
        pairs, inverse = np.unique(t[:, :2], axis=0, return_inverse=True)
        inverse = inverse.reshape(-1)
    else:
        pairs, inverse = np.zeros((0, 2), np.int64), np.zeros(0, np.int64)
    edges = np.zeros(len(pairs), EDGE_DTYPE)
    edges["neighbour"] = np.searchsorted(groups, pairs[:, 1])
    edges["neighbour_id"] = id_of(pairs[:, 1])
    edges["shared_n4"] = np.bincount(inverse[t[:, 2] == 0], minlength=len(pairs))
    edges["shared_diagonal"] = np.bincount(inverse[t[:, 2] == 1], minlength=len(pairs))
    owner = np.searchsorted(groups, pairs[:, 0])
    nodes["num_edges"] = np.bincount(owner, minlength=len(groups))
    nodes["first_edge"] = np.cumsum(nodes["num_edges"]) - nodes["num_edges"]
    nodes["border_shared"] = np.bincount(owner, weights=edges["shared_n4"], minlength=len(groups))
    return nodes, edges


def sides_of(nodes, edges):
    """The stats' `sides`: every bordering side and every diagonal contact, once per group it counts for."""
    return int(nodes["border_frame"].sum(dtype=np.int64) + nodes["border_uncovered"].sum(dtype=np.int64) +
               nodes["border_shared"].sum(dtype=np.int64) + edges["shared_diagonal"].sum(dtype=np.int64))


def edges_of(nodes, edges, k):
    return edges[nodes[k]["first_edge"]:nodes[k]["first_edge"] + nodes[k]["num_edges"]]


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
