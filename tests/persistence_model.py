"""Plain numpy model of boundary persistence (not collected by pytest; the persistence tests compare the
product against it byte for byte).

The definition.  The hierarchy has L = max(1, levels) levels; A_l(r) = GetParentId(r, 0, l), A_0(r) = r.
pers(a, b) is the number of l in [0, L) with A_l(a) != A_l(b); "no region" (-1) against a region is L, -1
against -1 is 0.  With P0 the level-0 id image, Q(x, y) is the larger of pers(P0(x, y), P0(x + 1, y)) and
pers(P0(x, y), P0(x, y + 1)), each only where the neighbour is in the frame.  The picture's bytes are
(s * (L - Q) + L // 2) // L.  The graph is level_adjacency_model.adjacency of P0 with pers of every directed
edge and, per level, the number of side-adjacent pixel pairs with two different non-negative ids.

`ancestors` below is what the functions take: (ids, table), ids the ascending ids of P0 and table an
(L, len(ids)) int64 array with table[l, k] = A_l(ids[k]).  The persistence of a pair is counted plainly, level
by level."""
import numpy as np

import level_adjacency_model as am
import render_model as rm


def height(hierarchy):
    return max(1, len(hierarchy))


def ancestors(ids0, hierarchy):
    """(ids, table) of the non-negative values of the plane ids0 under render_model.hierarchy_of's lists."""
    ids0 = np.asarray(ids0)
    ids = np.unique(ids0[ids0 >= 0]).astype(np.int64)
    L = height(hierarchy)
    table = np.empty((L, len(ids)), np.int64)
    for k, r in enumerate(ids.tolist()):
        for l in range(L):
            table[l, k] = rm.get_parent_id(r, l, hierarchy)
    return ids, table


def pers(a, b, anc):
    """pers of two arrays of ids (-1: no region), elementwise, int32."""
    ids, table = anc
    L = table.shape[0]
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    out = np.zeros(a.shape, np.int32)
    both = (a >= 0) & (b >= 0)
    if both.any():
        ca, cb = np.searchsorted(ids, a[both]), np.searchsorted(ids, b[both])
        count = np.zeros(ca.shape, np.int32)
        for l in range(L):
            count += table[l, ca] != table[l, cb]
        out[both] = count
    out[(a >= 0) != (b >= 0)] = L
    return out


def plane(ids0, anc):
    """Q: H x W int32."""
    p = np.maximum(np.asarray(ids0, np.int64), -1)
    q = np.zeros(p.shape, np.int32)
    q[:, :-1] = pers(p[:, :-1], p[:, 1:], anc)
    q[:-1] = np.maximum(q[:-1], pers(p[:-1], p[1:], anc))
    return q


def picture(q, L, src=None):
    """H x W x 3 uint8 from Q; src: the H x W x 3 uint8 source frame, or None for 255 everywhere."""
    q = np.asarray(q, np.int64)
    s = np.full(q.shape + (3,), 255, np.int64) if src is None else np.asarray(src, np.int64)
    return ((s * (L - q)[:, :, None] + L // 2) // L).astype(np.uint8)


def level_image(ids0, anc, l):
    """The id image of level l: P0 mapped through A_l, -1 kept."""
    ids, table = anc
    p = np.maximum(np.asarray(ids0, np.int64), -1)
    out = np.full(p.shape, -1, np.int64)
    out[p >= 0] = table[l, np.searchsorted(ids, p[p >= 0])]
    return out


def sides(ids0, anc):
    """level_sides: int64 per level, counted on each level's image."""
    out = np.zeros(anc[1].shape[0], np.int64)
    for l in range(len(out)):
        p = level_image(ids0, anc, l)
        for a, b in ((p[:, :-1], p[:, 1:]), (p[:-1], p[1:])):
            out[l] += int(((a >= 0) & (b >= 0) & (a != b)).sum())
    return out


def graph(ids0, hood, anc):
    """(nodes, edges, persistence, level_sides)."""
    nodes, edges = am.adjacency(ids0, hood)
    owner = np.repeat(nodes["id"], nodes["num_edges"])
    return nodes, edges, pers(owner, edges["neighbour_id"], anc), sides(ids0, anc)


def edge_mask(level_ids):
    """Where an id image differs from its in-frame right or below neighbour, -1 counting as a value: the
    pixels highlight_edges blackens."""
    p = np.asarray(level_ids)
    m = np.zeros(p.shape, bool)
    m[:, :-1] |= p[:, :-1] != p[:, 1:]
    m[:-1] |= p[:-1] != p[1:]
    return m
