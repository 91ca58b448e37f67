"""The two definitions of level_adjacency_model.py agree, the per-pixel loop and the shifted comparisons, on
every small case plane; and the graph they describe has the properties the definition promises, on every
case, both neighbourhoods, regions and components.  CPU only."""
import numpy as np
import pytest

import level_adjacency_cases as ac
import level_adjacency_model as am
import level_boundaries_model as bm
import level_components_model as cm
import level_regions_cases as lc

CASES = ac.all_cases()
BY_NAME = {c.name: c for c in CASES}
SMALL = [c for c in CASES if c.W * c.H <= 2048]      # the literal form is a Python loop over pixels
HOODS = (am.ADJACENT_N4, am.ADJACENT_N8)


def planes_of(c):
    """Every plane the device calls see for the case: per level the id plane, and the label images of its
    N4 and N8 components with their component lists."""
    out = []
    for level in c.levels:
        ids = lc.id_image(c.msg, level)
        out.append((ids, None))
        for connect in (cm.N4, cm.N8):
            comps, _, labels = cm.sweep(ids, connect)
            out.append((labels, comps))
    return out


def pair_table(nodes, edges):
    """{(node, neighbour): (shared_n4, shared_diagonal)}"""
    out = {}
    for k in range(len(nodes)):
        for e in am.edges_of(nodes, edges, k):
            assert (k, int(e["neighbour"])) not in out
            out[k, int(e["neighbour"])] = (int(e["shared_n4"]), int(e["shared_diagonal"]))
    return out


@pytest.mark.parametrize("case", SMALL, ids=lambda c: c.name)
def test_literal_equals_vectorised(case):
    for plane, comps in planes_of(case):
        for hood in HOODS:
            want = am.adjacency_literal(plane, hood, comps)
            got = am.adjacency(plane, hood, comps)
            assert am.same_bits(got[0], want[0]) and am.same_bits(got[1], want[1]), (case.name, hood)


def test_literal_equals_vectorised_on_random_planes():
    rng = np.random.RandomState(11)
    for k in range(200):
        H, W = rng.randint(1, 9), rng.randint(1, 11)
        plane = rng.randint(-1, rng.choice([2, 4, 30]), size=(H, W)).astype(np.int32)
        for hood in HOODS:
            want = am.adjacency_literal(plane, hood)
            got = am.adjacency(plane, hood)
            assert am.same_bits(got[0], want[0]) and am.same_bits(got[1], want[1]), (k, hood)


def test_a_plane_without_a_covered_pixel_has_no_node():
    for hood in HOODS:
        for f in (am.adjacency, am.adjacency_literal):
            nodes, edges = f(np.full((3, 4), -1, np.int32), hood)
            assert nodes.shape == (0,) and nodes.dtype == am.NODE_DTYPE
            assert edges.shape == (0,) and edges.dtype == am.EDGE_DTYPE
    assert am.NODE_DTYPE.itemsize == 28 and am.EDGE_DTYPE.itemsize == 16


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_identities(case):
    for plane, comps in planes_of(case):
        H, W = plane.shape
        covered = plane >= 0
        graphs = {hood: am.adjacency(plane, hood, comps) for hood in HOODS}
        for hood, (nodes, edges) in graphs.items():
            what = (case.name, hood, comps is not None)
            table = pair_table(nodes, edges)
            # symmetry: (a, b) has a mirror (b, a) with equal counts
            for (a, b), counts in table.items():
                assert a != b and table[b, a] == counts, what
            # neighbour strictly ascending within a node; ids and neighbour ids consistent
            for k in range(len(nodes)):
                mine = am.edges_of(nodes, edges, k)
                assert (np.diff(mine["neighbour"]) > 0).all(), what
                assert np.array_equal(mine["neighbour_id"], nodes["id"][mine["neighbour"]]), what
                assert nodes[k]["border_shared"] == mine["shared_n4"].sum(), what
                assert ((mine["shared_n4"] + mine["shared_diagonal"]) > 0).all(), what
            # edge lists are contiguous: first_edge is the running sum of num_edges
            assert np.array_equal(nodes["first_edge"], np.cumsum(nodes["num_edges"]) - nodes["num_edges"]), what
            assert nodes["num_edges"].sum() == len(edges), what
            if covered.all():
                assert nodes["border_frame"].sum() == 2 * W + 2 * H, what
                assert nodes["border_uncovered"].sum() == 0, what
            # shared sides, counted independently with two shifted comparisons
            a, b = plane[:, :-1], plane[:, 1:]
            c, d = plane[:-1, :], plane[1:, :]
            n_pairs = ((a >= 0) & (b >= 0) & (a != b)).sum() + ((c >= 0) & (d >= 0) & (c != d)).sum()
            assert edges["shared_n4"].sum() == 2 * n_pairs, what
            if hood == am.ADJACENT_N4:
                assert (edges["shared_diagonal"] == 0).all(), what
            # the perimeter, from the group's area and its inner sides
            for k in np.unique(plane[covered])[:40]:
                mask = plane == k
                inner = (mask[:, :-1] & mask[:, 1:]).sum() + (mask[:-1, :] & mask[1:, :]).sum()
                node = nodes[np.searchsorted(np.unique(plane[covered]), k)]
                total = int(node["border_frame"]) + int(node["border_uncovered"]) + int(node["border_shared"])
                assert total == 4 * mask.sum() - 2 * inner, what
        # N4 edges are the N8 edges with shared_diagonal zeroed, minus those whose shared_n4 is 0
        n4, n8 = pair_table(*graphs[am.ADJACENT_N4]), pair_table(*graphs[am.ADJACENT_N8])
        assert n4 == {k: (s, 0) for k, (s, d) in n8.items() if s > 0}, case.name
        for f in ("id", "component", "border_frame", "border_uncovered", "border_shared"):
            assert np.array_equal(graphs[am.ADJACENT_N4][0][f], graphs[am.ADJACENT_N8][0][f]), (case.name, f)


@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_n4_neighbours_are_the_groups_on_the_outer_boundary(case):
    """For every node, the set of its N4 neighbours equals the set of non-negative plane values found at
    the in-frame points of its outer boundary, as level_boundaries_model lists them."""
    for plane, comps in planes_of(case):
        H, W = plane.shape
        nodes, edges = am.adjacency(plane, am.ADJACENT_N4, comps)
        records, points = bm.boundaries(plane, True, comps)
        assert len(records) == len(nodes)
        assert np.array_equal(records["id"], nodes["id"]) and np.array_equal(records["component"], nodes["component"])
        for k, rec in enumerate(records):
            p = points[rec["first_point"]:rec["first_point"] + rec["num_points"]]
            inside = (p[:, 0] >= 0) & (p[:, 0] < W) & (p[:, 1] >= 0) & (p[:, 1] < H)
            values = plane[p[inside, 1], p[inside, 0]]
            want = set(values[values >= 0].tolist())
            got = set(am.edges_of(nodes, edges, k)["neighbour"].tolist())
            if comps is None:                      # the plane holds ids: neighbours are node indices
                got = set(nodes["id"][sorted(got)].tolist())
            assert got == want, (case.name, k)


def test_the_cases_built_for_the_graph():
    for name, (W, H) in (("star_300x2", (300, 2)), ("star_2x300", (2, 300))):
        c = BY_NAME[name]
        assert (c.W, c.H) == (W, H)
        nodes, edges = am.adjacency(lc.id_image(c.msg, 0), am.ADJACENT_N4)
        assert nodes[0]["id"] == ac.STAR_HUB and nodes[0]["num_edges"] == ac.STAR_LEAVES
        assert nodes["num_edges"].max() == ac.STAR_LEAVES and len(nodes) == ac.STAR_LEAVES + 1
        assert (am.edges_of(nodes, edges, 0)["shared_n4"] == 1).all()
    plane = lc.id_image(BY_NAME["diag_only"].msg, 0)
    comps, _, labels = cm.sweep(plane, cm.N4)
    assert len(comps) == plane.size
    nodes, edges = am.adjacency(labels, am.ADJACENT_N8, comps)
    own = edges[edges["neighbour_id"] == np.repeat(nodes["id"], nodes["num_edges"])]
    assert len(own) > 0 and (own["shared_n4"] == 0).all() and (own["shared_diagonal"] > 0).all()
    nodes4, edges4 = am.adjacency(labels, am.ADJACENT_N4, comps)
    assert (edges4["neighbour_id"] != np.repeat(nodes4["id"], nodes4["num_edges"])).all()
    nodes, edges = am.adjacency(lc.id_image(BY_NAME["max_id"].msg, 0), am.ADJACENT_N8)
    assert nodes["id"].tolist() == [0, ac.MAX_ID] and edges["neighbour_id"].tolist() == [ac.MAX_ID, 0]
    assert edges["neighbour"].tolist() == [1, 0] and edges["shared_n4"][0] == edges["shared_n4"][1] > 0
    nodes, edges = am.adjacency(lc.id_image(BY_NAME["hole"].msg, 0), am.ADJACENT_N4)
    assert nodes["id"].tolist() == [3, 8]
    assert min(nodes[0]["border_frame"], nodes[0]["border_uncovered"], nodes[0]["border_shared"]) > 0
    assert nodes[0]["border_frame"] == 2 * 12 + 2 * 10 and nodes[0]["border_shared"] == 2
    assert nodes[1]["border_frame"] == 0 and nodes[1]["border_uncovered"] == 8 and nodes[1]["border_shared"] == 2
