"""The numpy model of boundary persistence against its definitions, level by level, on every case of the
persistence tests.  Needs no device and no library."""
import numpy as np
import pytest

import level_adjacency_model as am
import level_regions_cases as lc
import persistence_cases as pc
import persistence_model as pm
import render_model as rm

CASES = pc.all_cases()
BY_NAME = {c.name: c for c in CASES}


def parts(case):
    ids0 = lc.id_image(case.msg, 0)
    hier = rm.hierarchy_of(case.msg)
    return ids0, pm.height(hier), pm.ancestors(ids0, hier)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_plane_thresholds_are_the_levels_edge_masks(name):
    case = BY_NAME[name]
    ids0, L, anc = parts(case)
    assert case.levels == tuple(range(L))
    q = pm.plane(ids0, anc)
    assert q.dtype == np.int32 and q.shape == (case.H, case.W) and q.min() >= 0 and q.max() <= L
    for l in range(L):
        level_ids = lc.id_image(case.msg, l)
        assert np.array_equal(level_ids, pm.level_image(ids0, anc, l)), (name, l)
        # the brute-force definition: right and below, in frame, -1 counting as a value
        want = np.zeros(q.shape, bool)
        for y in range(case.H):
            for x in range(case.W):
                want[y, x] = ((x + 1 < case.W and level_ids[y, x] != level_ids[y, x + 1]) or
                              (y + 1 < case.H and level_ids[y, x] != level_ids[y + 1, x]))
            if case.W * case.H > 4096:
                break                                   # large planes: the first row literally, all by shifts
        if case.W * case.H <= 4096:
            assert np.array_equal(q > l, want), (name, l)
        else:
            assert np.array_equal((q > l)[0], want[0]), (name, l)
        assert np.array_equal(q > l, pm.edge_mask(level_ids)), (name, l)
    assert not (q > L - 1).any() or (q == L).any()


@pytest.mark.parametrize("name", [c.name for c in CASES])
@pytest.mark.parametrize("hood", (am.ADJACENT_N4, am.ADJACENT_N8))
def test_graph_against_the_levels_own_graphs(name, hood):
    case = BY_NAME[name]
    ids0, L, anc = parts(case)
    nodes, edges, persistence, level_sides = pm.graph(ids0, hood, anc)
    want_nodes, want_edges = am.adjacency(ids0, hood)
    assert am.same_bits(nodes, want_nodes) and am.same_bits(edges, want_edges)
    assert persistence.dtype == np.int32 and persistence.shape == (len(edges),)
    assert level_sides.dtype == np.int64 and level_sides.shape == (L,)
    assert len(edges) == 0 or (persistence.min() >= 1 and persistence.max() <= L)
    # symmetric: the edge b -> a has the persistence of a -> b
    owner = np.repeat(np.arange(len(nodes)), nodes["num_edges"])
    back = {(int(o), int(n)): int(p) for o, n, p in zip(owner, edges["neighbour"], persistence)}
    assert all(back[n, o] == p for (o, n), p in back.items())
    for l in range(L):
        level_nodes, _ = am.adjacency(lc.id_image(case.msg, l), am.ADJACENT_N4)
        assert 2 * level_sides[l] == level_nodes["border_shared"].sum(dtype=np.int64), (name, l)
        assert 2 * level_sides[l] == edges["shared_n4"][persistence > l].sum(dtype=np.int64), (name, l)


@pytest.mark.parametrize("L", pc.LADDER_HEIGHTS)
def test_ladder_has_every_value(L):
    case = BY_NAME["ladder_%d" % L]
    ids0, height, anc = parts(case)
    assert height == L
    q = pm.plane(ids0, anc)
    assert q[0].tolist() == list(range(1, L)) + [L, 0] and q[1].tolist() == q[0].tolist()
    _, _, persistence, level_sides = pm.graph(ids0, am.ADJACENT_N4, anc)
    assert sorted(set(persistence.tolist())) == list(range(1, L + 1))
    # two rows: level l has lost l of the L column boundaries
    assert level_sides.tolist() == [2 * (L - l) for l in range(L)]


def test_uncovered_pixels_count_as_a_value_of_every_level():
    case = BY_NAME["uncovered"]
    ids0, L, anc = parts(case)
    q = pm.plane(ids0, anc)
    assert L == 1 and q[0, 4] == 1 and q[3].max() == 1 and q[3, 5] == 0    # row 3 is uncovered, row 4 nearly
    assert pm.pers(np.array([-1, -1, 2]), np.array([-1, 1, -1]), anc).tolist() == [0, 1, 1]


def test_picture_formula():
    rng = np.random.RandomState(5)
    src = rng.randint(0, 256, (3, 4, 3)).astype(np.uint8)
    for L in (1, 2, 3, 7, 20, 65535):
        zero, top = np.zeros((3, 4), np.int32), np.full((3, 4), L, np.int32)
        assert np.array_equal(pm.picture(zero, L, src), src)                 # Q = 0: the source as it is
        assert (pm.picture(zero, L) == 255).all()
        assert (pm.picture(top, L, src) == 0).all() and (pm.picture(top, L) == 0).all()   # Q = L: black
        if L > 1:
            q = np.full((3, 4), L // 2, np.int32)
            got = pm.picture(q, L, src)
            for s, g in zip(src.ravel().tolist(), got.ravel().tolist()):
                assert g == (s * (L - L // 2) + L // 2) // L
    assert pm.picture(np.array([[1]]), 2).tolist() == [[[128, 128, 128]]]     # (255 + 1) // 2
    assert pm.picture(np.array([[1]]), 3).tolist() == [[[170, 170, 170]]]     # (510 + 1) // 3
