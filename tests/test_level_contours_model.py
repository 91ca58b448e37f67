"""level_contours_model.py checked on every case by properties it was not built from: an even-odd fill of a
group's contours gives the group back, lengths sum to perimeters and areas to areas, outer contours number as
many as N4 components, lists start at their smallest turn and hold no collinear triple.  Needs no device."""
import numpy as np
import pytest

import level_adjacency_model as am
import level_components_model as cm
import level_contours_cases as tc
import level_contours_model as tm
import level_regions_cases as lc

CASES = tc.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODES = (0, cm.N4, cm.N8)


def planes_of(case):
    """(level, connectedness, plane, components or None) of every plane the case is asked for."""
    for level in case.levels:
        ids = lc.id_image(case.msg, level)
        yield level, 0, ids, None
        for connect in (cm.N4, cm.N8):
            comps, _, labels = cm.sweep(ids, connect)
            yield level, connect, labels, comps


@pytest.fixture(scope="module")
def traced():
    """The model's result for every plane of every case, computed once."""
    out = {}
    for c in CASES:
        for level, connect, plane, comps in planes_of(c):
            out[c.name, level, connect] = (plane, comps) + tm.contours(plane, comps)
    return out


def fill(vertices, W, H):
    """Even-odd scanline fill of closed rectilinear polygons: a pixel is inside when an odd number of vertical
    sides lie left of its centre."""
    acc = np.zeros((H, W + 1), np.int64)
    for poly in vertices:
        nxt = np.roll(poly, -1, axis=0)
        for (x0, y0), (x1, y1) in zip(poly.tolist(), nxt.tolist()):
            if x0 == x1:
                acc[min(y0, y1):max(y0, y1), x0] += 1
    return (np.cumsum(acc, axis=1)[:, :W] % 2) == 1


def polygons(records, vertices):
    return [vertices[r["first_vertex"]:r["first_vertex"] + r["num_vertices"]] for r in records]


def test_the_cases_are_what_their_names_say(traced):
    _, _, records, vertices = traced["one_region_1x1", 0, 0]
    assert len(records) == 1 and records[0]["num_vertices"] == 4 and records[0]["area2"] == 2
    assert records[0]["length"] == 4 and vertices.tolist() == [[0, 0], [1, 0], [1, 1], [0, 1]]
    for c in tc.full_cover():
        _, _, records, vertices = traced[c.name, 0, 0]
        assert vertices.tolist() == [[0, 0], [c.W, 0], [c.W, c.H], [0, c.H]], c.name
        assert records["length"].tolist() == [2 * c.W + 2 * c.H] and records["area2"].tolist() == [2 * c.W * c.H]
    c = BY_NAME["pixel_checker"]
    assert len(traced["pixel_checker", 0, 0][2]) == c.W * c.H
    for connect in MODES:
        records = traced["saddle", 0, connect][2]
        assert len(records) == 2 and (records["area2"] == 2).all() and (records["group"] == [0, 0 if connect != cm.N4 else 1]).all()
    _, _, records, vertices = traced["diagonal_hole", 0, 0]
    assert records["num_vertices"].tolist() == [4, 8] and records["area2"].tolist() == [72, -4]
    hole = [tuple(v) for v in polygons(records, vertices)[1].tolist()]
    assert hole.count((3, 3)) == 2 and len(set(hole)) == 7
    plane, _, records, vertices = traced["wide_hole", 0, 0]
    hole = records[(records["id"] == 4) & (records["area2"] < 0)]
    assert len(hole) == 2
    # the hole around region 9 starts at its top-right corner, not at the corner of its smallest crack
    around_9 = polygons(hole[:1], vertices)[0].tolist()
    assert around_9[0] == [6, 2] and len(around_9) == 4
    # its crack of smallest key, the bottom side of pixel (3, 1), starts at (4, 2): collinear, not listed
    assert min(k for k in tm.cracks_of(np.where(plane == 4, 4, -1)) if k // 4 == 9 + 3) == 4 * 12 + 2
    assert [4, 2] not in around_9
    records = traced["nested", 0, 0][2]
    assert (records["area2"] < 0).sum() == 4 and len(records) == 9
    records = traced["comb_8192", 0, 0][2]
    assert len(records) == 1 and records[0]["num_vertices"] > 1 << 14
    records = traced["comb", 0, 0][2]
    assert len(records) == 128 and (records["num_vertices"] == 4).all()
    plane, _, records, _ = traced["spiral_129x65", 0, 0]
    assert len(records) == 1 and records[0]["length"] == len(tm.cracks_of(plane)) > 129 * 65
    assert len(traced["uncovered_frame", 0, 0][2]) == 0


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_properties(traced, name):
    c = BY_NAME[name]
    for level, connect, _, _ in planes_of(c):
        plane, comps, records, vertices = traced[name, level, connect]
        what = (name, level, connect)
        groups = np.unique(plane[plane >= 0])
        assert sorted(set(records["group"].tolist())) == list(range(len(groups))), what
        assert (np.diff(records["group"]) >= 0).all(), what
        nodes, _ = am.adjacency(plane, am.ADJACENT_N4, comps)
        polys = polygons(records, vertices)
        assert records["first_vertex"].tolist() == np.cumsum([0] + [len(p) for p in polys])[:-1].tolist(), what
        for k, g in enumerate(groups.tolist()):
            mine = records["group"] == k
            of_k = [p for p, m in zip(polys, mine) if m]
            assert np.array_equal(fill(of_k, c.W, c.H), plane == g), what + (g,)
            perimeter = int(nodes[k]["border_frame"]) + int(nodes[k]["border_uncovered"]) + int(nodes[k]["border_shared"])
            assert records["length"][mine].sum() == perimeter, what + (g,)
            assert records["area2"][mine].sum() == 2 * int((plane == g).sum()), what + (g,)
            positive = int((records["area2"][mine] > 0).sum())
            assert records["area2"][mine][0] > 0, what + (g,)
            if connect == cm.N4:
                assert positive == 1, what + (g,)
            elif connect == 0:
                assert positive == int((traced[name, level, cm.N4][1]["id"] == g).sum()), what + (g,)
            if comps is None:
                assert (records["id"][mine] == g).all() and (records["component"][mine] == -1).all()
            else:
                assert (records["id"][mine] == comps["id"][g]).all()
                assert (records["component"][mine] == comps["component"][g]).all()
        for r, p in zip(records, polys):
            n = len(p)
            assert n >= 4 and n % 2 == 0, what
            d = np.roll(p, -1, axis=0) - p
            # sides alternate between horizontal and vertical: no collinear triple, no repeated vertex
            assert ((d[:, 0] != 0) != (d[:, 1] != 0)).all(), what
            assert ((d[:, 0] != 0) != (np.roll(d, -1, axis=0)[:, 0] != 0)).all(), what
            assert np.abs(d).sum() == r["length"], what
            assert (r["min_x"], r["min_y"], r["max_x"], r["max_y"]) == (p[:, 0].min(), p[:, 1].min(), p[:, 0].max(),
                                                                        p[:, 1].max()), what
        # every list starts at its smallest-key turn: among the turn cracks, which start at the vertices, the
        # first one's key is the smallest; keys of one contour's turn cracks are recovered from corner and
        # direction of the side that leaves it
        for r, p in zip(records, polys):
            d = np.sign(np.roll(p, -1, axis=0) - p)
            keys = []
            for (x, y), (dx, dy) in zip(p.tolist(), d.tolist()):
                s = tm.STEP.index((dx, dy))
                keys.append(4 * ((y - tm.START[s][1]) * c.W + (x - tm.START[s][0])) + s)
            assert keys[0] == min(keys), what
        # contours of a group by ascending first key
        firsts = []
        for r, p in zip(records, polys):
            dx, dy = np.sign(p[1] - p[0]).tolist()
            s = tm.STEP.index((dx, dy))
            firsts.append((int(r["group"]), 4 * ((int(p[0][1]) - tm.START[s][1]) * c.W + int(p[0][0]) - tm.START[s][0]) + s))
        assert firsts == sorted(firsts), what
        st = tm.stats_of(plane)
        assert st == {"cracks": int(records["length"].sum()), "vertices": len(vertices), "contours": len(records),
                      "holes": int((records["area2"] < 0).sum()),
                      "largest_contour_cracks": int(records["length"].max()) if len(records) else 0}
