"""level_mesh_model.py checked on every case and on random planes by what it was not built from: the loops
rebuilt from their refs are the contours of level_contours_model, every shared segment is referenced once in
each direction, the junctions' sides count every open segment's two ends, lengths sum to the adjacency model's
shared sides and borders, and a vector-only desc made of the mesh scan-converts back to the plane.  Needs no
device."""
import numpy as np
import pytest

import level_adjacency_model as am
import level_components_model as cm
import level_contours_model as tm
import level_mesh_cases as mc
import level_mesh_model as mm
import level_regions_cases as lc
import vector_cases as vc
import vector_raster_model as vm

CASES = mc.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODES = (0, cm.N4, cm.N8)


def planes_of(ids):
    yield 0, ids, None
    for connect in (cm.N4, cm.N8):
        comps, _, labels = cm.sweep(ids, connect)
        yield connect, labels, comps


def check_plane(plane, comps, what, ids=None):
    """Every property of the module's docstring on one plane.  ids: the id plane the label image `plane` is of."""
    from video_segment_amd import render
    assert render.MESH_SEGMENT_DTYPE == mm.SEGMENT_DTYPE and render.MESH_LOOP_DTYPE == mm.LOOP_DTYPE
    plane = np.asarray(plane, np.int32)
    H, W = plane.shape
    segments, vertices, loops, refs = result = mm.mesh(plane, comps)
    records, contour_vertices = tm.contours(plane, comps)
    # loops are the contours, in their order, and rebuild to their vertex lists
    assert len(loops) == len(records), what
    assert np.array_equal(loops["group"], records["group"]) and np.array_equal(loops["length"], records["length"]), what
    got = render.mesh_polygons(segments, vertices, loops, refs)
    want = render.contour_polygons(records, contour_vertices)
    assert len(got) == len(want), what
    for a, b in zip(got, want):
        assert len(a) == len(b) and all(tm.same_bits(x, np.ascontiguousarray(y)) for x, y in zip(a, b)), what
    assert loops["first_ref"].tolist() == (np.cumsum(loops["num_refs"]) - loops["num_refs"]).tolist(), what
    assert int(loops["num_refs"].sum()) == len(refs), what
    # references: a shared segment once in each direction, every other segment once forwards
    forwards = np.bincount(refs[refs >= 0], minlength=len(segments))
    backwards = np.bincount(~refs[refs < 0], minlength=len(segments))
    assert (forwards == 1).all() and np.array_equal(backwards, (segments["left"] >= 0).astype(np.int64)), what
    for loop in loops:
        mine = refs[loop["first_ref"]:loop["first_ref"] + loop["num_refs"]]
        for ref in mine.tolist():
            seg = segments[ref if ref >= 0 else ~ref]
            assert (seg["right"] if ref >= 0 else seg["left"]) == loop["group"], what
        assert sum(int(segments[r if r >= 0 else ~r]["length"]) for r in mine.tolist()) == loop["length"], what
    # segments: order, slices, vertex lists
    assert (segments["left"] < segments["right"]).all(), what
    assert (np.diff(segments["right"]) >= 0).all(), what
    assert segments["first_vertex"].tolist() == (np.cumsum(segments["num_vertices"]) - segments["num_vertices"]).tolist()
    assert int(segments["num_vertices"].sum()) == len(vertices), what
    for seg in segments:
        p = vertices[seg["first_vertex"]:seg["first_vertex"] + seg["num_vertices"]]
        d = (np.roll(p, -1, axis=0) - p) if seg["closed"] else np.diff(p, axis=0)
        assert ((d[:, 0] != 0) != (d[:, 1] != 0)).all(), what           # axis-parallel, no repeated vertex
        assert np.abs(d).sum() == seg["length"], what
        if seg["closed"]:
            assert len(p) >= 4 and len(p) % 2 == 0 and seg["start_sides"] == 0 and seg["end_sides"] == 0, what
        else:
            assert len(p) >= 2 and seg["start_sides"] in (3, 4) and seg["end_sides"] in (3, 4), what
            # interior corners are turns
            assert ((d[:-1, 0] != 0) != (d[1:, 0] != 0)).all(), what
    # junctions
    junctions = mm.junction_sides(plane)
    assert sum(junctions.values()) == 2 * int((segments["closed"] == 0).sum()), what
    # the adjacency model's sides
    nodes, edges = am.adjacency(plane, am.ADJACENT_N4, comps)
    pair_length = {}
    for seg in segments[segments["left"] >= 0]:
        key = (int(seg["left"]), int(seg["right"]))
        pair_length[key] = pair_length.get(key, 0) + int(seg["length"])
    want_pairs = {}
    for k in range(len(nodes)):
        for e in am.edges_of(nodes, edges, k):
            if e["shared_n4"] and e["neighbour"] > k:
                want_pairs[k, int(e["neighbour"])] = int(e["shared_n4"])
    assert pair_length == want_pairs, what
    open_border = np.bincount(segments["right"][segments["left"] < 0], segments["length"][segments["left"] < 0],
                              len(nodes)).astype(np.int64)
    assert np.array_equal(open_border, nodes["border_frame"].astype(np.int64) + nodes["border_uncovered"]), what
    # the counts
    st = mm.stats_of(plane, result)
    assert st["cracks"] == int(records["length"].sum()) and st["junctions"] == len(junctions), what
    # the round trip through a vector-only desc
    group_ids = np.unique(plane[plane >= 0]) if comps is None else comps["id"]
    msg = vc.Msg()
    msg.ParseFromString(render.mesh_desc(W, H, group_ids, segments, vertices, loops, refs))
    assert msg.rasterization_removed and (msg.frame_width, msg.frame_height) == (W, H), what
    assert [r.id for r in msg.region] == sorted(set(int(i) for i in np.asarray(group_ids)[:len(nodes)])), what
    corners = np.asarray(msg.vector_mesh.coord, np.float32).reshape(-1, 2)
    assert len(np.unique(corners, axis=0)) == len(corners), what          # every distinct corner once
    for r in msg.region:
        for p in r.vectorization.polygon:
            assert p.coord_idx[0] == p.coord_idx[-1], what
    rows, unspecified = vm.rasterize_desc(msg)
    assert unspecified == 0, what
    assert np.array_equal(vm.id_plane(rows, W, H), plane if ids is None else ids), what
    return result


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_every_case_in_every_mode_at_every_level(name):
    c = BY_NAME[name]
    for level in c.levels:
        ids = lc.id_image(c.msg, level)
        for connect, plane, comps in planes_of(ids):
            check_plane(plane, comps, (name, level, connect), ids)


def test_the_cases_are_what_their_names_say():
    def of(name, connect=0):
        ids = lc.id_image(BY_NAME[name].msg, 0)
        plane, comps = ids, None
        if connect:
            comps, _, plane = cm.sweep(ids, connect)
        return mm.mesh(plane, comps)

    for name in ("one_region_1x1", "one_region_7x1", "one_region_1x7"):
        segments, vertices, loops, refs = of(name)
        c = BY_NAME[name]
        assert len(segments) == 1 and segments[0].tolist() == (0, -1, 0, 4, 2 * c.W + 2 * c.H, 1, 0, 0)
        assert vertices.tolist() == [[0, 0], [c.W, 0], [c.W, c.H], [0, c.H]] and refs.tolist() == [0]
    segments, _, loops, refs = of("saddle_2x2")
    # a contour stays with its own pixel at a saddle: four loops whatever the connectedness
    assert len(loops) == 4 and loops["num_refs"].tolist() == [3] * 4 and (segments["length"] == 2).sum() == 4
    assert (segments["start_sides"].tolist() + segments["end_sides"].tolist()).count(4) == 4
    assert of("saddle_2x2", cm.N4)[2]["group"].tolist() == [0, 1, 2, 3]
    assert of("saddle_2x2", cm.N8)[2]["group"].tolist() == [0, 0, 1, 1]
    segments, vertices, _, _ = of("t_junction")
    bar = [vertices[s["first_vertex"]:s["first_vertex"] + s["num_vertices"]].tolist() for s in segments
           if s["left"] == 0]
    assert sorted(bar) == [[[0, 2], [3, 2]], [[3, 2], [6, 2]]]       # both list the corner the bar runs through
    hi, lo = of("island_7_in_2"), of("island_2_in_7")
    assert (hi[0]["closed"] == 1).all() and (lo[0]["closed"] == 1).all()
    shared_hi, shared_lo = hi[0][hi[0]["left"] >= 0][0], lo[0][lo[0]["left"] >= 0][0]
    a = hi[1][shared_hi["first_vertex"]:shared_hi["first_vertex"] + 4].tolist()
    b = lo[1][shared_lo["first_vertex"]:shared_lo["first_vertex"] + 4].tolist()
    assert a == [[2, 1], [4, 1], [4, 3], [2, 3]] and sorted(b) == sorted(a) and b != a     # the hole's direction
    assert hi[3].tolist() == [0, ~1, 1] and lo[3].tolist() == [~1, 0, 1]
    segments = of("uncovered_hole")[0]
    assert segments["closed"].tolist() == [1, 1] and segments["left"].tolist() == [-1, -1]
    segments = of("uncovered_edge_pixel")[0]
    assert len(segments) == 1 and segments[0]["closed"] == 1 and segments[0]["num_vertices"] == 8
    segments = of("border_to_edge")[0]
    assert len(segments) == 3 and (segments["closed"] == 0).all() and (segments["start_sides"] == 3).all()
    assert set(of("four_at_a_corner")[0]["start_sides"].tolist()) == {3, 4}
    assert 4 in of("abac")[0]["end_sides"].tolist()
    for name in ("diagonal_islands_5_5", "diagonal_islands_5_6"):
        segments, vertices, loops, _ = of(name)
        small = segments[segments["length"] == 4]
        assert len(small) == 2 and (small["closed"] == 0).all() and (small["num_vertices"] == 5).all()
        for s in small:
            assert vertices[s["first_vertex"]].tolist() == vertices[s["first_vertex"] + 4].tolist() == [3, 3]
    c = BY_NAME["pixel_checker"]
    segments = of("pixel_checker")[0]
    inner = segments[segments["left"] >= 0]
    assert (inner["length"] == 1).all() and len(inner) == (c.W - 1) * c.H + c.W * (c.H - 1)
    segments = of("stripes_4096x3")[0]
    border = segments[segments["left"] >= 0]
    assert len(border) == 1 and border[0]["length"] == 4096 and border[0]["num_vertices"] == 2
    segments = of("spiral_in_a_region")[0]
    assert segments["length"].max() > 129 * 65 // 2 and (segments["closed"] == 0).all()
    assert all(len(a) == 0 for a in of("uncovered_frame"))


def test_random_planes_with_uncovered_pixels():
    rng = np.random.default_rng(5)
    for k in range(40):
        W, H = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        plane = rng.integers(-1, 4, (H, W)).astype(np.int32)
        if k % 4 == 0:
            plane = np.repeat(np.repeat(plane, 2, 0), 2, 1)[:29, :39]       # thicker shapes, straight runs
        for connect, p, comps in planes_of(plane):
            check_plane(p, comps, ("random", k, connect), plane)
