"""The models of vsg_render_level_mesh_simplified against each other (no device): the level-by-level
Douglas-Peucker the device stages follow equals boundary_oracle.approx_poly_dp on every segment of every case,
on corner lists and on full lattice lists alike, and the case set reaches every branch of it.  That
approx_poly_dp equals csrc/boundary.cpp's ApproxPolyDP is what tests/test_boundary.py compares."""
import numpy as np
import pytest

import boundary_oracle as bo
import level_components_model as cm
import level_mesh_model as mm
import level_mesh_simplify_cases as sc
import level_mesh_simplify_model as sm
import level_regions_cases as lc

CASES = sc.all_cases()
BY_NAME = {c.name: c for c in CASES}


def meshes():
    """(what, mesh) of every case at level 0 in the regions' mode, and of random planes with -1."""
    for c in CASES:
        yield c.name, mm.mesh(np.array(lc.id_image(c.msg, 0), np.int32))
    rng = np.random.default_rng(11)
    for k in range(4):
        yield "random_%d" % k, mm.mesh(rng.integers(-1, 3, (40, 50)).astype(np.int32))


@pytest.fixture(scope="module")
def found():
    """{what: [(record, corners, {max_error: (list, info)})]}: dp_levels of every segment, computed once."""
    out = {}
    for what, result in meshes():
        out[what] = [(s, c, {e: sm.dp_levels(c, e, bool(s["closed"])) for e in sc.ERRORS})
                     for s, c in zip(result[0], sm.corner_lists(result))]
    return out


def test_the_level_by_level_model_equals_the_recursion_on_corners_and_on_lattice_points(found):
    compared = 0
    for what, segments in found.items():
        for s, corners, by_error in segments:
            closed = bool(s["closed"])
            q = sm.lattice(corners, closed)
            assert len(q) == int(s["length"]) + (0 if closed else 1), what
            for e, (got, _) in by_error.items():
                assert got == bo.approx_poly_dp(corners, e, closed), (what, e)
                assert got == bo.approx_poly_dp(q, e, closed), (what, e)
                compared += 1
    assert compared > 10000


def test_max_error_zero_returns_open_lists_unchanged_and_closed_lists_rotated(found):
    for what, segments in found.items():
        for s, corners, by_error in segments:
            got, info = by_error[0.0]
            if s["closed"]:
                k = info["start"]
                assert got == corners[k:] + corners[:k], what
            else:
                assert got == corners and len(got) >= 2, what


def test_an_open_segment_keeps_both_ends_and_every_vertex_is_a_corner(found):
    for what, segments in found.items():
        for s, corners, by_error in segments:
            for e, (got, info) in by_error.items():
                assert set(got) <= set(corners), (what, e)
                assert len(got) + len(info["dropped"]) == info["kept"], (what, e)
                if not s["closed"]:
                    assert got[0] == corners[0] and got[-1] == corners[-1] and len(got) >= 2, (what, e)


def test_the_cases_reach_every_branch(found):
    hit = set()
    for what, segments in found.items():
        if what.startswith("random"):
            continue
        for s, corners, by_error in segments:
            closed = bool(s["closed"])
            for e, (got, info) in by_error.items():
                hit.add("single_vertex_closed" if closed and len(got) == 1 else "")
                hit.add("start_not_0" if info["start"] else "")
                hit.add("tie" if info["ties"] else "")
                hit.add(("drop_closed" if closed else "drop_open") if info["dropped"] else "")
                hit.add("wrap_read_written" if info["wrap_read_written"] else "")
                hit.add("depth_64" if info["depth"] >= 64 else "")
                hit.add("coincide" if info["coincide"] else "")
            for _, msp in sc.PARAMS:
                hit.add("collapsed" if not closed and int(s["length"]) + 1 < sm.threshold(msp) else "")
            hit.add("beyond_wave" if len(corners) > sc.WAVE_POINTS else "")
            hit.add("beyond_workgroup" if len(corners) > 1024 else "")
            hit.add("beyond_lds" if len(corners) > sc.LDS_POINTS and not closed else "")
    assert hit - {""} == {"single_vertex_closed", "start_not_0", "tie", "drop_closed", "drop_open",
                          "wrap_read_written", "depth_64", "coincide", "collapsed", "beyond_wave",
                          "beyond_workgroup", "beyond_lds"}


def test_what_the_small_shapes_give():
    ids = np.array(lc.id_image(BY_NAME["tiny_islands"].msg, 0), np.int32)
    # the unit square: its diagonal is sqrt(2) long and its other corners 0.71 from it; the 2 x 2 square: twice that
    for e, counts in ((0.5, [4, 4]), (1.0, [2, 4]), (2.0, [1, 2]), (3.5, [1, 1])):
        segments, vertices, _, _ = sm.simplified(ids, None, e, 0)
        closed = segments[(segments["closed"] == 1) & (segments["left"] >= 0)]
        assert closed["num_vertices"].tolist() == counts, e
    # the one-pixel staircase goes at max_error 1, the two-pixel staircase stays
    for step, kept in ((1, False), (2, True)):
        ids = np.array(lc.id_image(BY_NAME["staircase_%d" % step].msg, 0), np.int32)
        segments, _, _, _ = sm.simplified(ids, None, 1.0, 4)
        border = segments[segments["left"] >= 0]
        assert len(border) == 1 and (border[0]["num_vertices"] > 2) == kept, step
    # the collapse rule counts lattice points: length + 1 < max(3, min_segment_points)
    ids = np.array(lc.id_image(BY_NAME["four_at_a_corner"].msg, 0), np.int32)
    result = mm.mesh(ids)
    for msp, t in ((0, 0), (1, 3), (4, 4), (9, 9)):
        assert sm.threshold(msp) == t
        st = sm.stats_of(result, 0.0, msp)
        assert st["collapsed_segments"] == int(((result[0]["closed"] == 0) & (result[0]["length"] + 1 < t)).sum())
    # an open segment with coinciding ends: one sweep; within max_error of its start it is that corner twice
    ids = np.array(lc.id_image(BY_NAME["diagonal_islands_5_5"].msg, 0), np.int32)
    segments, vertices, _, _ = sm.simplified(ids, None, 2.0, 0)
    small = segments[segments["length"] == 4]
    assert len(small) == 2 and (small["num_vertices"] == 2).all() and (small["closed"] == 0).all()
    for s in small:
        assert vertices[s["first_vertex"]].tolist() == vertices[s["first_vertex"] + 1].tolist() == [3, 3]


def test_simplified_keeps_everything_but_the_vertices():
    for name in ("euclidean_voronoi_200x150", "three_levels", "diagonal_islands_5_6"):
        c = BY_NAME[name]
        for level in c.levels:
            ids = np.array(lc.id_image(c.msg, level), np.int32)
            for connect in (0, cm.N4):
                plane, comps = (ids, None) if connect == 0 else (cm.sweep(ids, connect)[2], cm.sweep(ids, connect)[0])
                want = mm.mesh(plane, comps)
                for e, msp in sc.PARAMS:
                    got = sm.simplified(plane, comps, e, msp, result=want)
                    assert mm.same_bits(got[2], want[2]) and mm.same_bits(got[3], want[3])
                    a, b = got[0].copy(), want[0].copy()
                    for rec in (a, b):
                        rec["first_vertex"] = rec["num_vertices"] = 0
                    assert mm.same_bits(a, b)
                    assert got[0]["first_vertex"].tolist() == \
                        np.concatenate([[0], np.cumsum(got[0]["num_vertices"])[:-1]]).tolist()
                    assert len(got[1]) == int(got[0]["num_vertices"].sum())
                    st = sm.stats_of(want, e, msp)
                    assert st["vertices_out"] == len(got[1]) and st["vertices_in"] == len(want[1])
                    assert st["vertices_out"] <= st["vertices_kept"] <= st["vertices_in"] + st["segments"]
