"""The mesh simplification additions to the renderer's C ABI: vsg_render_level_mesh_simplified and
vsg_render_last_simplify_stats are declared in include/vsg_render.h with the documented signatures and struct,
exported by libvsg_render.so and bound by the Python layer with a matching layout; every refusal that needs no
device is answered before the handle is dereferenced.  Needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vsg_render_level_mesh_simplified", "vsg_render_last_simplify_stats")


@pytest.fixture(scope="module")
def raw_header():
    with open(os.path.join(ROOT, "include", "vsg_render.h")) as f:
        return f.read()


@pytest.fixture(scope="module")
def header(raw_header):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw_header, flags=re.S))


def test_header_declares_the_documented_signatures_and_struct(header):
    assert ("int vsg_render_level_mesh_simplified(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, float max_error, int min_segment_points, vsg_render_mesh_segment* segments, "
            "size_t capacity_segments, size_t* num_segments, int32_t* vertices, size_t capacity_vertices, "
            "size_t* num_vertices, vsg_render_mesh_loop* loops, size_t capacity_loops, size_t* num_loops, "
            "int32_t* refs, size_t capacity_refs, size_t* num_refs, int mem_out);") in header
    assert "int vsg_render_last_simplify_stats(vsg_render* h, vsg_render_simplify_stats* s);" in header
    m = re.search(r"typedef struct vsg_render_simplify_stats \{(.*?)\} vsg_render_simplify_stats;", header)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == [
        "int64_t segments, collapsed_segments, vertices_in, vertices_kept, vertices_out, single_vertex_closed, "
        "longest_segment_vertices_in",
        "float dp_us, clean_us, table_us", "int max_rounds, launches"]
    # the mesh call is as it was
    assert ("int vsg_render_level_mesh(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, vsg_render_mesh_segment* segments,") in header


def test_header_states_the_definition(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    for phrase in ("The point list.", "Collapse rule.",
                   "are exactly those of vsg_render_level_mesh for the same (level, connectedness)",
                   "Only `vertices`, and each record's first_vertex and num_vertices, change",
                   "An open segment has length + 1 points, both end corners included",
                   "A closed segment has length points",
                   "It begins at the first vertex the mesh call lists for it, and none is repeated",
                   "Let t = max(3, min_segment_points) if min_segment_points > 0, else 0",
                   "An open segment with length + 1 < t becomes {first corner, last corner}",
                   "The reference's call uses 4",
                   "ApproxPolyDP(Q, (double)max_error, closed = record.closed)",
                   "the first index wins a tie",
                   "max_dist max_dist <= eps (dx dx + dy dy)",
                   "the wrap-around read of a closed list included",
                   "An open segment whose two end corners coincide goes in as closed = false",
                   "An open segment always keeps both end corners (num_vertices >= 2)",
                   "A closed segment may come back with 1 vertex or more",
                   "Its vertex count need not be even",
                   "max_error = 0 with min_segment_points = 0 returns every open segment's corner list unchanged",
                   "every closed segment's list as a cyclic rotation",
                   "max_error has to be finite and >= 0, min_segment_points >= 0",
                   "before the handle is dereferenced",
                   "no output is touched",
                   "asks for the counts only",
                   "vsg_render_last_contour_stats and vsg_render_last_mesh_stats describe that run",
                   "no launch happens per round",
                   "80 bytes with 4 bytes of tail padding"):
        assert phrase in text, phrase
    head = text[:text.index("#ifndef VSG_RENDER_H_")]
    for phrase in ("vsg_render_level_mesh_simplified", "approxPolyDP", "still not offered", "min_hole_length",
                   "unordered_map hole order", "vector_mesh numbering"):
        assert phrase in head, phrase


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in NAMES:
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    at = render.EXPORTED_SYMBOLS.index("vsg_render_last_mesh_stats")
    assert tuple(render.EXPORTED_SYMBOLS[at + 1:at + 3]) == NAMES
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_level_mesh_simplified.argtypes == \
        [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, C.c_float, C.c_int] + [vp, C.c_size_t, psz] * 4 + [C.c_int]
    assert L.vsg_render_last_simplify_stats.argtypes == [vp, C.POINTER(render.VsgRenderSimplifyStats)]
    for method in ("level_mesh_simplified", "last_simplify_stats"):
        assert hasattr(render.SegmentationRenderer, method)
    assert callable(render.simplified_mesh_desc) and callable(render.mesh_desc)


def test_stats_struct_layout():
    from video_segment_amd import render
    import level_mesh_simplify_model as sm
    s = render.VsgRenderSimplifyStats
    assert [n for n, _ in s._fields_] == [
        "segments", "collapsed_segments", "vertices_in", "vertices_kept", "vertices_out", "single_vertex_closed",
        "longest_segment_vertices_in", "dp_us", "clean_us", "table_us", "max_rounds", "launches"]
    assert C.sizeof(s) == 80                                   # 76 bytes of fields, 4 of tail padding
    assert [getattr(s, n).offset for n, _ in s._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 60, 64, 68, 72]
    assert set(sm.COUNTS) <= {n for n, _ in s._fields_}


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    counts = [C.c_size_t(77) for _ in range(4)]
    outs = [np.full(8, 0x5A, np.int32) for _ in range(4)]

    def call(handle, connect=0, refs=None, mem_out=0, max_error=1.0, min_points=4):
        refs = [C.byref(c) for c in counts] if refs is None else refs
        args = []
        for o, r in zip(outs, refs):
            args += [o.ctypes.data_as(C.c_void_p), 1, r]
        return L.vsg_render_level_mesh_simplified(handle, b"", 0, 0, connect, max_error, min_points, *args, mem_out)

    def untouched():
        return all(c.value == 77 for c in counts) and all((o == 0x5A).all() for o in outs)

    assert call(None) == -1 and b"null" in L.vsg_render_last_error() and untouched()
    # everything below is looked at before a non-null handle is dereferenced
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    for k in range(4):
        refs = [C.byref(c) for c in counts]
        refs[k] = None
        assert call(fake, 0, refs) == -1 and b"count" in L.vsg_render_last_error() and untouched()
    for connect in (0, render.N4, render.N8):
        for mem in (2, -1, 7):
            assert call(fake, connect, mem_out=mem) == -1 and b"mem_out" in L.vsg_render_last_error() and untouched()
    for connect in (3, -1, 4):
        for mem in (0, 1):
            assert call(fake, connect, mem_out=mem) == -1 and b"connectedness" in L.vsg_render_last_error()
            assert untouched()
    for bad in (float("nan"), float("inf"), float("-inf"), -1.0, -1e-30):
        for connect in (0, render.N4):
            assert call(fake, connect, max_error=bad) == -1 and b"max_error" in L.vsg_render_last_error()
            assert untouched()
    for bad in (-1, -4, -2 ** 31):
        assert call(fake, min_points=bad) == -1 and b"min_segment_points" in L.vsg_render_last_error()
        assert untouched()
    assert L.vsg_render_last_simplify_stats(None, None) == -1
    s = render.VsgRenderSimplifyStats()
    assert L.vsg_render_last_simplify_stats(None, C.byref(s)) == -1
    assert L.vsg_render_last_simplify_stats(fake, None) == -1


def test_simplified_mesh_desc_drops_degenerate_loops_and_is_mesh_desc_otherwise():
    """Host numpy only: a loop whose polygon has fewer than three distinct vertices is left out, as the
    reference drops polygon.size() == 3 && polygon[0] == polygon[2]."""
    from video_segment_amd import render
    import level_mesh_model as mm
    import level_mesh_simplify_model as sm
    ids = np.full((8, 12), 1, np.int32)
    ids[3, 3] = 2
    ids[3:6, 6:10] = 3
    import level_regions_cases as lc
    want = mm.mesh(ids)
    # on the mesh itself no loop is dropped: mesh_desc's bytes
    assert render.simplified_mesh_desc(12, 8, [1, 2, 3], *want) == render.mesh_desc(12, 8, [1, 2, 3], *want)
    # at max_error 2 the one-pixel island is one vertex: its loop, and the hole it leaves in region 1, go
    got = sm.simplified(ids, None, 2.0, 0, result=want)
    island = [s for s in got[0] if s["right"] == 1 and s["left"] == 0][0]
    assert island["num_vertices"] == 1
    desc = render.simplified_mesh_desc(12, 8, [1, 2, 3], *got)
    m = lc.Msg()
    m.ParseFromString(desc)
    assert [r.id for r in m.region] == [1, 3]
    assert [len(r.vectorization.polygon) for r in m.region] == [2, 1]
    assert m.rasterization_removed and m.frame_width == 12 and m.frame_height == 8


def test_mesh_polygons_takes_the_simplified_lists():
    """Host numpy only: oblique edges, points repeated at joints and one-vertex loops go through mesh_polygons;
    every polygon keeps its loop's signed area and lists points of the loop only.  At (0, 0), where only the
    starts of closed segments moved, the polygons are those of the mesh itself, which the mesh tests hold against
    the contours call's."""
    from video_segment_amd import render
    import level_mesh_model as mm
    import level_mesh_simplify_cases as sc
    import level_mesh_simplify_model as sm
    import level_regions_cases as lc

    def area2(pts):
        pts = [tuple(int(v) for v in p) for p in pts]
        return sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(pts, pts[1:] + pts[:1]))

    for name in ("discs_200x150", "euclidean_voronoi_200x150", "tiny_islands", "diagonal_islands_5_5", "plus_island"):
        c = {c.name: c for c in sc.own() + sc.mc.small()}[name]
        ids = np.array(lc.id_image(c.msg, 0), np.int32)
        mesh = mm.mesh(ids)
        plain = render.mesh_polygons(*mesh)
        for e, msp in sc.PARAMS:
            got = sm.simplified(ids, None, e, msp, result=mesh)
            groups = render.mesh_polygons(*got)
            assert len(groups) == len(plain), (name, e)
            loops = iter(got[2])
            oblique = 0
            for polys in groups:
                for poly in polys:
                    loop = next(loops)
                    pts = render._loop_points(got[0], got[1], loop, got[3])
                    assert {tuple(p) for p in poly.tolist()} <= {tuple(p) for p in pts}, (name, e)
                    assert area2(poly.tolist()) == area2(pts), (name, e)
                    listed = poly.tolist()
                    assert all(listed[k] != listed[k - 1] for k in range(len(listed))) or len(listed) == 1, (name, e)
                    oblique += sum(a[0] != b[0] and a[1] != b[1] for a, b in zip(listed, listed[1:] + listed[:1]))
            if (e, msp) == (0.0, 0):
                # nothing but rotations of closed segments changed: the polygons of the mesh itself
                assert all(np.array_equal(a, b) for x, y in zip(groups, plain) for a, b in zip(x, y)), name
            if name == "discs_200x150" and e >= 1.0:
                assert oblique > 0
