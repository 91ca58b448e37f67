"""The level mesh additions to the renderer's C ABI: vsg_render_level_mesh and vsg_render_last_mesh_stats are
declared in include/vsg_render.h with the documented signatures and structs, exported by libvsg_render.so and
bound by the Python layer with matching layouts.  Needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vsg_render_level_mesh", "vsg_render_last_mesh_stats")


@pytest.fixture(scope="module")
def raw_header():
    with open(os.path.join(ROOT, "include", "vsg_render.h")) as f:
        return f.read()


@pytest.fixture(scope="module")
def header(raw_header):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw_header, flags=re.S))


def fields_of(header, name):
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header)
    assert m, name
    return [f.strip() for f in m.group(1).split(";") if f.strip()]


def test_header_declares_the_documented_signatures_and_structs(header):
    assert ("int vsg_render_level_mesh(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, vsg_render_mesh_segment* segments, size_t capacity_segments, size_t* num_segments, "
            "int32_t* vertices, size_t capacity_vertices, size_t* num_vertices, vsg_render_mesh_loop* loops, "
            "size_t capacity_loops, size_t* num_loops, int32_t* refs, size_t capacity_refs, size_t* num_refs, "
            "int mem_out);") in header
    assert "int vsg_render_last_mesh_stats(vsg_render* h, vsg_render_mesh_stats* s);" in header
    assert fields_of(header, "vsg_render_mesh_segment") == [
        "int32_t right, left", "int32_t first_vertex, num_vertices", "int32_t length", "int32_t closed",
        "int32_t start_sides, end_sides"]
    assert fields_of(header, "vsg_render_mesh_loop") == ["int32_t group, first_ref, num_refs, length"]
    assert fields_of(header, "vsg_render_mesh_stats") == [
        "int64_t cracks, segments, closed_segments, shared_segments, vertices, loops, refs, junctions, "
        "longest_segment_cracks",
        "float plane_us, classify_us, trace_us, split_us, table_us", "int rounds, launches"]


def test_header_states_the_definition(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    for phrase in ("Sides at a corner.", "Halves.", "Segments.", "Loops and refs.",
                   "are those of vsg_render_level_contours for the same (level, connectedness)",
                   "It is 0, 2, 3 or 4",
                   "A corner with sides >= 3 is a junction",
                   "The four frame corners and a -1/-1 contact are not junctions",
                   "It is cut at every crack whose start corner is a junction",
                   "A contour without a junction is one closed half that begins at its leader",
                   "A half is an owner when the group index of its other side is smaller than its own",
                   "-1 counts as smaller than every group",
                   "made of the opposite sides (pixel across, side + 2) in reverse order",
                   "(right group index, key of the half's first crack) order",
                   "Both end corners are always listed, including where the curve runs straight through the junction",
                   "Interior collinear corners are never listed",
                   "A closed segment lists exactly its contour's vertices and repeats none",
                   "A half that starts and ends at the same junction is open, not closed",
                   "Loop c is contour c of the sibling contours call",
                   "The list begins with the half that contains the contour's leader crack",
                   "The other half is written as ~s",
                   "no output is touched",
                   "asks for the counts only",
                   "answered before the handle is dereferenced",
                   "A frame with no covered pixel returns four zero counts",
                   "The call neither resolves nor changes the level the handle keeps for vsg_render_frame",
                   "is refused with VSG_ERR_INVALID",
                   "104 bytes with 4 bytes of tail padding"):
        assert phrase in text, phrase
    # the opening comment names the new call, what is still missing, and keeps what earlier tests pin
    head = text[:text.index("#ifndef VSG_RENDER_H_")]
    assert "Not offered" in head and "vsg_render_level_mesh" in head and "vsg_render_level_contours" in head
    assert "shared-segment mesh" in head and "approxPolyDP" in head and "still not offered" in head
    for phrase in ("Lab histograms", "ground truth", "vsg_render_level_regions", "vsg_render_level_components",
                   "vsg_render_level_boundaries", "vsg_render_level_adjacency", "vsg_render_level_overlap",
                   "vsg_render_persistence_image", "vsg_render_persistence_frame", "vsg_render_persistence_graph",
                   "vsg_render_level_colors", "vsg_render_mean_frame", "draw_shape_descriptors",
                   "vsg_render_boundary_distance", "vsg_render_boundary_benchmark"):
        assert phrase in head, phrase


def test_older_signatures_are_still_there(header):
    for text in (
            "int vsg_render_create(const vsg_render_options* o, int width, int height, vsg_render** h);",
            "int vsg_render_id_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int32_t* out_int32, int mem_out);",
            "int vsg_render_level_contours(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, vsg_render_level_contour* contours, size_t capacity_contours, "
            "size_t* num_contours, int32_t* vertices, size_t capacity_vertices, size_t* num_vertices, "
            "int mem_out);",
            "int vsg_render_last_contour_stats(vsg_render* h, vsg_render_contour_stats* s);",
            "int vsg_render_level_adjacency(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, int neighbourhood, vsg_render_level_node* nodes, size_t capacity_nodes, "
            "size_t* num_nodes, vsg_render_level_edge* edges, size_t capacity_edges, size_t* num_edges, "
            "int mem_out);",
            "int vsg_render_boundary_distance(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int32_t* out_int32, int mem_out);",
            "int vsg_render_rasterize(",
            "int vsg_render_last_stats(vsg_render* h, vsg_render_stats* s);",
            "void vsg_render_color(int region_id, uint8_t c[3]);"):
        assert text in header, text


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in NAMES:
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    at = render.EXPORTED_SYMBOLS.index("vsg_render_last_contour_stats")
    assert tuple(render.EXPORTED_SYMBOLS[at + 1:at + 3]) == NAMES
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_level_mesh.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int] + \
        [vp, C.c_size_t, psz] * 4 + [C.c_int]
    assert L.vsg_render_last_mesh_stats.argtypes == [vp, C.POINTER(render.VsgRenderMeshStats)]
    for method in ("level_mesh", "last_mesh_stats"):
        assert hasattr(render.SegmentationRenderer, method)
    assert callable(render.mesh_polygons) and callable(render.mesh_desc)


def test_stats_struct_layout():
    from video_segment_amd import render
    s = render.VsgRenderMeshStats
    assert [n for n, _ in s._fields_] == [
        "cracks", "segments", "closed_segments", "shared_segments", "vertices", "loops", "refs", "junctions",
        "longest_segment_cracks", "plane_us", "classify_us", "trace_us", "split_us", "table_us", "rounds", "launches"]
    assert C.sizeof(s) == 104                                  # 100 bytes of fields, 4 of tail padding
    assert [getattr(s, n).offset for n, _ in s._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 84, 88,
                                                             92, 96]


def test_records_are_32_and_16_bytes_with_the_documented_offsets():
    from video_segment_amd import render
    import level_mesh_model as mm
    d = render.MESH_SEGMENT_DTYPE
    assert d == mm.SEGMENT_DTYPE and d.itemsize == 32 and render.MESH_SEGMENT_WORDS == 8
    assert {n: d.fields[n][1] for n in d.names} == {
        "right": 0, "left": 4, "first_vertex": 8, "num_vertices": 12, "length": 16, "closed": 20, "start_sides": 24,
        "end_sides": 28}
    d = render.MESH_LOOP_DTYPE
    assert d == mm.LOOP_DTYPE and d.itemsize == 16 and render.MESH_LOOP_WORDS == 4
    assert {n: d.fields[n][1] for n in d.names} == {"group": 0, "first_ref": 4, "num_refs": 8, "length": 12}
    assert all(d.fields[n][0] == np.dtype(np.int32) for n in d.names)


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    counts = [C.c_size_t(77) for _ in range(4)]
    outs = [np.full(8, 0x5A, np.int32) for _ in range(4)]

    def mesh(handle, connect, refs=None, mem_out=0):
        refs = [C.byref(c) for c in counts] if refs is None else refs
        args = []
        for o, r in zip(outs, refs):
            args += [o.ctypes.data_as(C.c_void_p), 1, r]
        return L.vsg_render_level_mesh(handle, b"", 0, 0, connect, *args, mem_out)

    def untouched():
        return all(c.value == 77 for c in counts) and all((o == 0x5A).all() for o in outs)

    assert mesh(None, 0) == -1 and b"null" in L.vsg_render_last_error() and untouched()
    # everything below is looked at before a non-null handle is dereferenced
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    for k in range(4):
        refs = [C.byref(c) for c in counts]
        refs[k] = None
        assert mesh(fake, 0, refs) == -1 and b"count" in L.vsg_render_last_error() and untouched()
    for connect in (0, render.N4, render.N8):
        for mem in (2, -1, 7):
            assert mesh(fake, connect, mem_out=mem) == -1 and b"mem_out" in L.vsg_render_last_error() and untouched()
    for connect in (3, -1, 4):
        for mem in (0, 1):
            assert mesh(fake, connect, mem_out=mem) == -1 and b"connectedness" in L.vsg_render_last_error()
            assert untouched()
    assert L.vsg_render_last_mesh_stats(None, None) == -1
    s = render.VsgRenderMeshStats()
    assert L.vsg_render_last_mesh_stats(None, C.byref(s)) == -1
