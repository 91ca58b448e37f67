"""The boundary persistence additions to the renderer's C ABI: the three calls and their stats are declared in
include/vsg_render.h with the documented signatures and struct, exported by libvsg_render.so and bound by the
Python layer with matching layouts; the host-side table builder runs clean under the sanitizers as a
stand-alone program.  Needs no device."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsg_render_persistence_image", "vsg_render_persistence_frame", "vsg_render_persistence_graph",
       "vsg_render_last_persistence_stats")


@pytest.fixture(scope="module")
def raw_header():
    with open(os.path.join(ROOT, "include", "vsg_render.h")) as f:
        return f.read()


@pytest.fixture(scope="module")
def header(raw_header):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw_header, flags=re.S))


def test_header_declares_the_documented_signatures_and_struct(header):
    for text in (
            "int vsg_render_persistence_image(vsg_render* h, const uint8_t* seg, size_t seg_len, "
            "int32_t* out_int32, int* num_levels, int mem_out);",
            "int vsg_render_persistence_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, "
            "const uint8_t* bgr, size_t stride, int mem_in, uint8_t* out, size_t out_stride, int mem_out, "
            "int* num_levels);",
            "int vsg_render_persistence_graph(vsg_render* h, const uint8_t* seg, size_t seg_len, int neighbourhood, "
            "vsg_render_level_node* nodes, size_t capacity_nodes, size_t* num_nodes, "
            "vsg_render_level_edge* edges, size_t capacity_edges, size_t* num_edges, "
            "int32_t* persistence, int64_t* level_sides, size_t capacity_levels, size_t* num_levels, "
            "int mem_out);",
            "int vsg_render_last_persistence_stats(vsg_render* h, vsg_render_persistence_stats* s);"):
        assert text in header, text
    m = re.search(r"typedef struct vsg_render_persistence_stats \{(.*?)\} vsg_render_persistence_stats;", header)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == [
        "int64_t levels, regions, edge_pixels , top_pixels , nodes, edges",
        "float plane_us, persist_us, compose_us, graph_us", "int launches"]


def test_header_states_the_definitions(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    for phrase in ("Hierarchy.", "Height.", "Ancestors.", "Persistence of two region ids.",
                   "The persistence plane Q", "The persistence picture", "The persistence graph.",
                   "L = max(1, number of levels of that hierarchy)", "L > 65535 is VSG_ERR_INVALID",
                   "A_l(r) = GetParentId(r, 0, l)",
                   "pers(a, b) is the number of l in [0, L) with A_l(a) != A_l(b)",
                   "\"No region\" (-1) against a region is L",
                   "Q(x, y) = max( pers(P0(x,y), P0(x+1,y)) if x+1 < W, pers(P0(x,y), P0(x,y+1)) if y+1 < H )",
                   "Q > l holds exactly where vsg_render_id_image(level = l) differs",
                   "every byte is (s (L - Q) + L / 2) / L in unsigned integer arithmetic",
                   "out_stride 0 means vsg_render_default_stride",
                   "vsg_render_level_adjacency(level 0, connectedness 0, neighbourhood)",
                   "the number of unordered pairs of in-frame, side-adjacent pixels",
                   "still gets its persistence",
                   "The number of launches of each call does not depend on L",
                   "asks for the counts only"):
        assert phrase in text, phrase
    head = text[:text.index("#ifndef VSG_RENDER_H_")]
    assert "Not offered" in head and all(n in head for n in NEW[:3])


def test_older_signatures_are_still_there(header):
    for text in (
            "int vsg_render_create(const vsg_render_options* o, int width, int height, vsg_render** h);",
            "int vsg_render_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, const uint8_t* bgr, "
            "size_t stride, int mem_in, uint8_t* out, size_t out_stride, int mem_out);",
            "int vsg_render_id_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int32_t* out_int32, int mem_out);",
            "int vsg_render_level_adjacency(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, int neighbourhood, vsg_render_level_node* nodes, size_t capacity_nodes, "
            "size_t* num_nodes, vsg_render_level_edge* edges, size_t capacity_edges, size_t* num_edges, "
            "int mem_out);",
            "int vsg_render_last_adjacency_stats(vsg_render* h, vsg_render_adjacency_stats* s);",
            "int vsg_render_last_overlap_stats(vsg_render* h, vsg_render_overlap_stats* s);",
            "int vsg_render_last_stats(vsg_render* h, vsg_render_stats* s);",
            "void vsg_render_color(int region_id, uint8_t c[3]);"):
        assert text in header, text


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in NEW:
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    vp, psz, pint = C.c_void_p, C.POINTER(C.c_size_t), C.POINTER(C.c_int)
    assert L.vsg_render_persistence_image.argtypes == [vp, C.c_char_p, C.c_size_t, vp, pint, C.c_int]
    assert L.vsg_render_persistence_frame.argtypes == [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.c_int, vp,
                                                       C.c_size_t, C.c_int, pint]
    assert L.vsg_render_persistence_graph.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, vp, C.c_size_t, psz, vp,
                                                       C.c_size_t, psz, vp, vp, C.c_size_t, psz, C.c_int]
    assert L.vsg_render_last_persistence_stats.argtypes == [vp, C.POINTER(render.VsgRenderPersistenceStats)]
    for method in ("persistence_image", "persistence_frame", "persistence_graph", "last_persistence_stats"):
        assert hasattr(render.SegmentationRenderer, method), method


def test_stats_struct_layout():
    from video_segment_amd import render
    s = render.VsgRenderPersistenceStats
    assert [n for n, _ in s._fields_] == ["levels", "regions", "edge_pixels", "top_pixels", "nodes", "edges",
                                          "plane_us", "persist_us", "compose_us", "graph_us", "launches"]
    assert C.sizeof(s) == 6 * 8 + 4 * 4 + 4 + 4          # padded to the int64's alignment
    assert [getattr(s, n).offset for n, _ in s._fields_] == [0, 8, 16, 24, 32, 40, 48, 52, 56, 60, 64]


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    levels = C.c_int(77)
    plane = (C.c_int32 * 4)()
    frame = (C.c_uint8 * 12)()
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)     # never dereferenced by what follows

    def err():
        return L.vsg_render_last_error()

    # the image call
    assert L.vsg_render_persistence_image(None, b"", 0, plane, C.byref(levels), 0) == -1 and b"null" in err()
    assert L.vsg_render_persistence_image(fake, b"", 0, None, C.byref(levels), 0) == -1 and b"null" in err()
    assert L.vsg_render_persistence_image(fake, b"", 0, plane, None, 0) == -1 and b"null" in err()
    for mem in (2, -1):
        assert L.vsg_render_persistence_image(fake, b"", 0, plane, C.byref(levels), mem) == -1
        assert b"memory kind" in err()
    # the frame call
    assert L.vsg_render_persistence_frame(None, b"", 0, frame, 12, 0, frame, 0, 0, C.byref(levels)) == -1
    assert b"null" in err()
    assert L.vsg_render_persistence_frame(fake, b"", 0, frame, 12, 0, None, 0, 0, C.byref(levels)) == -1
    assert b"null" in err()
    assert L.vsg_render_persistence_frame(fake, b"", 0, frame, 12, 0, frame, 0, 0, None) == -1 and b"null" in err()
    for mem_in, mem_out in ((2, 0), (0, 2), (-1, 1)):
        assert L.vsg_render_persistence_frame(fake, b"", 0, frame, 12, mem_in, frame, 0, mem_out,
                                              C.byref(levels)) == -1
        assert b"memory kind" in err()
    assert levels.value == 77
    # the graph call
    nn, ne, nl = C.c_size_t(5), C.c_size_t(5), C.c_size_t(5)
    counts = (C.byref(nn), C.byref(ne), C.byref(nl))

    def graph(handle, hood, counts, mem=0):
        return L.vsg_render_persistence_graph(handle, b"", 0, hood, None, 0, counts[0], None, 0, counts[1], None,
                                              None, 0, counts[2], mem)

    assert graph(None, render.ADJACENT_N4, counts) == -1 and b"null" in err()
    for hood in (0, 3, -1):
        assert graph(fake, hood, counts) == -1 and b"neighbourhood" in err()
    for k in range(3):
        assert graph(fake, render.ADJACENT_N8, counts[:k] + (None,) + counts[k + 1:]) == -1 and b"null" in err()
    assert graph(fake, render.ADJACENT_N4, counts, mem=2) == -1 and b"memory kind" in err()
    assert L.vsg_render_last_persistence_stats(None, None) == -1
    s = render.VsgRenderPersistenceStats()
    assert L.vsg_render_last_persistence_stats(None, C.byref(s)) == -1


def test_table_builder_runs_clean_under_the_sanitizers(tmp_path):
    """The host-side ancestor table builder and its stand-alone main, compiled with AddressSanitizer and
    UndefinedBehaviorSanitizer and run on the CPU: ladders of every tested height, the tallest hierarchy, sparse
    ids, missing ids, empty inputs."""
    src = os.path.join(ROOT, "video_segment_amd", "render", "persistence_table_check.cpp")
    exe = str(tmp_path / "persistence_table_check")
    subprocess.check_call(["g++", "-std=c++17", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           src, "-o", exe])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.stdout, p.stderr)
