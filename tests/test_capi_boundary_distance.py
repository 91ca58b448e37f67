"""The boundary distance additions to the renderer's C ABI: the three calls, the record and the stats are declared
in include/vsg_render.h with the documented signatures, layouts and definitions, exported by libvsg_render.so and
bound by the Python layer with matching layouts; null and bad arguments are answered without a device.  Needs no
device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import boundary_distance_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("vsg_render_boundary_distance", "vsg_render_boundary_benchmark", "vsg_render_last_distance_stats")


@pytest.fixture(scope="module")
def raw_header():
    with open(os.path.join(ROOT, "include", "vsg_render.h")) as f:
        return f.read()


@pytest.fixture(scope="module")
def header(raw_header):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", raw_header, flags=re.S))


def test_header_declares_the_documented_signatures_and_structs(header):
    for text in (
            "#define VSG_RENDER_DISTANCE_NONE 0x7fffffff",
            "#define VSG_RENDER_MAX_TOLERANCE_SQ 4096",
            "int vsg_render_boundary_distance(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int32_t* out_int32, int mem_out);",
            "int vsg_render_boundary_benchmark(vsg_render* h, const uint8_t* seg, size_t seg_len, "
            "const int32_t* other, size_t other_pitch, int mem_other, int tolerance_sq, "
            "vsg_render_boundary_score* scores, size_t capacity_levels, size_t* num_levels, int mem_out);",
            "int vsg_render_last_distance_stats(vsg_render* h, vsg_render_distance_stats* s);"):
        assert text in header, text
    m = re.search(r"typedef struct vsg_render_boundary_score \{(.*?)\} vsg_render_boundary_score;", header)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == [
        "int64_t seg_edges", "int64_t seg_matched", "int64_t gt_edges", "int64_t gt_matched"]
    m = re.search(r"typedef struct vsg_render_distance_stats \{(.*?)\} vsg_render_distance_stats;", header)
    assert [f.strip() for f in m.group(1).split(";") if f.strip()] == [
        "int64_t levels, edge_pixels, other_edge_pixels, max_distance",
        "float plane_us, classify_us, columns_us, rows_us, match_us", "int launches"]


def test_header_states_the_definitions(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    for phrase in ("Edge set of a plane.", "The squared distance.",
                   "P(x, y) != P(x+1, y) with x+1 < W, or P(x, y) != P(x, y+1) with y+1 < H",
                   "-1 counting as a value",
                   "D(x, y) = min over (u, v) in E of (x - u)^2 + (y - v)^2",
                   "D is VSG_RENDER_DISTANCE_NONE everywhere when E is empty",
                   "at most 32768 x 32768", "below VSG_RENDER_DISTANCE_NONE",
                   "which is exactly Q > level of the persistence plane",
                   "On every refusal the output is untouched",
                   "B' = max(B, -1)", "G = E(B')",
                   "seg_matched[l] = #{ p : Q(p) > l and D_G(p) <= T }",
                   "gt_matched[l] = #{ p in G : D_l(p) <= T }",
                   "M(p) = max{ Q(q) : |p - q|^2 <= T }",
                   "The number of launches of a call does not depend on L",
                   "tolerance_sq outside [0, VSG_RENDER_MAX_TOLERANCE_SQ] is VSG_ERR_INVALID",
                   "asks for the count only"):
        assert phrase in text, phrase
    head = text[:text.index("#ifndef VSG_RENDER_H_")]
    assert "Not offered" in head and all(n in head for n in NEW[:2])


def test_older_signatures_are_still_there(header):
    for text in (
            "int vsg_render_id_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int32_t* out_int32, int mem_out);",
            "int vsg_render_persistence_image(vsg_render* h, const uint8_t* seg, size_t seg_len, "
            "int32_t* out_int32, int* num_levels, int mem_out);",
            "int vsg_render_last_persistence_stats(vsg_render* h, vsg_render_persistence_stats* s);",
            "int vsg_render_last_contour_stats(vsg_render* h, vsg_render_contour_stats* s);",
            "void vsg_render_color(int region_id, uint8_t c[3]);"):
        assert text in header, text


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    assert tuple(render.EXPORTED_SYMBOLS[-3:]) == NEW
    for name in NEW:
        assert hasattr(L, name), name
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_boundary_distance.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, vp, C.c_int]
    assert L.vsg_render_boundary_benchmark.argtypes == [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int,
                                                        vp, C.c_size_t, psz, C.c_int]
    assert L.vsg_render_last_distance_stats.argtypes == [vp, C.POINTER(render.VsgRenderDistanceStats)]
    for method in ("boundary_distance", "boundary_benchmark", "last_distance_stats"):
        assert hasattr(render.SegmentationRenderer, method), method
    assert render.DISTANCE_NONE == dm.NONE == 0x7fffffff and render.MAX_TOLERANCE_SQ == dm.MAX_TOLERANCE_SQ == 4096


def test_struct_layouts():
    from video_segment_amd import render
    s = render.VsgRenderDistanceStats
    assert [n for n, _ in s._fields_] == ["levels", "edge_pixels", "other_edge_pixels", "max_distance", "plane_us",
                                          "classify_us", "columns_us", "rows_us", "match_us", "launches"]
    assert C.sizeof(s) == 4 * 8 + 5 * 4 + 4
    assert [getattr(s, n).offset for n, _ in s._fields_] == [0, 8, 16, 24, 32, 36, 40, 44, 48, 52]
    d = render.BOUNDARY_SCORE_DTYPE
    assert d == dm.SCORE_DTYPE and d.itemsize == 32 and render.BOUNDARY_SCORE_WORDS == 4
    assert [d.fields[n][1] for n in ("seg_edges", "seg_matched", "gt_edges", "gt_matched")] == [0, 8, 16, 24]


def test_boundary_scores_are_the_models_quotients():
    from video_segment_amd import render
    rec = np.zeros(4, render.BOUNDARY_SCORE_DTYPE)
    rec[0] = (10, 5, 8, 8)
    rec[1] = (4, 4, 8, 2)
    rec[2] = (0, 0, 8, 0)
    rec[3] = (3, 0, 0, 0)
    got = render.boundary_scores(rec)
    p, r, f, best = dm.scores(rec)
    assert got["precision"].dtype == np.float64 and got["precision"].tolist() == p.tolist() == [0.5, 1.0, 0.0, 0.0]
    assert got["recall"].tolist() == r.tolist() == [1.0, 0.25, 0.0, 0.0]
    assert got["f"].tolist() == f.tolist() and got["best_level"] == best == 0
    assert render.boundary_scores(rec[:0])["best_level"] is None


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    plane = (C.c_int32 * 4)(*([0x5A5A5A5A] * 4))
    other = (C.c_int32 * 4)()
    scores = (C.c_int64 * 8)(*([0x5A5A5A5A] * 8))
    levels = C.c_size_t(77)
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)     # never dereferenced by what follows

    def err():
        return L.vsg_render_last_error()

    # the distance call
    assert L.vsg_render_boundary_distance(None, b"", 0, 0, plane, 0) == -1 and b"null" in err()
    assert L.vsg_render_boundary_distance(fake, b"", 0, 0, None, 0) == -1 and b"null" in err()
    for mem in (2, -1):
        assert L.vsg_render_boundary_distance(fake, b"", 0, 0, plane, mem) == -1 and b"memory kind" in err()

    # the benchmark call
    def bench(handle, other_, mem_other, T, scores_, cap, count, mem_out):
        return L.vsg_render_boundary_benchmark(handle, b"", 0, other_, 0, mem_other, T, scores_, cap, count, mem_out)

    n = C.byref(levels)
    assert bench(None, other, 0, 4, scores, 2, n, 0) == -1 and b"null" in err()
    assert bench(fake, other, 0, 4, scores, 2, None, 0) == -1 and b"null" in err()
    assert bench(fake, None, 0, 4, scores, 2, n, 0) == -1 and b"null" in err()
    assert bench(fake, other, 0, 4, None, 2, n, 0) == -1 and b"null" in err()
    for mem_other in (2, -1):
        assert bench(fake, other, mem_other, 4, scores, 2, n, 0) == -1 and b"mem_other" in err()
    for mem_out in (2, -1):
        assert bench(fake, other, 0, 4, scores, 2, n, mem_out) == -1 and b"memory kind" in err()
    for T in (-1, 4097, 1 << 30, -(1 << 31)):
        assert bench(fake, other, 0, T, scores, 2, n, 0) == -1 and b"tolerance_sq" in err()
        assert bench(fake, other, 1, T, None, 0, n, 1) == -1 and b"tolerance_sq" in err()
    assert levels.value == 77
    assert list(plane) == [0x5A5A5A5A] * 4 and list(scores) == [0x5A5A5A5A] * 8
    # the stats
    assert L.vsg_render_last_distance_stats(None, None) == -1
    s = render.VsgRenderDistanceStats()
    assert L.vsg_render_last_distance_stats(None, C.byref(s)) == -1
    assert L.vsg_render_last_distance_stats(fake, None) == -1
