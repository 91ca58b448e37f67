"""The level colour additions to the renderer's C ABI: vsg_render_level_colors, vsg_render_mean_frame and
vsg_render_last_color_stats are declared in include/vsg_render.h with the documented signatures and structs,
exported by libvsg_render.so and bound by the Python layer with matching layouts.  Needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vsg_render_level_colors", "vsg_render_mean_frame", "vsg_render_last_color_stats")


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
    assert ("int vsg_render_level_colors(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, const uint8_t* bgr, size_t stride, int mem_in, "
            "vsg_render_level_color* colors, size_t capacity_colors, size_t* num_colors, int mem_out);") in header
    assert ("int vsg_render_mean_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, const uint8_t* bgr, size_t stride, int mem_in, "
            "uint8_t* out, size_t out_stride, int mem_out);") in header
    assert "int vsg_render_last_color_stats(vsg_render* h, vsg_render_color_stats* s);" in header
    assert fields_of(header, "vsg_render_level_color") == [
        "int32_t id", "int32_t component", "int32_t area", "uint8_t mean[3]", "uint8_t reserved0",
        "int64_t sum[3]", "int64_t sum_sq[3]", "uint8_t min[3], max[3]", "uint8_t reserved1[2]"]
    assert fields_of(header, "vsg_render_color_stats") == [
        "int64_t groups, intervals, covered, largest_group_intervals",
        "float plane_us, sums_us, table_us, paint_us", "int launches"]


def test_header_states_the_definition(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    for phrase in ("The planes.", "The table.", "The picture.",
                   "P is the plane of vsg_render_level_overlap",
                   "Only the first 3 W bytes of a row are read; a stride below 3 W is VSG_ERR_INVALID",
                   "F is required whatever the handle's has_video",
                   "It is read once per call",
                   "Pixels with P < 0 enter no record",
                   "rounded half up, in integers: (2 sum[c] + area) / (2 area)",
                   "Nothing else is derived on the device",
                   "0 (black) where P < 0, exactly as the cleared plane of vsg_render_frame",
                   "two touching groups with equal means show no edge between them",
                   "The call neither resolves nor changes the level the handle keeps for vsg_render_frame",
                   "num_colors is always set on VSG_OK and when the capacity is too small",
                   "colors == NULL with capacity 0 asks for the count only",
                   "answered before the handle is dereferenced",
                   "The stride is the exception",
                   "A frame with no covered pixel returns zero records",
                   "there are no floats, no colour conversion and no histogram in it"):
        assert phrase in text, phrase
    # the "Not offered" paragraph names the new calls
    head = text[:text.index("#ifndef VSG_RENDER_H_")]
    assert "Not offered" in head and "Lab histograms" in head
    assert "vsg_render_level_colors" in head and "vsg_render_mean_frame" in head


def test_older_signatures_are_still_there(header):
    for text in (
            "int vsg_render_create(const vsg_render_options* o, int width, int height, vsg_render** h);",
            "int vsg_render_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, const uint8_t* bgr, "
            "size_t stride, int mem_in, uint8_t* out, size_t out_stride, int mem_out);",
            "int vsg_render_id_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int32_t* out_int32, int mem_out);",
            "int vsg_render_level_regions(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "vsg_render_level_region* regions, size_t capacity_regions, size_t* num_regions, "
            "int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, int mem_out);",
            "int vsg_render_level_components(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, vsg_render_level_component* components, size_t capacity_components, "
            "size_t* num_components, int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, "
            "int32_t* label_image, int mem_out);",
            "int vsg_render_level_overlap(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, const int32_t* other, size_t other_pitch, int mem_other, "
            "vsg_render_overlap_row* rows, size_t capacity_rows, size_t* num_rows, "
            "vsg_render_overlap_col* cols, size_t capacity_cols, size_t* num_cols, "
            "vsg_render_overlap_pair* pairs, size_t capacity_pairs, size_t* num_pairs, int mem_out);",
            "int vsg_render_persistence_image(vsg_render* h, const uint8_t* seg, size_t seg_len, "
            "int32_t* out_int32, int* num_levels, int mem_out);",
            "int vsg_render_last_persistence_stats(vsg_render* h, vsg_render_persistence_stats* s);",
            "int vsg_render_last_overlap_stats(vsg_render* h, vsg_render_overlap_stats* s);",
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
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_level_colors.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t,
                                                  C.c_int, vp, C.c_size_t, psz, C.c_int]
    assert L.vsg_render_mean_frame.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t,
                                                C.c_int, vp, C.c_size_t, C.c_int]
    assert L.vsg_render_last_color_stats.argtypes == [vp, C.POINTER(render.VsgRenderColorStats)]
    for method in ("level_colors", "mean_frame", "last_color_stats"):
        assert hasattr(render.SegmentationRenderer, method)
    assert callable(render.color_moments)


def test_stats_struct_layout():
    from video_segment_amd import render
    s = render.VsgRenderColorStats
    assert [n for n, _ in s._fields_] == ["groups", "intervals", "covered", "largest_group_intervals", "plane_us",
                                          "sums_us", "table_us", "paint_us", "launches"]
    assert C.sizeof(s) == 56
    assert [getattr(s, n).offset for n, _ in s._fields_] == [0, 8, 16, 24, 32, 36, 40, 44, 48]


def test_record_is_72_bytes_with_the_documented_offsets():
    from video_segment_amd import render
    import level_colors_model as km
    d = render.LEVEL_COLOR_DTYPE
    assert d == km.COLOR_DTYPE and d.itemsize == 72 and render.LEVEL_COLOR_WORDS == 18
    assert {n: d.fields[n][1] for n in d.names} == {
        "id": 0, "component": 4, "area": 8, "mean": 12, "reserved0": 15, "sum": 16, "sum_sq": 40, "min": 64,
        "max": 67, "reserved1": 70}
    assert d.fields["sum"][0] == np.dtype((np.int64, (3,))) and d.fields["mean"][0] == np.dtype((np.uint8, (3,)))


def test_color_moments():
    from video_segment_amd import render
    rec = np.zeros(2, render.LEVEL_COLOR_DTYPE)
    rec["area"] = [4, 1]
    rec["sum"] = [[4, 8, 2], [9, 0, 255]]
    rec["sum_sq"] = [[4, 24, 2], [81, 0, 255 * 255]]
    mean, var = render.color_moments(rec)
    assert mean.dtype == var.dtype == np.float64
    assert mean.tolist() == [[1.0, 2.0, 0.5], [9.0, 0.0, 255.0]]
    assert var.tolist() == [[0.0, 2.0, 0.25], [0.0, 0.0, 0.0]]


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    n = C.c_size_t(77)
    frame = (C.c_uint8 * 12)()
    out = (C.c_uint8 * 12)()

    def colors(handle, connect, bgr, mem_in, count, mem_out=0):
        return L.vsg_render_level_colors(handle, b"", 0, 0, connect, bgr, 12, mem_in, None, 0, count, mem_out)

    def picture(handle, connect, bgr, mem_in, dst, mem_out=0):
        return L.vsg_render_mean_frame(handle, b"", 0, 0, connect, bgr, 12, mem_in, dst, 0, mem_out)

    assert colors(None, 0, frame, 0, C.byref(n)) == -1 and b"null" in L.vsg_render_last_error()
    assert picture(None, 0, frame, 0, out) == -1 and b"null" in L.vsg_render_last_error()
    # everything below is looked at before a non-null handle is dereferenced
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    assert colors(fake, 0, frame, 0, None) == -1 and b"count" in L.vsg_render_last_error()
    assert picture(fake, 0, frame, 0, None) == -1 and b"out is null" in L.vsg_render_last_error()
    for connect in (0, render.N4, render.N8):
        for mem in (0, 1):
            assert colors(fake, connect, None, mem, C.byref(n)) == -1
            assert b"bgr is null" in L.vsg_render_last_error()
            assert picture(fake, connect, None, mem, out) == -1
            assert b"bgr is null" in L.vsg_render_last_error()
        for mem in (2, -1, 7):
            assert colors(fake, connect, frame, mem, C.byref(n)) == -1 and b"mem_in" in L.vsg_render_last_error()
            assert picture(fake, connect, frame, mem, out) == -1 and b"mem_in" in L.vsg_render_last_error()
            assert colors(fake, connect, frame, 0, C.byref(n), mem) == -1
            assert b"mem_out" in L.vsg_render_last_error()
            assert picture(fake, connect, frame, 0, out, mem) == -1 and b"mem_out" in L.vsg_render_last_error()
    for connect in (3, -1, 4):
        for mem in (0, 1):
            assert colors(fake, connect, frame, mem, C.byref(n)) == -1
            assert b"connectedness" in L.vsg_render_last_error()
            assert picture(fake, connect, frame, mem, out) == -1 and b"connectedness" in L.vsg_render_last_error()
    assert L.vsg_render_last_color_stats(None, None) == -1
    s = render.VsgRenderColorStats()
    assert L.vsg_render_last_color_stats(None, C.byref(s)) == -1
