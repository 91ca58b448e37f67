"""The volume session additions to the renderer's C ABI: vsg_render_volume_begin, _add, _table and
vsg_render_last_volume_stats are declared in include/vsg_render.h with the documented signatures and structs,
exported by libvsg_render.so and bound by the Python layer with matching layouts.  Needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import volume_model as vm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vsg_render_volume_begin", "vsg_render_volume_add", "vsg_render_volume_table",
         "vsg_render_last_volume_stats")


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
    for text in (
            "int vsg_render_volume_begin(vsg_render* h, int level, int with_colors, int with_labels);",
            "int vsg_render_volume_add(vsg_render* h, const uint8_t* seg, size_t seg_len, int frame, "
            "const uint8_t* bgr, size_t stride, int mem_in, const int32_t* other, size_t other_pitch, "
            "int mem_other);",
            "int vsg_render_volume_table(vsg_render* h, vsg_render_volume_row* rows, size_t capacity_rows, "
            "size_t* num_rows, vsg_render_volume_col* cols, size_t capacity_cols, size_t* num_cols, "
            "vsg_render_volume_pair* pairs, size_t capacity_pairs, size_t* num_pairs, int mem_out);",
            "int vsg_render_last_volume_stats(vsg_render* h, vsg_render_volume_stats* s);"):
        assert text in header, text
    assert fields_of(header, "vsg_render_volume_row") == [
        "int32_t id, first_frame, last_frame, frames", "int32_t min_x, min_y, max_x, max_y",
        "int32_t first_pair, num_pairs, best_label, reserved0", "int64_t volume, unlabelled, best_count",
        "int64_t sum_x, sum_y, sum_t", "int64_t sum[3], sum_sq[3]", "uint8_t min[3], max[3], reserved1[2]"]
    assert fields_of(header, "vsg_render_volume_col") == [
        "int32_t label, num_pairs, best_row, first_frame, last_frame, frames",
        "int64_t volume, uncovered, best_count"]
    assert fields_of(header, "vsg_render_volume_pair") == ["int32_t row, col, label, frames", "int64_t count"]
    assert fields_of(header, "vsg_render_volume_stats") == [
        "int64_t frames, rows, cols, pairs", "int64_t new_rows, new_cols, new_pairs, resorts",
        "int64_t covered, labelled, both", "float frame_us, geometry_us, merge_us, sort_us, table_us",
        "int launches"]


def test_header_states_the_definition(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    for phrase in ("Connected components are not offered as groups: their indices mean nothing across frames",
                   "adding an index twice counts it twice (unchecked)",
                   "Without a session the call returns VSG_ERR_STATE",
                   "A failed add leaves the session as it was before the call",
                   "Other calls on the handle between two adds do not disturb the session",
                   "may be called at any time of a session and does not end it",
                   "ascending by id", "ascending by label",
                   "grouped by row in row order and within a row by ascending label",
                   "Without with_labels: unlabelled = 0, best_label = -1, best_count = 0, first_pair = num_pairs = 0",
                   "Without with_colors: the colour fields are 0",
                   "volume - unlabelled is the sum of the counts of the row's pairs",
                   "volume - uncovered the sum of the counts of the column's pairs",
                   "The table equals the field-wise sum (minimum and maximum for the extrema) over the added frames",
                   "no output is touched", "asks for the counts only",
                   "reserved0 is written as 0", "reserved1 is written as 0"):
        assert phrase in text, phrase
    # the "Not offered" paragraph names the new calls
    head = text[:text.index("#ifndef VSG_RENDER_H_")]
    assert "Not offered" in head and "vsg_render_volume_begin" in head and "volume session" in head


def test_older_signatures_are_still_there(header):
    for text in (
            "int vsg_render_level_overlap(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, const int32_t* other, size_t other_pitch, int mem_other, "
            "vsg_render_overlap_row* rows, size_t capacity_rows, size_t* num_rows, "
            "vsg_render_overlap_col* cols, size_t capacity_cols, size_t* num_cols, "
            "vsg_render_overlap_pair* pairs, size_t capacity_pairs, size_t* num_pairs, int mem_out);",
            "int vsg_render_level_colors(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, const uint8_t* bgr, size_t stride, int mem_in, vsg_render_level_color* colors, "
            "size_t capacity_colors, size_t* num_colors, int mem_out);",
            "int vsg_render_level_regions(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "vsg_render_level_region* regions, size_t capacity_regions, size_t* num_regions, "
            "int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, int mem_out);",
            "int vsg_render_last_distance_stats(vsg_render* h, vsg_render_distance_stats* s);"):
        assert text in header, text


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in NAMES:
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    at = render.EXPORTED_SYMBOLS.index("vsg_render_last_color_stats")
    assert tuple(render.EXPORTED_SYMBOLS[at + 1:at + 5]) == NAMES
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_volume_begin.argtypes == [vp, C.c_int, C.c_int, C.c_int]
    assert L.vsg_render_volume_add.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_int, vp,
                                                C.c_size_t, C.c_int]
    assert L.vsg_render_volume_table.argtypes == [vp, vp, C.c_size_t, psz, vp, C.c_size_t, psz, vp, C.c_size_t, psz,
                                                  C.c_int]
    assert L.vsg_render_last_volume_stats.argtypes == [vp, C.POINTER(render.VsgRenderVolumeStats)]
    for method in ("volume_begin", "volume_add", "volume_table", "last_volume_stats"):
        assert hasattr(render.SegmentationRenderer, method), method
    assert callable(render.volume_scores)


def test_stats_struct_layout():
    from video_segment_amd import render
    s = render.VsgRenderVolumeStats
    assert [n for n, _ in s._fields_] == ["frames", "rows", "cols", "pairs", "new_rows", "new_cols", "new_pairs",
                                          "resorts", "covered", "labelled", "both", "frame_us", "geometry_us",
                                          "merge_us", "sort_us", "table_us", "launches"]
    assert C.sizeof(s) == 11 * 8 + 5 * 4 + 4 == 112
    assert [getattr(s, n).offset for n, _ in s._fields_] == [8 * k for k in range(11)] + [88, 92, 96, 100, 104, 108]


def test_row_col_and_pair_structs_have_no_padding():
    from video_segment_amd import render
    for d, model, offsets, size, words in (
            (render.VOLUME_ROW_DTYPE, vm.ROW_DTYPE, vm.ROW_OFFSETS, 152, render.VOLUME_ROW_WORDS),
            (render.VOLUME_COL_DTYPE, vm.COL_DTYPE, vm.COL_OFFSETS, 48, render.VOLUME_COL_WORDS),
            (render.VOLUME_PAIR_DTYPE, vm.PAIR_DTYPE, vm.PAIR_OFFSETS, 24, render.VOLUME_PAIR_WORDS)):
        assert d == model and d.itemsize == size == 4 * words
        assert {n: d.fields[n][1] for n in d.names} == offsets
        # no padding: the fields tile the record
        spans = sorted((d.fields[n][1], d.fields[n][1] + d.fields[n][0].itemsize) for n in d.names)
        assert spans[0][0] == 0 and spans[-1][1] == size
        assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))
    assert render.VOLUME_ROW_DTYPE["sum"].shape == (3,) and render.VOLUME_ROW_DTYPE["min"].base == np.uint8


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    err = L.vsg_render_last_error
    nr, nc, npairs = C.c_size_t(), C.c_size_t(), C.c_size_t()
    counts = (C.byref(nr), C.byref(nc), C.byref(npairs))
    # all of these are looked at before a non-null handle is dereferenced: the fake one is 8 bytes of zeros
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    plane = (C.c_int32 * 4)()
    frame = (C.c_uint8 * 12)()

    assert L.vsg_render_volume_begin(None, 0, 0, 0) == -1 and b"null" in err()
    for level in (-1, -7):
        assert L.vsg_render_volume_begin(fake, level, 0, 0) == -1 and b"level" in err()
    for flag in (2, -1, 7):
        assert L.vsg_render_volume_begin(fake, 0, flag, 0) == -1 and b"with_colors" in err()
        assert L.vsg_render_volume_begin(fake, 0, 0, flag) == -1 and b"with_labels" in err()
        assert L.vsg_render_volume_begin(fake, 0, 1, flag) == -1 and b"with_labels" in err()

    assert L.vsg_render_volume_add(None, b"", 0, 0, frame, 12, 0, plane, 0, 0) == -1 and b"null" in err()
    for index in (-1, -(1 << 31)):
        assert L.vsg_render_volume_add(fake, b"", 0, index, frame, 12, 0, plane, 0, 0) == -1 and b"frame" in err()

    def table(handle, counts, mem_out=0):
        return L.vsg_render_volume_table(handle, None, 0, counts[0], None, 0, counts[1], None, 0, counts[2], mem_out)

    assert table(None, counts) == -1 and b"null" in err()
    for k in range(3):
        assert table(fake, counts[:k] + (None,) + counts[k + 1:]) == -1 and b"null" in err()
    for mem in (2, -1, 7):
        assert table(fake, counts, mem) == -1 and b"memory kind" in err()
    assert L.vsg_render_last_volume_stats(None, None) == -1
    s = render.VsgRenderVolumeStats()
    assert L.vsg_render_last_volume_stats(None, C.byref(s)) == -1
