"""The vector additions to the renderer's C ABI: vsg_render_rasterize and vsg_render_last_vector_stats
are declared in include/vsg_render.h with the documented signatures, exported by libvsg_render.so and
bound by the Python layer with matching argument lists and struct layout.  Needs no device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def header():
    with open(os.path.join(ROOT, "include", "vsg_render.h")) as f:
        text = f.read()
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", text, flags=re.S))


def test_header_declares_the_documented_signatures(header):
    assert ("int vsg_render_rasterize(vsg_render* h, const uint8_t* seg, size_t seg_len, int32_t* out, "
            "size_t capacity_intervals, size_t* count, int mem_out);") in header
    assert "int vsg_render_last_vector_stats(vsg_render* h, vsg_render_vector_stats* s);" in header
    m = re.search(r"typedef struct vsg_render_vector_stats \{(.*?)\} vsg_render_vector_stats;", header)
    assert m
    fields = [f.strip() for f in m.group(1).split(";") if f.strip()]
    assert fields == ["int64_t lines", "int64_t crossings", "int64_t groups", "int64_t largest_group",
                      "float walk_us, sort_us, pairs_us", "int launches"]
    # additive: what was there is still there, letter for letter
    assert ("int vsg_render_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, const uint8_t* bgr, "
            "size_t stride, int mem_in, uint8_t* out, size_t out_stride, int mem_out);") in header
    assert ("int vsg_render_id_image(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int32_t* out_int32, int mem_out);") in header


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in ("vsg_render_rasterize", "vsg_render_last_vector_stats"):
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    vp = C.c_void_p
    assert L.vsg_render_rasterize.argtypes == [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.POINTER(C.c_size_t),
                                               C.c_int]
    s = render.VsgRenderVectorStats
    assert [n for n, _ in s._fields_] == ["lines", "crossings", "groups", "largest_group", "walk_us", "sort_us",
                                          "pairs_us", "launches"]
    assert C.sizeof(s) == 4 * 8 + 3 * 4 + 4 and s.walk_us.offset == 32 and s.launches.offset == 44
    assert hasattr(render.SegmentationRenderer, "rasterize")
    # null arguments are answered without a device
    assert L.vsg_render_rasterize(None, b"", 0, None, 0, None, 0) == -1
    assert L.vsg_render_last_vector_stats(None, None) == -1
