"""The level pool additions to the renderer's C ABI: vsg_render_level_pool, vsg_render_level_unpool and
vsg_render_last_pool_stats are declared in include/vsg_render.h with the documented signatures and structs,
exported by libvsg_render.so and bound by the Python layer with matching layouts.  Needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vsg_render_level_pool", "vsg_render_level_unpool", "vsg_render_last_pool_stats")


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
    assert ("int vsg_render_level_pool(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, const void* features, int dtype, int channels, "
            "ptrdiff_t chan_stride, ptrdiff_t row_stride, ptrdiff_t pixel_stride, int mem_in, "
            "vsg_render_pool_group* groups, double* sum, double* sum_sq, float* min, float* max, "
            "size_t capacity_groups, size_t* num_groups, int mem_out);") in header
    assert ("int vsg_render_level_unpool(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, const float* values, size_t num_values, int channels, int mem_in, float fill, "
            "void* out, int dtype, ptrdiff_t chan_stride, ptrdiff_t row_stride, "
            "ptrdiff_t pixel_stride, int mem_out);") in header
    assert "int vsg_render_last_pool_stats(vsg_render* h, vsg_render_pool_stats* s);" in header
    assert fields_of(header, "vsg_render_pool_group") == [
        "int32_t id", "int32_t component", "int32_t area", "int32_t reserved"]
    assert fields_of(header, "vsg_render_pool_stats") == [
        "int64_t groups, intervals, covered, largest_group_intervals, feature_bytes",
        "float plane_us, sums_us, table_us, paint_us", "int launches"]
    for define in ("#define VSG_POOL_F32 0", "#define VSG_POOL_F16 1", "#define VSG_POOL_BF16 2"):
        assert define in header


def test_header_states_the_definition(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    for phrase in ("The plane.", "The features.", "The table.", "Unpool.",
                   "P is the plane of vsg_render_level_overlap, exactly as for vsg_render_level_colors",
                   "Pixels with P < 0 enter no group, and their feature values are never read",
                   "Strides are in elements",
                   "features[c chan_stride + y row_stride + x pixel_stride]",
                   "Planar: pixel_stride == 1",
                   "Channels-last: chan_stride == 1 and pixel_stride >= channels",
                   "any negative stride, is VSG_ERR_INVALID",
                   "1 <= channels <= 65535",
                   "a statistic that is not wanted is not computed",
                   "Every element is first widened exactly to f64",
                   "the f64 sum of their squares",
                   "a function of the interval list and the layout only",
                   "there are no floating-point atomics anywhere",
                   "the extreme non-NaN values as f32, +inf and -inf when the group has none",
                   "A NaN in a group's channel makes that channel's sum and sum_sq NaN and touches nothing else",
                   "num_groups is always set on VSG_OK and when the capacity is too small",
                   "answered before the handle is dereferenced",
                   "A frame with no covered pixel returns zero groups",
                   "The call neither resolves nor changes the level the handle keeps for vsg_render_frame",
                   "num_values has to equal the number of groups of the level",
                   "converted to `dtype` with round-to-nearest-even",
                   "padding is never touched"):
        assert phrase in text, phrase
    # the "Not offered" paragraph names the new calls and keeps what it said
    head = text[:text.index("#ifndef VSG_RENDER_H_")]
    assert "Not offered" in head and "Lab histograms" in head
    assert "vsg_render_level_colors" in head and "vsg_render_mean_frame" in head
    assert "vsg_render_level_pool" in head and "vsg_render_level_unpool" in head


def test_older_signatures_are_still_there(header):
    for text in (
            "int vsg_render_create(const vsg_render_options* o, int width, int height, vsg_render** h);",
            "int vsg_render_level_regions(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "vsg_render_level_region* regions, size_t capacity_regions, size_t* num_regions, "
            "int32_t* intervals, size_t capacity_intervals, size_t* num_intervals, int mem_out);",
            "int vsg_render_level_colors(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, const uint8_t* bgr, size_t stride, int mem_in, "
            "vsg_render_level_color* colors, size_t capacity_colors, size_t* num_colors, int mem_out);",
            "int vsg_render_mean_frame(vsg_render* h, const uint8_t* seg, size_t seg_len, int level, "
            "int connectedness, const uint8_t* bgr, size_t stride, int mem_in, "
            "uint8_t* out, size_t out_stride, int mem_out);",
            "int vsg_render_last_color_stats(vsg_render* h, vsg_render_color_stats* s);",
            "int vsg_render_volume_begin(vsg_render* h, int level, int with_colors, int with_labels);",
            "int vsg_render_last_stats(vsg_render* h, vsg_render_stats* s);"):
        assert text in header, text


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in NAMES:
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    vp, psz, ss = C.c_void_p, C.POINTER(C.c_size_t), C.c_ssize_t
    assert C.sizeof(ss) == C.sizeof(C.c_void_p)          # ptrdiff_t
    assert L.vsg_render_level_pool.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_int, C.c_int,
                                                ss, ss, ss, C.c_int, vp, vp, vp, vp, vp, C.c_size_t, psz, C.c_int]
    assert L.vsg_render_level_unpool.argtypes == [vp, C.c_char_p, C.c_size_t, C.c_int, C.c_int, vp, C.c_size_t,
                                                  C.c_int, C.c_int, C.c_float, vp, C.c_int, ss, ss, ss, C.c_int]
    assert L.vsg_render_last_pool_stats.argtypes == [vp, C.POINTER(render.VsgRenderPoolStats)]
    for method in ("level_pool", "level_unpool", "last_pool_stats"):
        assert hasattr(render.SegmentationRenderer, method)
    assert callable(render.pool_moments) and callable(render.region_pool)
    assert (render.POOL_F32, render.POOL_F16, render.POOL_BF16) == (0, 1, 2)


def test_struct_layouts():
    from video_segment_amd import render
    import level_pool_model as pm
    s = render.VsgRenderPoolStats
    assert [n for n, _ in s._fields_] == ["groups", "intervals", "covered", "largest_group_intervals",
                                          "feature_bytes", "plane_us", "sums_us", "table_us", "paint_us", "launches"]
    assert C.sizeof(s) == 64
    assert [getattr(s, n).offset for n, _ in s._fields_] == [0, 8, 16, 24, 32, 40, 44, 48, 52, 56]
    d = render.POOL_GROUP_DTYPE
    assert d == pm.GROUP_DTYPE and d.itemsize == 16 and render.POOL_GROUP_WORDS == 4
    assert {n: d.fields[n][1] for n in d.names} == {"id": 0, "component": 4, "area": 8, "reserved": 12}


def test_pool_moments():
    from video_segment_amd import render
    g = np.zeros(2, render.POOL_GROUP_DTYPE)
    g["area"] = [4, 1]
    mean, var = render.pool_moments(g, np.array([[4.0, 8.0, 2.0], [9.0, 0.0, -255.0]]),
                                    np.array([[4.0, 24.0, 2.0], [81.0, 0.0, 255.0 * 255.0]]))
    assert mean.dtype == var.dtype == np.float64
    assert mean.tolist() == [[1.0, 2.0, 0.5], [9.0, 0.0, -255.0]]
    assert var.tolist() == [[0.0, 2.0, 0.25], [0.0, 0.0, 0.0]]


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    n = C.c_size_t(77)
    feat = (C.c_float * 64)()
    out = (C.c_float * 64)()
    vals = (C.c_float * 4)()
    PLANAR, LAST = (16, 4, 1), (1, 16, 4)          # chan, row, pixel strides of 4 channels of 4 x 4

    def pool(handle, features, count, connect=0, dtype=0, channels=4, strides=PLANAR, mem_in=0, mem_out=0):
        return L.vsg_render_level_pool(handle, b"", 0, 0, connect, features, dtype, channels, *strides, mem_in,
                                       None, None, None, None, None, 0, count, mem_out)

    def unpool(handle, values, dst, connect=0, dtype=0, channels=4, strides=PLANAR, mem_in=0, mem_out=0):
        return L.vsg_render_level_unpool(handle, b"", 0, 0, connect, values, 1, channels, mem_in, 0.0, dst, dtype,
                                         *strides, mem_out)

    def refused(rc, word):
        return rc == -1 and word in L.vsg_render_last_error()

    assert refused(pool(None, feat, C.byref(n)), b"null") and n.value == 0
    assert refused(unpool(None, vals, out), b"null")
    # everything below is looked at before a non-null handle is dereferenced
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    assert refused(pool(fake, feat, None), b"count")
    assert refused(pool(fake, None, C.byref(n)), b"features is null")
    assert refused(unpool(fake, vals, None), b"out is null")
    assert refused(unpool(fake, None, out), b"values is null")
    for strides in (PLANAR, LAST):
        for dtype in (3, -1, 16):
            assert refused(pool(fake, feat, C.byref(n), dtype=dtype, strides=strides), b"dtype")
            assert refused(unpool(fake, vals, out, dtype=dtype, strides=strides), b"dtype")
        for channels in (0, 65536, -3):
            assert refused(pool(fake, feat, C.byref(n), channels=channels, strides=strides), b"channels")
            assert refused(unpool(fake, vals, out, channels=channels, strides=strides), b"channels")
        for mem in (2, -1, 7):
            assert refused(pool(fake, feat, C.byref(n), strides=strides, mem_in=mem), b"mem_in")
            assert refused(pool(fake, feat, C.byref(n), strides=strides, mem_out=mem), b"mem_out")
            assert refused(unpool(fake, vals, out, strides=strides, mem_in=mem), b"mem_in")
            assert refused(unpool(fake, vals, out, strides=strides, mem_out=mem), b"mem_out")
        for connect in (3, -1, 4):
            assert refused(pool(fake, feat, C.byref(n), connect=connect, strides=strides), b"connectedness")
            assert refused(unpool(fake, vals, out, connect=connect, strides=strides), b"connectedness")
    # neither layout: the pixel stride is not 1 and the channel stride is not 1, or the pixels are too close
    for strides in ((16, 8, 2), (2, 16, 4), (1, 16, 3), (1, 4, 2), (0, 8, 2)):
        assert refused(pool(fake, feat, C.byref(n), strides=strides), b"neither planar")
        assert refused(unpool(fake, vals, out, strides=strides), b"neither planar")
    for strides in ((-16, 4, 1), (16, -4, 1), (16, 4, -1), (1, -16, 4), (-1, 16, 4)):
        assert refused(pool(fake, feat, C.byref(n), strides=strides), b"negative")
        assert refused(unpool(fake, vals, out, strides=strides), b"negative")
    # a 16-bit map at an odd address, a 32-bit one off by two bytes
    odd = C.cast(C.addressof(feat) + 1, C.c_void_p)
    assert refused(pool(fake, odd, C.byref(n), dtype=1), b"aligned")
    assert refused(pool(fake, C.cast(C.addressof(feat) + 2, C.c_void_p), C.byref(n), dtype=0), b"aligned")
    assert refused(unpool(fake, vals, odd, dtype=2), b"aligned")
    assert L.vsg_render_last_pool_stats(None, None) == -1
    s = render.VsgRenderPoolStats()
    assert L.vsg_render_last_pool_stats(None, C.byref(s)) == -1
    assert L.vsg_render_last_pool_stats(fake, None) == -1


def test_python_refuses_what_fits_neither_layout_without_a_copy():
    from video_segment_amd import render

    class Shell(render.SegmentationRenderer):
        def __init__(self, W, H):
            self.W, self.H, self.h = W, H, None

    r = Shell(6, 4)
    base = np.zeros((3, 4, 12), np.float32)
    ok = r._feature_layout(base[:, :, :6], "features")
    assert ok[1:6] == (render.POOL_F32, 3, 48, 12, 1)                    # a row-sliced planar view
    last = np.zeros((4, 6, 5), np.float16)[:, :, :3].transpose(2, 0, 1)
    assert r._feature_layout(last, "features")[1:6] == (render.POOL_F16, 3, 1, 30, 5)
    assert r._feature_layout(np.zeros((4, 6), np.float32), "features")[2] == 1
    assert r._feature_layout(np.zeros((2, 4, 6), np.uint16), "features", "bf16")[1] == render.POOL_BF16
    for bad in (base[:, :, ::2],                                       # x stride 2, channel stride 48
                np.zeros((3, 4, 6), np.float32)[:, :, ::-1],           # negative
                np.zeros((6, 4, 3), np.float32).transpose(2, 1, 0)):   # x-major
        with pytest.raises(ValueError):
            r._feature_layout(bad, "features")
    with pytest.raises(TypeError):
        r._feature_layout(np.zeros((3, 4, 6), np.float64), "features")
    with pytest.raises(TypeError):
        r._feature_layout(np.zeros((3, 4, 6), np.uint16), "features")
    with pytest.raises(ValueError):
        r._feature_layout(np.zeros((3, 4, 7), np.float32), "features")
