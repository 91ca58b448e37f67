"""CPU-side checks of libvsg_resize.so: it exports exactly what include/vsg_resize.h declares, its
host-only calls (the reader's size rule and the filter tables the kernels use) equal the model
tests/resize_model.py bit for bit, arguments are checked, and it refuses to run without a GPU."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import resize_model as rm
from resize_cases import FILTER_CASES, SIZE_TABLE
from video_segment_amd import resize

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def library():
    resize.build()
    return resize.lib()


def test_header_symbols_exported(library):
    header = open(os.path.join(ROOT, "include", "vsg_resize.h")).read()
    declared = set(re.findall(r"\b(vsg_resize_[a-z0-9_]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(resize.EXPORTED_SYMBOLS)
    for name in declared:
        assert hasattr(library, name), name
    out = subprocess.check_output(["nm", "-D", "--defined-only", resize.LIB_PATH], text=True)
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("vsg_")}
    assert exported == set(resize.EXPORTED_SYMBOLS)


def test_constants_match_the_model(library):
    assert (resize.DOWNSCALE_NONE, resize.DOWNSCALE_BY_FACTOR, resize.DOWNSCALE_TO_MIN_SIZE,
            resize.DOWNSCALE_TO_MAX_SIZE) == (rm.NONE, rm.BY_FACTOR, rm.TO_MIN_SIZE, rm.TO_MAX_SIZE)
    header = open(os.path.join(ROOT, "include", "vsg_resize.h")).read()
    assert int(re.search(r"#define VSG_RESIZE_MAX_TAPS_H (\d+)", header).group(1)) == resize.MAX_TAPS_H
    o = resize.default_resize_options()
    assert (o.mode, o.size, o.device) == (resize.DOWNSCALE_NONE, 0, -1) and o.factor == 0.5


@pytest.mark.parametrize("in_w,in_h,mode,size,out_w,out_h", SIZE_TABLE)
def test_output_size_table(library, in_w, in_h, mode, size, out_w, out_h):
    got = resize.output_size(mode, in_w, in_h, size=size)
    assert got[:2] == (out_w, out_h)
    assert got == rm.output_size(mode, in_w, in_h, size=size)


def test_output_size_by_factor_and_none(library):
    assert resize.output_size(resize.DOWNSCALE_BY_FACTOR, 97, 61, factor=0.5) == (50, 31, 152)
    assert resize.output_size(resize.DOWNSCALE_NONE, 96, 72) == (96, 72, 288)
    assert resize.output_size(resize.DOWNSCALE_NONE, 97, 61) == (98, 61, 296)
    rng = np.random.default_rng(11)
    for _ in range(300):    # the f32 path of the rule, wherever it rounds
        w, h, size = int(rng.integers(1, 4200)), int(rng.integers(1, 4200)), int(rng.integers(1, 800))
        for mode in (rm.TO_MIN_SIZE, rm.TO_MAX_SIZE):
            assert resize.output_size(mode, w, h, size=size) == rm.output_size(mode, w, h, size=size), (mode, w, h, size)
        factor = float(rng.uniform(0.05, 1.0))
        assert resize.output_size(rm.BY_FACTOR, w, h, factor=factor) == rm.output_size(rm.BY_FACTOR, w, h, factor=factor)


@pytest.mark.parametrize("args,message", [
    ((resize.DOWNSCALE_BY_FACTOR, 1.5, 0, 97, 61), b"Only downscaling is supported"),
    ((resize.DOWNSCALE_TO_MIN_SIZE, 1.0, 0, 97, 61), b"positive"),
    ((resize.DOWNSCALE_TO_MAX_SIZE, 1.0, -4, 97, 61), b"positive"),
    ((resize.DOWNSCALE_BY_FACTOR, 0.0, 0, 97, 61), b"empty"),
    ((resize.DOWNSCALE_BY_FACTOR, -1.0, 0, 97, 61), b"empty"),
    ((resize.DOWNSCALE_NONE, 1.0, 0, 0, 61), b"65535"),
    ((resize.DOWNSCALE_NONE, 1.0, 0, 97, 65536), b"65535"),
    ((9, 1.0, 0, 97, 61), b"mode"),
])
def test_output_size_rejects(library, args, message):
    w = C.c_int(-7)
    assert library.vsg_resize_output_size(*args, C.byref(w), None, None) == -1
    assert message in library.vsg_resize_last_error()
    assert w.value == -7


@pytest.mark.parametrize("n_in,n_out", FILTER_CASES)
def test_filter_tables_equal_the_model(library, n_in, n_out):
    first, count, weights = resize.filter_tables(n_in, n_out)
    m_first, m_count, m_weights = rm.filter_tables(n_in, n_out)
    assert weights.shape == m_weights.shape
    assert (first == m_first).all() and (count == m_count).all()
    assert (weights.view(np.uint32) == m_weights.view(np.uint32)).all()


def test_filter_arguments(library):
    taps = C.c_int(-1)
    assert library.vsg_resize_filter(97, 78, None, None, None, 0, C.byref(taps)) == 0 and taps.value == 5
    first, count = np.full(78, -5, np.int32), np.full(78, -5, np.int32)
    weights = np.full(78 * 5, 9.0, np.float32)
    p = (first.ctypes.data, count.ctypes.data, weights.ctypes.data)
    assert library.vsg_resize_filter(97, 78, *p, 78 * 5 - 1, C.byref(taps)) == -1     # one float short
    assert library.vsg_resize_filter(97, 78, p[0], None, p[2], 78 * 5, C.byref(taps)) == -1
    assert (first == -5).all() and (count == -5).all() and (weights == 9.0).all()
    assert library.vsg_resize_filter(97, 78, *p, 78 * 5, None) == -1
    for n_in, n_out in [(0, 4), (4, 0), (65536, 4), (4, 65536)]:
        assert library.vsg_resize_filter(n_in, n_out, *p, 78 * 5, C.byref(taps)) == -1
    assert library.vsg_resize_filter(97, 78, *p, 78 * 5, C.byref(taps)) == 0 and (count >= 4).all()


def _create(library, in_w, in_h, **kw):
    o = resize.default_resize_options(**kw)
    h = C.c_void_p()
    rc = library.vsg_resize_create(C.byref(o), in_w, in_h, C.byref(h))
    if rc == 0:
        library.vsg_resize_destroy(h)
    return rc


def test_create_checks_arguments_before_the_device(library):
    assert library.vsg_resize_create(None, 96, 72, None) == -1
    assert _create(library, 0, 72) == -1
    assert _create(library, 96, 65536) == -1
    assert _create(library, 96, 72, mode=resize.DOWNSCALE_BY_FACTOR, factor=1.25) == -1
    assert b"Only downscaling is supported" in library.vsg_resize_last_error()
    assert _create(library, 96, 72, mode=resize.DOWNSCALE_TO_MIN_SIZE, size=0) == -1
    # 8192 -> 16 columns: 2048 source pixels per output pixel, above the horizontal pass's limit
    assert _create(library, 8192, 4, mode=resize.DOWNSCALE_BY_FACTOR, factor=1.0 / 512) == -1
    assert b"ratio too large" in library.vsg_resize_last_error()
    # calls on a null handle
    s = resize.VsgResizeStats()
    assert library.vsg_resize_last_stats(None, C.byref(s)) == -1
    assert library.vsg_resize_get_output_size(None, None, None, None) == -1
    buf = np.zeros(16, np.uint8)
    assert library.vsg_resize_process(None, buf.ctypes.data, 6, 0, buf.ctypes.data, 6, 0) == -1
    library.vsg_resize_destroy(None)


def test_last_error_is_each_librarys_own(library):
    """The three libraries compile the same support header and are loaded into one process: a failure
    in one must not replace the text the others return for this thread."""
    from video_segment_amd import flow, render
    flow.build()
    render.build()
    h = C.c_void_p()
    assert _create(library, 96, 72, mode=resize.DOWNSCALE_BY_FACTOR, factor=1.25) == -1
    o = flow.default_flow_options(iterations=0)
    assert flow.lib().vsg_flow_create(C.byref(o), 96, 72, C.byref(h)) == -1 and not h.value
    o = render.default_render_options(hierarchy_level=-1.0)
    assert render.lib().vsg_render_create(C.byref(o), 96, 72, C.byref(h)) == -1 and not h.value
    for _ in range(2):   # reading one does not disturb another
        assert library.vsg_resize_last_error() == b"Only downscaling is supported."
        assert flow.lib().vsg_flow_last_error() == b"iterations has to be in [1, 1000]"
        assert render.lib().vsg_render_last_error() == b"bad hierarchy_level"


def test_no_cpu_fallback(library):
    """Without a HIP device vsg_resize_create must fail with VSG_ERR_DEVICE."""
    from video_segment_amd import _lib
    if _lib.lib().vsg_device_count() > 0:
        pytest.skip("a GPU is present")
    assert _create(library, 96, 72, mode=resize.DOWNSCALE_TO_MAX_SIZE, size=48) == -2
    assert b"no usable HIP device" in library.vsg_resize_last_error()
