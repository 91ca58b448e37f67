"""Python host layer of the downscale stage (C ABI: include/vsg_resize.h, libvsg_resize.so).

``Downscaler`` mirrors the scaling of the reference's reader (VideoReaderOptions::downscale,
video_reader_unit.cpp:155-206): BGR24 frames go in, the downscaled frame comes out, as a numpy array
or as a device tensor that ``DenseFlow.process_frame_device`` and ``DenseSegmentation.process_frame``
take as they are.  All per-pixel work happens in the HIP library; there is no Python or CPU fallback.
The output size is the reference's rule; the resampling is defined by tests/resize_model.py (parity
with swscale is unpinned).
"""
import ctypes as C

import numpy as np

from . import _capi
from ._lib import VSG_MEM_DEVICE, VSG_MEM_HOST, VSG_OK, VsgError  # noqa: F401 (part of the module)

LIB_PATH = _capi.lib_path("vsg_resize")

DOWNSCALE_NONE, DOWNSCALE_BY_FACTOR, DOWNSCALE_TO_MIN_SIZE, DOWNSCALE_TO_MAX_SIZE = 0, 1, 2, 3
MAX_TAPS_H = 1024


class VsgResizeOptions(_capi.Structure):
    _fields_ = [("mode", C.c_int), ("factor", C.c_float), ("size", C.c_int), ("device", C.c_int)]


class VsgResizeStats(_capi.Structure):
    _fields_ = [
        ("launches", C.c_int), ("host_syncs", C.c_int), ("taps_h", C.c_int), ("taps_v", C.c_int),
        ("device_allocations", C.c_int64),
        ("upload_us", C.c_float), ("horizontal_us", C.c_float), ("vertical_us", C.c_float),
        ("download_us", C.c_float), ("copy_us", C.c_float),
    ]


# Every symbol include/vsg_resize.h declares.
EXPORTED_SYMBOLS = [
    "vsg_resize_last_error", "vsg_resize_default_options", "vsg_resize_output_size", "vsg_resize_filter",
    "vsg_resize_create", "vsg_resize_destroy", "vsg_resize_get_output_size", "vsg_resize_process",
    "vsg_resize_last_stats",
]


def build(force=False):
    """Compiles libvsg_resize.so in-tree (hipcc --offload-arch=gfx950); make decides what is stale."""
    _capi.make("resize", force)
    return LIB_PATH


_handle = None


def lib():
    global _handle
    if _handle is not None:
        return _handle
    L = _capi.load(LIB_PATH, "libvsg_resize.so")
    vp, ip = C.c_void_p, C.POINTER(C.c_int)
    L.vsg_resize_last_error.restype = C.c_char_p
    L.vsg_resize_default_options.argtypes = [C.POINTER(VsgResizeOptions)]
    L.vsg_resize_default_options.restype = None
    L.vsg_resize_output_size.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, ip, ip, ip]
    L.vsg_resize_filter.argtypes = [C.c_int, C.c_int, vp, vp, vp, C.c_size_t, ip]
    L.vsg_resize_create.argtypes = [C.POINTER(VsgResizeOptions), C.c_int, C.c_int, C.POINTER(vp)]
    L.vsg_resize_destroy.argtypes = [vp]
    L.vsg_resize_destroy.restype = None
    L.vsg_resize_get_output_size.argtypes = [vp, ip, ip, ip]
    L.vsg_resize_process.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, C.c_size_t, C.c_int]
    L.vsg_resize_last_stats.argtypes = [vp, C.POINTER(VsgResizeStats)]
    _handle = L
    return L


check = _capi.checker("vsg_resize", lambda: lib().vsg_resize_last_error())


def default_resize_options(**kw):
    return _capi.default_options(VsgResizeOptions, lib().vsg_resize_default_options, "resize", **kw)


def output_size(mode, in_w, in_h, size=0, factor=1.0):
    """(out_w, out_h, width_step) of the reader's size rule.  Host only."""
    w, h, step = C.c_int(), C.c_int(), C.c_int()
    check(lib().vsg_resize_output_size(mode, factor, size, in_w, in_h, C.byref(w), C.byref(h), C.byref(step)))
    return w.value, h.value, step.value


def filter_tables(n_in, n_out):
    """(first int32[n_out], count int32[n_out], weights f32[n_out, max_taps]) of one axis, the
    tables the kernels use: tap j of output o reads clamp(first[o] + j, 0, n_in - 1).  Host only."""
    taps = C.c_int()
    check(lib().vsg_resize_filter(n_in, n_out, None, None, None, 0, C.byref(taps)))
    first = np.zeros(n_out, np.int32)
    count = np.zeros(n_out, np.int32)
    weights = np.zeros((n_out, taps.value), np.float32)
    check(lib().vsg_resize_filter(n_in, n_out, first.ctypes.data, count.ctypes.data, weights.ctypes.data,
                                  weights.size, C.byref(taps)))
    return first, count, weights


class Downscaler(_capi.Handle):
    """The reader's downscale on one MI355X.

    mode: DOWNSCALE_NONE / BY_FACTOR (factor) / TO_MIN_SIZE / TO_MAX_SIZE (size).  ``out_size`` is
    (out_w, out_h); ``width_step`` the padded row size the reference gives the stream."""

    def __init__(self, in_w, in_h, mode=DOWNSCALE_TO_MIN_SIZE, size=360, factor=0.5, device=-1):
        self.W, self.H = in_w, in_h
        self.opts = default_resize_options(mode=mode, size=size, factor=factor, device=device)
        h = C.c_void_p()
        check(lib().vsg_resize_create(C.byref(self.opts), in_w, in_h, C.byref(h)))
        self.h = h
        self._destroy = lib().vsg_resize_destroy
        w, ht, step = C.c_int(), C.c_int(), C.c_int()
        check(lib().vsg_resize_get_output_size(h, C.byref(w), C.byref(ht), C.byref(step)))
        self.out_size = (w.value, ht.value)
        self.width_step = step.value
        self._dev_out = None

    def close(self):
        super().close()
        self._dev_out = None

    def _input(self, frame):
        """(pointer, row stride, mem kind) of an H x W x 3 uint8 frame with packed pixels."""
        return _capi.frame_ptr(frame, self.H, self.W, 3, "frame", "%d x %d x 3 (BGR)" % (self.H, self.W))

    def process_frame(self, frame):
        """The downscaled frame as out_h x out_w x 3 uint8 numpy."""
        p, stride, mem_in = self._input(frame)
        w, h = self.out_size
        out = np.empty((h, w, 3), np.uint8)
        check(lib().vsg_resize_process(self.h, p, stride, mem_in, out.ctypes.data_as(C.c_void_p), w * 3, VSG_MEM_HOST))
        return out

    def process_frame_device(self, frame):
        """The same, left on the device: an out_h x out_w x 3 uint8 torch CUDA tensor owned by this
        object and overwritten by the next call.  frame: numpy, or a torch tensor on either side."""
        import torch
        p, stride, mem_in = self._input(frame)
        w, h = self.out_size
        if self._dev_out is None:
            dev = torch.device("cuda", self.opts.device if self.opts.device >= 0 else torch.cuda.current_device())
            self._dev_out = torch.empty((h, w, 3), dtype=torch.uint8, device=dev)
            torch.cuda.current_stream(dev).synchronize()
        check(lib().vsg_resize_process(self.h, p, stride, mem_in, C.c_void_p(self._dev_out.data_ptr()), w * 3,
                                       VSG_MEM_DEVICE))
        return self._dev_out

    def last_stats(self):
        """vsg_resize_last_stats of the last process call, as a dict."""
        s = VsgResizeStats()
        check(lib().vsg_resize_last_stats(self.h, C.byref(s)))
        return s.as_dict()
