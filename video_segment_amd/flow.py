"""Python host layer of the dense flow unit (C ABI: include/vsg_flow.h, libvsg_flow.so).

``DenseFlow`` mirrors the reference's LuminanceUnit -> DenseFlowUnit pair (conversion_units.cpp:75-105,
flow_reader.cpp:226-371) without its stream plumbing: BGR24 (or 8-bit luminance) frames go in, the
Dual TV-L1 flow from each frame to its predecessor (and / or successor) comes out, as numpy arrays or
as device pointers that ``DenseSegmentation.process_frame`` takes with device memory.  All per-pixel
work happens in the HIP library; there is no Python or CPU fallback.  tests/flow_model.py defines
the arithmetic.
"""
import ctypes as C

import numpy as np

from . import _capi
from ._lib import VSG_MEM_DEVICE, VSG_MEM_HOST, VSG_OK, VsgError  # noqa: F401 (part of the module)

LIB_PATH = _capi.lib_path("vsg_flow")

FLOW_BACKWARD, FLOW_FORWARD, FLOW_BOTH = 0, 1, 2


class VsgFlowOptions(_capi.Structure):
    _fields_ = [("flow_type", C.c_int), ("iterations", C.c_int), ("warps", C.c_int), ("device", C.c_int)]


class VsgFlowStats(_capi.Structure):
    _fields_ = [
        ("scales", C.c_int), ("launches", C.c_int), ("iterations_run", C.c_int), ("host_syncs", C.c_int),
        ("device_allocations", C.c_int64),
        ("pyramid_us", C.c_float), ("warp_us", C.c_float), ("iterate_us", C.c_float), ("export_us", C.c_float),
    ]


# Every symbol include/vsg_flow.h declares.
EXPORTED_SYMBOLS = [
    "vsg_flow_last_error", "vsg_flow_default_options", "vsg_flow_create", "vsg_flow_destroy",
    "vsg_flow_process_frame", "vsg_flow_process_luminance", "vsg_flow_restart", "vsg_flow_last_stats",
    "vsg_flow_luminance",
]


def build(force=False):
    """Compiles libvsg_flow.so in-tree (hipcc --offload-arch=gfx950); make decides what is stale."""
    _capi.make("flow", force)
    return LIB_PATH


_handle = None


def lib():
    global _handle
    if _handle is not None:
        return _handle
    L = _capi.load(LIB_PATH, "libvsg_flow.so")
    vp = C.c_void_p
    L.vsg_flow_last_error.restype = C.c_char_p
    L.vsg_flow_default_options.argtypes = [C.POINTER(VsgFlowOptions)]
    L.vsg_flow_default_options.restype = None
    L.vsg_flow_create.argtypes = [C.POINTER(VsgFlowOptions), C.c_int, C.c_int, C.POINTER(vp)]
    L.vsg_flow_destroy.argtypes = [vp]
    L.vsg_flow_destroy.restype = None
    for f in (L.vsg_flow_process_frame, L.vsg_flow_process_luminance):
        f.argtypes = [vp, vp, C.c_size_t, C.c_int, vp, vp, C.c_int, C.POINTER(C.c_int)]
    L.vsg_flow_restart.argtypes = [vp]
    L.vsg_flow_last_stats.argtypes = [vp, C.POINTER(VsgFlowStats)]
    L.vsg_flow_luminance.argtypes = [vp, C.c_size_t, C.c_int, C.c_int, vp]
    _handle = L
    return L


check = _capi.checker("vsg_flow", lambda: lib().vsg_flow_last_error())


def default_flow_options(**kw):
    return _capi.default_options(VsgFlowOptions, lib().vsg_flow_default_options, "flow", **kw)


def luminance(bgr):
    """H x W uint8 luminance of an H x W x 3 BGR frame (packed pixels, rows may be padded).  Host only."""
    H, W = bgr.shape[:2]
    if bgr.dtype != np.uint8 or bgr.shape[2:] != (3,) or bgr.strides[2] != 1 or bgr.strides[1] != 3:
        raise ValueError("bgr has to be H x W x 3 uint8 with packed pixels")
    out = np.empty((H, W), np.uint8)
    check(lib().vsg_flow_luminance(bgr.ctypes.data_as(C.c_void_p), bgr.strides[0], W, H,
                                   out.ctypes.data_as(C.c_void_p)))
    return out


class DenseFlow(_capi.Handle):
    """Dual TV-L1 flow between consecutive frames on one MI355X.

    options: flow_type (FLOW_BACKWARD), iterations (10), warps (2), device (-1).  The first frame
    after construction or restart() has no flow: the process calls return None for it."""

    def __init__(self, width, height, **options):
        self.W, self.H = width, height
        self.opts = default_flow_options(**options)
        h = C.c_void_p()
        check(lib().vsg_flow_create(C.byref(self.opts), width, height, C.byref(h)))
        self.h = h
        self._destroy = lib().vsg_flow_destroy
        self._dev_out = None

    def close(self):
        super().close()
        self._dev_out = None

    def restart(self):
        check(lib().vsg_flow_restart(self.h))

    def _input(self, frame):
        """(pointer, row stride, mem kind, entry point) of an H x W x 3 or H x W uint8 frame."""
        bgr = len(frame.shape) == 3
        fn = lib().vsg_flow_process_frame if bgr else lib().vsg_flow_process_luminance
        expected = "%d x %d x 3 (BGR) or %d x %d (luminance)" % (self.H, self.W, self.H, self.W)
        return _capi.frame_ptr(frame, self.H, self.W, 3 if bgr else 1, "frame", expected) + (fn,)

    def _which(self):
        t = self.opts.flow_type
        return t != FLOW_FORWARD, t != FLOW_BACKWARD

    def process_frame(self, frame):
        """The flow of this frame as H x W x 2 f32 numpy (x, y): backward (to the previous frame) or
        forward (previous frame to this one) as flow_type says, a (backward, forward) pair for
        FLOW_BOTH; None for the first frame."""
        p, stride, mem_in, fn = self._input(frame)
        want_b, want_f = self._which()
        b = np.empty((self.H, self.W, 2), np.float32) if want_b else None
        f = np.empty((self.H, self.W, 2), np.float32) if want_f else None
        has = C.c_int()
        check(fn(self.h, p, stride, mem_in, b.ctypes.data_as(C.c_void_p) if want_b else None,
                 f.ctypes.data_as(C.c_void_p) if want_f else None, VSG_MEM_HOST, C.byref(has)))
        if not has.value:
            return None
        return (b, f) if want_b and want_f else (b if want_b else f)

    def process_frame_device(self, frame):
        """The same, left on the device: an H x W x 2 f32 torch CUDA tensor (a pair for FLOW_BOTH)
        owned by this object and overwritten by the next call; None for the first frame.  It can be
        handed to DenseSegmentation.process_frame as the flow of a device frame."""
        import torch
        p, stride, mem_in, fn = self._input(frame)
        want_b, want_f = self._which()
        if self._dev_out is None:
            dev = torch.device("cuda", self.opts.device if self.opts.device >= 0 else torch.cuda.current_device())
            self._dev_out = torch.empty((2, self.H, self.W, 2), dtype=torch.float32, device=dev)
            torch.cuda.current_stream(dev).synchronize()
        b, f = self._dev_out[0], self._dev_out[1]
        has = C.c_int()
        check(fn(self.h, p, stride, mem_in, C.c_void_p(b.data_ptr()) if want_b else None,
                 C.c_void_p(f.data_ptr()) if want_f else None, VSG_MEM_DEVICE, C.byref(has)))
        if not has.value:
            return None
        return (b, f) if want_b and want_f else (b if want_b else f)

    def last_stats(self):
        """vsg_flow_last_stats of the last process call, as a dict."""
        s = VsgFlowStats()
        check(lib().vsg_flow_last_stats(self.h, C.byref(s)))
        return s.as_dict()
