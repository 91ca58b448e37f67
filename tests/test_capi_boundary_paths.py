"""The chunk boundary's path counters across the C ABI: the ctypes mirror VsgBoundaryPaths has the fields
of vsg_boundary_paths (include/vsg.h) in the header's order and with its types, and the library exports
the getter.  No GPU needed."""
import ctypes as C

from test_capi_spine_paths import header_struct_fields, mirror_fields
from video_segment_amd import _lib


def test_boundary_paths_mirror_matches_header():
    declared = header_struct_fields("vsg_boundary_paths")
    mirrored = mirror_fields(_lib.VsgBoundaryPaths)
    assert declared == mirrored, "vsg_boundary_paths and VsgBoundaryPaths differ:\n%s\n%s" % (declared, mirrored)
    assert C.sizeof(_lib.VsgBoundaryPaths) == 8 * len(declared)
    assert [k for k, _ in declared] == ["halo_planes_in_pool"]


def test_getter_exported_and_refuses_null():
    _lib.build()
    L = _lib.lib()
    assert "vsg_stream_last_boundary_paths" in _lib.EXPORTED_SYMBOLS
    assert hasattr(L, "vsg_stream_last_boundary_paths")
    out = _lib.VsgBoundaryPaths()
    assert L.vsg_stream_last_boundary_paths(None, C.byref(out)) == -1   # VSG_ERR_INVALID
