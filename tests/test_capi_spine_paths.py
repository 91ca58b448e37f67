"""The tree replay's path counters across the C ABI: the ctypes mirror VsgSpinePaths has the fields of
vsg_spine_paths (include/vsg.h) in the header's order and with its types, and the library exports both
getters.  No GPU needed."""
import ctypes as C
import os
import re

import pytest

from video_segment_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_struct_fields(name):
    """[(field, array length or None)] of `typedef struct <name> { int64_t ...; } <name>;` in vsg.h."""
    header = open(os.path.join(ROOT, "include", "vsg.h")).read()
    m = re.search(r"typedef\s+struct\s+%s\s*\{(.*?)\}\s*%s\s*;" % (name, name), header, re.S)
    assert m, "struct %s not found in include/vsg.h" % name
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        d = re.fullmatch(r"int64_t\s+(.+)", decl, re.S)
        assert d, "not an int64_t declaration: %r" % decl
        for item in d.group(1).split(","):
            f = re.fullmatch(r"\s*([a-z_][a-z0-9_]*)\s*(?:\[(\d+)\])?\s*", item)
            assert f, "cannot parse %r" % item
            fields.append((f.group(1), int(f.group(2)) if f.group(2) else None))
    return fields


def mirror_fields(struct):
    out = []
    for name, t in struct._fields_:
        if issubclass(t, C.Array):
            assert t._type_ is C.c_int64, name
            out.append((name, t._length_))
        else:
            assert t is C.c_int64, name
            out.append((name, None))
    return out


def test_parser_reads_arrays_and_order():
    """The parser itself, on the struct the suite has relied on since the merge paths were added."""
    f = header_struct_fields("vsg_merge_paths")
    assert f[0] == ("hub_stages", None) and ("hub_reasons", 6) in f and f[-1] == ("conservative_replays", None)
    assert f == mirror_fields(_lib.VsgMergePaths)


def test_spine_paths_mirror_matches_header():
    declared = header_struct_fields("vsg_spine_paths")
    mirrored = mirror_fields(_lib.VsgSpinePaths)
    assert declared == mirrored, "vsg_spine_paths and VsgSpinePaths differ:\n%s\n%s" % (declared, mirrored)
    assert C.sizeof(_lib.VsgSpinePaths) == 8 * sum(n or 1 for _, n in declared)
    # the counters the tests of the tree replay rely on
    names = dict(declared)
    for k in ("replays", "components", "nested_replays", "deepest_level", "forest_rounds", "forest_rounds_ahead",
              "forest_compactions_ahead", "forest_compactions_sync", "forest_lists_refused", "ranked_by_sampling",
              "ranked_plain", "rank_sampling_refused", "jump_loops_ended_early", "streamed_passes",
              "streamed_refused", "top_level_fallbacks", "nested_fallbacks", "assumption_reruns",
              "limit_bucket_moves", "zero_pool_flips", "windows_run", "rle_stages", "wide_launches"):
        assert k in names and names[k] is None, k
    assert names["pool_fallbacks"] == 4 and names["low_bucket_failures"] == 2 and names["low_bucket_skips"] == 2


def test_mirror_check_notices_a_field_on_one_side_only():
    """A field added to the header alone (or to the mirror alone) makes the comparison fail."""
    declared = header_struct_fields("vsg_spine_paths")
    mirrored = mirror_fields(_lib.VsgSpinePaths)
    assert declared + [("new_counter", None)] != mirrored
    assert declared != mirrored[:-1]
    assert declared[::-1] != mirrored   # (and the order counts)


def test_getters_exported_and_refuse_null():
    _lib.build()
    L = _lib.lib()
    for name in ("vsg_stream_last_spine_paths", "vsg_graph_spine_paths"):
        assert name in _lib.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    out = _lib.VsgSpinePaths()
    assert L.vsg_stream_last_spine_paths(None, C.byref(out)) == -1   # VSG_ERR_INVALID
    assert L.vsg_graph_spine_paths(None, C.byref(out)) == -1
