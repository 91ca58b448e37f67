"""The tree cut additions to the renderer's C ABI: vsg_render_tree_cut, vsg_render_tree_cut_tuning and
vsg_render_last_cut_stats are declared in include/vsg_render.h with the documented signatures and structs,
exported by libvsg_render.so and bound by the Python layer with matching layouts.  Needs no device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("vsg_render_tree_cut", "vsg_render_tree_cut_tuning", "vsg_render_last_cut_stats")


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
    assert ("int vsg_render_tree_cut(vsg_render* h, const uint8_t* seg, size_t seg_len, "
            "const int32_t* labels, size_t labels_pitch, int mem_labels, int64_t penalty, "
            "const vsg_render_cut_gain* gains, size_t num_gains, int mem_gains, "
            "vsg_render_cut_node* nodes, size_t capacity_nodes, size_t* num_nodes, "
            "int32_t* plane, int64_t* total, int mem_out);") in header
    assert "int vsg_render_tree_cut_tuning(vsg_render* h, int64_t block_nodes);" in header
    assert "int vsg_render_last_cut_stats(vsg_render* h, vsg_render_cut_stats* s);" in header
    assert fields_of(header, "vsg_render_cut_gain") == ["int32_t level, id", "int64_t gain"]
    assert fields_of(header, "vsg_render_cut_node") == [
        "int32_t level, id, area, leaves, children, best_label, best_count, reserved", "int64_t gain, split_value"]
    assert fields_of(header, "vsg_render_cut_stats") == [
        "int64_t levels, leaves, tree_nodes, pairs, entries, cut_nodes, covered, total, block_nodes",
        "float plane_us, table_us, lift_us, dp_us, paint_us", "int dp_path, dp_launches, launches"]


def test_header_states_the_definition(raw_header):
    text = re.sub(r"[\s*]+", " ", raw_header)
    for phrase in ("Hierarchy, height L, ancestors A_l(r).", "Nodes.", "Gain g(n), int64.", "The cut.",
                   "Consequences.", "Size.", "Two DP paths.",
                   "Exactly those of the persistence calls",
                   "L > 65535 is VSG_ERR_INVALID",
                   "A node with one child has that child's pixels",
                   "Exactly one of two sources is given; both, or neither, is VSG_ERR_INVALID",
                   "ties go to the smallest label",
                   "g(n) = best(n) - penalty, 0 <= penalty <= 2^32",
                   "refused before the handle is dereferenced",
                   "strictly ascending by (level, id), |gain| <= 2^32",
                   "the check runs on the device, and no output is touched",
                   "Entries that name no node of this frame are ignored; nodes not listed have gain 0",
                   "keep(n) <=> g(n) >= S(n) -- a tie keeps the coarser node -- and opt(n) = max(g(n), S(n))",
                   "Leaves always keep",
                   "the first kept node met when descending from the top",
                   "it equals the sum of opt over the top-level nodes",
                   "the cut is the coarsest partition that reaches it",
                   "With a penalty above every best(n) the cut is the top level",
                   "the cuts are nested",
                   "one record per selected node, ascending by (level, id)",
                   "split_value = S(n), 0 where children == 0",
                   "-1 where the level-0 id image is -1; NULL means not wanted and not painted",
                   "num_nodes and total are set on VSG_OK and when the capacity is too small",
                   "asks for the count and the total only",
                   "L R + L P > 2^27 is VSG_ERR_INVALID; the message names L, R and P",
                   "0: always per level. INT64_MAX: always one workgroup. -1: the default",
                   "dp_path: 0 not run (no node), 1 one workgroup, 2 per level",
                   "dp_launches: 1 on the one-workgroup path, L on the per-level path",
                   "on the one-workgroup path it does not depend on L"):
        assert phrase in text, phrase


def test_library_exports_and_python_binds_them():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    for name in NAMES:
        assert name in render.EXPORTED_SYMBOLS
        assert hasattr(L, name), name
    vp, psz = C.c_void_p, C.POINTER(C.c_size_t)
    assert L.vsg_render_tree_cut.argtypes == [vp, C.c_char_p, C.c_size_t, vp, C.c_size_t, C.c_int, C.c_int64, vp,
                                              C.c_size_t, C.c_int, vp, C.c_size_t, psz, vp, C.POINTER(C.c_int64),
                                              C.c_int]
    assert L.vsg_render_tree_cut_tuning.argtypes == [vp, C.c_int64]
    assert L.vsg_render_last_cut_stats.argtypes == [vp, C.POINTER(render.VsgRenderCutStats)]
    for method in ("tree_cut", "tree_cut_tuning", "last_cut_stats"):
        assert hasattr(render.SegmentationRenderer, method)
    assert callable(render.cut_scores) and callable(render.tree_cut_for_count)
    assert render.CUT_MAX_PENALTY == 1 << 32 and render.CUT_BLOCK_ALWAYS == (1 << 63) - 1


def test_struct_layouts():
    from video_segment_amd import render
    import tree_cut_model as tm
    s = render.VsgRenderCutStats
    assert [n for n, _ in s._fields_] == ["levels", "leaves", "tree_nodes", "pairs", "entries", "cut_nodes", "covered",
                                          "total", "block_nodes", "plane_us", "table_us", "lift_us", "dp_us",
                                          "paint_us", "dp_path", "dp_launches", "launches"]
    assert C.sizeof(s) == 104
    assert [getattr(s, n).offset for n, _ in s._fields_] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 72, 76, 80, 84, 88, 92,
                                                             96, 100]
    d = render.CUT_NODE_DTYPE
    assert d == tm.NODE_DTYPE and d.itemsize == 48 and render.CUT_NODE_WORDS == 12
    assert {n: d.fields[n][1] for n in d.names} == {"level": 0, "id": 4, "area": 8, "leaves": 12, "children": 16,
                                                    "best_label": 20, "best_count": 24, "reserved": 28, "gain": 32,
                                                    "split_value": 40}
    g = render.CUT_GAIN_DTYPE
    assert g == tm.GAIN_DTYPE and g.itemsize == 16 and render.CUT_GAIN_WORDS == 4
    assert {n: g.fields[n][1] for n in g.names} == {"level": 0, "id": 4, "gain": 8}


def test_cut_scores():
    from video_segment_amd import render
    nodes = np.zeros(3, render.CUT_NODE_DTYPE)
    nodes["level"] = [0, 2, 2]
    nodes["best_count"] = [(1 << 31) - 1, (1 << 31) - 1, 5]
    assert render.cut_scores(nodes) == {"nodes": 3, "best_sum": (1 << 32) + 3, "per_level": {0: 1, 2: 2}}
    assert render.cut_scores(nodes[:0]) == {"nodes": 0, "best_sum": 0, "per_level": {}}


def test_null_and_bad_arguments_are_answered_without_a_device():
    from video_segment_amd import render
    render.build()
    L = render.lib()
    labels = (C.c_int32 * 16)()
    gains = (C.c_int64 * 2)()
    n, total = C.c_size_t(77), C.c_int64(77)

    def cut(handle, labels=labels, gains=None, penalty=0, count=n, tot=total, mem_labels=0, mem_gains=0, mem_out=0):
        return L.vsg_render_tree_cut(handle, b"", 0, labels, 0, mem_labels, penalty, gains, 1 if gains else 0,
                                     mem_gains, None, 0, C.byref(count) if count is not None else None, None,
                                     C.byref(tot) if tot is not None else None, mem_out)

    def refused(rc, word):
        return rc == -1 and word in L.vsg_render_last_error()

    assert refused(cut(None), b"null") and n.value == 77
    # everything below is looked at before a non-null handle is dereferenced
    fake = C.cast(C.create_string_buffer(8), C.c_void_p)
    for penalty in (-1, (1 << 32) + 1, -(1 << 63), (1 << 63) - 1):
        assert refused(cut(fake, penalty=penalty), b"penalty")
        assert refused(cut(None, penalty=penalty), b"penalty")
        assert refused(cut(fake, labels=None, gains=gains, penalty=penalty), b"penalty")
    assert refused(cut(fake, gains=gains), b"both")
    assert refused(cut(fake, labels=None), b"neither")
    assert refused(cut(fake, count=None), b"count")
    assert refused(cut(fake, tot=None), b"count")
    for mem in (2, -1, 7):
        assert refused(cut(fake, mem_labels=mem), b"memory kind")
        assert refused(cut(fake, labels=None, gains=gains, mem_gains=mem), b"memory kind")
        assert refused(cut(fake, mem_out=mem), b"memory kind")
    assert n.value == 0 and total.value == 0
    assert L.vsg_render_tree_cut_tuning(None, 0) == -1
    assert L.vsg_render_last_cut_stats(None, None) == -1
    s = render.VsgRenderCutStats()
    assert L.vsg_render_last_cut_stats(None, C.byref(s)) == -1
    assert L.vsg_render_last_cut_stats(fake, None) == -1
