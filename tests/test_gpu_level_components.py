"""vsg_render_level_components on the MI355X (libvsg_render.so: the level pipeline's front half,
k_comp_link's union-find, the sort by component, k_comp_table, the moments kernel, the label fill)
against level_components_model.py.  Components, intervals and label images are compared as raw bytes,
the float fields as their uint32 patterns: there is no tolerance anywhere in this file."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import level_components_cases as cc
import level_components_model as cm
import level_regions_cases as lc
import level_regions_model as lm
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
CASES = cc.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODES = (cm.N4, cm.N8)


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert (render.N4, render.N8) == MODES
    return v


def assert_same(got, want, what):
    assert len(got) == len(want), what
    got_c, got_i = got[0], got[1]
    want_c, want_i = want[0], want[1]
    assert got_i.dtype == np.int32 and got_i.shape == want_i.shape, (what, got_i.shape, want_i.shape)
    assert lm.same_bits(got_i, want_i), what
    assert got_c.dtype == cm.COMPONENT_DTYPE and got_c.shape == want_c.shape, (what, got_c.shape, want_c.shape)
    for f in cm.COMPONENT_DTYPE.names:
        assert np.array_equal(got_c[f].view(np.uint32), want_c[f].view(np.uint32)), (what, f)
    assert lm.same_bits(got_c, want_c), what
    if len(want) == 3:
        assert got[2].dtype == np.int32 and lm.same_bits(got[2], want[2]), (what, "labels")


def check_ids(r, seg, ids, level, what):
    """Both connectednesses of one level against the sweep, with the label image and the counts."""
    out = {}
    for connect in MODES:
        stats = {}
        want = cm.sweep(ids, connect, stats)
        got = r.level_components(seg, level, connect, label_image=True)
        assert_same(got, want, (what, level, connect))
        assert np.array_equal(got[2] == -1, ids == -1)
        st = r.last_component_stats()
        assert st["runs"] == stats["runs"] == len(want[1]) and st["components"] == len(want[0])
        assert st["links"] == stats["links"] and st["links"] < 2 * max(st["runs"], 1)
        assert st["regions"] == len(np.unique(want[0]["id"]))
        assert st["largest_component_intervals"] == (want[0]["num_intervals"].max() if len(want[0]) else 0)
        # without the label image the lists are the same
        assert_same(r.level_components(seg, level, connect), want[:2], (what, level, connect, "lists only"))
        out[connect] = got
    return out


def check_case(vsg, case):
    r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    seg = case.msg.SerializeToString()
    out = {level: check_ids(r, seg, lc.id_image(case.msg, level), level, case.name) for level in case.levels}
    r.close()
    return out


@pytest.mark.parametrize("name", ["one_region_1x1", "one_region_7x1", "one_region_1x7", "one_region_9x5"])
def test_degenerate_frames_and_one_region(vsg, name):
    got = check_case(vsg, BY_NAME[name])[0]
    for connect in MODES:
        assert len(got[connect][0]) == 1 and got[connect][0]["region_components"].tolist() == [1]


@pytest.mark.parametrize("W", lc.BOUNDARY_WIDTHS)
def test_widths_around_wavefront_and_block_boundaries(vsg, W):
    for H in (1, 2, 3, 4, 5):
        check_case(vsg, BY_NAME["boundary_%dx%d" % (W, H)])


def test_uncovered_pixels_rows_and_frame(vsg):
    check_case(vsg, BY_NAME["uncovered"])
    c = BY_NAME["uncovered_frame"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    comps, intervals, labels = r.level_components(c.msg.SerializeToString(), 0, cm.N8, label_image=True)
    assert comps.shape == (0,) and comps.dtype == cm.COMPONENT_DTYPE and intervals.shape == (0, 4)
    assert labels.shape == (c.H, c.W) and (labels == -1).all()
    st = r.last_component_stats()
    assert st["runs"] == 0 and st["components"] == 0 and st["links"] == 0
    r.close()


def test_checker_where_the_two_modes_differ_most(vsg):
    got = check_case(vsg, BY_NAME["checker"])
    for connect in MODES:
        assert len(got[0][connect][0]) == 6144 and len(got[0][connect][1]) == 6144
    n4, n8 = got[1][cm.N4][0], got[1][cm.N8][0]
    assert len(n4) == 6144 and set(n4["region_components"].tolist()) == {3072}
    assert n4["id"].tolist() == [100] * 3072 + [101] * 3072 and n4["component"].tolist() == list(range(3072)) * 2
    assert len(n8) == 2 and n8["region_components"].tolist() == [1, 1] and n8["num_intervals"].tolist() == [3072, 3072]


@pytest.mark.parametrize("name", ["serpentine", "spiral", "comb_up", "comb_down"])
def test_long_union_chains(vsg, name):
    """One component whose runs are linked end to end, and combs whose teeth join in their last row
    (pointing up) or their first (pointing down).  When labels merge cannot be seen in the result: what is
    checked is the result, bytes against the sweep, and that there is one component of all the runs."""
    got = check_case(vsg, BY_NAME[name])[0]
    for connect in MODES:
        assert len(got[connect][0]) == 1
        assert got[connect][0]["num_intervals"][0] == {"serpentine": 2113, "spiral": 1057}.get(name, 257)


@pytest.mark.parametrize("name", ["fan_down", "fan_up", "fan_offset", "fan_diagonal"])
def test_fan_out_in_one_row_pair(vsg, name):
    got = check_case(vsg, BY_NAME[name])[0]
    assert len(got[cm.N8][0]) == 1
    assert len(got[cm.N4][0]) == (256 if name == "fan_diagonal" else 1)


def test_nested_rings_and_uncovered_hole(vsg):
    got = check_case(vsg, BY_NAME["rings"])[0]
    for connect in MODES:
        comps, _, labels = got[connect]
        assert comps["id"].tolist() == [11, 11, 12] and comps["component"].tolist() == [0, 1, 0]
        assert comps["region_components"].tolist() == [2, 2, 1]
        assert (labels[9:24, 9:24][labels[9:24, 9:24] != 1] == -1).all() and (labels[13:20, 13:20] == 1).all()


def test_interleaved_ids_up_to_2_30(vsg):
    got = check_case(vsg, BY_NAME["interleaved"])[0]
    assert len(got[cm.N4][0]) == 72 and got[cm.N8][0]["id"].tolist() == [7, 1 << 30]
    check_case(vsg, BY_NAME["region_ids"])
    got = check_case(vsg, BY_NAME["parts"])
    assert [len(got[1][c][0]) for c in MODES] == [4, 3]


def test_three_level_hierarchy_and_refusals(vsg):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    c = BY_NAME["three_levels"]
    check_case(vsg, c)
    r = vsg.SegmentationRenderer(c.W, c.H)
    seg = c.msg.SerializeToString()
    for level in (3, 4, -1):
        with pytest.raises(VsgError) as e:
            r.level_components(seg, level, cm.N4)
        assert e.value.code == VSG_ERR_INVALID
    for connect in (0, 3):
        with pytest.raises(VsgError) as e:
            r.level_components(seg, 0, connect)
        assert e.value.code == VSG_ERR_INVALID
    r.close()


def test_capacities_and_count_only(vsg):
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    seg = c.msg.SerializeToString()
    want_c, want_i, want_l = cm.sweep(lc.id_image(c.msg, 1), cm.N4)
    nc_, ni_ = len(want_c), len(want_i)
    L = render.lib()
    r = vsg.SegmentationRenderer(c.W, c.H)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    def call(comps, cap_c, intervals, cap_i, labels):
        nc, ni = C.c_size_t(77), C.c_size_t(77)
        rc = L.vsg_render_level_components(r.h, seg, len(seg), 1, cm.N4, ptr(comps), cap_c, C.byref(nc),
                                           ptr(intervals), cap_i, C.byref(ni), ptr(labels), 0)
        return rc, nc.value, ni.value

    assert call(None, 0, None, 0, None) == (0, nc_, ni_)                      # count only
    comps = np.zeros(nc_ + 2, cm.COMPONENT_DTYPE)
    intervals = np.full((ni_ + 2, 4), -7, np.int32)
    labels = np.full((c.H, c.W), -7, np.int32)
    pattern = np.frombuffer(b"\x5a" * comps.nbytes, cm.COMPONENT_DTYPE)
    for cap_c, cap_i in ((nc_ - 1, ni_), (nc_, ni_ - 1), (nc_ - 1, ni_ - 1), (0, ni_), (nc_, 0)):
        comps[:] = pattern
        assert call(comps, cap_c, intervals, cap_i, labels) == (-1, nc_, ni_), (cap_c, cap_i)
        assert lm.same_bits(comps, pattern) and (intervals == -7).all() and (labels == -7).all(), (cap_c, cap_i)
    assert call(comps, nc_, intervals, ni_, labels) == (0, nc_, ni_)          # exact capacities
    assert_same((comps[:nc_], intervals[:ni_], labels), (want_c, want_i, want_l), "exact")
    assert lm.same_bits(comps[nc_:], pattern[nc_:]) and (intervals[ni_:] == -7).all()
    r.close()


def test_device_outputs_equal_host_outputs(vsg):
    import torch
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    seg = c.msg.SerializeToString()
    dev = torch.device("cuda", 0)
    r = vsg.SegmentationRenderer(c.W, c.H)
    for level in c.levels:
        for connect in MODES:
            host_c, host_i, host_l = r.level_components(seg, level, connect, label_image=True)
            nc_, ni_ = len(host_c), len(host_i)
            d_comps = torch.full((nc_ + 3, render.LEVEL_COMPONENT_WORDS), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            d_intervals = torch.full((ni_ + 3, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            d_labels = torch.full((c.H, c.W), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            got_c, got_i, got_l = r.level_components(seg, level, connect, components_out=d_comps,
                                                     intervals_out=d_intervals, labels_out=d_labels)
            assert got_c.is_cuda and got_i.is_cuda and got_l.is_cuda
            assert got_c.shape == (nc_, 16) and got_i.shape == (ni_, 4)
            assert got_c.cpu().numpy().tobytes() == host_c.tobytes()
            assert np.array_equal(got_i.cpu().numpy(), host_i) and np.array_equal(got_l.cpu().numpy(), host_l)
            assert bool((d_comps[nc_:] == 0x5A5A5A5A).all()) and bool((d_intervals[ni_:] == 0x5A5A5A5A).all())
            # one component too few: refused, nothing written
            for t in (d_comps, d_intervals, d_labels):
                t.fill_(0x5A5A5A5A)
            with pytest.raises(render.VsgError):
                r.level_components(seg, level, connect, components_out=d_comps[:nc_ - 1], intervals_out=d_intervals,
                                   labels_out=d_labels)
            assert all(bool((t == 0x5A5A5A5A).all()) for t in (d_comps, d_intervals, d_labels))
    r.close()


def test_vector_only_desc(vsg):
    W, H = 64, 48
    m = vc.vector_only(vc.l1_voronoi(11, W, H, 12))
    seg = m.SerializeToString()
    r = vsg.SegmentationRenderer(W, H)
    check_ids(r, seg, vm.id_plane(r.rasterize(seg), W, H), 0, "vector-only")
    # at another size than the desc's: scan converted at the handle's
    r2 = vsg.SegmentationRenderer(96, 72)
    check_ids(r2, seg, vm.id_plane(r2.rasterize(seg), 96, 72), 0, "vector-only, scaled")
    r.close()
    r2.close()


def test_handle_reuse_and_level_regions_before_and_after(vsg):
    small, large = BY_NAME["reuse_small"], BY_NAME["reuse_large"]
    r = vsg.SegmentationRenderer(small.W, small.H)
    before = {c.name: r.level_regions(c.msg.SerializeToString(), 0) for c in (small, large)}
    want = {c.name: cm.sweep(lc.id_image(c.msg, 0), cm.N8) for c in (small, large)}
    results, allocs = [], []
    for _ in range(2):
        for c in (small, large, small):
            got = r.level_components(c.msg.SerializeToString(), 0, cm.N8, label_image=True)
            assert_same(got, want[c.name], c.name)
            results.append(got)
            allocs.append(r.last_stats()["device_allocations"])
    assert all(lm.same_bits(a, b) for a, b in zip(results[2], results[0]))
    # the second round of identical calls allocates nothing
    assert allocs[1] > allocs[0] > 0 and allocs[3:] == [allocs[2]] * 3, allocs
    for c in (small, large):
        after = r.level_regions(c.msg.SerializeToString(), 0)
        assert lm.same_bits(after[0], before[c.name][0]) and lm.same_bits(after[1], before[c.name][1])
        assert lm.same_bits(after[1], lm.runs(lc.id_image(c.msg, 0))[1])
    r.close()


STREAM = (64, 48, 16, 8)   # W, H, frames, chunk size


@pytest.fixture(scope="module")
def stream(vsg):
    """A synth stream through the dense unit and the region stage: the serialized descs."""
    W, H, N, chunk = STREAM
    fl = synth.const_flow(W, H)
    frames = [synth.soft_frame(W, H, k) for k in range(N)]
    d = vsg.DenseSegmentation(W, H, vsg.default_options(chunk_size=chunk), has_flow=True)
    reg = vsg.RegionSegmentation(W, H, vsg.default_region_options(chunk_set_size=3, chunk_set_overlap=1,
                                                                  constraint_chunks=1, min_region_num=3))
    over, segs = [], []
    for k in range(N):
        n = d.process_frame(frames[k], fl if k > 0 else None, flush=(k == N - 1))
        over += [d.result_bytes(i) for i in range(n)]
    for k, seg in enumerate(over):
        n = reg.process_frame(seg, frames[k], fl if k > 0 else None, flush=(k == N - 1))
        segs += [reg.result_bytes(i) for i in range(n)]
    d.close()
    reg.close()
    assert len(segs) == N
    return segs


def test_dense_and_region_stage_end_to_end(vsg, stream):
    W, H, N, _ = STREAM
    r = vsg.SegmentationRenderer(W, H)
    model = rm.RenderModel(W, H)
    heights = []
    chunks = set()
    for k, seg in enumerate(stream):
        m = lc.Msg()
        m.ParseFromString(seg)
        chunks.add(m.chunk_id)
        hier = model._ingest(m)              # a desc without a hierarchy uses the kept one, as the handle does
        heights.append(len(hier))
        for level in range(len(hier)):
            check_ids(r, seg, model.id_image(m, level), level, ("stream", k))
    assert len(chunks) >= 2 and min(heights) >= 1 and max(heights) >= 2, heights
    r.close()


def test_full_hd_level_0_and_top(vsg):
    W, H = 1920, 1080
    ids = vc.l1_voronoi(12, W, H, 300)
    m = vc.vectorize(ids)                     # rasters; the vectorization is not looked at
    top = {int(i): 5 + int(i) % 7 for i in np.unique(ids)}
    lc.add_hierarchy(m, [top])
    seg = m.SerializeToString()
    lut = np.zeros(int(ids.max()) + 1, np.int32)
    for i, p in top.items():
        lut[i] = p
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    for level, plane in ((0, ids), (1, lut[ids])):
        for connect in MODES:
            want = cm.sweep(plane, connect)
            assert_same(r.level_components(seg, level, connect, label_image=True), want, ("1080p", level, connect))
    st = r.last_component_stats()
    assert all(st[k] > 0 for k in ("runs_us", "sort_us", "link_us", "order_us", "moments_us", "label_us"))
    r.close()


def test_driver_prints_the_python_paths_sums(vsg, stream):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    r = vsg.SegmentationRenderer(W, H)
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3", "--nouse_pipeline"]
    for flags, connect in ((["--level_components", "0"], cm.N4), (["--level_components", "0", "--components_n8"], cm.N8)):
        lists = [r.level_components(seg, 0, connect) for seg in stream]
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        m = re.search(r"level_components=(\d+) component_intervals=(\d+) component_fnv1a32=(\w+)", p.stdout)
        assert m, p.stdout
        assert int(m.group(1)) == sum(len(c) for c, _ in lists)
        assert int(m.group(2)) == sum(len(i) for _, i in lists)
        assert int(m.group(3), 16) == rm.fnv1a32(a for pair in lists for a in pair)
    r.close()
