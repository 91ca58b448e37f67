"""vsg_render_level_contours on the MI355X (libvsg_render.so: the id plane or the component label image,
k_contour_classify and its scan, k_contour_emit, the two pointer doublings, the contours' sort, the vertex
scatter, k_contour_table, k_contour_measure, k_contour_finish, k_copy_lists) against
level_contours_model.py.  Records and vertices are compared as raw bytes: there is no tolerance anywhere in
this file."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import level_components_model as cm
import level_contours_cases as tc
import level_contours_model as tm
import level_regions_cases as lc
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
CASES = tc.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODES = (0, cm.N4, cm.N8)          # the regions' contours, the N4 components', the N8 components'
COUNTS = ("cracks", "vertices", "contours", "holes", "largest_contour_cracks")


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert (render.N4, render.N8) == (cm.N4, cm.N8)
    assert render.LEVEL_CONTOUR_DTYPE == tm.CONTOUR_DTYPE
    return v


def assert_same(got, want, what):
    got_r, got_v = got
    want_r, want_v = want
    assert got_v.dtype == np.int32 and got_v.shape == want_v.shape, (what, got_v.shape, want_v.shape)
    assert got_r.dtype == tm.CONTOUR_DTYPE and got_r.shape == want_r.shape, (what, got_r.shape, want_r.shape)
    assert tm.same_bits(got_r, want_r), what
    assert tm.same_bits(got_v, want_v), what


def plane_of(ids, connect):
    """(plane, components or None) of a mode."""
    if connect == 0:
        return ids, None
    comps, _, labels = cm.sweep(ids, connect)
    return labels, comps


def model(ids, connect):
    plane, comps = plane_of(ids, connect)
    return tm.contours(plane, comps)


def rounds_of(cracks):
    """Both doublings, ceil(log2 cracks) rounds each, made even: a launch does two."""
    return 2 * ((int(cracks - 1).bit_length() + 1) // 2 * 2) if cracks else 0


def check_stats(st, records, vertices, what):
    want = {"cracks": int(records["length"].sum()), "vertices": len(vertices), "contours": len(records),
            "holes": int((records["area2"] < 0).sum()),
            "largest_contour_cracks": int(records["length"].max()) if len(records) else 0}
    assert {k: st[k] for k in COUNTS} == want, what
    assert st["rounds"] == rounds_of(want["cracks"]), what


def check_ids(r, seg, ids, level, what, modes=MODES):
    """Every mode of one level against the model, with the counts and the sibling calls on the same handle."""
    out = {}
    for connect in modes:
        plane, comps = plane_of(ids, connect)
        want = tm.contours(plane, comps)
        got = r.level_contours(seg, level, connect)
        assert_same(got, want, (what, level, connect))
        st = r.last_contour_stats()
        check_stats(st, want[0], want[1], (what, level, connect))
        assert {k: st[k] for k in COUNTS} == tm.stats_of(plane), (what, level, connect)
        records = got[0]
        out[connect] = got
        if not len(records):
            continue
        # record k of the sibling call is group k
        if connect == 0:
            siblings, _ = r.level_regions(seg, level)
            assert (records["component"] == -1).all()
        else:
            siblings, _ = r.level_components(seg, level, connect)
            assert np.array_equal(siblings["component"][records["group"]], records["component"])
        assert np.array_equal(siblings["id"][records["group"]], records["id"]), (what, level, connect)
        assert sorted(set(records["group"].tolist())) == list(range(len(siblings))), (what, level, connect)
        nodes, _ = r.level_adjacency(seg, level, connect)
        length = np.bincount(records["group"], records["length"], len(siblings)).astype(np.int64)
        area2 = np.zeros(len(siblings), np.int64)
        np.add.at(area2, records["group"], records["area2"])
        perimeter = nodes["border_frame"].astype(np.int64) + nodes["border_uncovered"] + nodes["border_shared"]
        assert np.array_equal(length, perimeter), (what, level, connect)
        assert np.array_equal(area2, 2 * siblings["area"].astype(np.int64)), (what, level, connect)
    return out


def check_case(vsg, case, modes=MODES):
    r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    seg = case.msg.SerializeToString()
    out = {level: check_ids(r, seg, lc.id_image(case.msg, level), level, case.name, modes) for level in case.levels}
    r.close()
    return out


@pytest.mark.parametrize("name", sorted(n for n in BY_NAME if not n.startswith("cover_")))
def test_every_case_in_every_mode_at_every_level(vsg, name):
    check_case(vsg, BY_NAME[name])


@pytest.mark.parametrize("W", sorted({c.W for c in tc.full_cover()}))
def test_one_region_covering_the_frame(vsg, W):
    for c in tc.full_cover():
        if c.W == W:
            got = check_case(vsg, c)[0]
            for connect in MODES:
                records, vertices = got[connect]
                assert vertices.tolist() == [[0, 0], [c.W, 0], [c.W, c.H], [0, c.H]]
                assert records["length"].tolist() == [2 * c.W + 2 * c.H]


def test_the_shapes_a_tracer_gets_wrong(vsg):
    got = check_case(vsg, BY_NAME["one_region_1x1"])[0][0]
    assert got[0]["num_vertices"].tolist() == [4] and got[0]["area2"].tolist() == [2] and got[0]["length"].tolist() == [4]
    c = BY_NAME["pixel_checker"]
    assert len(check_case(vsg, c)[0][0][0]) == c.W * c.H
    for connect, got in check_case(vsg, BY_NAME["saddle"])[0].items():
        assert len(got[0]) == 2 and got[0]["group"].tolist() == [0, 1 if connect == cm.N4 else 0]
    records, vertices = check_case(vsg, BY_NAME["diagonal_hole"])[0][0]
    assert records["num_vertices"].tolist() == [4, 8] and vertices[4:].tolist().count([3, 3]) == 2
    records, vertices = check_case(vsg, BY_NAME["wide_hole"])[0][0]
    assert vertices[records[1]["first_vertex"]].tolist() == [6, 2] and records[1]["area2"] == -12
    records, _ = check_case(vsg, BY_NAME["nested"])[0][0]
    assert len(records) == 9 and (records["area2"] < 0).sum() == 4
    records, _ = check_case(vsg, BY_NAME["comb_8192"], (0,))[0][0]
    assert len(records) == 1 and records[0]["num_vertices"] > 1 << 14
    c = BY_NAME["spiral_129x65"]
    records, _ = check_case(vsg, c, (0,))[0][0]
    assert len(records) == 1 and records[0]["length"] > c.W * c.H


def test_a_frame_without_a_covered_pixel(vsg):
    c = BY_NAME["uncovered_frame"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    for connect in MODES:
        records, vertices = r.level_contours(c.msg.SerializeToString(), 0, connect)
        assert records.shape == (0,) and records.dtype == tm.CONTOUR_DTYPE
        assert vertices.shape == (0, 2) and vertices.dtype == np.int32
        st = r.last_contour_stats()
        assert all(st[k] == 0 for k in COUNTS) and st["rounds"] == 0
    r.close()


def test_bad_levels_and_bad_connectedness(vsg):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    c = BY_NAME["three_levels"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    seg = c.msg.SerializeToString()
    for level in (3, 4, -1):
        for connect in MODES:
            with pytest.raises(VsgError) as e:
                r.level_contours(seg, level, connect)
            assert e.value.code == VSG_ERR_INVALID
    for connect in (3, -1):
        with pytest.raises(VsgError) as e:
            r.level_contours(seg, 0, connect)
        assert e.value.code == VSG_ERR_INVALID
    assert_same(r.level_contours(seg, 2, cm.N8), model(lc.id_image(c.msg, 2), cm.N8), "after the refusals")
    r.close()


def test_capacities_and_count_only(vsg):
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    seg = c.msg.SerializeToString()
    L = render.lib()
    r = vsg.SegmentationRenderer(c.W, c.H)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    for connect in (0, cm.N4):
        want_r, want_v = model(lc.id_image(c.msg, 1), connect)
        nc_, nv_ = len(want_r), len(want_v)

        def call(records, cap_r, vertices, cap_v):
            nc, nv = C.c_size_t(77), C.c_size_t(77)
            rc = L.vsg_render_level_contours(r.h, seg, len(seg), 1, connect, ptr(records), cap_r, C.byref(nc),
                                             ptr(vertices), cap_v, C.byref(nv), 0)
            return rc, nc.value, nv.value

        assert call(None, 0, None, 0) == (0, nc_, nv_)                    # count only
        records = np.zeros(nc_ + 2, tm.CONTOUR_DTYPE)
        vertices = np.full((nv_ + 2, 2), -7, np.int32)
        pattern = np.frombuffer(b"\x5a" * records.nbytes, tm.CONTOUR_DTYPE)
        for cap_r, cap_v in ((nc_ - 1, nv_), (nc_, nv_ - 1), (nc_ - 1, nv_ - 1), (0, nv_), (nc_, 0)):
            records[:] = pattern
            assert call(records, cap_r, vertices, cap_v) == (-1, nc_, nv_), (cap_r, cap_v)
            assert tm.same_bits(records, pattern) and (vertices == -7).all(), (cap_r, cap_v)
        assert call(records, nc_, vertices, nv_) == (0, nc_, nv_)         # exact capacities, usable afterwards
        assert_same((records[:nc_], vertices[:nv_]), (want_r, want_v), "exact")
        assert tm.same_bits(records[nc_:], pattern[nc_:]) and (vertices[nv_:] == -7).all()
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
            host_r, host_v = r.level_contours(seg, level, connect)
            nc_, nv_ = len(host_r), len(host_v)
            d_records = torch.full((nc_ + 3, render.LEVEL_CONTOUR_WORDS), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            d_vertices = torch.full((nv_ + 3, 2), 0x5A5A5A5A, dtype=torch.int32, device=dev)
            got_r, got_v = r.level_contours(seg, level, connect, contours_out=d_records, vertices_out=d_vertices)
            assert got_r.is_cuda and got_v.is_cuda and got_r.shape == (nc_, 12) and got_v.shape == (nv_, 2)
            assert got_r.cpu().numpy().tobytes() == host_r.tobytes()
            assert np.array_equal(got_v.cpu().numpy(), host_v)
            assert bool((d_records[nc_:] == 0x5A5A5A5A).all()) and bool((d_vertices[nv_:] == 0x5A5A5A5A).all())
            # one record, then one vertex too few: refused, nothing written
            for cut_r, cut_v in ((1, 0), (0, 1)):
                d_records.fill_(0x5A5A5A5A)
                d_vertices.fill_(0x5A5A5A5A)
                with pytest.raises(render.VsgError):
                    r.level_contours(seg, level, connect, contours_out=d_records[:nc_ - cut_r],
                                     vertices_out=d_vertices[:nv_ - cut_v])
                assert bool((d_records == 0x5A5A5A5A).all()) and bool((d_vertices == 0x5A5A5A5A).all())
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


def test_handle_reuse_with_the_other_level_calls_before_and_after(vsg):
    small, large = tc.reuse()
    r = vsg.SegmentationRenderer(small.W, small.H)
    segs = {c.name: c.msg.SerializeToString() for c in (small, large)}

    def siblings(s):
        return (r.level_regions(s, 0), r.level_components(s, 0, cm.N8, label_image=True),
                r.level_boundaries(s, 0, cm.N4), r.level_adjacency(s, 0))

    before = {n: siblings(s) for n, s in segs.items()}
    want = {(c.name, k): model(lc.id_image(c.msg, 0), k) for c in (small, large) for k in (0, cm.N8)}
    allocs = []
    for _ in range(2):
        for c in (small, large, small):
            for k in (0, cm.N8):
                assert_same(r.level_contours(segs[c.name], 0, k), want[c.name, k], (c.name, k))
                r.level_boundaries(segs[c.name], 0, k)         # interleaved: shares the sort's work space
            allocs.append(r.last_stats()["device_allocations"])
    # the second round of identical calls allocates nothing
    assert allocs[1] > allocs[0] > 0 and allocs[3:] == [allocs[2]] * 3, allocs
    for n, s in segs.items():
        for a, b in zip(siblings(s), before[n]):
            assert all(tm.same_bits(x, y) for x, y in zip(a, b)), n
    r.close()


def test_the_level_of_render_is_neither_resolved_nor_changed(vsg):
    c = BY_NAME["three_levels"]
    seg = c.msg.SerializeToString()
    r = vsg.SegmentationRenderer(c.W, c.H, hierarchy_level=1, has_video=False)
    assert r.level is None
    for level in c.levels:
        r.level_contours(seg, level, cm.N4)
        assert r.level is None
    first = r.render(seg)
    assert r.level == 1
    for level in c.levels:
        r.level_contours(seg, level)
        assert r.level == 1
    assert tm.same_bits(r.render(seg), first)
    r.close()


def test_launches_are_a_function_of_the_mode_and_the_rounds(vsg):
    """Over every case at level 0, host outputs: one value per (connectedness, ceil(log2 cracks))."""
    seen = {}
    for c in CASES:
        r = vsg.SegmentationRenderer(c.W, c.H, has_video=False)
        seg = c.msg.SerializeToString()
        for connect in MODES:
            r.level_contours(seg, 0, connect)
            st = r.last_contour_stats()
            if st["cracks"]:
                seen.setdefault((connect, st["rounds"]), {}).setdefault(st["launches"], []).append(c.name)
        r.close()
    assert all(len(v) == 1 for v in seen.values()), {k: v for k, v in seen.items() if len(v) > 1}
    assert max(len(names) for v in seen.values() for names in v.values()) >= 5      # shared by different content
    by_mode = {connect: sorted((rounds, list(v)[0]) for (m, rounds), v in seen.items() if m == connect)
               for connect in MODES}
    for connect, pairs in by_mode.items():
        # two more rounds of either doubling are one more launch each and nothing else
        assert len({launches - rounds // 2 for rounds, launches in pairs}) == 1, (connect, pairs)


STREAM = (96, 64, 16, 8)   # W, H, frames, chunk size


@pytest.fixture(scope="module")
def stream(vsg):
    """The synth stream through the dense unit and the hierarchical stage: the serialized descs."""
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


def test_a_real_stream_every_frame_at_every_level(vsg, stream):
    W, H, N, _ = STREAM
    r = vsg.SegmentationRenderer(W, H)
    model_ = rm.RenderModel(W, H)
    heights = []
    for k, seg in enumerate(stream):
        m = lc.Msg()
        m.ParseFromString(seg)
        hier = model_._ingest(m)                 # a desc without a hierarchy uses the kept one, as the handle does
        heights.append(len(hier))
        for level in range(max(len(hier), 1)):
            # every frame and level in the regions' mode, a few frames in all three
            modes = MODES if k % 5 == 1 or k == N - 1 else (0,)
            check_ids(r, seg, model_.id_image(m, level), level, ("stream", k), modes)
    assert min(heights) >= 1 and max(heights) >= 2, heights
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
    comps, _, labels = cm.sweep(lut[ids], cm.N4)
    for level, connect, plane, of in ((0, 0, ids, None), (0, cm.N4, None, None), (1, 0, lut[ids], None),
                                      (1, cm.N4, labels, comps)):
        if plane is None:
            of, _, plane = cm.sweep(ids, cm.N4)
        want = tm.contours(plane, of)
        assert_same(r.level_contours(seg, level, connect), want, ("1080p", level, connect))
        st = r.last_contour_stats()
        check_stats(st, want[0], want[1], ("1080p", level, connect))
        assert all(st[k] > 0 for k in ("plane_us", "classify_us", "trace_us", "table_us")), st
    r.close()


def test_driver_prints_the_python_paths_sums(vsg, stream):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    r = vsg.SegmentationRenderer(W, H)
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3", "--nouse_pipeline"]
    for flags, connect in ((["--level_contours", "0"], 0),
                           (["--level_contours", "0", "--contours_components", "--components_n8"], cm.N8)):
        lists = [r.level_contours(seg, 0, connect) for seg in stream]
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        m = re.search(r"level_contours_count=(\d+) level_contours_fnv1a32=(\w+)", p.stdout)
        assert m, p.stdout
        assert int(m.group(1)) == sum(len(c) for c, _ in lists)
        assert int(m.group(2), 16) == rm.fnv1a32(a for pair in lists for a in pair)
    r.close()
