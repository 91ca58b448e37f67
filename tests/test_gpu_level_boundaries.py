"""vsg_render_level_boundaries on the MI355X (libvsg_render.so: the id plane or the component label image,
k_bound_classify's count and emit passes, the key sort, k_bound_table, k_bound_finish, k_copy_lists) against
level_boundaries_model.py.  Records and points are compared as raw bytes: there is no tolerance anywhere in
this file."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import level_boundaries_cases as bc
import level_boundaries_model as bm
import level_components_model as cm
import level_regions_cases as lc
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
CASES = bc.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODES = (0, cm.N4, cm.N8)          # the regions' boundaries, the N4 components', the N8 components'


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert (render.N4, render.N8) == (cm.N4, cm.N8)
    assert render.LEVEL_BOUNDARY_DTYPE == bm.BOUNDARY_DTYPE
    return v


def assert_same(got, want, what):
    got_r, got_p = got
    want_r, want_p = want
    assert got_p.dtype == np.int32 and got_p.shape == want_p.shape, (what, got_p.shape, want_p.shape)
    assert got_r.dtype == bm.BOUNDARY_DTYPE and got_r.shape == want_r.shape, (what, got_r.shape, want_r.shape)
    assert bm.same_bits(got_r, want_r), what
    assert bm.same_bits(got_p, want_p), what


def model(ids, connect, outer):
    if connect == 0:
        return bm.boundaries(ids, outer)
    comps, _, labels = cm.sweep(ids, connect)
    return bm.boundaries(labels, outer, comps)


def check_ids(r, seg, ids, level, what):
    """All six combinations of one level against the model, with the counts and the neighbouring calls."""
    out = {}
    for connect in MODES:
        for outer in (False, True):
            want = model(ids, connect, outer)
            got = r.level_boundaries(seg, level, connect, outer)
            assert_same(got, want, (what, level, connect, outer))
            st = r.last_boundary_stats()
            assert st["points"] == len(want[1]) and st["boundaries"] == len(want[0])
            assert st["largest_boundary_points"] == (want[0]["num_points"].max() if len(want[0]) else 0)
            out[connect, outer] = got
        # record k belongs to record k of the call the mode is named after
        records = out[connect, False][0]
        if connect == 0:
            regions, _ = r.level_regions(seg, level)
            assert np.array_equal(records["id"], regions["id"]) and (records["component"] == -1).all()
        else:
            comps, _ = r.level_components(seg, level, connect)
            assert np.array_equal(records["id"], comps["id"])
            assert np.array_equal(records["component"], comps["component"])
        for f in ("id", "component"):
            assert np.array_equal(out[connect, True][0][f], records[f]), (what, level, connect, f)
    return out


def check_case(vsg, case):
    r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    seg = case.msg.SerializeToString()
    out = {level: check_ids(r, seg, lc.id_image(case.msg, level), level, case.name) for level in case.levels}
    r.close()
    return out


@pytest.mark.parametrize("name", ["one_region_1x1", "one_region_7x1", "one_region_1x7", "one_region_9x5",
                                  "full_5x4", "full_300x3"])
def test_degenerate_frames_and_one_region_covering_the_frame(vsg, name):
    c = BY_NAME[name]
    got = check_case(vsg, c)[0]
    for connect in MODES:
        records, points = got[connect, True]
        # the outer boundary lies entirely outside the frame and has no corners
        assert records["num_points"].tolist() == [2 * c.W + 2 * c.H]
        x, y = points[:, 0], points[:, 1]
        assert (((x == -1) | (x == c.W)) ^ ((y == -1) | (y == c.H))).all()
        inner = got[connect, False][0]["num_points"].tolist()
        assert inner == [c.W * c.H - max(c.W - 2, 0) * max(c.H - 2, 0)]


@pytest.mark.parametrize("W", bc.WIDTHS)
def test_widths_around_wavefront_and_block_boundaries(vsg, W):
    for H in bc.HEIGHTS:
        check_case(vsg, BY_NAME["width_%dx%d" % (W, H)])


def test_uncovered_pixels_rows_and_frame(vsg):
    check_case(vsg, BY_NAME["uncovered"])
    c = BY_NAME["uncovered_frame"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    for connect in MODES:
        for outer in (False, True):
            records, points = r.level_boundaries(c.msg.SerializeToString(), 0, connect, outer)
            assert records.shape == (0,) and records.dtype == bm.BOUNDARY_DTYPE
            assert points.shape == (0, 2) and points.dtype == np.int32
            st = r.last_boundary_stats()
            assert st["points"] == 0 and st["boundaries"] == 0 and st["largest_boundary_points"] == 0
    r.close()


def test_one_pixel_checker_where_a_position_belongs_to_four_groups(vsg):
    c = BY_NAME["pixel_checker"]
    got = check_case(vsg, c)[0]
    assert got[0, False][0]["num_points"].sum() == c.W * c.H              # every pixel is inner
    points = got[0, True][1]
    inside = (points[:, 0] > 0) & (points[:, 0] < c.W - 1) & (points[:, 1] > 0) & (points[:, 1] < c.H - 1)
    assert inside.sum() == 4 * (c.W - 2) * (c.H - 2)


def test_a_position_flanked_on_several_sides_is_listed_once(vsg):
    got = check_case(vsg, BY_NAME["flanked"])[0]
    records, points = got[0, True]
    assert records["id"][0] == 5
    five = points[:records["num_points"][0]].tolist()
    for p in ([2, 2], [6, 2], [10, 1], [3, 6], [7, 6], [12, 6]):
        assert five.count(p) == 1, p
    assert len(set(map(tuple, five))) == len(five)


def test_nested_rings_and_diagonal_blobs(vsg):
    got = check_case(vsg, BY_NAME["rings"])[0]
    assert got[cm.N4, False][0]["id"].tolist() == [11, 11, 12]
    assert got[cm.N4, False][0]["component"].tolist() == [0, 1, 0]
    for name in ("diagonal", "fan_diagonal", "parts", "comb_up"):
        got = check_case(vsg, BY_NAME[name])
        top = got[max(got)]
        assert len(top[cm.N4, False][0]) > len(top[cm.N8, False][0]) or name == "comb_up", name


def test_interleaved_ids_up_to_2_30(vsg):
    got = check_case(vsg, BY_NAME["interleaved"])[0]
    assert got[0, False][0]["id"].tolist() == [7, 1 << 30]
    assert len(got[cm.N4, True][0]) == 72 and got[cm.N8, True][0]["id"].tolist() == [7, 1 << 30]
    check_case(vsg, BY_NAME["region_ids"])


def test_three_level_hierarchy_and_refusals(vsg):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    c = BY_NAME["three_levels"]
    check_case(vsg, c)
    r = vsg.SegmentationRenderer(c.W, c.H)
    seg = c.msg.SerializeToString()
    for level in (3, 4, -1):
        for connect in MODES:
            with pytest.raises(VsgError) as e:
                r.level_boundaries(seg, level, connect)
            assert e.value.code == VSG_ERR_INVALID
    for connect in (3, -1):
        with pytest.raises(VsgError) as e:
            r.level_boundaries(seg, 0, connect)
        assert e.value.code == VSG_ERR_INVALID
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
        for which in (0, 1):
            want_r, want_p = model(lc.id_image(c.msg, 1), connect, bool(which))
            nb_, np_ = len(want_r), len(want_p)

            def call(records, cap_r, points, cap_p):
                nb, npts = C.c_size_t(77), C.c_size_t(77)
                rc = L.vsg_render_level_boundaries(r.h, seg, len(seg), 1, connect, which, ptr(records), cap_r,
                                                   C.byref(nb), ptr(points), cap_p, C.byref(npts), 0)
                return rc, nb.value, npts.value

            assert call(None, 0, None, 0) == (0, nb_, np_)                    # count only
            records = np.zeros(nb_ + 2, bm.BOUNDARY_DTYPE)
            points = np.full((np_ + 2, 2), -7, np.int32)
            pattern = np.frombuffer(b"\x5a" * records.nbytes, bm.BOUNDARY_DTYPE)
            for cap_r, cap_p in ((nb_ - 1, np_), (nb_, np_ - 1), (nb_ - 1, np_ - 1), (0, np_), (nb_, 0)):
                records[:] = pattern
                assert call(records, cap_r, points, cap_p) == (-1, nb_, np_), (cap_r, cap_p)
                assert bm.same_bits(records, pattern) and (points == -7).all(), (cap_r, cap_p)
            assert call(records, nb_, points, np_) == (0, nb_, np_)           # exact capacities
            assert_same((records[:nb_], points[:np_]), (want_r, want_p), "exact")
            assert bm.same_bits(records[nb_:], pattern[nb_:]) and (points[np_:] == -7).all()
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
            for outer in (False, True):
                host_r, host_p = r.level_boundaries(seg, level, connect, outer)
                nb_, np_ = len(host_r), len(host_p)
                d_records = torch.full((nb_ + 3, render.LEVEL_BOUNDARY_WORDS), 0x5A5A5A5A, dtype=torch.int32, device=dev)
                d_points = torch.full((np_ + 3, 2), 0x5A5A5A5A, dtype=torch.int32, device=dev)
                got_r, got_p = r.level_boundaries(seg, level, connect, outer, boundaries_out=d_records,
                                                  points_out=d_points)
                assert got_r.is_cuda and got_p.is_cuda and got_r.shape == (nb_, 4) and got_p.shape == (np_, 2)
                assert got_r.cpu().numpy().tobytes() == host_r.tobytes()
                assert np.array_equal(got_p.cpu().numpy(), host_p)
                assert bool((d_records[nb_:] == 0x5A5A5A5A).all()) and bool((d_points[np_:] == 0x5A5A5A5A).all())
                # one record, then one point too few: refused, nothing written
                for cut_r, cut_p in ((1, 0), (0, 1)):
                    d_records.fill_(0x5A5A5A5A)
                    d_points.fill_(0x5A5A5A5A)
                    with pytest.raises(render.VsgError):
                        r.level_boundaries(seg, level, connect, outer, boundaries_out=d_records[:nb_ - cut_r],
                                           points_out=d_points[:np_ - cut_p])
                    assert bool((d_records == 0x5A5A5A5A).all()) and bool((d_points == 0x5A5A5A5A).all())
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
    small, large = BY_NAME["reuse_small"], BY_NAME["reuse_large"]
    r = vsg.SegmentationRenderer(small.W, small.H)
    segs = {c.name: c.msg.SerializeToString() for c in (small, large)}
    before = {n: (r.level_regions(s, 0), r.level_components(s, 0, cm.N8, label_image=True)) for n, s in segs.items()}
    combos = [(connect, outer) for connect in (0, cm.N8) for outer in (False, True)]
    want = {(c.name, k): model(lc.id_image(c.msg, 0), *k) for c in (small, large) for k in combos}
    allocs = []
    for _ in range(2):
        for c in (small, large, small):
            for k in combos:
                assert_same(r.level_boundaries(segs[c.name], 0, *k), want[c.name, k], (c.name, k))
            allocs.append(r.last_stats()["device_allocations"])
    # the second round of identical calls allocates nothing
    assert allocs[1] > allocs[0] > 0 and allocs[3:] == [allocs[2]] * 3, allocs
    for n, s in segs.items():
        after = (r.level_regions(s, 0), r.level_components(s, 0, cm.N8, label_image=True))
        for a, b in zip(after, before[n]):
            assert all(bm.same_bits(x, y) for x, y in zip(a, b)), n
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
    model_ = rm.RenderModel(W, H)
    heights = []
    for k, seg in enumerate(stream):
        m = lc.Msg()
        m.ParseFromString(seg)
        hier = model_._ingest(m)             # a desc without a hierarchy uses the kept one, as the handle does
        heights.append(len(hier))
        if k % 5 == 0 or k == N - 1:         # every frame is ingested, a few are compared at every level
            for level in range(len(hier)):
                check_ids(r, seg, model_.id_image(m, level), level, ("stream", k))
        else:
            r.level_boundaries(seg, 0)
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
    for level, connect, plane, of in ((0, 0, ids, None), (1, 0, lut[ids], None), (1, cm.N4, labels, comps)):
        for outer in (False, True):
            assert_same(r.level_boundaries(seg, level, connect, outer), bm.boundaries(plane, outer, of),
                        ("1080p", level, connect, outer))
    st = r.last_boundary_stats()
    assert all(st[k] > 0 for k in ("plane_us", "count_us", "emit_us", "sort_us", "table_us"))
    r.close()


def test_driver_prints_the_python_paths_sums(vsg, stream):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    r = vsg.SegmentationRenderer(W, H)
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3", "--nouse_pipeline"]
    for flags, connect, outer in ((["--level_boundaries", "0"], 0, False),
                                  (["--level_boundaries", "0", "--boundaries_outer", "--boundaries_components",
                                    "--components_n8"], cm.N8, True)):
        lists = [r.level_boundaries(seg, 0, connect, outer) for seg in stream]
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        m = re.search(r"level_boundaries=(\d+) boundary_points=(\d+) boundary_fnv1a32=(\w+)", p.stdout)
        assert m, p.stdout
        assert int(m.group(1)) == sum(len(b) for b, _ in lists)
        assert int(m.group(2)) == sum(len(q) for _, q in lists)
        assert int(m.group(3), 16) == rm.fnv1a32(a for pair in lists for a in pair)
    r.close()
