"""vsg_render_level_regions on the MI355X (libvsg_render.so: k_level_runs, radix sort, scan,
k_level_table, k_level_moments) against level_regions_model.py.  Regions and intervals are compared as
raw bytes, the float fields as their uint32 patterns: there is no tolerance anywhere in this file.

The moments case: the issue asks for a 3840 x 4 frame, intervals at x >= 3000 and a region of at least
2 000 one-pixel-apart intervals; right of x = 3000 four rows hold 4 * 420 = 1 680 of them, which is
what the case has (level_regions_cases.moments)."""
import ctypes as C

import numpy as np
import pytest

import level_regions_cases as lc
import level_regions_model as lm
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

CASES = lc.all_cases()
BY_NAME = {c.name: c for c in CASES}


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    return v


def literal_of(msg, level, hier=None):
    return lm.literal(msg, level, rm.hierarchy_of(msg) if hier is None else hier)


def assert_same(got, want, what):
    got_r, got_i = got
    want_r, want_i = want
    assert got_i.dtype == np.int32 and got_i.shape == want_i.shape, (what, got_i.shape, want_i.shape)
    assert lm.same_bits(got_i, want_i), what
    assert got_r.dtype == lm.REGION_DTYPE and got_r.shape == want_r.shape, (what, got_r.shape, want_r.shape)
    for f in lm.REGION_DTYPE.names:
        assert np.array_equal(got_r[f].view(np.uint32), want_r[f].view(np.uint32)), (what, f)
    assert lm.same_bits(got_r, want_r), what


def check_case(vsg, case):
    r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    seg = case.msg.SerializeToString()
    for level in case.levels:
        want = literal_of(case.msg, level)
        assert_same(r.level_regions(seg, level), want, (case.name, level))
        st = r.last_level_stats()
        assert st["runs"] == len(want[1]) and st["regions"] == len(want[0])
        assert st["largest_region_intervals"] == (want[0]["num_intervals"].max() if len(want[0]) else 0)
    r.close()


@pytest.mark.parametrize("name", ["one_region_1x1", "one_region_7x1", "one_region_1x7", "one_region_9x5"])
def test_degenerate_frames_and_one_region(vsg, name):
    check_case(vsg, BY_NAME[name])
    got = vsg.SegmentationRenderer(9, 5).level_regions(BY_NAME["one_region_9x5"].msg.SerializeToString())
    assert got[1].tolist() == [[y, 0, 8, 3] for y in range(5)]      # never merged across the row end


@pytest.mark.parametrize("W", lc.BOUNDARY_WIDTHS)
def test_runs_on_and_around_wavefront_and_block_boundaries(vsg, W):
    for H in (1, 2, 3, 4, 5):
        check_case(vsg, BY_NAME["boundary_%dx%d" % (W, H)])


def test_uncovered_pixels_rows_and_frame(vsg):
    check_case(vsg, BY_NAME["uncovered"])
    c = BY_NAME["uncovered_frame"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    regions, intervals = r.level_regions(c.msg.SerializeToString())
    assert regions.shape == (0,) and regions.dtype == lm.REGION_DTYPE and intervals.shape == (0, 4)
    assert r.last_level_stats()["runs"] == 0 and r.last_level_stats()["regions"] == 0
    r.close()


def test_checker_of_one_pixel_regions(vsg):
    c = BY_NAME["checker"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    seg = c.msg.SerializeToString()
    got = r.level_regions(seg, 0)
    assert len(got[0]) == 6144 and len(got[1]) == 6144
    assert_same(got, lm.runs(lc.id_image(c.msg, 0)), "checker level 0")
    got = r.level_regions(seg, 1)
    assert got[0]["num_intervals"].tolist() == [3072, 3072]
    # the runs model here; test_level_regions_model.py ties it to the literal one for this case
    assert_same(got, lm.runs(lc.id_image(c.msg, 1)), "checker level 1")
    assert r.last_level_stats()["largest_region_intervals"] == 3072
    r.close()


def test_three_level_hierarchy(vsg):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    c = BY_NAME["three_levels"]
    check_case(vsg, c)
    r = vsg.SegmentationRenderer(c.W, c.H)
    seg = c.msg.SerializeToString()
    for level in (3, 4, -1):
        with pytest.raises(VsgError) as e:
            r.level_regions(seg, level)
        assert e.value.code == VSG_ERR_INVALID
    # a later desc without a hierarchy uses the kept one
    hier = rm.hierarchy_of(c.msg)
    bare = lc.Msg()
    bare.CopyFrom(c.msg)
    del bare.hierarchy[:]
    r.level_regions(seg, 0)
    for level in (2, 1, 0):
        assert_same(r.level_regions(bare.SerializeToString(), level), literal_of(bare, level, hier), ("kept", level))
    r.close()
    # without any hierarchy only level 0 exists
    r = vsg.SegmentationRenderer(c.W, c.H)
    assert_same(r.level_regions(bare.SerializeToString(), 0), literal_of(bare, 0, []), "no hierarchy")
    with pytest.raises(VsgError):
        r.level_regions(bare.SerializeToString(), 1)
    # an id missing from a level, an unsorted level
    missing = lc.Msg()
    missing.CopyFrom(c.msg)
    del missing.hierarchy[0].region[5]
    unsorted_ = lc.Msg()
    unsorted_.CopyFrom(c.msg)
    a, b = unsorted_.hierarchy[0].region[0], unsorted_.hierarchy[0].region[1]
    a.id, b.id = b.id, a.id
    for m in (missing, unsorted_):
        with pytest.raises(VsgError) as e:
            r.level_regions(m.SerializeToString(), 1)
        assert e.value.code == VSG_ERR_INVALID
    r.close()


def test_region_ids_small_sparse_and_near_2_30(vsg):
    check_case(vsg, BY_NAME["region_ids"])


def test_moments_keep_the_order_of_the_sums(vsg):
    c = BY_NAME["moments"]
    want = literal_of(c.msg, 0)
    assert len(want[0]) == 2 and (want[1][:, 1] >= 3000).all() and want[0]["num_intervals"].max() >= 1680
    back = lm.reversed_moments(*want)
    assert not lm.same_bits(back, want[0])          # another order would show
    r = vsg.SegmentationRenderer(c.W, c.H)
    assert_same(r.level_regions(c.msg.SerializeToString(), 0), want, "moments")
    r.close()


def test_capacities_and_modes(vsg):
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    seg = c.msg.SerializeToString()
    want_r, want_i = literal_of(c.msg, 1)
    nr_, ni_ = len(want_r), len(want_i)
    L = render.lib()
    r = vsg.SegmentationRenderer(c.W, c.H)

    def call(regions, cap_r, intervals, cap_i):
        nr, ni = C.c_size_t(77), C.c_size_t(77)
        rc = L.vsg_render_level_regions(r.h, seg, len(seg), 1,
                                        regions.ctypes.data_as(C.c_void_p) if regions is not None else None, cap_r,
                                        C.byref(nr), intervals.ctypes.data_as(C.c_void_p) if intervals is not None
                                        else None, cap_i, C.byref(ni), 0)
        return rc, nr.value, ni.value

    assert call(None, 0, None, 0) == (0, nr_, ni_)                      # count only
    regions = np.zeros(nr_ + 2, lm.REGION_DTYPE)
    intervals = np.full((ni_ + 2, 4), -7, np.int32)
    pattern = np.frombuffer(b"\x5a" * regions.nbytes, lm.REGION_DTYPE)
    for cap_r, cap_i in ((nr_ - 1, ni_), (nr_, ni_ - 1), (nr_ - 1, ni_ - 1), (0, ni_), (nr_, 0)):
        regions[:] = pattern
        intervals[:] = -7
        assert call(regions, cap_r, intervals, cap_i) == (-1, nr_, ni_), (cap_r, cap_i)
        assert lm.same_bits(regions, pattern) and (intervals == -7).all(), (cap_r, cap_i)
    regions[:] = pattern
    assert call(regions, nr_, intervals, ni_) == (0, nr_, ni_)          # exact capacities
    assert_same((regions[:nr_], intervals[:ni_]), (want_r, want_i), "exact")
    assert lm.same_bits(regions[nr_:], pattern[nr_:]) and (intervals[ni_:] == -7).all()
    r.close()


def test_device_outputs_equal_host_outputs(vsg):
    import torch
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    seg = c.msg.SerializeToString()
    dev = torch.device("cuda", 0)
    r = vsg.SegmentationRenderer(c.W, c.H)
    for level in c.levels:
        host_r, host_i = r.level_regions(seg, level)
        nr_, ni_ = len(host_r), len(host_i)
        d_regions = torch.full((nr_ + 3, render.LEVEL_REGION_WORDS), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_intervals = torch.full((ni_ + 3, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        got_r, got_i = r.level_regions(seg, level, regions_out=d_regions, intervals_out=d_intervals)
        assert got_r.is_cuda and got_i.is_cuda and got_r.shape == (nr_, 14) and got_i.shape == (ni_, 4)
        assert got_r.cpu().numpy().tobytes() == host_r.tobytes()
        assert np.array_equal(got_i.cpu().numpy(), host_i)
        assert bool((d_regions[nr_:] == 0x5A5A5A5A).all()) and bool((d_intervals[ni_:] == 0x5A5A5A5A).all())
        # one region too few: refused on the device, nothing written
        d_regions.fill_(0x5A5A5A5A)
        d_intervals.fill_(0x5A5A5A5A)
        with pytest.raises(render.VsgError):
            r.level_regions(seg, level, regions_out=d_regions[:nr_ - 1], intervals_out=d_intervals)
        assert bool((d_regions == 0x5A5A5A5A).all()) and bool((d_intervals == 0x5A5A5A5A).all())
    r.close()


def test_device_outputs_one_entry_short_in_turn_stay_untouched(vsg):
    import torch
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    seg = c.msg.SerializeToString()
    dev = torch.device("cuda", 0)
    r = vsg.SegmentationRenderer(c.W, c.H)
    for level in c.levels:
        nr_, ni_ = (len(a) for a in r.level_regions(seg, level))
        d_regions = torch.full((nr_ + 3, render.LEVEL_REGION_WORDS), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        d_intervals = torch.full((ni_ + 3, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
        # one region, then one interval too few: refused, nothing written
        for cut_r, cut_i in ((1, 0), (0, 1)):
            with pytest.raises(render.VsgError):
                r.level_regions(seg, level, regions_out=d_regions[:nr_ - cut_r],
                                intervals_out=d_intervals[:ni_ - cut_i])
            assert bool((d_regions == 0x5A5A5A5A).all()) and bool((d_intervals == 0x5A5A5A5A).all()), (cut_r, cut_i)
    r.close()


def test_device_outputs_larger_than_one_pass_of_the_copy_grid(vsg):
    """768 x 256 in one-pixel vertical stripes of two ids: 196 608 intervals, 786 432 copied words, more than the
    2048 x 256 threads of the copy's grid take in one pass of its stride loop."""
    import torch
    from video_segment_amd import render
    W, H = 768, 256
    ids = np.tile(np.arange(W, dtype=np.int32) % 2 + 5, (H, 1))
    seg = lc.desc_from_ids(ids).SerializeToString()
    dev = torch.device("cuda", 0)
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    host_r, host_i = r.level_regions(seg, 0)
    nr_, ni_ = len(host_r), len(host_i)
    assert (nr_, ni_) == (2, W * H) and nr_ * render.LEVEL_REGION_WORDS + ni_ * 4 > 2048 * 256
    # region 5 has the even columns, row after row, region 6 the odd ones
    yy, xx = np.divmod(np.arange(W * H // 2), W // 2)
    for k, rid in enumerate((5, 6)):
        want = np.stack([yy, 2 * xx + k, 2 * xx + k, np.full_like(yy, rid)], 1)
        assert np.array_equal(host_i[k * len(yy):(k + 1) * len(yy)], want), rid
    d_regions = torch.full((nr_ + 3, render.LEVEL_REGION_WORDS), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    d_intervals = torch.full((ni_ + 3, 4), 0x5A5A5A5A, dtype=torch.int32, device=dev)
    got_r, got_i = r.level_regions(seg, 0, regions_out=d_regions, intervals_out=d_intervals)
    assert got_r.shape == (nr_, render.LEVEL_REGION_WORDS) and got_i.shape == (ni_, 4)
    assert got_r.cpu().numpy().tobytes() == host_r.tobytes()
    assert got_i.cpu().numpy().tobytes() == host_i.tobytes()
    assert bool((d_regions[nr_:] == 0x5A5A5A5A).all()) and bool((d_intervals[ni_:] == 0x5A5A5A5A).all())
    r.close()


def test_vector_only_desc(vsg):
    W, H = 64, 48
    m = vc.vector_only(vc.l1_voronoi(11, W, H, 12))
    seg = m.SerializeToString()
    r = vsg.SegmentationRenderer(W, H)
    rows = r.rasterize(seg)
    want = lm.runs(vm.id_plane(rows, W, H))
    assert len(want[0]) == 12
    assert_same(r.level_regions(seg, 0), want, "vector-only")
    assert r.last_vector_stats()["crossings"] == 2 * len(rows)
    # at another size than the desc's: scan converted at the handle's
    r2 = vsg.SegmentationRenderer(96, 72)
    assert_same(r2.level_regions(seg, 0), lm.runs(vm.id_plane(r2.rasterize(seg), 96, 72)), "vector-only, scaled")
    r.close()
    r2.close()


def test_handle_reuse_small_large_small(vsg):
    small, large = BY_NAME["reuse_small"], BY_NAME["reuse_large"]
    r = vsg.SegmentationRenderer(small.W, small.H)
    want = {c.name: literal_of(c.msg, 0) for c in (small, large)}
    results, allocs = [], []
    for _ in range(2):
        for c in (small, large, small):
            seg = c.msg.SerializeToString()
            nr = len(want[c.name][0])
            regions, intervals = np.zeros(nr, lm.REGION_DTYPE), np.zeros((len(want[c.name][1]), 4), np.int32)
            got = r.level_regions(seg, 0, regions_out=regions, intervals_out=intervals)
            assert_same(got, want[c.name], c.name)
            st = r.last_level_stats()
            assert st["runs"] == len(got[1]) and st["regions"] == len(got[0]) and st["launches"] > 0
            results.append(got)
            allocs.append(r.last_stats()["device_allocations"])
    assert lm.same_bits(results[2][0], results[0][0]) and lm.same_bits(results[2][1], results[0][1])
    # the second round of identical calls allocates nothing
    assert allocs[1] > allocs[0] > 0 and allocs[3:] == [allocs[2]] * 3, allocs
    assert want["reuse_large"][0]["num_intervals"].max() == 1 and len(want["reuse_large"][0]) == 160 * 120 // 2
    r.close()


def test_dense_and_region_stage_end_to_end(vsg):
    W, H, N, chunk = 64, 48, 16, 8
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
    r = vsg.SegmentationRenderer(W, H)
    model = rm.RenderModel(W, H)
    chunks, heights = set(), []
    for k, seg in enumerate(segs):
        m = lc.Msg()
        m.ParseFromString(seg)
        chunks.add(m.chunk_id)
        hier = model._ingest(m)
        heights.append(len(hier))
        for level in range(len(hier)):
            got = r.level_regions(seg, level)
            assert_same(got, lm.literal(m, level, hier), (k, level))
            if level == len(hier) - 1:
                assert int(got[0]["area"].sum()) == int((model.id_image(m, level) != -1).sum())
    assert len(chunks) >= 2 and min(heights) >= 1 and max(heights) >= 2, heights
    r.close()


def test_full_hd_level_0_and_top(vsg):
    W, H = 1920, 1080
    ids = vc.l1_voronoi(12, W, H, 300)
    m = vc.vectorize(ids)                     # rasters; the vectorization is not looked at
    top = {int(i): 5 + int(i) % 7 for i in np.unique(ids)}
    lc.add_hierarchy(m, [top])
    seg = m.SerializeToString()
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    assert_same(r.level_regions(seg, 0), lm.runs(ids), "1080p level 0")
    lut = np.zeros(int(ids.max()) + 1, np.int32)
    for i, p in top.items():
        lut[i] = p
    mapped = lut[ids]
    want = lm.runs(mapped)
    assert len(want[0]) == 7
    assert_same(r.level_regions(seg, 1), want, "1080p top level")
    st = r.last_level_stats()
    assert st["runs_us"] > 0 and st["sort_us"] > 0 and st["table_us"] > 0 and st["moments_us"] > 0
    r.close()
