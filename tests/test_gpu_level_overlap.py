"""vsg_render_level_overlap on the MI355X (libvsg_render.so: the id plane or the component label image,
k_overlap_runs' count and emit passes, the sort of the runs, the scans, k_overlap_table, k_overlap_pairs,
k_overlap_rows, the sort by label, k_overlap_col_heads, k_overlap_cols, k_copy_lists) against
level_overlap_model.py.  Rows, cols and pairs are compared as raw bytes: there is no tolerance anywhere in
this file."""
import ctypes as C
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

import level_adjacency_model as am
import level_boundaries_cases as bc
import level_components_model as cm
import level_overlap_cases as oc
import level_overlap_model as om
import level_regions_cases as lc
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
CASES = oc.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODES = (0, cm.N4, cm.N8)          # the regions' table, the N4 components', the N8 components'
NAMES = ("rows", "cols", "pairs")
DTYPES = (om.ROW_DTYPE, om.COL_DTYPE, om.PAIR_DTYPE)
FILL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert (render.N4, render.N8) == (cm.N4, cm.N8)
    assert (render.OVERLAP_ROW_DTYPE, render.OVERLAP_COL_DTYPE, render.OVERLAP_PAIR_DTYPE) == DTYPES
    return v


def assert_same(got, want, what):
    for g, w, dtype, name in zip(got, want, DTYPES, NAMES):
        assert g.dtype == dtype and g.shape == w.shape, (what, name, g.shape, w.shape)
        assert om.same_bits(g, w), (what, name)


def planes(ids, connect):
    if connect == 0:
        return ids, None
    comps, _, labels = cm.sweep(ids, connect)
    return labels, comps


def model(ids, B, connect):
    P, comps = planes(ids, connect)
    return om.overlap(P, B, comps)


def check_stats(st, ids, B, connect, want, what):
    P, _ = planes(ids, connect)
    rows, cols, pairs = want
    covered, labelled, both = om.totals(P, B)
    assert (st["covered"], st["labelled"], st["both"]) == (covered, labelled, both), (what, st)
    assert st["both"] == pairs["count"].sum(dtype=np.int64), (what, st)
    assert st["runs"] == om.runs_of(P, B), (what, st)
    assert (st["rows"], st["cols"], st["pairs"]) == (len(rows), len(cols), len(pairs)), (what, st)
    assert st["largest_row_pairs"] == (rows["num_pairs"].max() if len(rows) else 0), (what, st)


def check_ids(r, seg, ids, B, level, what):
    """The three modes of one level against the model, with the stats and the sibling calls."""
    out = {}
    for connect in MODES:
        want = model(ids, B, connect)
        got = r.level_overlap(seg, level, B, connect)
        assert_same(got, want, (what, level, connect))
        check_stats(r.last_overlap_stats(), ids, B, connect, want, (what, level, connect))
        out[connect] = got
        # record k belongs to record k of the call the mode is named after
        rows = got[0]
        if connect == 0:
            regions, _ = r.level_regions(seg, level)
            assert np.array_equal(rows["id"], regions["id"]) and (rows["component"] == -1).all()
            assert np.array_equal(rows["area"], regions["area"])
        else:
            comps, _ = r.level_components(seg, level, connect)
            assert np.array_equal(rows["id"], comps["id"]) and np.array_equal(rows["component"], comps["component"])
            assert np.array_equal(rows["area"], comps["area"])
    return out


def check_case(vsg, c):
    r = vsg.SegmentationRenderer(c.case.W, c.case.H, has_video=False)
    out = check_ids(r, c.case.msg.SerializeToString(), lc.id_image(c.case.msg, 0), c.B, 0, c.name)
    r.close()
    return out


@pytest.mark.parametrize("W", bc.WIDTHS)
def test_widths_around_wavefront_and_block_boundaries(vsg, W):
    for H in bc.HEIGHTS:
        check_case(vsg, BY_NAME["width_%dx%d" % (W, H)])


@pytest.mark.parametrize("name", [c.name for c in CASES if c.name.startswith("wrap_")])
def test_a_pair_that_continues_in_the_next_row_is_two_runs_and_one_pair(vsg, name):
    c = BY_NAME[name]
    r = vsg.SegmentationRenderer(c.case.W, c.case.H)
    out = check_ids(r, c.case.msg.SerializeToString(), lc.id_image(c.case.msg), c.B, 0, name)
    for connect in MODES:
        r.level_overlap(c.case.msg.SerializeToString(), 0, c.B, connect)
        st = r.last_overlap_stats()
        assert st["runs"] == c.case.H and st["pairs"] == 1 and len(out[connect][2]) == 1
    r.close()


@pytest.mark.parametrize("name", ["same_hole", "same_three_levels"])
def test_the_table_of_a_plane_with_itself_is_diagonal(vsg, name):
    rows, cols, pairs = check_case(vsg, BY_NAME[name])[0]
    assert len(rows) == len(cols) == len(pairs) > 1
    assert np.array_equal(pairs["row"], pairs["col"]) and np.array_equal(pairs["count"], rows["area"])
    assert np.array_equal(rows["best_label"], rows["id"]) and np.array_equal(cols["best_row"], np.arange(len(cols)))


def test_a_plane_without_a_label(vsg):
    for connect, (rows, cols, pairs) in check_case(vsg, BY_NAME["void"]).items():
        assert len(cols) == 0 and len(pairs) == 0 and len(rows) > 0
        assert np.array_equal(rows["unlabelled"], rows["area"]) and (rows["best_label"] == -1).all()
        assert (rows["num_pairs"] == 0).all() and (rows["best_count"] == 0).all()


def test_a_frame_without_a_covered_pixel(vsg):
    c = BY_NAME["uncovered_frame"]
    for connect, (rows, cols, pairs) in check_case(vsg, c).items():
        assert len(rows) == 0 and len(pairs) == 0
        assert cols["label"].tolist() == [3, 8] and np.array_equal(cols["uncovered"], cols["area"])
        assert (cols["best_row"] == -1).all() and (cols["num_pairs"] == 0).all()
    # and with nothing labelled either: no run at all
    r = vsg.SegmentationRenderer(c.case.W, c.case.H)
    for connect in MODES:
        got = r.level_overlap(c.case.msg.SerializeToString(), 0, np.full((c.case.H, c.case.W), -3, np.int32), connect)
        assert [len(a) for a in got] == [0, 0, 0] and [a.dtype for a in got] == list(DTYPES)
        st = r.last_overlap_stats()
        assert all(st[k] == 0 for k in ("covered", "labelled", "both", "runs", "rows", "cols", "pairs"))
    r.close()


def test_a_frame_of_one_pixel_runs(vsg):
    c = BY_NAME["checker_offset"]
    assert c.case.W * c.case.H <= 64 * 8
    r = vsg.SegmentationRenderer(c.case.W, c.case.H)
    check_ids(r, c.case.msg.SerializeToString(), lc.id_image(c.case.msg), c.B, 0, c.name)
    for connect in MODES:
        r.level_overlap(c.case.msg.SerializeToString(), 0, c.B, connect)
        assert r.last_overlap_stats()["runs"] == c.case.W * c.case.H
    r.close()


@pytest.mark.parametrize("name", ["labels_300x2", "labels_2x300"])
def test_a_region_under_300_labels(vsg, name):
    for connect, (rows, cols, pairs) in check_case(vsg, BY_NAME[name]).items():
        assert rows["num_pairs"].tolist() == [oc.MANY] and len(cols) == oc.MANY
        assert np.array_equal(pairs["col"], np.arange(oc.MANY)) and np.array_equal(pairs["label"], cols["label"])
        assert rows["best_label"].tolist() == [100] and rows["best_count"].tolist() == [1]


@pytest.mark.parametrize("name", ["regions_300x2", "regions_2x300"])
def test_a_label_over_300_regions(vsg, name):
    for connect, (rows, cols, pairs) in check_case(vsg, BY_NAME[name]).items():
        assert cols["num_pairs"].tolist() == [oc.MANY] and len(rows) == oc.MANY + 1
        assert np.array_equal(pairs["row"], 1 + np.arange(oc.MANY)) and (pairs["col"] == 0).all()
        assert cols["best_row"].tolist() == [1] and rows[0]["unlabelled"] == rows[0]["area"] == oc.MANY


def test_largest_row_pairs_is_300(vsg):
    c = BY_NAME["labels_300x2"]
    r = vsg.SegmentationRenderer(c.case.W, c.case.H)
    for connect in MODES:
        r.level_overlap(c.case.msg.SerializeToString(), 0, c.B, connect)
        assert r.last_overlap_stats()["largest_row_pairs"] == oc.MANY
    r.close()


def test_id_and_label_of_31_bits_together(vsg):
    rows, cols, pairs = check_case(vsg, BY_NAME["max_values"])[0]
    assert rows["id"].tolist() == [0, oc.MAX] and cols["label"].tolist() == [0, oc.MAX]
    assert pairs[-1].tolist() == (1, 1, oc.MAX, 4)


def test_a_pitch_beyond_the_width_whose_padding_holds_labels(vsg):
    import torch
    c = BY_NAME["width_65x5"]
    W, H = c.case.W, c.case.H
    seg = c.case.msg.SerializeToString()
    padded = np.empty((H, W + 5), np.int32)
    padded[:] = 777 + np.arange(W + 5) % 2          # labels that are nowhere in B
    padded[:, :W] = c.B
    r = vsg.SegmentationRenderer(W, H)
    d_padded = torch.from_numpy(padded).cuda()
    for connect in MODES:
        want = model(lc.id_image(c.case.msg), c.B, connect)
        assert_same(r.level_overlap(seg, 0, padded[:, :W], connect), want, ("host pitch", connect))
        check_stats(r.last_overlap_stats(), lc.id_image(c.case.msg), c.B, connect, want, ("host pitch", connect))
        assert_same(r.level_overlap(seg, 0, d_padded[:, :W], connect), want, ("device pitch", connect))
        check_stats(r.last_overlap_stats(), lc.id_image(c.case.msg), c.B, connect, want, ("device pitch", connect))
    r.close()


def test_host_other_and_device_other_give_the_same_bytes(vsg):
    import torch
    c = lc.three_levels()
    seg = c.msg.SerializeToString()
    B = oc.stripes(c.W, c.H)
    d_B = torch.from_numpy(B).cuda()
    r = vsg.SegmentationRenderer(c.W, c.H)
    for level in c.levels:
        for connect in MODES:
            want = model(lc.id_image(c.msg, level), B, connect)
            assert_same(r.level_overlap(seg, level, B, connect), want, ("host", level, connect))
            assert_same(r.level_overlap(seg, level, d_B, connect), want, ("device", level, connect))
    assert bool((d_B.cpu() == torch.from_numpy(B)).all())          # B is read only
    r.close()


def test_refusals(vsg):
    from video_segment_amd import render
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    c = lc.three_levels()
    r = vsg.SegmentationRenderer(c.W, c.H)
    seg = c.msg.SerializeToString()
    B = oc.stripes(c.W, c.H)
    for level in (3, 4, -1):
        for connect in MODES:
            with pytest.raises(VsgError) as e:
                r.level_overlap(seg, level, B, connect)
            assert e.value.code == VSG_ERR_INVALID
    for connect in (3, -1):
        with pytest.raises(VsgError) as e:
            r.level_overlap(seg, 0, B, connect)
        assert e.value.code == VSG_ERR_INVALID
    # a pitch that is neither 0 nor >= W; 0 means W
    L = render.lib()
    n = [C.c_size_t(), C.c_size_t(), C.c_size_t()]

    def call(pitch):
        return L.vsg_render_level_overlap(r.h, seg, len(seg), 0, 0, B.ctypes.data_as(C.c_void_p), pitch, 0, None, 0,
                                          C.byref(n[0]), None, 0, C.byref(n[1]), None, 0, C.byref(n[2]), 0)

    for pitch in (1, c.W - 1):
        assert call(pitch) == VSG_ERR_INVALID and b"pitch" in L.vsg_render_last_error()
    want = model(lc.id_image(c.msg, 0), B, 0)
    for pitch in (0, c.W):
        assert call(pitch) == 0 and [k.value for k in n] == [len(a) for a in want]
    r.close()


def test_capacities_and_count_only(vsg):
    from video_segment_amd import render
    c = lc.three_levels()
    seg = c.msg.SerializeToString()
    B = oc.stripes(c.W, c.H)
    L = render.lib()
    r = vsg.SegmentationRenderer(c.W, c.H)

    def ptr(a):
        return a.ctypes.data_as(C.c_void_p) if a is not None else None

    for connect in (0, cm.N4):
        want = model(lc.id_image(c.msg, 1), B, connect)
        sizes = tuple(len(a) for a in want)
        assert min(sizes) > 1

        def call(outs, caps):
            n = [C.c_size_t(77), C.c_size_t(77), C.c_size_t(77)]
            rc = L.vsg_render_level_overlap(r.h, seg, len(seg), 1, connect, ptr(B), 0, 0, ptr(outs[0]), caps[0],
                                            C.byref(n[0]), ptr(outs[1]), caps[1], C.byref(n[1]), ptr(outs[2]),
                                            caps[2], C.byref(n[2]), 0)
            return (rc,) + tuple(k.value for k in n)

        assert call((None, None, None), (0, 0, 0)) == (0,) + sizes                  # count only
        outs = [np.zeros(k + 2, d) for k, d in zip(sizes, DTYPES)]
        patterns = [np.frombuffer(b"\x5a" * o.nbytes, d) for o, d in zip(outs, DTYPES)]
        # every combination of capacities one too small, and one of each at 0
        cuts = [cut for cut in itertools.product((0, 1), repeat=3) if any(cut)]
        caps = [tuple(k - d for k, d in zip(sizes, cut)) for cut in cuts]
        caps += [tuple(0 if j == k else sizes[j] for j in range(3)) for k in range(3)]
        for cap in caps:
            for o, p in zip(outs, patterns):
                o[:] = p
            assert call(outs, cap) == (-1,) + sizes, cap
            assert all(om.same_bits(o, p) for o, p in zip(outs, patterns)), cap
        assert call(outs, sizes) == (0,) + sizes                                    # exact capacities
        assert_same([o[:k] for o, k in zip(outs, sizes)], want, "exact")
        assert all(om.same_bits(o[k:], p[k:]) for o, p, k in zip(outs, patterns, sizes))
    r.close()


def test_device_outputs_equal_host_outputs(vsg):
    import torch
    from video_segment_amd import render
    c = lc.three_levels()
    seg = c.msg.SerializeToString()
    B = oc.stripes(c.W, c.H)
    dev = torch.device("cuda", 0)
    words = (render.OVERLAP_ROW_WORDS, render.OVERLAP_COL_WORDS, render.OVERLAP_PAIR_WORDS)
    r = vsg.SegmentationRenderer(c.W, c.H)
    for level in c.levels:
        for connect in MODES:
            host = r.level_overlap(seg, level, B, connect)
            sizes = [len(a) for a in host]
            outs = [torch.full((k + 3, w), FILL, dtype=torch.int32, device=dev) for k, w in zip(sizes, words)]
            got = r.level_overlap(seg, level, B, connect, rows_out=outs[0], cols_out=outs[1], pairs_out=outs[2])
            for g, h_, o, k, w in zip(got, host, outs, sizes, words):
                assert g.is_cuda and g.shape == (k, w) and g.cpu().numpy().tobytes() == h_.tobytes()
                assert bool((o[k:] == FILL).all())
            # one row, one column, one pair too few: refused, nothing written
            for cut in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
                for o in outs:
                    o.fill_(FILL)
                with pytest.raises(render.VsgError):
                    r.level_overlap(seg, level, B, connect, rows_out=outs[0][:sizes[0] - cut[0]],
                                    cols_out=outs[1][:sizes[1] - cut[1]], pairs_out=outs[2][:sizes[2] - cut[2]])
                assert all(bool((o == FILL).all()) for o in outs), cut
    r.close()


def test_vector_only_desc(vsg):
    W, H = 64, 48
    m = vc.vector_only(vc.l1_voronoi(11, W, H, 12))
    seg = m.SerializeToString()
    r = vsg.SegmentationRenderer(W, H)
    check_ids(r, seg, vm.id_plane(r.rasterize(seg), W, H), oc.stripes(W, H), 0, "vector-only")
    # at another size than the desc's: scan converted at the handle's
    r2 = vsg.SegmentationRenderer(96, 72)
    check_ids(r2, seg, vm.id_plane(r2.rasterize(seg), 96, 72), oc.stripes(96, 72), 0, "vector-only, scaled")
    r.close()
    r2.close()


def test_handle_reuse_with_the_other_level_calls_before_and_after(vsg):
    by = {c.name: c for c in lc.reuse_sequence()}
    small, large = by["reuse_small"], by["reuse_large"]
    r = vsg.SegmentationRenderer(small.W, small.H)
    segs = {c.name: c.msg.SerializeToString() for c in (small, large)}
    B = oc.stripes(small.W, small.H)

    def siblings(s):
        return (r.level_regions(s, 0), r.level_components(s, 0, cm.N8, label_image=True),
                r.level_boundaries(s, 0, cm.N4, True), r.level_adjacency(s, 0, cm.N4, am.ADJACENT_N8))

    before = {n: siblings(s) for n, s in segs.items()}
    combos = (0, cm.N8)
    want = {(c.name, k): model(lc.id_image(c.msg, 0), B, k) for c in (small, large) for k in combos}
    allocs = []
    for _ in range(2):
        for c in (small, large, small):
            for k in combos:
                assert_same(r.level_overlap(segs[c.name], 0, B, k), want[c.name, k], (c.name, k))
            allocs.append(r.last_stats()["device_allocations"])
    # the second round of identical calls allocates nothing
    assert allocs[1] > allocs[0] > 0 and allocs[3:] == [allocs[2]] * 3, allocs
    for n, s in segs.items():
        for a, b in zip(siblings(s), before[n]):
            assert all(om.same_bits(x, y) for x, y in zip(a, b)), n
    assert r.last_stats()["device_allocations"] == allocs[-1]
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


def test_the_previous_frames_id_image_passed_straight_back_in(vsg, stream):
    import torch
    W, H, N, _ = STREAM
    r = vsg.SegmentationRenderer(W, H)
    model_ = rm.RenderModel(W, H)
    dev = torch.device("cuda", 0)
    heights, compared = [], 0
    prev = None                                  # (device id images, model id images) of the frame before
    for k, seg in enumerate(stream):
        m = lc.Msg()
        m.ParseFromString(seg)
        hier = model_._ingest(m)                 # a desc without a hierarchy uses the kept one, as the handle does
        levels = max(len(hier), 1)
        heights.append(len(hier))
        want_ids = [model_.id_image(m, level) for level in range(levels)]
        if prev is not None:
            for level in range(min(levels, len(prev[0]))):
                if k % 5 == 1 or k == N - 1:     # a few frames in all modes, the others in one
                    check_ids(r, seg, want_ids[level], prev[1][level], level, ("stream", k))
                    compared += 1
                got = r.level_overlap(seg, level, prev[0][level])
                assert_same(got, om.overlap(want_ids[level], prev[1][level]), ("stream, device", k, level))
        ids = [r.id_image(seg, level, out=torch.empty((H, W), dtype=torch.int32, device=dev))
               for level in range(levels)]
        assert all(np.array_equal(a.cpu().numpy(), b) for a, b in zip(ids, want_ids))
        prev = (ids, want_ids)
    assert min(heights) >= 1 and max(heights) >= 2 and compared >= 4, (heights, compared)
    r.close()


def test_full_hd_level_0_and_top(vsg):
    import torch
    W, H = 1920, 1080
    ids = vc.l1_voronoi(12, W, H, 300)
    B = np.ascontiguousarray(vc.l1_voronoi(13, W, H, 300), np.int32)
    m = vc.vectorize(ids)                     # rasters; the vectorization is not looked at
    top = {int(i): 5 + int(i) % 7 for i in np.unique(ids)}
    lc.add_hierarchy(m, [top])
    seg = m.SerializeToString()
    lut = np.zeros(int(ids.max()) + 1, np.int32)
    for i, p in top.items():
        lut[i] = p
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    d_B = torch.from_numpy(B).cuda()
    comps, _, labels = cm.sweep(lut[ids], cm.N4)
    for level, connect, plane, of in ((0, 0, ids, None), (1, 0, lut[ids], None), (1, cm.N4, labels, comps)):
        want = om.overlap(plane, B, of)
        assert_same(r.level_overlap(seg, level, d_B, connect), want, ("1080p", level, connect))
        st = r.last_overlap_stats()
        assert st["runs"] == om.runs_of(plane, B), st
        assert (st["covered"], st["labelled"], st["both"]) == om.totals(plane, B), st
        assert (st["rows"], st["cols"], st["pairs"]) == tuple(len(a) for a in want), st
        assert st["largest_row_pairs"] == want[0]["num_pairs"].max(), st
        assert all(st[k] > 0 for k in ("plane_us", "count_us", "emit_us", "sort_us", "table_us")), st
    r.close()


def test_driver_prints_the_python_paths_sums(vsg, stream):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    r = vsg.SegmentationRenderer(W, H)
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3", "--nouse_pipeline"]
    for flags, connect in ((["--level_overlap", "0"], 0),
                           (["--level_overlap", "0", "--overlap_components", "--components_n8"], cm.N8)):
        lists, prev = [], None
        for seg in stream:
            if prev is not None:
                lists.append(r.level_overlap(seg, 0, prev, connect))
            prev = r.id_image(seg, 0)
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        m = re.search(r"level_overlap_rows=(\d+) overlap_cols=(\d+) overlap_pairs=(\d+) overlap_fnv1a32=(\w+)",
                      p.stdout)
        assert m, p.stdout
        assert [int(m.group(k)) for k in (1, 2, 3)] == [sum(len(t[k]) for t in lists) for k in range(3)]
        assert int(m.group(4), 16) == rm.fnv1a32(a for t in lists for a in t)
    r.close()
