"""The boundary distance calls on the device: D at every level and the benchmark's records at every tolerance of
every case of boundary_distance_cases against the numpy model, as raw bytes, in host and in device memory; the
cross-checks between the two calls and with the handle's id_image and persistence_image; the stats, the launch
counts, handle reuse, a vector-only desc, the hierarchy bookkeeping, the refusals, a real stream and the driver's
lines."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import boundary_distance_cases as dc
import boundary_distance_model as dm
import level_regions_cases as lc
import persistence_model as pm
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
CASES = dc.all_cases()
BY_NAME = {c.name: c for c in CASES}
GUARD = 0x5A5A5A5A
PATTERN = 0x5A


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert render.DISTANCE_NONE == dm.NONE and render.BOUNDARY_SCORE_DTYPE == dm.SCORE_DTYPE
    return v


class Expected:
    """The model's outputs of one desc, computed once: Q, D of every level, and per ground truth the records."""

    def __init__(self, ids0, hierarchy):
        self.ids0 = ids0
        self.L = pm.height(hierarchy)
        self.anc = pm.ancestors(ids0, hierarchy)
        self.q = pm.plane(ids0, self.anc)
        self.d = dm.level_distances(self.q, self.L)
        self._d_other = {}

    def records(self, name, other, T):
        if name not in self._d_other:
            self._d_other[name] = dm.distance(dm.other_edges(other))
        return dm.benchmark(self.q, self.L, other, T, self._d_other[name], self.d)


_expected = {}


def expected_of(case):
    if case.name not in _expected:
        _expected[case.name] = Expected(lc.id_image(case.msg, 0), rm.hierarchy_of(case.msg))
    return _expected[case.name]


def check_distance(r, seg, want, what, levels=None):
    """D of every level in host and in device memory, with the stats."""
    import torch
    H, W = want.q.shape
    for l in (range(want.L) if levels is None else levels):
        model = want.d[l]
        got = r.boundary_distance(seg, l)
        assert got.dtype == np.int32 and got.shape == (H, W) and got.tobytes() == model.tobytes(), (what, l)
        st = r.last_distance_stats()
        finite = model[model != dm.NONE]
        assert st["levels"] == 0 and st["other_edge_pixels"] == 0, (what, l, st)
        assert st["edge_pixels"] == int((model == 0).sum()) == int((want.q > l).sum()), (what, l, st)
        assert st["max_distance"] == (int(finite.max()) if len(finite) else 0), (what, l, st)
        assert st["launches"] > 0 and st["match_us"] == 0, (what, l, st)
        if st["edge_pixels"] == 0:
            assert st["columns_us"] == 0 and st["rows_us"] == 0, (what, l, st)
        d = torch.full((H + 1, W), GUARD, dtype=torch.int32, device="cuda:0")
        dev = r.boundary_distance(seg, l, out=d[:H])
        assert dev.is_cuda and dev.cpu().numpy().tobytes() == model.tobytes(), (what, l)
        assert bool((d[H] == GUARD).all()), (what, l)


def strided_device(plane, extra=3):
    """The plane on the device with rows W + extra apart."""
    import torch
    H, W = plane.shape
    buf = torch.full((H, W + extra), 88888, dtype=torch.int32, device="cuda:0")
    buf[:, :W] = torch.from_numpy(np.ascontiguousarray(plane))
    return buf[:, :W]


def check_benchmark(r, seg, want, others, what, tolerances=dc.TOLERANCES):
    """The records against every ground truth at every tolerance, everything in host and everything in device
    memory, with the stats."""
    import torch
    from video_segment_amd import render
    for name, other in others:
        g = dm.other_edges(other)
        d_other = strided_device(other) if name == "pitched" else torch.from_numpy(np.ascontiguousarray(other)).to("cuda:0")
        for T in tolerances:
            model = want.records(name, other, T)
            got = r.boundary_benchmark(seg, other, T)
            assert got.dtype == render.BOUNDARY_SCORE_DTYPE and got.shape == (want.L,), (what, name, T)
            assert got.tobytes() == model.tobytes(), (what, name, T, got, model)
            st = r.last_distance_stats()
            assert st["levels"] == want.L and st["edge_pixels"] == int((want.q > 0).sum()), (what, name, T, st)
            assert st["other_edge_pixels"] == int(g.sum()) and st["max_distance"] == 0, (what, name, T, st)
            if not g.any():
                assert st["columns_us"] == 0 and st["rows_us"] == 0, (what, name, T, st)
            out = torch.full((want.L + 1, render.BOUNDARY_SCORE_WORDS), GUARD, dtype=torch.int64, device="cuda:0")
            dev = r.boundary_benchmark(seg, d_other, T, out=out)
            assert dev.is_cuda and dev.shape[0] == want.L, (what, name, T)
            assert dev.cpu().numpy().tobytes() == model.tobytes(), (what, name, T)
            assert bool((out[want.L] == GUARD).all()), (what, name, T)


def cross_check(r, seg, want, others, what):
    """Between the two calls, and against the handle's sibling calls, level by level."""
    q, levels = r.persistence_image(seg)
    assert levels == want.L
    name, other = others[1]
    g = dm.other_edges(other)
    for l in range(want.L):
        d = r.boundary_distance(seg, l)
        edges = pm.edge_mask(r.id_image(seg, l))
        assert np.array_equal(d == 0, edges) and np.array_equal(edges, q > l), (what, l)
        for T in (2, 25):
            rec = r.boundary_benchmark(seg, other, T)
            assert int(rec["gt_matched"][l]) == int(((d <= T) & g).sum()), (what, l, T)
            assert int(rec["seg_edges"][l]) == int(edges.sum()), (what, l, T)


def check_case(vsg, case, tolerances=dc.TOLERANCES):
    want = expected_of(case)
    seg = case.msg.SerializeToString()
    others = dc.others(case, want.ids0)
    r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    check_distance(r, seg, want, case.name)
    check_benchmark(r, seg, want, others, case.name, tolerances)
    cross_check(r, seg, want, others, case.name)
    r.close()


@pytest.mark.parametrize("W", dc.pc.bc.WIDTHS)
def test_widths_around_tile_and_block_edges(vsg, W):
    for H in dc.pc.bc.HEIGHTS:
        check_case(vsg, BY_NAME["width_%dx%d" % (W, H)])


@pytest.mark.parametrize("L", dc.pc.LADDER_HEIGHTS)
def test_ladders(vsg, L):
    check_case(vsg, BY_NAME["ladder_%d" % L])


@pytest.mark.parametrize("name", ["three_levels", "checker", "uncovered", "uncovered_frame", "max_id", "out_of_order",
                                  "narrow_5", "narrow_7", "reuse_small", "reuse_large"])
def test_reused_case(vsg, name):
    check_case(vsg, BY_NAME[name])


@pytest.mark.parametrize("name", [c.name for c in dc.planted()])
def test_planted_frame(vsg, name):
    check_case(vsg, BY_NAME[name])


def test_closed_forms_on_the_device(vsg):
    yy, xx = np.mgrid[0:dc.PH, 0:dc.PW].astype(np.int64)
    for name, form in (("first_column", xx ** 2), ("first_row", yy ** 2)):
        case = BY_NAME[name]
        r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
        seg = case.msg.SerializeToString()
        assert np.array_equal(r.boundary_distance(seg, 0), form), name
        assert (r.boundary_distance(seg, 1) == dm.NONE).all(), name
        assert r.last_distance_stats()["edge_pixels"] == 0
        r.close()


def test_widest_frame_stages_its_row_in_128_kib(vsg):
    """32768 x 2 with column 0 different: D = x^2, the longest search there is, from the largest row buffer."""
    W, H = 32768, 2
    ids = np.ones((H, W), np.int32)
    ids[:, 0] = 0
    seg = lc.desc_from_ids(ids).SerializeToString()
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    d = r.boundary_distance(seg, 0)
    assert np.array_equal(d, np.tile(np.arange(W, dtype=np.int64) ** 2, (H, 1)))
    st = r.last_distance_stats()
    assert st["edge_pixels"] == H and st["max_distance"] == (W - 1) ** 2
    other = np.ones((H, W), np.int32)
    other[:, W - 1] = -5                                   # G is column W - 2
    rec = r.boundary_benchmark(seg, other, 4096)
    assert rec.tolist() == [(H, 0, H, 0)]
    r.close()


def test_launches_do_not_depend_on_the_height(vsg):
    counts = {}
    for L in (2, 20):
        case = BY_NAME["ladder_%d" % L]
        seg = case.msg.SerializeToString()
        other = np.tile((np.arange(case.W) % 2).astype(np.int32), (case.H, 1))
        r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
        out = []
        for _ in range(2):                                  # the second round has nothing left to allocate
            out = []
            r.boundary_distance(seg, 0)
            out.append(r.last_distance_stats()["launches"])
            for T in (0, 25):
                r.boundary_benchmark(seg, other, T)
                out.append(r.last_distance_stats()["launches"])
        assert all(n > 0 for n in out), out
        counts[L] = out
        r.close()
    assert counts[2] == counts[20], counts


def test_handle_reuse_small_large_small(vsg):
    small, large = BY_NAME["reuse_small"], BY_NAME["reuse_large"]
    r = vsg.SegmentationRenderer(small.W, small.H, has_video=False)
    allocs = []
    for _ in range(2):
        for case in (small, large, small):
            want, seg = expected_of(case), case.msg.SerializeToString()
            check_distance(r, seg, want, case.name)
            check_benchmark(r, seg, want, dc.others(case, want.ids0)[:2], case.name, (2, 25))
            allocs.append(r.last_stats()["device_allocations"])
    assert allocs[1] >= allocs[0] > 0 and allocs[3:] == [allocs[2]] * 3, allocs
    r.close()


def test_vector_only_desc(vsg):
    W, H = 64, 48
    ids = vc.l1_voronoi(11, W, H, 12)
    m = vc.vector_only(ids)
    present = sorted(int(i) for i in np.unique(ids))
    lc.add_hierarchy(m, [{i: 100 + i % 4 for i in present}, {100 + k: 200 + k // 2 for k in range(4)}])
    seg = m.SerializeToString()
    for w, h in ((W, H), (96, 72)):                    # at the desc's size, and scan converted at another
        r = vsg.SegmentationRenderer(w, h, has_video=False)
        want = Expected(vm.id_plane(r.rasterize(seg), w, h), rm.hierarchy_of(m))
        assert want.L == 3
        case = lc.Case("vector-only", m, w, h, (0, 1, 2))
        others = dc.others(case, want.ids0)
        check_distance(r, seg, want, "vector-only")
        check_benchmark(r, seg, want, others, "vector-only", (0, 4, 25))
        cross_check(r, seg, want, others, "vector-only")
        r.close()


def test_hierarchy_bookkeeping(vsg):
    """A frame with a hierarchy, then one without uses the kept one, then one of another height replaces it."""
    ids = lc.id_image(BY_NAME["ladder_4"].msg, 0)
    with_4 = BY_NAME["ladder_4"].msg
    without = lc.desc_from_ids(ids)
    with_2 = lc.desc_from_ids(ids, [{k: 70 + k // 2 for k in range(5)}])
    r = vsg.SegmentationRenderer(5, 2, has_video=False)
    want_4 = Expected(ids, rm.hierarchy_of(with_4))
    want_2 = Expected(ids, rm.hierarchy_of(with_2))
    assert (want_4.L, want_2.L) == (4, 2)
    case = lc.Case("ladder", with_4, 5, 2, ())
    others = dc.others(case, ids)[:2]
    for msg, want, what in ((with_4, want_4, "own"), (without, want_4, "kept"), (with_2, want_2, "replaced"),
                            (without, want_2, "kept again")):
        seg = msg.SerializeToString()
        check_distance(r, seg, want, what)
        check_benchmark(r, seg, want, others, what, (0, 2))
    r.close()


def _filled(n, dtype):
    return np.frombuffer(bytes([PATTERN]) * (n * np.dtype(dtype).itemsize), dtype).copy()


def test_refusals_leave_the_outputs_untouched(vsg):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    from video_segment_amd import render
    base = BY_NAME["three_levels"]
    missing = lc.Msg()
    missing.CopyFrom(base.msg)
    del missing.hierarchy[1].region[3]                     # an id level 1 lacks
    unsorted = lc.Msg()
    unsorted.CopyFrom(base.msg)
    a, b = unsorted.hierarchy[0].region[0], unsorted.hierarchy[0].region[1]
    a.id, b.id = b.id, a.id
    tall = lc.desc_from_ids(np.array([[0, 1]], np.int32))
    for l in range(65536):                                 # L = 65536
        level = tall.hierarchy.add()
        for k in (0, 1):
            c = level.region.add()
            c.id, c.size, c.parent_id = k, 1, k
    tallest = lc.Msg()
    tallest.CopyFrom(tall)
    del tallest.hierarchy[-1]                              # L = 65535 is served
    r = vsg.SegmentationRenderer(base.W, base.H, has_video=False)
    r2 = vsg.SegmentationRenderer(2, 1, has_video=False)
    for handle, msg, W, H, level in ((r, missing, base.W, base.H, 2), (r, unsorted, base.W, base.H, 1),
                                     (r2, tall, 2, 1, 0)):
        seg = msg.SerializeToString()
        plane = _filled(W * H, np.int32).reshape(H, W)
        records = _filled(65536, dm.SCORE_DTYPE)
        other = np.zeros((H, W), np.int32)
        calls = [lambda: handle.boundary_benchmark(seg, other, 4, out=records)]
        if handle is r:                                    # the distance call has no limit on L: it looks at one level
            calls.append(lambda: handle.boundary_distance(seg, level, out=plane))
        for call in calls:
            with pytest.raises(VsgError) as e:
                call()
            assert e.value.code == VSG_ERR_INVALID
        assert all((np.frombuffer(x.tobytes(), np.uint8) == PATTERN).all() for x in (plane, records))
    for level in (-1, 3):                                  # a level the hierarchy does not have
        plane = _filled(base.W * base.H, np.int32).reshape(base.H, base.W)
        with pytest.raises(VsgError) as e:
            r.boundary_distance(base.msg.SerializeToString(), level, out=plane)
        assert e.value.code == VSG_ERR_INVALID and (plane == GUARD).all()
    other = np.array([[0, 1]], np.int32)
    rec = r2.boundary_benchmark(tallest.SerializeToString(), other, 0)
    assert len(rec) == 65535 and (rec["seg_edges"] == 1).all() and (rec["seg_matched"] == 1).all()
    assert (rec["gt_edges"] == 1).all() and (rec["gt_matched"] == 1).all()

    # the capacity one too small, the count-only call, a pitch below the width, the tolerance's range
    L = render.lib()
    seg = base.msg.SerializeToString()
    want = expected_of(base)
    other = dc.random_labels(base.W, base.H, 9)
    model = want.records("refusals", other, 25)
    assert want.L == 3

    def call(scores, capacity, T=25, pitch=0):
        n = C.c_size_t(77)
        rc = L.vsg_render_boundary_benchmark(r.h, seg, len(seg), other.ctypes.data_as(C.c_void_p), pitch, 0, T,
                                             scores.ctypes.data_as(C.c_void_p) if scores is not None else None,
                                             capacity, C.byref(n), 0)
        return rc, n.value

    assert call(None, 0) == (0, 3)                                                     # count only
    records = _filled(5, dm.SCORE_DTYPE)
    for capacity in (2, 1, 0):
        assert call(records, capacity) == (-1, 3)
        assert (np.frombuffer(records.tobytes(), np.uint8) == PATTERN).all(), capacity
    assert call(records, 3, pitch=base.W - 1) == (-1, 77)
    assert call(records, 3, T=4097) == (-1, 77) and call(records, 3, T=-1) == (-1, 77)
    assert (np.frombuffer(records.tobytes(), np.uint8) == PATTERN).all()
    assert call(records, 3) == (0, 3)
    assert records[:3].tobytes() == model.tobytes()
    assert (np.frombuffer(records[3:].tobytes(), np.uint8) == PATTERN).all()
    assert call(records, 5) == (0, 3)
    for x in (r, r2):
        x.close()


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
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    model_ = rm.RenderModel(W, H)
    heights, previous = [], None
    for k, seg in enumerate(stream):
        m = lc.Msg()
        m.ParseFromString(seg)
        hier = model_._ingest(m)             # a desc without a hierarchy uses the kept one, as the handle does
        heights.append(len(hier))
        ids0 = np.ascontiguousarray(model_.id_image(m, 0), dtype=np.int32)
        if previous is not None and (k % 5 == 0 or k == N - 1):   # every frame is ingested, a few are compared
            want = Expected(ids0, hier)
            others = [("previous", previous), ("random", dc.random_labels(W, H, k))]
            check_distance(r, seg, want, ("stream", k))
            check_benchmark(r, seg, want, others, ("stream", k), (0, 4, 25))
            cross_check(r, seg, want, others, ("stream", k))
        else:
            r.boundary_distance(seg, 0)
            assert r.last_distance_stats()["levels"] == 0
        previous = ids0
    assert min(heights) >= 1 and max(heights) >= 2, heights
    r.close()


def test_driver_prints_the_python_paths_sums(vsg, stream):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3", "--nouse_pipeline"]
    # --boundary_distance <level>
    level = 1
    arrays, edge_pixels, largest = [], 0, 0
    for seg in stream:
        d = r.boundary_distance(seg, level)
        st = r.last_distance_stats()
        edge_pixels += st["edge_pixels"]
        largest = max(largest, st["max_distance"])
        arrays.append(d)
    p = subprocess.run(base + ["--boundary_distance", str(level)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    m = re.search(r"boundary_distance_level=(\d+) boundary_distance_edge_pixels=(\d+) boundary_distance_max=(\d+) "
                  r"boundary_distance_fnv1a32=(\w+)", p.stdout)
    assert m, p.stdout
    assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (level, edge_pixels, largest)
    assert int(m.group(4), 16) == rm.fnv1a32(arrays)
    # --boundary_benchmark <tolerance_sq>
    T = 4
    arrays, sums, levels, previous = [], np.zeros(4, np.int64), 0, None
    for seg in stream:
        if previous is not None:
            rec = r.boundary_benchmark(seg, previous, T)
            levels = len(rec)
            sums += [int(rec[f].sum()) for f in ("seg_edges", "seg_matched", "gt_edges", "gt_matched")]
            arrays.append(rec)
        previous = r.id_image(seg, 0)
    p = subprocess.run(base + ["--boundary_benchmark", str(T)], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr
    m = re.search(r"boundary_benchmark_levels=(\d+) boundary_seg_edges=(\d+) boundary_seg_matched=(\d+) "
                  r"boundary_gt_edges=(\d+) boundary_gt_matched=(\d+) boundary_benchmark_fnv1a32=(\w+)", p.stdout)
    assert m, p.stdout
    assert int(m.group(1)) == levels and [int(m.group(k)) for k in (2, 3, 4, 5)] == sums.tolist()
    assert int(m.group(6), 16) == rm.fnv1a32(arrays)
    r.close()
