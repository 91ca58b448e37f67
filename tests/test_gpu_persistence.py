"""Boundary persistence on the device: the plane, the picture and the graph of every case of persistence_cases
against the numpy model, as raw bytes, in host and in device memory; the cross-checks with the handle's own
id_image and level_adjacency at every level; the hierarchy bookkeeping, the refusals, the stats, a real
stream and the driver's line."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import level_adjacency_model as am
import level_regions_cases as lc
import persistence_cases as pc
import persistence_model as pm
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
CASES = pc.all_cases()
BY_NAME = {c.name: c for c in CASES}
HOODS = (am.ADJACENT_N4, am.ADJACENT_N8)
PATTERN = 0x5A


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert (render.ADJACENT_N4, render.ADJACENT_N8) == HOODS
    assert render.LEVEL_NODE_DTYPE == am.NODE_DTYPE and render.LEVEL_EDGE_DTYPE == am.EDGE_DTYPE
    return v


def source_frame(W, H):
    return np.random.RandomState(W * 131 + H).randint(0, 256, (H, W, 3)).astype(np.uint8)


def strided(W, H, stride, offset, device=None):
    """(buffer, H x W x 3 view of it) with rows `stride` bytes apart, the first one `offset` bytes in."""
    n = offset + stride * H
    if device is None:
        buf = np.full(n, PATTERN, np.uint8)
        return buf, np.lib.stride_tricks.as_strided(buf[offset:], (H, W, 3), (stride, 3, 1))
    import torch
    buf = torch.full((n,), PATTERN, dtype=torch.uint8, device=device)
    return buf, torch.as_strided(buf, (H, W, 3), (stride, 3, 1), offset)


def gaps_untouched(buf, W, H, stride, offset):
    """Everything of the buffer but the first 3 * W bytes of each row still holds the pattern."""
    b = np.array(buf.cpu().numpy() if hasattr(buf, "cpu") else buf, copy=True)
    for y in range(H):
        b[offset + y * stride:offset + y * stride + 3 * W] = PATTERN
    return bool((b == PATTERN).all())


class Expected:
    """The model's outputs of one desc, computed once."""

    def __init__(self, ids0, hierarchy):
        self.ids0 = ids0
        self.L = pm.height(hierarchy)
        self.anc = pm.ancestors(ids0, hierarchy)
        self.q = pm.plane(ids0, self.anc)
        self.graph = {hood: pm.graph(ids0, hood, self.anc) for hood in HOODS}


_expected = {}


def expected_of(case):
    if case.name not in _expected:
        _expected[case.name] = Expected(lc.id_image(case.msg, 0), rm.hierarchy_of(case.msg))
    return _expected[case.name]


def check_plane(r, seg, want, what, regions=None):
    import torch
    H, W = want.q.shape
    q, levels = r.persistence_image(seg)
    assert levels == want.L, (what, levels)
    assert q.dtype == np.int32 and q.tobytes() == want.q.tobytes(), what
    st = r.last_persistence_stats()
    assert st["levels"] == want.L and st["edge_pixels"] == int((want.q > 0).sum()), (what, st)
    assert st["top_pixels"] == int((want.q == want.L).sum()), (what, st)
    assert st["regions"] == (len(want.anc[0]) if regions is None else regions), (what, st)
    assert st["nodes"] == 0 and st["edges"] == 0 and st["graph_us"] == 0 and st["compose_us"] == 0, (what, st)
    d = torch.full((H + 1, W), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    got, levels = r.persistence_image(seg, out=d[:H])
    assert levels == want.L and got.is_cuda and got.cpu().numpy().tobytes() == want.q.tobytes(), what
    assert bool((d[H] == 0x5A5A5A5A).all()), what
    return st


def check_pictures(r, seg, want, src, what):
    """The picture in host and in device memory, with the default, an aligned and an odd row stride, and from
    an odd address.  src: the handle's source frame, or None for a handle without video."""
    import torch
    H, W = want.q.shape
    pic = pm.picture(want.q, want.L, src)
    got = r.persistence_frame(seg, src)
    assert got.dtype == np.uint8 and got.tobytes() == pic.tobytes(), what
    st = r.last_persistence_stats()
    assert st["levels"] == want.L and st["edge_pixels"] == int((want.q > 0).sum()), (what, st)
    assert st["top_pixels"] == int((want.q == want.L).sum()) and st["nodes"] == 0 and st["edges"] == 0, (what, st)
    d_src = None if src is None else torch.from_numpy(src).to("cuda:0")
    aligned = (3 * W + 3) // 4 * 4 + 4
    odd = 3 * W + 1 + (3 * W) % 2                      # an odd number of bytes
    for stride, offset in ((aligned, 0), (odd, 0), (aligned, 1), (3 * W, 3)):
        for device in (None, "cuda:0"):
            buf, view = strided(W, H, stride, offset, device)
            r.persistence_frame(seg, d_src if device else src, out=view)
            back = view.cpu().numpy() if device else view
            assert np.ascontiguousarray(back).tobytes() == pic.tobytes(), (what, stride, offset, device)
            assert gaps_untouched(buf, W, H, stride, offset), (what, stride, offset, device)


def assert_graph(got, want, what):
    names = ("nodes", "edges", "persistence", "level_sides")
    dtypes = (am.NODE_DTYPE, am.EDGE_DTYPE, np.int32, np.int64)
    for g, w, n, dt in zip(got, want, names, dtypes):
        assert g.dtype == dt and g.shape == w.shape, (what, n, g.shape, w.shape)
        assert np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes(), (what, n)


def check_graph(r, seg, want, what):
    import torch
    from video_segment_amd import render
    for hood in HOODS:
        model = want.graph[hood]
        got = r.persistence_graph(seg, hood)
        assert_graph(got, model, (what, hood))
        st = r.last_persistence_stats()
        assert st["levels"] == want.L and st["nodes"] == len(model[0]) and st["edges"] == len(model[1]), (what, st)
        assert st["edge_pixels"] == 0 and st["top_pixels"] == 0 and st["compose_us"] == 0, (what, st)
        nn, ne = len(model[0]), len(model[1])
        outs = (torch.full((nn + 1, render.LEVEL_NODE_WORDS), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0"),
                torch.full((ne + 1, render.LEVEL_EDGE_WORDS), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0"),
                torch.full((ne + 1,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0"),
                torch.full((want.L + 1,), 0x5A5A5A5A, dtype=torch.int64, device="cuda:0"))
        dev = r.persistence_graph(seg, hood, *outs)
        assert all(t.is_cuda for t in dev)
        for t, w, full in zip(dev, model, outs):
            assert t.cpu().numpy().tobytes() == np.ascontiguousarray(w).tobytes(), (what, hood)
            assert bool((full[len(w):] == 0x5A5A5A5A).all()), (what, hood)


def cross_check(r, seg, want, what):
    """Against the handle's own sibling calls, level by level."""
    q = want.q
    for l in range(want.L):
        assert np.array_equal(q > l, pm.edge_mask(r.id_image(seg, l))), (what, l)
        level_nodes, _ = r.level_adjacency(seg, l)
        assert 2 * int(want.graph[am.ADJACENT_N4][3][l]) == int(level_nodes["border_shared"].sum(dtype=np.int64))
    for hood in HOODS:
        nodes, edges = r.level_adjacency(seg, 0, 0, hood)
        assert am.same_bits(nodes, want.graph[hood][0]) and am.same_bits(edges, want.graph[hood][1]), (what, hood)


def check_case(vsg, case):
    want = expected_of(case)
    seg = case.msg.SerializeToString()
    plain = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    check_plane(plain, seg, want, case.name)
    check_graph(plain, seg, want, case.name)
    cross_check(plain, seg, want, case.name)
    check_pictures(plain, seg, want, None, case.name)
    video = vsg.SegmentationRenderer(case.W, case.H)
    check_pictures(video, seg, want, source_frame(case.W, case.H), case.name)
    video.close()
    plain.close()


@pytest.mark.parametrize("W", pc.bc.WIDTHS)
def test_widths_around_tile_and_block_edges(vsg, W):
    for H in pc.bc.HEIGHTS:
        check_case(vsg, BY_NAME["width_%dx%d" % (W, H)])


@pytest.mark.parametrize("L", pc.LADDER_HEIGHTS)
def test_ladder_hits_every_value_and_every_end_of_the_bisection(vsg, L):
    case = BY_NAME["ladder_%d" % L]
    want = expected_of(case)
    assert want.L == L and sorted(set(want.q.ravel().tolist())) == list(range(L + 1))
    check_case(vsg, case)


@pytest.mark.parametrize("name", ["three_levels", "checker", "uncovered", "uncovered_frame", "max_id", "out_of_order",
                                  "narrow_5", "narrow_7"])
def test_named_case(vsg, name):
    check_case(vsg, BY_NAME[name])


def test_handle_reuse_small_large_small(vsg):
    small, large = BY_NAME["reuse_small"], BY_NAME["reuse_large"]
    r = vsg.SegmentationRenderer(small.W, small.H, has_video=False)
    video = vsg.SegmentationRenderer(small.W, small.H)
    src = source_frame(small.W, small.H)
    allocs, video_allocs = [], []
    for _ in range(2):
        for case in (small, large, small):
            want, seg = expected_of(case), case.msg.SerializeToString()
            check_plane(r, seg, want, case.name)
            check_graph(r, seg, want, case.name)
            check_pictures(r, seg, want, None, case.name)
            allocs.append(r.last_stats()["device_allocations"])
            check_pictures(video, seg, want, src, case.name)
            video_allocs.append(video.last_stats()["device_allocations"])
    for a in (allocs, video_allocs):
        assert a[1] > a[0] > 0 and a[3:] == [a[2]] * 3, a
    r.close()
    video.close()


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
        check_plane(r, seg, want, "vector-only", regions=len(present))
        check_graph(r, seg, want, "vector-only")
        cross_check(r, seg, want, "vector-only")
        check_pictures(r, seg, want, None, "vector-only")
        video = vsg.SegmentationRenderer(w, h)
        check_pictures(video, seg, want, source_frame(w, h), "vector-only")
        r.close()
        video.close()


def test_hierarchy_bookkeeping(vsg):
    """A frame with a hierarchy, then one without uses the kept one, then one of another height replaces it."""
    ids = lc.id_image(BY_NAME["ladder_4"].msg, 0)
    with_4 = BY_NAME["ladder_4"].msg
    without = lc.desc_from_ids(ids)
    with_2 = lc.desc_from_ids(ids, [{k: 70 + k // 2 for k in range(5)}])
    r = vsg.SegmentationRenderer(5, 2, has_video=False)
    fresh = vsg.SegmentationRenderer(5, 2, has_video=False)
    want_1 = Expected(ids, [])
    check_plane(fresh, without.SerializeToString(), want_1, "no hierarchy at all")
    fresh.close()
    want_4 = Expected(ids, rm.hierarchy_of(with_4))
    want_2 = Expected(ids, rm.hierarchy_of(with_2))
    assert (want_1.L, want_4.L, want_2.L) == (1, 4, 2)
    for msg, want, what in ((with_4, want_4, "own"), (without, want_4, "kept"), (with_2, want_2, "replaced"),
                            (without, want_2, "kept again")):
        seg = msg.SerializeToString()
        check_plane(r, seg, want, what)
        check_graph(r, seg, want, what)
        _, _, _, level_sides = r.persistence_graph(seg)
        assert len(level_sides) == want.L, what
    r.close()


def _filled(n, dtype):
    return np.frombuffer(bytes([PATTERN]) * (n * np.dtype(dtype).itemsize), dtype).copy()


def test_refusals_leave_the_outputs_untouched(vsg):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    from video_segment_amd import render
    base = BY_NAME["three_levels"]
    ids = lc.id_image(base.msg, 0)
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
    for handle, msg, W, H in ((r, missing, base.W, base.H), (r, unsorted, base.W, base.H), (r2, tall, 2, 1)):
        seg = msg.SerializeToString()
        plane = _filled(W * H, np.int32).reshape(H, W)
        frame = _filled(W * H * 3, np.uint8).reshape(H, W, 3)
        lists = (_filled(64, am.NODE_DTYPE), _filled(256, am.EDGE_DTYPE), _filled(256, np.int32),
                 _filled(65536, np.int64))
        for call in (lambda: handle.persistence_image(seg, out=plane),
                     lambda: handle.persistence_frame(seg, out=frame),
                     lambda: handle.persistence_graph(seg, am.ADJACENT_N4, *lists)):
            with pytest.raises(VsgError) as e:
                call()
            assert e.value.code == VSG_ERR_INVALID
        assert all((np.frombuffer(x.tobytes(), np.uint8) == PATTERN).all() for x in (plane, frame) + lists)
    q, levels = r2.persistence_image(tallest.SerializeToString())
    assert levels == 65535 and q.tolist() == [[65535, 0]]
    _, _, persistence, level_sides = r2.persistence_graph(tallest.SerializeToString())
    assert persistence.tolist() == [65535, 65535] and len(level_sides) == 65535 and (level_sides == 1).all()

    # capacities one too small, count-only calls
    L = render.lib()
    seg = base.msg.SerializeToString()
    want = expected_of(base)
    for hood in HOODS:
        nodes_, edges_, pers_, sides_ = want.graph[hood]
        nn_, ne_, nl_ = len(nodes_), len(edges_), want.L
        assert nn_ > 1 and ne_ > 1 and nl_ == 3

        def ptr(x):
            return x.ctypes.data_as(C.c_void_p) if x is not None else None

        def call(nodes, cap_n, edges, cap_e, pers, sides, cap_l):
            nn, ne, nl = C.c_size_t(77), C.c_size_t(77), C.c_size_t(77)
            rc = L.vsg_render_persistence_graph(r.h, seg, len(seg), hood, ptr(nodes), cap_n, C.byref(nn), ptr(edges),
                                                cap_e, C.byref(ne), ptr(pers), ptr(sides), cap_l, C.byref(nl), 0)
            return rc, nn.value, ne.value, nl.value

        assert call(None, 0, None, 0, None, None, 0) == (0, nn_, ne_, nl_)             # count only
        lists = (_filled(nn_ + 2, am.NODE_DTYPE), _filled(ne_ + 2, am.EDGE_DTYPE), _filled(ne_ + 2, np.int32),
                 _filled(nl_ + 2, np.int64))
        for cap_n, cap_e, cap_l in ((nn_ - 1, ne_, nl_), (nn_, ne_ - 1, nl_), (nn_, ne_, nl_ - 1), (0, ne_, nl_),
                                    (nn_, ne_, 0)):
            got = call(lists[0], cap_n, lists[1], cap_e, lists[2], lists[3], cap_l)
            assert got == (-1, nn_, ne_, nl_), (cap_n, cap_e, cap_l, got)
            assert all((np.frombuffer(x.tobytes(), np.uint8) == PATTERN).all() for x in lists), (cap_n, cap_e, cap_l)
        assert call(lists[0], nn_, lists[1], ne_, lists[2], lists[3], nl_) == (0, nn_, ne_, nl_)
        assert_graph((lists[0][:nn_], lists[1][:ne_], lists[2][:ne_], lists[3][:nl_]), want.graph[hood], "exact")
        for x, n in zip(lists, (nn_, ne_, ne_, nl_)):
            assert (np.frombuffer(x[n:].tobytes(), np.uint8) == PATTERN).all()
    for hood in (0, 3, -1):
        with pytest.raises(VsgError) as e:
            r.persistence_graph(seg, hood)
        assert e.value.code == VSG_ERR_INVALID
    video = vsg.SegmentationRenderer(base.W, base.H)
    with pytest.raises(ValueError):
        video.persistence_frame(seg)                       # has_video: the source frame is required
    levels = C.c_int(0)
    out = np.zeros((base.H, base.W, 3), np.uint8)
    assert L.vsg_render_persistence_frame(video.h, seg, len(seg), None, 0, 0, out.ctypes.data_as(C.c_void_p), 0, 0,
                                          C.byref(levels)) == -1
    # ... and ignored without has_video
    assert L.vsg_render_persistence_frame(r.h, seg, len(seg), None, 0, 0, out.ctypes.data_as(C.c_void_p), 3 * base.W,
                                          0, C.byref(levels)) == 0 and levels.value == 3
    assert out.tobytes() == pm.picture(want.q, 3).tobytes()
    for x in (r, r2, video):
        x.close()


def test_launches_do_not_depend_on_the_height(vsg):
    counts = {}
    for L in (2, 20):
        case = BY_NAME["ladder_%d" % L]
        seg = case.msg.SerializeToString()
        plain = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
        video = vsg.SegmentationRenderer(case.W, case.H)
        src = source_frame(case.W, case.H)
        out = []
        for _ in range(2):                                  # the second round has nothing left to allocate
            out = []
            plain.persistence_image(seg)
            out.append(plain.last_persistence_stats()["launches"])
            plain.persistence_frame(seg)
            out.append(plain.last_persistence_stats()["launches"])
            video.persistence_frame(seg, src)
            out.append(video.last_persistence_stats()["launches"])
            for hood in HOODS:
                plain.persistence_graph(seg, hood)
                out.append(plain.last_persistence_stats()["launches"])
        assert all(n > 0 for n in out), out
        counts[L] = out
        plain.close()
        video.close()
    assert counts[2] == counts[20], counts


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
    video = vsg.SegmentationRenderer(W, H)
    src = source_frame(W, H)
    model_ = rm.RenderModel(W, H)
    heights = []
    for k, seg in enumerate(stream):
        m = lc.Msg()
        m.ParseFromString(seg)
        hier = model_._ingest(m)             # a desc without a hierarchy uses the kept one, as the handle does
        heights.append(len(hier))
        if k % 5 == 0 or k == N - 1:         # every frame is ingested, a few are compared at every level
            want = Expected(model_.id_image(m, 0), hier)
            check_plane(r, seg, want, ("stream", k))
            check_graph(r, seg, want, ("stream", k))
            cross_check(r, seg, want, ("stream", k))
            check_pictures(r, seg, want, None, ("stream", k))
            check_pictures(video, seg, want, src, ("stream", k))
        else:
            _, levels = r.persistence_image(seg)
            assert levels == max(1, len(hier))
            video.persistence_frame(seg, src)
            assert video.last_persistence_stats()["levels"] == levels
    assert min(heights) >= 1 and max(heights) >= 2, heights
    r.close()
    video.close()


def test_driver_prints_the_python_paths_sums(vsg, stream):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    r = vsg.SegmentationRenderer(W, H, has_video=False)
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3", "--nouse_pipeline"]
    for flags, hood in ((["--persistence"], am.ADJACENT_N4), (["--persistence", "--adjacency_n8"], am.ADJACENT_N8)):
        arrays, edge_pixels, edges, levels = [], 0, 0, 0
        for seg in stream:
            q, levels = r.persistence_image(seg)
            edge_pixels += int((q > 0).sum())
            _, e, persistence, level_sides = r.persistence_graph(seg, hood)
            edges += len(e)
            arrays += [q, persistence, level_sides]
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        m = re.search(r"persistence_levels=(\d+) persistence_edge_pixels=(\d+) persistence_edges=(\d+) "
                      r"persistence_fnv1a32=(\w+)", p.stdout)
        assert m, p.stdout
        assert (int(m.group(1)), int(m.group(2)), int(m.group(3))) == (levels, edge_pixels, edges)
        assert int(m.group(4), 16) == rm.fnv1a32(arrays)
    r.close()
