"""vsg_render_level_mesh on the MI355X (libvsg_render.so: the contour stages, then k_mesh_junctions, k_mesh_seed,
the third pointer doubling, k_mesh_loop_counts, k_mesh_halves, the segments' sort, k_mesh_seg_heads,
k_mesh_vertices, k_mesh_records, k_mesh_links, k_mesh_measure, k_mesh_finish, k_copy_lists) against
level_mesh_model.py, and against the contours, adjacency and rasterize calls of the same handle.  All four lists
are compared as raw bytes: there is no tolerance anywhere in this file."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import level_components_model as cm
import level_contours_model as tm
import level_mesh_cases as mc
import level_mesh_model as mm
import level_regions_cases as lc
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
CASES = mc.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODES = (0, cm.N4, cm.N8)
NAMES = ("segments", "vertices", "loops", "refs")


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert (render.N4, render.N8) == (cm.N4, cm.N8)
    assert render.MESH_SEGMENT_DTYPE == mm.SEGMENT_DTYPE and render.MESH_LOOP_DTYPE == mm.LOOP_DTYPE
    return v


def assert_same(got, want, what):
    assert len(got) == len(want) == 4
    for name, a, b in zip(NAMES, got, want):
        assert a.dtype == b.dtype and a.shape == b.shape, (what, name, a.shape, b.shape)
        assert mm.same_bits(a, b), (what, name)


def plane_of(ids, connect):
    """(plane, components or None) of a mode."""
    if connect == 0:
        return ids, None
    comps, _, labels = cm.sweep(ids, connect)
    return labels, comps


def model(ids, connect):
    plane, comps = plane_of(ids, connect)
    return mm.mesh(plane, comps)


def rounds_of(cracks):
    """Three doublings, ceil(log2 cracks) rounds each, made even: a launch does two."""
    return 3 * ((int(cracks - 1).bit_length() + 1) // 2 * 2) if cracks else 0


def check_ids(r, seg, ids, level, what, modes=MODES):
    """Every mode of one level against the model, with the counts and the sibling calls on the same handle."""
    from video_segment_amd import render
    out = {}
    for connect in modes:
        plane, comps = plane_of(ids, connect)
        want = mm.mesh(plane, comps)
        got = r.level_mesh(seg, level, connect)
        assert_same(got, want, (what, level, connect))
        st = r.last_mesh_stats()
        assert {k: st[k] for k in mm.COUNTS} == mm.stats_of(plane, want), (what, level, connect)
        assert st["rounds"] == rounds_of(st["cracks"]), (what, level, connect)
        # the internal contour run is the one the contour stats describe
        ct = r.last_contour_stats()
        assert ct["cracks"] == st["cracks"] and ct["contours"] == st["loops"], (what, level, connect)
        out[connect] = got
        segments, vertices, loops, refs = got
        if not len(segments):
            continue
        # the polygons of the contours call
        records, contour_vertices = r.level_contours(seg, level, connect)
        assert np.array_equal(loops["group"], records["group"]), (what, level, connect)
        assert np.array_equal(loops["length"], records["length"]), (what, level, connect)
        mine = render.mesh_polygons(segments, vertices, loops, refs)
        theirs = render.contour_polygons(records, contour_vertices)
        assert len(mine) == len(theirs), (what, level, connect)
        for a, b in zip(mine, theirs):
            assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b)), (what, level, connect)
        # the border lengths of the adjacency call
        nodes, edges = r.level_adjacency(seg, level, connect)
        shared = segments[segments["left"] >= 0]
        pair = {}
        for s in shared:
            pair[int(s["left"]), int(s["right"])] = pair.get((int(s["left"]), int(s["right"])), 0) + int(s["length"])
        theirs = {}
        for k, node in enumerate(nodes):
            for e in edges[node["first_edge"]:node["first_edge"] + node["num_edges"]]:
                if e["shared_n4"] and e["neighbour"] > k:
                    theirs[k, int(e["neighbour"])] = int(e["shared_n4"])
        assert pair == theirs, (what, level, connect)
        alone = segments[segments["left"] < 0]
        border = np.bincount(alone["right"], alone["length"], len(nodes)).astype(np.int64)
        assert np.array_equal(border, nodes["border_frame"].astype(np.int64) + nodes["border_uncovered"]), (what, level)
    return out


def check_case(vsg, case, modes=MODES):
    r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    seg = case.msg.SerializeToString()
    out = {level: check_ids(r, seg, lc.id_image(case.msg, level), level, case.name, modes) for level in case.levels}
    r.close()
    return out


@pytest.mark.parametrize("name", sorted(BY_NAME))
def test_every_case_in_every_mode_at_every_level(vsg, name):
    check_case(vsg, BY_NAME[name])


def test_the_shapes_a_mesh_gets_wrong(vsg):
    for name in ("one_region_1x1", "one_region_7x1", "one_region_1x7"):
        c = BY_NAME[name]
        for connect, got in check_case(vsg, c)[0].items():
            assert got[0].tolist() == [(0, -1, 0, 4, 2 * c.W + 2 * c.H, 1, 0, 0)] and got[3].tolist() == [0]
            assert got[1].tolist() == [[0, 0], [c.W, 0], [c.W, c.H], [0, c.H]]
    got = check_case(vsg, BY_NAME["saddle_2x2"])[0]
    assert [len(set(got[k][2]["group"].tolist())) for k in MODES] == [2, 4, 2]
    assert all((got[k][0]["start_sides"].tolist() + got[k][0]["end_sides"].tolist()).count(4) == 4 for k in MODES)
    segments, vertices, _, _ = check_case(vsg, BY_NAME["t_junction"], (0,))[0][0]
    bar = [vertices[s["first_vertex"]:s["first_vertex"] + s["num_vertices"]].tolist() for s in segments
           if s["left"] == 0]
    assert sorted(bar) == [[[0, 2], [3, 2]], [[3, 2], [6, 2]]]
    hi = check_case(vsg, BY_NAME["island_7_in_2"], (0,))[0][0]
    lo = check_case(vsg, BY_NAME["island_2_in_7"], (0,))[0][0]
    assert hi[3].tolist() == [0, ~1, 1] and lo[3].tolist() == [~1, 0, 1]
    segments = check_case(vsg, BY_NAME["uncovered_hole"], (0,))[0][0][0]
    assert segments["closed"].tolist() == [1, 1] and segments["left"].tolist() == [-1, -1]
    r = vsg.SegmentationRenderer(5, 4, has_video=False)
    r.level_mesh(BY_NAME["uncovered_edge_pixel"].msg.SerializeToString())
    assert r.last_mesh_stats()["junctions"] == 0 and r.last_mesh_stats()["closed_segments"] == 1
    r.close()
    segments = check_case(vsg, BY_NAME["border_to_edge"], (0,))[0][0][0]
    assert (segments["start_sides"] == 3).all() and (segments["end_sides"] == 3).all() and len(segments) == 3
    for name in ("diagonal_islands_5_5", "diagonal_islands_5_6"):
        segments, vertices, _, _ = check_case(vsg, BY_NAME[name], (0,))[0][0]
        small = segments[segments["length"] == 4]
        assert len(small) == 2 and (small["closed"] == 0).all() and (small["num_vertices"] == 5).all()
        for s in small:
            assert vertices[s["first_vertex"]].tolist() == vertices[s["first_vertex"] + 4].tolist() == [3, 3]
    c = BY_NAME["pixel_checker"]
    segments = check_case(vsg, c, (0,))[0][0][0]
    inner = segments[segments["left"] >= 0]
    assert (inner["length"] == 1).all() and len(inner) == (c.W - 1) * c.H + c.W * (c.H - 1)
    segments = check_case(vsg, BY_NAME["stripes_4096x3"], (0,))[0][0][0]
    border = segments[segments["left"] >= 0]
    assert len(border) == 1 and border[0]["length"] == 4096 and border[0]["num_vertices"] == 2
    segments = check_case(vsg, BY_NAME["spiral_in_a_region"], (0,))[0][0][0]
    assert segments["length"].max() > 129 * 65 // 2


def test_a_frame_without_a_covered_pixel(vsg):
    c = BY_NAME["uncovered_frame"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    for connect in MODES:
        segments, vertices, loops, refs = r.level_mesh(c.msg.SerializeToString(), 0, connect)
        assert segments.shape == (0,) and segments.dtype == mm.SEGMENT_DTYPE
        assert vertices.shape == (0, 2) and vertices.dtype == np.int32
        assert loops.shape == (0,) and loops.dtype == mm.LOOP_DTYPE and refs.shape == (0,) and refs.dtype == np.int32
        st = r.last_mesh_stats()
        assert all(st[k] == 0 for k in mm.COUNTS) and st["rounds"] == 0
    r.close()


def round_trip(r, seg, level, W, H, what):
    """mesh_desc of the level's mesh scan-converts back to the level's id plane, bit for bit."""
    from video_segment_amd import render
    ids = r.id_image(seg, level)
    for connect in (0, cm.N4):
        segments, vertices, loops, refs = r.level_mesh(seg, level, connect)
        if connect == 0:
            group_ids = r.level_regions(seg, level)[0]["id"]
        else:
            group_ids = r.level_components(seg, level, connect)[0]["id"]
        desc = render.mesh_desc(W, H, group_ids, segments, vertices, loops, refs)
        rows = r.rasterize(desc)                      # k_vec_walk, the radix sort, k_vec_pairs
        assert r.last_vector_stats()["lines"] > 0
        assert np.array_equal(vm.id_plane(rows, W, H), ids), (what, level, connect)


def test_a_desc_made_of_the_mesh_rasterizes_back_to_the_id_plane(vsg):
    c = BY_NAME["three_levels"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    seg = c.msg.SerializeToString()
    for level in (0, max(c.levels)):
        round_trip(r, seg, level, c.W, c.H, c.name)
    r.close()
    c = BY_NAME["voronoi_640x360"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    round_trip(r, c.msg.SerializeToString(), 0, c.W, c.H, c.name)
    r.close()


def test_bad_levels_and_bad_connectedness(vsg):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    c = BY_NAME["three_levels"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    seg = c.msg.SerializeToString()
    for level in (3, 4, -1):
        for connect in MODES:
            with pytest.raises(VsgError) as e:
                r.level_mesh(seg, level, connect)
            assert e.value.code == VSG_ERR_INVALID
    for connect in (3, -1):
        with pytest.raises(VsgError) as e:
            r.level_mesh(seg, 0, connect)
        assert e.value.code == VSG_ERR_INVALID
    assert_same(r.level_mesh(seg, 2, cm.N8), model(lc.id_image(c.msg, 2), cm.N8), "after the refusals")
    r.close()


def test_capacities_and_count_only(vsg):
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    seg = c.msg.SerializeToString()
    L = render.lib()
    r = vsg.SegmentationRenderer(c.W, c.H)
    for connect in (0, cm.N4):
        want = model(lc.id_image(c.msg, 1), connect)
        sizes = tuple(len(a) for a in want)

        def call(outs, caps):
            counts = [C.c_size_t(77) for _ in range(4)]
            args = []
            for o, cap, n in zip(outs, caps, counts):
                args += [o.ctypes.data_as(C.c_void_p) if o is not None else None, cap, C.byref(n)]
            rc = L.vsg_render_level_mesh(r.h, seg, len(seg), 1, connect, *args, 0)
            return (rc,) + tuple(n.value for n in counts)

        assert call([None] * 4, [0] * 4) == (0,) + sizes                      # count only
        outs = [np.zeros(sizes[0] + 2, mm.SEGMENT_DTYPE), np.zeros((sizes[1] + 2, 2), np.int32),
                np.zeros(sizes[2] + 2, mm.LOOP_DTYPE), np.zeros(sizes[3] + 2, np.int32)]

        def fill():
            for o in outs:
                o.view(np.uint8).reshape(-1)[:] = 0x5A

        def untouched(o, start=0):
            return (o[start:].view(np.uint8) == 0x5A).all()

        for k in range(4):                                                    # each capacity one too small
            caps = list(sizes)
            caps[k] -= 1
            fill()
            assert call(outs, caps) == (-1,) + sizes, k
            assert all(untouched(o) for o in outs), k
        fill()
        assert call(outs, [0] * 4) == (-1,) + sizes and all(untouched(o) for o in outs)
        fill()
        assert call(outs, list(sizes)) == (0,) + sizes                        # exact capacities
        assert_same([o[:n] for o, n in zip(outs, sizes)], want, "exact")
        assert all(untouched(o, n) for o, n in zip(outs, sizes))
    r.close()


def test_device_outputs_equal_host_outputs(vsg):
    import torch
    from video_segment_amd import render
    c = BY_NAME["three_levels"]
    seg = c.msg.SerializeToString()
    dev = torch.device("cuda", 0)
    r = vsg.SegmentationRenderer(c.W, c.H)
    widths = (render.MESH_SEGMENT_WORDS, 2, render.MESH_LOOP_WORDS, 0)
    guard = 0x5A5A5A5A
    for level in c.levels:
        for connect in MODES:
            host = r.level_mesh(seg, level, connect)
            sizes = [len(a) for a in host]
            outs = [torch.full((n + 3, w) if w else (n + 3,), guard, dtype=torch.int32, device=dev)
                    for n, w in zip(sizes, widths)]
            got = r.level_mesh(seg, level, connect, *outs)
            for name, g, h, n, w in zip(NAMES, got, host, sizes, widths):
                assert g.is_cuda and tuple(g.shape) == ((n, w) if w else (n,)), name
                assert g.cpu().numpy().tobytes() == h.tobytes(), (name, level, connect)
            assert all(bool((o[n:] == guard).all()) for o, n in zip(outs, sizes))
            # each list one entry too short: refused, nothing written
            for k in range(4):
                for o in outs:
                    o.fill_(guard)
                cut = [o[:n - (1 if j == k else 0)] for j, (o, n) in enumerate(zip(outs, sizes))]
                with pytest.raises(render.VsgError):
                    r.level_mesh(seg, level, connect, *cut)
                assert all(bool((o == guard).all()) for o in outs), (k, level, connect)
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
    small, large = lc.reuse_sequence()
    r = vsg.SegmentationRenderer(small.W, small.H)
    segs = {c.name: c.msg.SerializeToString() for c in (small, large)}

    def siblings(s):
        return (r.level_regions(s, 0), r.level_components(s, 0, cm.N8, label_image=True),
                r.level_boundaries(s, 0, cm.N4), r.level_adjacency(s, 0), r.level_contours(s, 0, cm.N4))

    before = {n: siblings(s) for n, s in segs.items()}
    want = {(c.name, k): model(lc.id_image(c.msg, 0), k) for c in (small, large) for k in (0, cm.N8)}
    allocs = []
    for _ in range(2):
        for c in (small, large, small):
            for k in (0, cm.N8):
                assert_same(r.level_mesh(segs[c.name], 0, k), want[c.name, k], (c.name, k))
                r.level_contours(segs[c.name], 0, k)           # interleaved: shares the contour stages' blocks
                r.level_boundaries(segs[c.name], 0, k)         # and the sort's work space
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
        r.level_mesh(seg, level, cm.N4)
        assert r.level is None
    first = r.render(seg)
    assert r.level == 1
    for level in c.levels:
        r.level_mesh(seg, level)
        assert r.level == 1
    assert tm.same_bits(r.render(seg), first)
    r.close()


def test_launches_are_a_function_of_the_mode_and_the_rounds(vsg):
    """Over every case at level 0, host outputs: one value per (connectedness, rounds)."""
    seen = {}
    for c in CASES:
        r = vsg.SegmentationRenderer(c.W, c.H, has_video=False)
        seg = c.msg.SerializeToString()
        for connect in MODES:
            r.level_mesh(seg, 0, connect)
            st = r.last_mesh_stats()
            if st["cracks"]:
                seen.setdefault((connect, st["rounds"]), {}).setdefault(st["launches"], []).append(c.name)
        r.close()
    assert all(len(v) == 1 for v in seen.values()), {k: v for k, v in seen.items() if len(v) > 1}
    assert max(len(names) for v in seen.values() for names in v.values()) >= 5      # shared by different content
    by_mode = {connect: sorted((rounds, list(v)[0]) for (m, rounds), v in seen.items() if m == connect)
               for connect in MODES}
    for connect, pairs in by_mode.items():
        # two more rounds of each of the three doublings are one more launch each and nothing else
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


def test_driver_prints_the_python_paths_sums(vsg, stream):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    r = vsg.SegmentationRenderer(W, H)
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3", "--nouse_pipeline"]
    for flags, connect in ((["--level_mesh", "0"], 0),
                           (["--level_mesh", "0", "--mesh_components", "--components_n8"], cm.N8)):
        lists = [r.level_mesh(seg, 0, connect) for seg in stream]
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        m = re.search(r"level_mesh_count=(\d+) level_mesh_fnv1a32=(\w+)", p.stdout)
        assert m, p.stdout
        assert int(m.group(1)) == sum(len(four[0]) for four in lists)
        assert int(m.group(2), 16) == rm.fnv1a32(a for four in lists for a in four)
    r.close()
