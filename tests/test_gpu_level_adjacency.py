"""vsg_render_level_adjacency on the MI355X (libvsg_render.so: the id plane or the component label image,
k_adj_classify's count and emit passes, the key sort, the scan, k_adj_table, k_adj_finish, k_adj_resolve,
k_copy_lists) against level_adjacency_model.py.  Nodes and edges are compared as raw bytes: there is no
tolerance anywhere in this file."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import level_adjacency_cases as ac
import level_adjacency_model as am
import level_boundaries_cases as bc
import level_components_model as cm
import level_regions_cases as lc
import render_model as rm
import synth
import vector_cases as vc
import vector_raster_model as vm

pytestmark = pytest.mark.gpu

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "video_segment_amd", "host")
CASES = ac.all_cases()
BY_NAME = {c.name: c for c in CASES}
MODES = (0, cm.N4, cm.N8)          # the regions' graph, the N4 components', the N8 components'
HOODS = (am.ADJACENT_N4, am.ADJACENT_N8)


@pytest.fixture(scope="module")
def vsg():
    import video_segment_amd as v
    from video_segment_amd import _lib, render
    _lib.build()
    render.build()
    assert _lib.lib().vsg_device_count() > 0
    assert (render.N4, render.N8) == (cm.N4, cm.N8)
    assert (render.ADJACENT_N4, render.ADJACENT_N8) == HOODS
    assert render.LEVEL_NODE_DTYPE == am.NODE_DTYPE and render.LEVEL_EDGE_DTYPE == am.EDGE_DTYPE
    return v


def assert_same(got, want, what):
    got_n, got_e = got
    want_n, want_e = want
    assert got_n.dtype == am.NODE_DTYPE and got_n.shape == want_n.shape, (what, got_n.shape, want_n.shape)
    assert got_e.dtype == am.EDGE_DTYPE and got_e.shape == want_e.shape, (what, got_e.shape, want_e.shape)
    assert am.same_bits(got_n, want_n), what
    assert am.same_bits(got_e, want_e), what


def model(ids, connect, hood):
    if connect == 0:
        return am.adjacency(ids, hood)
    comps, _, labels = cm.sweep(ids, connect)
    return am.adjacency(labels, hood, comps)


def check_stats(st, want, what):
    nodes, edges = want
    assert st["sides"] == am.sides_of(nodes, edges), (what, st)
    assert st["keys"] >= 1 or st["sides"] == 0, (what, st)
    assert st["keys"] <= st["sides"], (what, st)
    assert st["nodes"] == len(nodes) and st["edges"] == len(edges), (what, st)
    assert st["largest_node_edges"] == (nodes["num_edges"].max() if len(nodes) else 0), (what, st)


def check_ids(r, seg, ids, level, what):
    """All six combinations of one level against the model, with the stats and the sibling calls."""
    out = {}
    for connect in MODES:
        for hood in HOODS:
            want = model(ids, connect, hood)
            got = r.level_adjacency(seg, level, connect, hood)
            assert_same(got, want, (what, level, connect, hood))
            check_stats(r.last_adjacency_stats(), want, (what, level, connect, hood))
            out[connect, hood] = got
        # record k belongs to record k of the call the mode is named after
        nodes = out[connect, am.ADJACENT_N4][0]
        if connect == 0:
            regions, _ = r.level_regions(seg, level)
            assert np.array_equal(nodes["id"], regions["id"]) and (nodes["component"] == -1).all()
        else:
            comps, _ = r.level_components(seg, level, connect)
            assert np.array_equal(nodes["id"], comps["id"])
            assert np.array_equal(nodes["component"], comps["component"])
    return out


def check_case(vsg, case):
    r = vsg.SegmentationRenderer(case.W, case.H, has_video=False)
    seg = case.msg.SerializeToString()
    out = {level: check_ids(r, seg, lc.id_image(case.msg, level), level, case.name) for level in case.levels}
    r.close()
    return out


NAMED = ("star_300x2", "star_2x300", "diag_only", "max_id", "hole", "uncovered_frame")


@pytest.mark.parametrize("W", bc.WIDTHS)
def test_widths_around_wavefront_and_block_boundaries(vsg, W):
    for H in bc.HEIGHTS:
        check_case(vsg, BY_NAME["width_%dx%d" % (W, H)])


@pytest.mark.parametrize("name", [c.name for c in CASES if not c.name.startswith("width_") and c.name not in NAMED])
def test_every_other_case(vsg, name):
    check_case(vsg, BY_NAME[name])


@pytest.mark.parametrize("name", ["star_300x2", "star_2x300"])
def test_a_node_with_300_edges(vsg, name):
    got = check_case(vsg, BY_NAME[name])[0]
    for connect in MODES:
        for hood in HOODS:
            nodes, edges = got[connect, hood]
            assert len(nodes) == ac.STAR_LEAVES + 1
            assert nodes[0]["id"] == ac.STAR_HUB and nodes[0]["num_edges"] == ac.STAR_LEAVES
            hub = am.edges_of(nodes, edges, 0)
            assert np.array_equal(hub["neighbour"], 1 + np.arange(ac.STAR_LEAVES))
            assert np.array_equal(hub["neighbour_id"], 100 + np.arange(ac.STAR_LEAVES))
            assert (hub["shared_n4"] == 1).all() and nodes[0]["border_shared"] == ac.STAR_LEAVES


def test_components_of_one_region_that_touch_diagonally(vsg):
    c = BY_NAME["diag_only"]
    got = check_case(vsg, c)[0]
    nodes, edges = got[cm.N4, am.ADJACENT_N8]
    assert len(nodes) == c.W * c.H
    own = edges[edges["neighbour_id"] == np.repeat(nodes["id"], nodes["num_edges"])]
    assert len(own) > 0 and (own["shared_n4"] == 0).all() and (own["shared_diagonal"] > 0).all()
    nodes, edges = got[cm.N4, am.ADJACENT_N4]
    assert (edges["neighbour_id"] != np.repeat(nodes["id"], nodes["num_edges"])).all()
    assert (edges["shared_diagonal"] == 0).all()


def test_ids_of_31_bits(vsg):
    got = check_case(vsg, BY_NAME["max_id"])[0]
    for hood in HOODS:
        nodes, edges = got[0, hood]
        assert nodes["id"].tolist() == [0, ac.MAX_ID]
        assert edges["neighbour"].tolist() == [1, 0] and edges["neighbour_id"].tolist() == [ac.MAX_ID, 0]


def test_a_node_with_all_three_kinds_of_border(vsg):
    got = check_case(vsg, BY_NAME["hole"])[0]
    nodes, _ = got[0, am.ADJACENT_N4]
    assert nodes["id"].tolist() == [3, 8]
    assert min(nodes[0]["border_frame"], nodes[0]["border_uncovered"], nodes[0]["border_shared"]) > 0
    assert nodes[1].tolist()[4:] == (0, 8, 2)


def test_a_frame_without_a_covered_pixel(vsg):
    c = BY_NAME["uncovered_frame"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    for connect in MODES:
        for hood in HOODS:
            nodes, edges = r.level_adjacency(c.msg.SerializeToString(), 0, connect, hood)
            assert nodes.shape == (0,) and nodes.dtype == am.NODE_DTYPE
            assert edges.shape == (0,) and edges.dtype == am.EDGE_DTYPE
            st = r.last_adjacency_stats()
            assert all(st[k] == 0 for k in ("sides", "keys", "nodes", "edges", "largest_node_edges"))
    r.close()


def test_refusals(vsg):
    from video_segment_amd._lib import VSG_ERR_INVALID, VsgError
    c = BY_NAME["three_levels"]
    r = vsg.SegmentationRenderer(c.W, c.H)
    seg = c.msg.SerializeToString()
    for level in (3, 4, -1):
        for connect in MODES:
            with pytest.raises(VsgError) as e:
                r.level_adjacency(seg, level, connect)
            assert e.value.code == VSG_ERR_INVALID
    for connect in (3, -1):
        with pytest.raises(VsgError) as e:
            r.level_adjacency(seg, 0, connect)
        assert e.value.code == VSG_ERR_INVALID
    for hood in (0, 3, -1):
        with pytest.raises(VsgError) as e:
            r.level_adjacency(seg, 0, 0, hood)
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
        for hood in HOODS:
            want_n, want_e = model(lc.id_image(c.msg, 1), connect, hood)
            nn_, ne_ = len(want_n), len(want_e)
            assert nn_ > 1 and ne_ > 1

            def call(nodes, cap_n, edges, cap_e):
                nn, ne = C.c_size_t(77), C.c_size_t(77)
                rc = L.vsg_render_level_adjacency(r.h, seg, len(seg), 1, connect, hood, ptr(nodes), cap_n,
                                                  C.byref(nn), ptr(edges), cap_e, C.byref(ne), 0)
                return rc, nn.value, ne.value

            assert call(None, 0, None, 0) == (0, nn_, ne_)                    # count only
            nodes = np.zeros(nn_ + 2, am.NODE_DTYPE)
            edges = np.zeros(ne_ + 2, am.EDGE_DTYPE)
            pattern_n = np.frombuffer(b"\x5a" * nodes.nbytes, am.NODE_DTYPE)
            pattern_e = np.frombuffer(b"\x5a" * edges.nbytes, am.EDGE_DTYPE)
            for cap_n, cap_e in ((nn_ - 1, ne_), (nn_, ne_ - 1), (nn_ - 1, ne_ - 1), (0, ne_), (nn_, 0)):
                nodes[:] = pattern_n
                edges[:] = pattern_e
                assert call(nodes, cap_n, edges, cap_e) == (-1, nn_, ne_), (cap_n, cap_e)
                assert am.same_bits(nodes, pattern_n) and am.same_bits(edges, pattern_e), (cap_n, cap_e)
            assert call(nodes, nn_, edges, ne_) == (0, nn_, ne_)              # exact capacities
            assert_same((nodes[:nn_], edges[:ne_]), (want_n, want_e), "exact")
            assert am.same_bits(nodes[nn_:], pattern_n[nn_:]) and am.same_bits(edges[ne_:], pattern_e[ne_:])
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
            for hood in HOODS:
                host_n, host_e = r.level_adjacency(seg, level, connect, hood)
                nn_, ne_ = len(host_n), len(host_e)
                d_nodes = torch.full((nn_ + 3, render.LEVEL_NODE_WORDS), 0x5A5A5A5A, dtype=torch.int32, device=dev)
                d_edges = torch.full((ne_ + 3, render.LEVEL_EDGE_WORDS), 0x5A5A5A5A, dtype=torch.int32, device=dev)
                got_n, got_e = r.level_adjacency(seg, level, connect, hood, nodes_out=d_nodes, edges_out=d_edges)
                assert got_n.is_cuda and got_e.is_cuda and got_n.shape == (nn_, 7) and got_e.shape == (ne_, 4)
                assert got_n.cpu().numpy().tobytes() == host_n.tobytes()
                assert got_e.cpu().numpy().tobytes() == host_e.tobytes()
                assert bool((d_nodes[nn_:] == 0x5A5A5A5A).all()) and bool((d_edges[ne_:] == 0x5A5A5A5A).all())
                # one node, then one edge too few: refused, nothing written
                for cut_n, cut_e in ((1, 0), (0, 1)):
                    if ne_ - cut_e < 0:
                        continue
                    d_nodes.fill_(0x5A5A5A5A)
                    d_edges.fill_(0x5A5A5A5A)
                    with pytest.raises(render.VsgError):
                        r.level_adjacency(seg, level, connect, hood, nodes_out=d_nodes[:nn_ - cut_n],
                                          edges_out=d_edges[:ne_ - cut_e])
                    assert bool((d_nodes == 0x5A5A5A5A).all()) and bool((d_edges == 0x5A5A5A5A).all())
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

    def siblings(s):
        return (r.level_regions(s, 0), r.level_components(s, 0, cm.N8, label_image=True),
                r.level_boundaries(s, 0, cm.N4, True))

    before = {n: siblings(s) for n, s in segs.items()}
    combos = [(connect, hood) for connect in (0, cm.N8) for hood in HOODS]
    want = {(c.name, k): model(lc.id_image(c.msg, 0), *k) for c in (small, large) for k in combos}
    allocs = []
    for _ in range(2):
        for c in (small, large, small):
            for k in combos:
                assert_same(r.level_adjacency(segs[c.name], 0, *k), want[c.name, k], (c.name, k))
            allocs.append(r.last_stats()["device_allocations"])
    # the second round of identical calls allocates nothing
    assert allocs[1] > allocs[0] > 0 and allocs[3:] == [allocs[2]] * 3, allocs
    for n, s in segs.items():
        for a, b in zip(siblings(s), before[n]):
            assert all(am.same_bits(x, y) for x, y in zip(a, b)), n
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
            r.level_adjacency(seg, 0)
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
        for hood in HOODS:
            want = am.adjacency(plane, hood, of)
            assert_same(r.level_adjacency(seg, level, connect, hood), want, ("1080p", level, connect, hood))
            st = r.last_adjacency_stats()
            check_stats(st, want, ("1080p", level, connect, hood))
            assert all(st[k] > 0 for k in ("plane_us", "count_us", "emit_us", "sort_us", "table_us")), st
    r.close()


def test_driver_prints_the_python_paths_sums(vsg, stream):
    subprocess.check_call(["make", "-C", HOST, "-s"])
    W, H, N, chunk = STREAM
    r = vsg.SegmentationRenderer(W, H)
    base = [os.path.join(HOST, "seg_tree_synth"), "--width", str(W), "--height", str(H), "--frames", str(N),
            "--chunk_size", str(chunk), "--input", "soft", "--flow", "--region_segmentation",
            "--chunk_set_size", "3", "--chunk_set_overlap", "1", "--min_region_num", "3", "--nouse_pipeline"]
    for flags, connect, hood in ((["--level_adjacency", "0"], 0, am.ADJACENT_N4),
                                 (["--level_adjacency", "0", "--adjacency_n8", "--adjacency_components",
                                   "--components_n8"], cm.N8, am.ADJACENT_N8)):
        lists = [r.level_adjacency(seg, 0, connect, hood) for seg in stream]
        p = subprocess.run(base + flags, capture_output=True, text=True, timeout=300)
        assert p.returncode == 0, p.stderr
        m = re.search(r"level_adjacency_nodes=(\d+) adjacency_edges=(\d+) adjacency_fnv1a32=(\w+)", p.stdout)
        assert m, p.stdout
        assert int(m.group(1)) == sum(len(n) for n, _ in lists)
        assert int(m.group(2)) == sum(len(e) for _, e in lists)
        assert int(m.group(3), 16) == rm.fnv1a32(a for pair in lists for a in pair)
    r.close()
